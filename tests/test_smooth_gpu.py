"""The LargeSteps solves on the GPU (csrc/psdr_smooth.hip through psdr_cuda.LargeSteps and the C ABI): both launch forms against the float64 direct solve
(smooth_cases.BOUND) and against the host harness of the same header (1e-5 relative: the two differ only in the order of their sums; iteration counts within 2),
the vertex counts at which the one-workgroup kernel changes its shape, determinism, stream order, autograd and one render through the parameterisation.
Right-hand sides are the Gaussian tables of tests/test_smooth_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
import smooth_cases as sc
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from psdr_cuda import _abi

pytestmark = pytest.mark.gpu

FORMS = {"one_workgroup": 1, "multi_launch": 0}


def _b(name, seed=11):
    v, _ = sc.case(name)
    b = np.random.default_rng(seed).standard_normal((len(v), 3)).astype(np.float32)
    if name == "grid40":
        b[:, 2] = 0.0
    return b


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["ico3", "ico4", "grid40", "components", "hub1000"])
def test_both_launch_forms(name, form):
    v, f = sc.case(name)
    for lam in (10.0, 100.0):
        ls = psdr_cuda.LargeSteps(f, len(v), lmbda=lam, one_workgroup=FORMS[form])
        b = _b(name)
        x = ls.from_differential(_dev(b)).cpu().numpy()
        info = ls.info()
        xh, ih = sc.host_solve(len(v), f, lam, b)
        e_ref, e_host = sc.rel_l2(x, sc.reference_solve(name, lam, b)), sc.rel_l2(x, xh)
        print("%s %s lambda %g: %d iterations (host %d), rel-L2 vs direct solve %.2e, vs host %.2e" % (name, form, lam, info["iterations"], ih["iterations"], e_ref, e_host))
        assert info["form"] == form and info["converged"]
        assert np.isfinite(x).all() and e_ref <= sc.BOUND, e_ref
        assert e_host <= 1e-5, e_host
        assert abs(info["iterations"] - ih["iterations"]) <= 2, (info, ih)
        if name == "grid40":
            assert (x[:, 2] == 0).all()
        if name == "hub1000":
            assert info["long_rows"] == 1
        # the operator, against float64
        u = ls.to_differential(_dev(b)).cpu().numpy()
        assert sc.rel_l2(u, sc.reference_apply(name, lam, b)) <= 1e-6


def _limit():
    ls = psdr_cuda.LargeSteps(np.array([[0, 1, 2]], np.int32), 3)
    return ls.info()["one_workgroup_limit"], ls.info()["one_workgroup_default"]


def _padded(V):
    if V == 1:
        return np.array([[0.25, -1.0, 2.0]]), np.zeros((0, 3), np.int32)
    v, f = sc.case("ico1") if V < 2562 else sc.case("ico4")
    return sc.padded(v, f, V)


@pytest.mark.parametrize("option", [-1, 0, 1])
@pytest.mark.parametrize("which", ["1", "63", "64", "65", "limit", "limit+1"])
def test_vertex_counts_where_the_one_workgroup_kernel_changes_shape(which, option):
    """V = 1 without a face; one lane short of a wave, a wave, a wave and a lane; the one-workgroup limit and one vertex more -- a sphere padded with isolated
    vertices.  Option -1 takes the form the limit implies; forcing the one-workgroup form past its limit is an error, not a fallback."""
    limit, default = _limit()
    assert limit >= 2562 and default <= limit
    V = {"limit": limit, "limit+1": limit + 1}.get(which) or int(which)
    v, f = _padded(V)
    assert len(v) == V
    lam = 19.0
    if option == 1 and V > limit:
        ls = psdr_cuda.LargeSteps(f, V, lmbda=lam, one_workgroup=1)
        with pytest.raises(RuntimeError, match="at most"):
            ls.from_differential(_dev(v))
        return
    ls = psdr_cuda.LargeSteps(f, V, lmbda=lam, one_workgroup=option)
    b = np.random.default_rng(V).standard_normal((V, 3)).astype(np.float32)
    x = ls.from_differential(_dev(b)).cpu().numpy()
    info = ls.info()
    want = "one_workgroup" if option == 1 or (option == -1 and V <= default) else "multi_launch"
    assert info["form"] == want and info["converged"] and info["num_vertices"] == V
    ref = sc.reference_solve_mesh(V, f, lam, b)
    assert sc.rel_l2(x, ref) <= sc.BOUND
    if len(f):          # the isolated vertices are identity rows: x_i - b_i is the residual's entry, and |r_i| <= ||r|| <= tol ||b|| (twice that: rounding)
        used = np.zeros(V, bool); used[f.ravel()] = True
        assert np.abs(x[~used] - b[~used]).max() <= 2 * sc.TOL * np.linalg.norm(b, axis=0).max()
    # warm start from the answer, in place of nothing: at most one step
    x2 = ls.from_differential(_dev(b), x0=_dev(ref)).cpu().numpy()
    assert ls.info()["iterations"] <= 1 and sc.rel_l2(x2, ref) <= sc.BOUND


def test_large_mesh_on_the_multi_launch_form():
    """the 40962-vertex sphere at lambda = 100: the hardest of the cases (189 iterations on the host) converges within the default max_iter"""
    v, f = sc.case("ico6")
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=100.0)
    b = _b("ico6")
    x = ls.from_differential(_dev(b)).cpu().numpy()
    info = ls.info()
    e = sc.rel_l2(x, sc.reference_solve("ico6", 100.0, b))
    print("ico6 lambda 100: %d iterations of at most %d, %d launches, rel-L2 %.2e" % (info["iterations"], ls.max_iter, info["launches"], e))
    assert info["form"] == "multi_launch" and info["converged"] and info["iterations"] < ls.max_iter
    assert e <= sc.BOUND, e


@pytest.mark.parametrize("form", list(FORMS))
def test_iteration_limit_and_non_finite_input(form):
    v, f = sc.case("ico4")
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=100.0, max_iter=3, one_workgroup=FORMS[form])
    x = ls.from_differential(_dev(_b("ico4")))
    info = ls.info()
    assert not info["converged"] and info["iterations"] == 3 and bool(torch.isfinite(x).all())
    b = _b("ico4")
    b[7, 1] = np.nan
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=10.0, max_iter=12, one_workgroup=FORMS[form])
    x = ls.from_differential(_dev(b))
    info = ls.info()
    assert info["iterations"] == 12 and not info["converged"]
    assert not bool(torch.isfinite(x[:, 1]).any()) and bool(torch.isfinite(x[:, 0]).all()) and bool(torch.isfinite(x[:, 2]).all())


@pytest.mark.parametrize("form", list(FORMS))
def test_two_solves_return_the_same_bits(form):
    """fixed-order reductions, no float atomics: the same input gives torch.equal results and the same iteration count, cold and warm, on one handle and on two"""
    v, f = sc.case("ico4")
    b, x0 = _dev(_b("ico4")), _dev(v)
    runs = []
    for _ in range(2):
        ls = psdr_cuda.LargeSteps(f, len(v), lmbda=100.0, one_workgroup=FORMS[form])
        for guess in (None, x0, None):
            x = ls.from_differential(b, x0=guess)
            runs.append((x.clone(), ls.info()["iterations"]))
    for k in (0, 1, 2):
        assert torch.equal(runs[k][0], runs[k + 3][0]) and runs[k][1] == runs[k + 3][1]
    assert torch.equal(runs[0][0], runs[2][0]) and runs[0][1] == runs[2][1]


@pytest.mark.parametrize("form", list(FORMS))
def test_solve_is_ordered_on_the_callers_stream(form):
    """a solve on a side stream followed, without a synchronise, by a torch operation on its output = the synchronised result"""
    v, f = sc.case("ico4")
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=100.0, one_workgroup=FORMS[form])
    b = _dev(_b("ico4"))
    want = ls.from_differential(b) * 2.0 + 1.0
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = ls.from_differential(b) * 2.0 + 1.0
    side.synchronize()
    assert torch.equal(got, want)


def test_gradient_of_a_solve_is_a_solve():
    v, f = sc.case("ico3")
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=19.0)
    u = _dev(_b("ico3")).requires_grad_(True)
    w = _dev(_b("ico3", seed=2))
    (ls.from_differential(u) * w).sum().backward()
    want = ls.precondition(w)
    assert not want.requires_grad
    assert sc.rel_l2(u.grad.cpu().numpy(), want.cpu().numpy()) <= 1e-6
    assert sc.rel_l2(u.grad.cpu().numpy(), sc.reference_solve("ico3", 19.0, w.cpu().numpy())) <= sc.BOUND


def test_gradient_of_the_operator_is_the_operator():
    v, f = sc.case("ico3")
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=19.0)
    x = Vector3fD._wrap(_dev(v))
    ek.set_requires_gradient(x)
    w = _dev(_b("ico3", seed=2))
    u = ls.to_differential(x)
    assert isinstance(u, Vector3fD)
    (u.t * w).sum().backward()
    assert sc.rel_l2(x.t.grad.cpu().numpy(), ls.to_differential(w).cpu().numpy()) <= 1e-6
    assert sc.rel_l2(x.t.grad.cpu().numpy(), sc.reference_apply("ico3", 19.0, w.cpu().numpy())) <= 1e-6


def test_forward_mode_through_a_solve():
    """enoki.forward's double backward (enoki/_array.py _jvp_wrt) through from_differential and to_differential: the tangent of M^-1 (u0 + P d) is M^-1 d"""
    from enoki._array import _jvp_wrt
    v, f = sc.case("ico3")
    ls = psdr_cuda.LargeSteps(f, len(v), lmbda=19.0)
    P = FloatD(0.0)
    ek.set_requires_gradient(P)
    d = _dev(_b("ico3", seed=3))
    u = Vector3fD._wrap(_dev(_b("ico3"))) + Vector3fD._wrap(d) * P
    x = ls.from_differential(u)
    y = ls.to_differential(x)
    tx, ty = _jvp_wrt([x.t, y.t], P.t)
    assert sc.rel_l2(tx.cpu().numpy(), ls.precondition(d).cpu().numpy()) <= 1e-5
    assert sc.rel_l2(ty.cpu().numpy(), d.cpu().numpy()) <= 1e-5


# ---------------------------------------------------------------- one render through the parameterisation
def _sphere_scene():
    from psdr_cuda.fixtures import scene_path
    s = psdr_cuda.Scene()
    s.load_file(scene_path("cbox_occluder"), False)
    s.opts.width = s.opts.height = 32
    s.opts.spp, s.opts.sppe, s.opts.sppse, s.opts.log_level = 4, 4, 4, 0
    v, f = sc.icosphere(2)
    mesh = s.param_map["Mesh[id=occluder]"]
    mesh.set_geometry(v * 40.0, f)
    return s, mesh


def test_render_gradient_through_from_differential():
    """DirectIntegrator renderD (interior, primary- and secondary-edge terms) of the Cornell box with a sphere in place of the occluder, once with the vertex
    positions a leaf and once with vertex_positions = from_differential(u), the same adjoint image: u.grad = M^-1 x.grad."""
    integ = psdr_cuda.DirectIntegrator(1, 1)
    s0, mesh0 = _sphere_scene()
    ls = psdr_cuda.LargeSteps(mesh0)
    u0 = ls.to_differential(mesh0.vertex_positions)
    x_val = ek.detach(ls.from_differential(u0))          # the positions of both runs, bit for bit (two solves of one input return the same bits)
    adj = torch.rand(32 * 32, 3, generator=torch.Generator().manual_seed(3)).cuda()
    # (a) the positions are the parameter
    x = Vector3fD._wrap(x_val.t.clone())
    ek.set_requires_gradient(x)
    mesh0.vertex_positions = x
    s0.configure()
    (integ.renderD(s0).t * adj).sum().backward()
    gx = x.t.grad.clone()
    assert float(gx.abs().sum()) > 0
    # (b) u is the parameter, on a fresh scene object
    s1, mesh1 = _sphere_scene()
    u = Vector3fD._wrap(u0.t.detach().clone())
    ek.set_requires_gradient(u)
    mesh1.vertex_positions = ls.from_differential(u)
    s1.configure()
    (integ.renderD(s1).t * adj).sum().backward()
    want = ls.precondition(gx)
    e = sc.rel_l2(u.t.grad.cpu().numpy(), want.cpu().numpy())
    print("u.grad vs precondition(x.grad): rel-L2 %.2e" % e)
    assert e <= 1e-5, e


# ---------------------------------------------------------------- error cases through the ABI
def test_abi_error_cases():
    lib = _abi.load_hip()

    def fails(rc, word):
        msg = lib.psdr_last_error().decode()
        assert rc != 0 and word in msg, (rc, msg)

    h = C.c_void_p()
    good = np.array([[0, 1, 2]], np.int32)
    bad = np.array([[0, 1, 3]], np.int32)
    fails(lib.psdr_smooth_create(3, 1, bad.ctypes.data, C.byref(h)), "outside")
    assert not h.value
    fails(lib.psdr_smooth_create(0, 0, None, C.byref(h)), "V must be positive")
    fails(lib.psdr_smooth_create(3, 1, good.ctypes.data, None), "null")
    x, y = torch.zeros(3, 3, device="cuda"), torch.zeros(3, 3, device="cuda")
    fails(lib.psdr_smooth_apply(None, 1.0, x.data_ptr(), y.data_ptr(), None), "null handle")
    fails(lib.psdr_smooth_solve(None, 1.0, x.data_ptr(), None, y.data_ptr(), 1e-6, 10, None), "null handle")
    fails(lib.psdr_smooth_set_option(None, b"one_workgroup", 1), "null handle")
    fails(lib.psdr_smooth_info(None, C.byref(_abi.SmoothInfo())), "null handle")
    lib.psdr_smooth_destroy(None)          # a no-op
    assert lib.psdr_smooth_create(3, 1, good.ctypes.data, C.byref(h)) == 0 and h.value
    try:
        fails(lib.psdr_smooth_solve(h, -1.0, x.data_ptr(), None, y.data_ptr(), 1e-6, 10, None), "lambda")
        fails(lib.psdr_smooth_solve(h, float("nan"), x.data_ptr(), None, y.data_ptr(), 1e-6, 10, None), "lambda")
        fails(lib.psdr_smooth_apply(h, -1.0, x.data_ptr(), y.data_ptr(), None), "lambda")
        fails(lib.psdr_smooth_solve(h, 1.0, x.data_ptr(), None, y.data_ptr(), 0.0, 10, None), "tol")
        fails(lib.psdr_smooth_solve(h, 1.0, x.data_ptr(), None, y.data_ptr(), 1e-6, 0, None), "max_iter")
        fails(lib.psdr_smooth_solve(h, 1.0, x.data_ptr(), None, x.data_ptr(), 1e-6, 10, None), "two device tables")
        fails(lib.psdr_smooth_set_option(h, b"no_such_option", 1), "unknown option")
        fails(lib.psdr_smooth_set_option(h, b"one_workgroup", 2), "one_workgroup")
        s = _abi.SmoothInfo()
        assert lib.psdr_smooth_info(h, C.byref(s)) == 0 and s.form == -1 and s.num_vertices == 3 and s.num_entries == 6
    finally:
        lib.psdr_smooth_destroy(h)
