"""The LightStageIntegrator on the GPU (csrc/psdr_lightstage.hip), through the C ABI and the Python surface: every plane of the stack against the
PointLightIntegrator's launch for that light on the same handle (kind 4: tests/test_pointlight_gpu.py) and against the host harness that runs the same
estimator (tests/hostcheck/hostcheck_lightstage.cpp; tests/test_lightstage_host.py pins that one on the single-light harness)."""
import ctypes as C

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from colloc_microfacet_helpers import scene as mf_scene
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import dot_tables, isolated_pixels_unbiased, load_scene, random_tangents, rel_l2, tangents_wrt
from lightstage_helpers import BELOW_FLOOR, OCCLUDER_LIGHTS, StackScene, host_stack_render, lights_of, stack_opts
from pointlight_helpers import point_opts
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)


def _planes_match(plane, ref, label):
    """two instantiations of one expression: per pixel within 4 eps32 of the plane's maximum (COVERAGE, "256 against 257 words"); returns the worst ratio"""
    top = float(np.abs(ref).max())
    if top == 0:
        assert not np.any(plane), label
        return 0.0
    ratio = float(np.abs(plane.astype(np.float64) - ref).max() / (EPS32 * top))
    assert ratio <= 4.0, (label, ratio)
    return ratio


@pytest.mark.parametrize("name,tree", [("cbox_occluder", False), ("cbox_rough", False), ("bunny_light", True), ("cbox_bunny", True), ("cbox_env", False)])
def test_render_c_planes(name, tree):
    """renderC on the five scene forms at 19 x 19 x 3 (atomic splat, a partly filled last workgroup) and 32 x 32 x 16 (plain stores) into a buffer of NaN: every
    plane finite; plane l within 4 eps32 of its maximum, per pixel, of the kind-4 launch for light l at the same options; the stack against the host harness at
    test_pointlight_gpu's bounds (rel-L2 1e-4 outside helpers.isolated_pixels_unbiased's pixels, at most 0.5 % of them)."""
    worst = 0.0
    for res, spp in ((19, 3), (32, 16)):
        sc, _ = load_scene(name, res=res, spp=spp)
        tb = sc.tables(0)
        pos = lights_of(name, tb)
        g = StackScene(tb).set_lights(pos)
        off = (7, 0, 0)
        img = g.stack_render_c(stack_opts(spp, rng_offset=off))
        assert img.shape[0] == len(pos) and np.isfinite(img).all()
        for l, p in enumerate(pos):
            worst = max(worst, _planes_match(img[l], g.set_light(p).render_c(point_opts(spp, rng_offset=off)), (name, res, l)))
        ref = host_stack_render(tb, stack_opts(spp, rng_offset=off), pos)
        for l in range(len(pos)):
            if name == "cbox_occluder" and l == BELOW_FLOOR:
                assert not np.any(img[l]) and not np.any(ref[l])
                continue
            bad = np.abs(img[l] - ref[l]).max(axis=1) > 1e-3 * (1 + np.abs(ref[l]).max(axis=1)) if tree else np.zeros(len(ref[l]), bool)
            assert ref[l].max() > 0          # (lit and dark pixels of every light set: tests/test_lightstage_host.py)
            assert bad.mean() <= 5e-3, (l, bad.mean())
            assert rel_l2(img[l][~bad], ref[l][~bad]) < 1e-4, (l, rel_l2(img[l][~bad], ref[l][~bad]))
            isolated_pixels_unbiased(img[l], ref[l], bad, "%s plane %d" % (name, l))
        if name == "cbox_occluder":
            assert np.array_equal(img[0], img[2])          # coincident lights
    print("%s: worst |stack plane - kind-4 launch| / (eps32 * plane max) = %.2f" % (name, worst))


def test_one_light_and_256_lights():
    """L = 1 and L = 256 at 8 x 8 x 1: plane 0 of the one-light stack and plane 255 of the full stack equal the single-light render of their own light; nothing
    behind plane L - 1 is written (a guard plane of NaN)."""
    sc, _ = load_scene("cbox_occluder", res=8, spp=1)
    tb = sc.tables(0)
    g = StackScene(tb)
    o, po = stack_opts(1, rng_offset=(5, 0, 0)), point_opts(1, rng_offset=(5, 0, 0))
    rng = np.random.default_rng(11)
    pos = np.stack([rng.uniform(-90, 90, 256), rng.uniform(110, 195, 256), rng.uniform(-90, 190, 256)], axis=1).astype(np.float32)
    pos[255] = OCCLUDER_LIGHTS[1]
    for L in (1, 256):
        img = g.set_lights(pos[256 - L:]).stack_render_c(o, guard_planes=1)
        assert np.isfinite(img[:L]).all() and np.isnan(img[L]).all()
        _planes_match(img[L - 1], g.set_light(pos[255]).render_c(po), L)
        assert img[L - 1].max() > 0
        if L == 256:
            _planes_match(img[0], g.set_light(pos[0]).render_c(po), 0)
            _planes_match(img[100], g.set_light(pos[100]).render_c(po), 100)


def test_forward_mode():
    """Forward mode: material duals against per-light kind-4 launches at 1e-5 rel-L2 (test_pointlight_gpu's bound between its own launches); geometry duals with
    sppe and sppse on against the harness at 1e-3 and against the kind-4 launches at 1e-5; one light's tangent leaves every other plane's derivative exactly 0;
    K = 3 gives the columns of K = 1 launches."""
    sc, _ = load_scene("cbox_rough", res=24, spp=8)
    tb = sc.tables(0)
    pos = lights_of("cbox_rough", tb)
    o, po = stack_opts(8, rng_offset=(3, 0, 0)), point_opts(8, rng_offset=(3, 0, 0))
    ts = random_tangents(tb, ["texels"], seed=2)
    g = StackScene(tb).set_lights(pos)
    img, d = g.stack_render_d_fwd(o, [ts])
    assert np.isfinite(img).all() and np.isfinite(d).all()
    for l, p in enumerate(pos):
        rimg, rd = g.set_light(p).render_d_fwd(po, [ts])
        assert np.abs(rd).max() > 0 and rel_l2(img[l], rimg) < 1e-5 and rel_l2(d[0, l], rd[0]) < 1e-5, (l, rel_l2(d[0, l], rd[0]))

    sc2, P = load_scene("cbox_occluder", res=24, spp=8, sppe=8, sppse=16, translate=(1, (1.0, 0.5, 0.0)))
    tb2 = sc2.tables(0)
    pos2 = OCCLUDER_LIGHTS
    L = len(pos2)
    tan = tangents_wrt(tb2, P)
    o2, po2 = stack_opts(8, 8, 16, rng_offset=(3, 4, 5)), point_opts(8, 8, 16, rng_offset=(3, 4, 5))
    g2 = StackScene(tb2).set_lights(pos2)
    img, d = g2.stack_render_d_fwd(o2, [tan])
    ref_img, ref_d = host_stack_render(tb2, o2, pos2, mode=1, tangent_sets=[tan])
    for l in range(L):
        rimg, rd = g2.set_light(pos2[l]).render_d_fwd(po2, [tan])
        if not np.any(ref_d[0, l]):
            assert not np.any(d[0, l])
            continue
        print("forward, occluder translation, light %d: against the harness %.2e, against kind 4 %.2e" % (l, rel_l2(d[0, l], ref_d[0, l]), rel_l2(d[0, l], rd[0])))
        assert rel_l2(d[0, l], ref_d[0, l]) < 1e-3 and rel_l2(d[0, l], rd[0]) < 1e-5
    # one light's tangent
    dl = np.zeros((1, L, 3), np.float32)
    dl[0, 1] = (1.0, 0.5, 0.0)
    g2.set_lights(pos2, d_pos=dl)
    _, d_l = g2.stack_render_d_fwd(o2, [{}])
    _, ref_dl = host_stack_render(tb2, o2, pos2, mode=1, d_pos=dl)
    assert np.abs(ref_dl[0, 1]).max() > 0 and rel_l2(d_l[0, 1], ref_dl[0, 1]) < 1e-3, rel_l2(d_l[0, 1], ref_dl[0, 1])
    for l in range(L):
        assert l == 1 or not np.any(d_l[0, l]), l
    # K = 3: columns (occluder, the light, nothing)
    d3 = np.zeros((3, L, 3), np.float32)
    d3[1] = dl[0]
    g2.set_lights(pos2, d_pos=d3)
    _, dk = g2.stack_render_d_fwd(o2, [tan, {}, {}])
    assert rel_l2(dk[0], d[0]) < 1e-5 and rel_l2(dk[1], d_l[0]) < 1e-5 and not np.any(dk[2]), (rel_l2(dk[0], d[0]), rel_l2(dk[1], d_l[0]))


@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_rough", "bunny_light"])
def test_reverse_mode(name):
    """<A, J t> = <J^T A, t> per table and for the lights' positions with a random adjoint stack and all three terms on (1e-4 of the scale, test_pointlight_gpu's
    bound); the tables and g_pos against the sum of kind-4 reverse launches over the lights with A_l (1e-4, 1e-3 on bunny_light: that test's bounds against its
    harness); an adjoint stack that is zero except plane l gives g_pos zero except row l."""
    res, spp, sppe, sppse = 16, 4, 4, 8
    sc, _ = load_scene(name, res=res, spp=spp, sppe=sppe, sppse=sppse)
    tb = sc.tables(0)
    pos = lights_of(name, tb)
    L = len(pos)
    A = np.random.default_rng(5).random((L, res * res, 3)).astype(np.float32)
    A64 = A.astype(np.float64)
    o, po = stack_opts(spp, sppe, sppse, rng_offset=(2, 3, 4)), point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    tol = 1e-3 if name == "bunny_light" else 1e-4
    names = ["tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge"]
    g = StackScene(tb).set_lights(pos, want_grad=True)
    img_r, grads = g.stack_render_d_rev(o, A, want=names)
    g_pos = g.lights_grad()
    assert np.isfinite(img_r).all()
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = g.set_lights(pos).stack_render_d_fwd(o, [tan])
        assert rel_l2(img_r, img) < 1e-5
        lhs, rhs, scale = float((A64 * dimg[0]).sum()), dot_tables(grads, tan), float(np.abs(A64 * dimg[0]).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
    dl = (np.random.default_rng(6).random((1, L, 3)) - 0.5).astype(np.float32)
    _, dimg = g.set_lights(pos, d_pos=dl).stack_render_d_fwd(o, [{}])
    for l in range(L):          # per light: row l of g_pos against plane l of the derivative
        lhs, rhs, scale = float((A64[l] * dimg[0, l]).sum()), float(g_pos[l].astype(np.float64) @ dl[0, l]), float(np.abs(A64[l] * dimg[0, l]).sum())
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (l, lhs, rhs, scale)
    # the sum of kind-4 reverse launches
    total = {n: np.zeros_like(grads[n], np.float64) for n in grads}
    for l in range(L):
        g.set_light(pos[l], want_grad=True)
        _, g1 = g.render_d_rev(po, A[l], want=names)
        gp1 = g.light_grad()
        for n in g1:
            total[n] += g1[n]
        if np.any(gp1):
            assert rel_l2(g_pos[l], gp1) < tol, (l, g_pos[l], gp1)
        else:
            assert not np.any(g_pos[l])
    for n in total:
        print("%s %s: stack against the sum of kind-4 launches %.2e" % (name, n, rel_l2(grads[n], total[n])))
        assert np.abs(total[n]).max() > 0 and rel_l2(grads[n], total[n]) < tol, (n, rel_l2(grads[n], total[n]))
    # one plane of adjoint
    one = np.zeros_like(A)
    one[1] = A[1]
    g.set_lights(pos, want_grad=True)
    g.stack_render_d_rev(o, one, want=[], with_image=False)
    gp = g.lights_grad()
    assert np.any(gp[1]) and not np.any(np.delete(gp, 1, axis=0)), gp


def test_edge_terms_alone_are_the_kind_4_launches():
    """an empty spp range: only the PointLightIntegrator's edge kernels run, once per light with the light's planes -- bit for bit the kind-4 launch's.
    k_point_edge / k_point_sedge add one float per run of equal pixels with atomics, so a launch of several waves is not reproducible to the bit: a pixel that
    receives more than two adds sums them in the order the waves arrive (measured at 16 x 16, sppe 4, sppse 16: two kind-4 launches of one light differ in 3 to
    34 of 768 floats by up to 2.2e-7 of the plane's maximum -- test_edge_terms_alone_within_the_atomics_order).  Bit for bit is therefore asked where the
    reference reproduces itself: 8 x 8 with one sppe / sppse slot per pixel in the shard, 64 slots = ONE wave per launch, whose adds to a pixel come from one
    instruction stream in its order; four such shards of sppe = sppse = 4, six lights.  The test checks that premise too (kind 4 against a second kind-4
    launch), so that a reference that does not reproduce is reported as that.  What can differ between the two kinds here is all host side: the plane pointer
    and stride, the light handed over by value, the shard and the rng offsets."""
    S = 4
    sc, P = load_scene("cbox_occluder", res=8, spp=1, sppe=S, sppse=S, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    pos = OCCLUDER_LIGHTS
    g = StackScene(tb).set_lights(pos)
    nonzero = 0
    for i in range(S):
        kw = dict(rng_offset=(0, 8, 9), spp_range=(0, 0), sppe_range=(i, i + 1), sppse_range=(i, i + 1))
        img, d = g.stack_render_d_fwd(stack_opts(1, S, S, **kw), [tan])
        assert not np.any(img)
        for l, p in enumerate(pos):
            ref = g.set_light(p).render_d_fwd(point_opts(1, S, S, **kw), [tan])[1][0]
            again = g.render_d_fwd(point_opts(1, S, S, **kw), [tan])[1][0]
            assert np.array_equal(again, ref), ("kind 4 does not reproduce itself", i, l)
            assert np.array_equal(d[0, l], ref), (i, l)
            nonzero += int(np.count_nonzero(ref))
    assert nonzero > 50, nonzero          # (measured: 180 floats of the 24 reference planes)


def test_edge_terms_alone_within_the_atomics_order():
    """the edge terms alone in launches of several waves (16 x 16, sppe 4, sppse 16), where the order of the float atomics differs from launch to launch: the
    stack's planes against the kind-4 launches at the project's bound for two evaluations of one expression, 4 eps32 of the plane's maximum per pixel.
    Measured: the stack against kind 4 up to 1.8e-7 of the maximum (1.5 eps32), kind 4 against a second kind-4 launch up to 2.2e-7."""
    sc, P = load_scene("cbox_occluder", res=16, spp=4, sppe=4, sppse=16, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    pos = OCCLUDER_LIGHTS
    kw = dict(rng_offset=(0, 8, 9), spp_range=(0, 0))
    g = StackScene(tb).set_lights(pos)
    img, d = g.stack_render_d_fwd(stack_opts(4, 4, 16, **kw), [tan])
    assert not np.any(img)
    refs = [g.set_light(p).render_d_fwd(point_opts(4, 4, 16, **kw), [tan])[1][0] for p in pos]
    assert any(np.any(r) for r in refs)
    for l in range(len(pos)):
        print("edge terms alone, light %d: |stack plane - kind 4| / (eps32 * max) = %.2f" % (l, _planes_match(d[0, l], refs[l], l)))


def test_shards_sum_to_the_full_launch():
    """spp / sppe / sppse shards of psdr_render_d_fwd sum to the unsharded launch: 1e-6"""
    sc, P = load_scene("cbox_occluder", res=16, spp=6, sppe=4, sppse=8, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    g = StackScene(tb).set_lights(OCCLUDER_LIGHTS[:3])
    full_img, full_d = g.stack_render_d_fwd(stack_opts(6, 4, 8, rng_offset=(1, 2, 3)), [tan])
    img, d = np.zeros_like(full_img, np.float64), np.zeros_like(full_d[0], np.float64)
    for a, b, c in (((0, 2), (0, 1), (0, 3)), ((2, 6), (1, 4), (3, 8))):
        i, dd = g.stack_render_d_fwd(stack_opts(6, 4, 8, rng_offset=(1, 2, 3), spp_range=a, sppe_range=b, sppse_range=c), [tan])
        img += i
        d += dd[0]
    assert rel_l2(img, full_img) < 1e-6 and rel_l2(d, full_d[0]) < 1e-6, (rel_l2(img, full_img), rel_l2(d, full_d[0]))


def test_error_returns_and_both_kinds_on_one_handle():
    """kind 5 without lights, L outside 1..256, a position that is not finite, K not 1 or 3 in forward mode: each an error before any launch, with its own message.
    Kind 4 works on a handle that holds a stack and kind 5 on one that holds a light; removing one leaves the other."""
    sc, _ = load_scene("cbox", res=8, spp=1)
    tb = sc.tables(0)
    g = StackScene(tb)
    g.L = 1
    o, po = stack_opts(1), point_opts(1)
    adj = np.ones((1, 64, 3), np.float32)
    for call in (lambda: g.stack_render_c(o), lambda: g.stack_render_d_fwd(o, [{}]), lambda: g.stack_render_d_rev(o, adj, want=["texels"])):
        with pytest.raises(RuntimeError, match="no lights set"):
            call()
    for L in (-1, 257):
        with pytest.raises(RuntimeError, match="L must be 1..256"):
            g.set_lights(np.zeros((257, 3), np.float32), L=L)
    with pytest.raises(RuntimeError, match="not finite"):
        g.set_lights([(0.0, 1.0, 2.0), (0.0, float("inf"), 0.0)])
    with pytest.raises(RuntimeError, match="K must be 0..3"):
        g.set_lights(np.zeros((2, 3), np.float32), d_pos=np.zeros((4, 2, 3), np.float32))
    pos = lights_of("cbox", tb)
    g.set_lights(pos)
    with pytest.raises(RuntimeError, match="K must be 1 or 3"):
        g.stack_render_d_fwd(o, [{}, {}])
    with pytest.raises(RuntimeError, match="no light set"):          # a stack is not kind 4's light
        g.render_c(po)
    stack = g.stack_render_c(o)
    single = g.set_light(pos[1]).render_c(po)
    _planes_match(stack[1], single, "kind 4 beside a stack")
    assert np.array_equal(g.stack_render_c(o), stack)                # ... and kind 4's light is not the stack's
    g.set_lights(None)                                               # the stack removed: kind 4 keeps its light
    g.L = 1
    with pytest.raises(RuntimeError, match="no lights set"):
        g.stack_render_c(o)
    assert np.array_equal(g.render_c(po), single)


# ---------------------------------------------------------------- the Python surface
def _surface_scene(res=16, spp=4, sppe=4, sppse=8):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_occluder"), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    return sc


@pytest.mark.parametrize("combine", [False, True])
def test_python_surface_matches_the_c_abi(combine):
    """LightStageIntegrator.renderC / renderD against the C ABI on the same tables and RNG offsets, stacked and combined; enoki.forward through one light's
    position; enoki.backward to the intensities and the positions against the C ABI's reverse launch."""
    pos = OCCLUDER_LIGHTS[[0, 1, 5]]
    inten = np.array([(2.0, 1.0, 0.5), (0.3, 0.6, 0.9), (1.5, 1.5, 0.2)], np.float32)
    L, n = 3, 16 * 16
    sc = _surface_scene()
    sc.configure()
    integ = psdr_cuda.LightStageIntegrator(pos, inten, combine=combine)
    tb = sc.tables(0)
    g = StackScene(tb).set_lights(pos)

    def shaped(stack):          # [L, n, 3] unit planes -> what the integrator returns
        s = stack * inten[:, None, :]
        return s.sum(axis=0) if combine else s.reshape(-1, 3)
    ref = shaped(g.stack_render_c(stack_opts(4, rng_offset=tuple(sc._rng_offset))))
    img = integ.renderC(sc).numpy()
    assert img.shape == ((n, 3) if combine else (L * n, 3)) and rel_l2(img, ref) < 1e-6, rel_l2(img, ref)
    # forward mode through the position of light 1
    P = FloatD(0.)
    ek.set_requires_gradient(P)
    dl = np.zeros((1, L, 3), np.float32)
    dl[0, 1] = (1.0, 0.5, 0.0)
    integ.m_positions = Vector3fD(torch.from_numpy(pos.copy())) + Vector3fD(torch.from_numpy(dl[0].copy())) * P
    off = tuple(sc._rng_offset)
    imgd = integ.renderD(sc)
    ek.forward(P)
    d = ek.gradient(imgd).numpy()
    ref_img, ref_d = g.set_lights(pos, d_pos=dl).stack_render_d_fwd(stack_opts(4, 4, 8, rng_offset=off), [{}])
    assert rel_l2(imgd.numpy(), shaped(ref_img)) < 1e-6 and np.abs(ref_d).max() > 0
    assert rel_l2(d, shaped(ref_d[0])) < 1e-5, rel_l2(d, shaped(ref_d[0]))
    # reverse mode: d loss / d positions and d loss / d intensities
    integ2 = psdr_cuda.LightStageIntegrator(pos, inten, combine=combine)
    ek.set_requires_gradient(integ2.m_positions)
    ek.set_requires_gradient(integ2.m_intensities)
    off = tuple(sc._rng_offset)
    imgd = integ2.renderD(sc)
    w = np.random.default_rng(3).random(imgd.t.shape).astype(np.float32)
    ek.backward(FloatD._wrap((imgd.t * torch.as_tensor(w, device=imgd.t.device)).sum().reshape(1)))
    gp, gi = ek.gradient(integ2.m_positions).numpy().reshape(L, 3), ek.gradient(integ2.m_intensities).numpy().reshape(L, 3)
    wl = np.broadcast_to(w[None], (L, n, 3)) if combine else w.reshape(L, n, 3)
    g.set_lights(pos, want_grad=True)
    unit, _ = g.stack_render_d_rev(stack_opts(4, 4, 8, rng_offset=off), (wl * inten[:, None, :]).astype(np.float32), want=[])
    ref_gp, ref_gi = g.lights_grad(), (unit.astype(np.float64) * wl).sum(axis=1)
    print("python surface (combine=%s): g_pos %s ref %s" % (combine, gp.ravel(), ref_gp.ravel()))
    assert np.abs(ref_gp).max() > 0 and rel_l2(gp, ref_gp) < 1e-5 and rel_l2(gi, ref_gi) < 1e-5, (rel_l2(gp, ref_gp), rel_l2(gi, ref_gi))


def test_recover_albedo_and_normal_maps_under_one_stack():
    """tests/test_pointlight_gpu.py's three-lamp recovery with the lamps as ONE LightStageIntegrator (their planes are the separate photographs): the same quad,
    maps, targets at 64 spp, 40 Adam steps of the same length, and that test's own thresholds: the mean kd texel error and the mean angular error of the normals
    both end below half of their start."""
    from colloc_microfacet_helpers import RECOVERY
    from test_pointlight_gpu import RECOVERY_LAMPS
    R = RECOVERY["normal"]

    def view(spp, kd, nm):
        def maps(sc):
            b = sc.m_bsdfs[0]
            b.diffuse_reflectance.resolution = b.normal_map.resolution = (4, 4)
            b.diffuse_reflectance.data, b.normal_map.data = kd, nm
        return mf_scene(R.xml((0.0, 0.0)), 32, spp, 0, extra=maps)
    kd_true, n_true = R.truth()
    integ = psdr_cuda.LightStageIntegrator(np.asarray(RECOVERY_LAMPS, np.float32), R.intensity)
    target = integ.renderC(view(64, Vector3fD(torch.from_numpy(kd_true)), Vector3fD(torch.from_numpy(n_true)))).torch().clone()
    kd0, nm0 = R.start()
    kd, nm = Vector3fD(torch.from_numpy(kd0)), Vector3fD(torch.from_numpy(nm0))
    ek.set_requires_gradient(kd)
    ek.set_requires_gradient(nm)
    sc = view(4, kd, nm)
    start = R.errors(kd.numpy(), nm.numpy())
    opt = torch.optim.Adam([kd.t, nm.t], lr=R.lr)
    for it in range(R.steps):
        opt.zero_grad()
        sc.configure()
        img = integ.renderD(sc)
        # (the three single-light losses are means over W H pixels each: their sum is three times the mean over the stack's 3 W H rows)
        ek.backward(ek.hmean(ek.hsum(ek.sqr(img - Vector3fD._wrap(target)))) * 3.0)
        opt.step()
        kd.t.data.clamp_(0.01, 0.99)
        nm.t.data.clamp_(0.0, 1.0)
    end = R.errors(kd.numpy(), nm.numpy())
    print("one-stack recovery: mean kd texel error %.4f -> %.4f, mean angular error of the normals %.2f -> %.2f degrees" % (start[0], end[0], start[1], end[1]))
    assert end[0] < 0.5 * start[0] and end[1] < 0.5 * start[1], (start, end)
