"""HyperCubeDistribution{2,3}f.sample_reuse and Scene.sample_boundary_segment_direct on the GPU (csrc/psdr_hip.hip k_cube_sample_reuse,
k_boundary_segment_direct): against the CPU oracle's sample_reuse, the torch mirror, psdr_oracle_debug_secondary and fp64 recomputations."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import enoki as ek
import oracle
import psdr_cuda
from enoki.cuda import Vector2f as Vector2fC, Vector3f as Vector3fC
from psdr_cuda import _abi
from psdr_cuda.scene import make_desc

from helpers import load_scene

pytestmark = pytest.mark.gpu

EPS = EDGE_EPS = 1e-5            # include/psdr/constants.h Epsilon, EdgeEpsilon
NEAR = 1e-5                      # a validity flip is allowed only where a deciding quantity is this close to its threshold


# ------------------------------------------------------------------------------------------------------------------- cube sampler
def _grid(reso, seed):
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(reso))
    # small whole numbers: every prefix sum is exact in fp32, so a zero-mass cell has the cmf of its predecessor in whatever order the device scan
    # adds (with random fractions a parallel scan can leave such a cell a sliver of cmf, and the search then stops on it -- in the reference too)
    mass = torch.randint(1, 16, (n,), generator=g).float()
    mass[torch.rand(n, generator=g) < 0.25] = 0.0
    mass[-1] = 8.0          # u * sum can round above the last cmf entry: the search then keeps the last cell
    cls = psdr_cuda.HyperCubeDistribution2f if len(reso) == 2 else psdr_cuda.HyperCubeDistribution3f
    d = cls()
    d.set_resolution(reso)
    d.set_mass(mass.cuda())
    return d, mass.numpy().astype(np.float32)


def _uniform(m, ndim, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(m, ndim, generator=g).clamp(min=2.0 ** -24)      # u = 0 may stop on a leading zero-mass cell (the reference does the same)


def _oracle_compose(d, s):
    """HyperCubeDistribution::sample_reuse composed in numpy over psdr_oracle_sample_reuse, sample by sample."""
    L = oracle.lib()
    cmf = d.m_distrb.m_cmf.cpu().numpy().astype(np.float32)
    pmf = d.m_distrb.m_pmf.cpu().numpy().astype(np.float32)
    reso, n = d.m_resolution, d.m_num_cells
    out = s.astype(np.float32).copy()
    idx = np.zeros(len(s), np.int64)
    pdf = np.zeros(len(s), np.float32)
    u, p = C.c_float(), C.c_float()
    for i in range(len(s)):
        u.value = float(s[i, -1])
        idx[i] = L.psdr_oracle_sample_reuse(cmf.ctypes.data, pmf.ctypes.data, float(d.m_distrb.m_sum), n, C.byref(u), C.byref(p))
        out[i, -1] = u.value
        pdf[i] = np.float32(p.value) * np.float32(n)
    rem = idx.copy()
    for k in range(len(reso) - 1, -1, -1):
        c = rem % reso[k]
        rem //= reso[k]
        out[:, k] = (out[:, k] + c.astype(np.float32)) * np.float32(1.0 / reso[k])
    return out, idx, pdf


def _cells_of(w, reso):
    idx = np.zeros(len(w), np.int64)
    for k, r in enumerate(reso):
        idx = idx * r + np.clip(np.floor(w[:, k].astype(np.float64) * r), 0, r - 1).astype(np.int64)
    return idx


def _on_face(w, reso, ulps=4):
    """samples within a few float32 ulp of a cell face: the cell they fall in is a matter of rounding (u clamped to 1 lands exactly on one)"""
    w = np.asarray(w, dtype=np.float32)
    x = w.astype(np.float64) * np.asarray(reso, dtype=np.float64)
    tol = ulps * np.spacing(np.maximum(np.abs(w), np.float32(2.0 ** -24))).astype(np.float64) * np.asarray(reso, dtype=np.float64)
    return np.any(np.abs(x - np.round(x)) <= tol, axis=1)


@pytest.mark.parametrize("reso", [(7, 5), (40, 5, 5), (1024, 1024), (128, 128, 64)])
def test_cube_sample_reuse_matches_the_oracle(reso):
    d, mass = _grid(reso, 1)
    s = _uniform(4096, len(reso), 2)
    w = s.cuda()
    pdf = d.sample_reuse(Vector2fC._wrap(w) if len(reso) == 2 else Vector3fC._wrap(w)).t.cpu().numpy()
    w = w.cpu().numpy()
    want, idx, want_pdf = _oracle_compose(d, s.numpy())
    # warped samples to 2 ulp (the kernel divides with v_rcp_f32), pdf to 1e-6
    ulp = np.spacing(np.maximum(np.abs(w), np.abs(want)).astype(np.float32))
    assert np.all(np.abs(w - want) <= 2 * ulp)
    np.testing.assert_allclose(pdf, want_pdf, rtol=1e-6)
    # the cell of every sample is the oracle's, and it has mass
    got_idx = _cells_of(w, reso)
    face = _on_face(w, reso)
    # (on a million cells u * sum has an ulp of a few hundredths of a cell's mass: the reused coordinate comes in coarse steps, 0 among
    #  them -- a few per cent of the samples sit exactly on a face, in the reference as here)
    assert np.all((got_idx == idx) | face) and face.mean() < 0.05
    assert np.all(mass[idx] > 0)
    # pdf(warped) is the pdf returned, except on a cell face
    back = d.pdf(Vector2fC._wrap(torch.as_tensor(w).cuda()) if len(reso) == 2 else Vector3fC._wrap(torch.as_tensor(w).cuda())).t.cpu().numpy()
    ok = np.isclose(back, pdf, rtol=1e-6)
    assert np.all(ok | face)


def _chi2_crit(k, z=4.26):
    """Wilson-Hilferty: the chi-square quantile with k degrees of freedom at the normal quantile z (4.26: p = 1e-5)"""
    return k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3


@pytest.mark.parametrize("reso", [(7, 5), (40, 5, 5)])
def test_cube_sample_reuse_chi_square(reso):
    d, mass = _grid(reso, 3)
    m = 1 << 22
    w = torch.rand(m, len(reso), generator=torch.Generator().manual_seed(4)).clamp(min=2.0 ** -24).cuda()
    d.sample_reuse(Vector2fC._wrap(w) if len(reso) == 2 else Vector3fC._wrap(w))
    # a histogram twice as fine as the grid along every axis: the cell probabilities AND the uniform warp inside a cell
    fine = tuple(2 * r for r in reso)
    w = w.cpu().numpy()
    face = _on_face(w, fine)
    assert face.mean() < 1e-3
    w = w[~face].astype(np.float64)          # (a sample on a face belongs to either cell)
    m = len(w)
    h = np.bincount(_cells_of(w, fine), minlength=int(np.prod(fine))).astype(np.float64)
    p = (mass.astype(np.float64) / mass.astype(np.float64).sum()).reshape(reso)
    for k in range(len(reso)):
        p = np.repeat(p, 2, axis=k)
    p = p.reshape(-1) / 2 ** len(reso)
    assert h[p == 0].sum() == 0
    e = p[p > 0] * m
    chi2 = float(((h[p > 0] - e) ** 2 / e).sum())
    assert chi2 < _chi2_crit(len(e) - 1), (chi2, len(e))


def test_cube_sample_reuse_in_place_and_shortcuts():
    d, _ = _grid((7, 5), 5)
    v = Vector2fC._wrap(_uniform(1000, 2, 6).cuda())
    t0, before = v.t, v.t.clone()
    pdf = d.sample_reuse(v)
    assert isinstance(pdf, psdr_cuda.core.FloatC) and pdf.t.shape == (1000,) and pdf.t.is_cuda
    assert v.t is t0 and not torch.equal(v.t, before)                     # the caller's array, warped in place
    # a non-contiguous / float64 device tensor: computed, then copied back into it
    x = before.double().t().contiguous().t()
    assert not x.is_contiguous()
    pdf2 = d.sample_reuse(x)
    assert torch.equal(x.float(), v.t) and torch.equal(pdf2.t, pdf.t)
    # before set_mass: RuntimeError (psdr_assert(m_ready))
    e = psdr_cuda.HyperCubeDistribution3f()
    e.set_resolution((2, 2, 2))
    with pytest.raises(RuntimeError):
        e.sample_reuse(torch.rand(8, 3, device="cuda"))
    # a one-cell grid: pdf 1, the samples as they were
    one = psdr_cuda.HyperCubeDistribution3f()
    one.set_resolution((1, 1, 1))
    one.set_mass(torch.tensor([2.0], device="cuda"))
    s = torch.rand(64, 3, device="cuda")
    s0 = s.clone()
    assert torch.equal(one.sample_reuse(s).t, torch.ones(64, device="cuda")) and torch.equal(s, s0)
    # an all-zero mass: pdf 0, every sample in cell 0
    z = psdr_cuda.HyperCubeDistribution2f()
    z.set_resolution((4, 4))
    z.set_mass(torch.zeros(16, device="cuda"))
    s = torch.rand(64, 2, device="cuda")
    assert torch.equal(z.sample_reuse(s).t, torch.zeros(64, device="cuda")) and bool((s < 0.25).all())


def test_cube_sample_reuse_c_abi_one_cell():
    """psdr_cube_sample_reuse keeps DiscreteDistribution's size-1 shortcut whatever the mass: pdf 1, samples unchanged"""
    lib = _abi.load_hip()
    for ndim, total in ((2, 0.0), (3, 0.0), (3, 2.5)):
        reso = (C.c_int32 * ndim)(*([1] * ndim))
        cmf = torch.tensor([total], device="cuda")
        s = torch.rand(256, ndim, device="cuda")
        s0 = s.clone()
        pdf = torch.full((256,), -1.0, device="cuda")
        _abi.check(lib, lib.psdr_cube_sample_reuse(ndim, reso, cmf.data_ptr(), cmf.data_ptr(), total, 1, 256, s.data_ptr(), pdf.data_ptr(),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        assert torch.equal(pdf, torch.ones(256, device="cuda")) and torch.equal(s, s0)


def test_cube_sample_reuse_on_the_guiding_grid():
    sc, _ = load_scene("cbox_bunny", res=16, spp=1, sppse=64)
    integ = psdr_cuda.DirectIntegrator()
    grid = integ.preprocess_secondary_edges(sc, 0, [16, 4, 4, 4], 1)
    assert isinstance(grid, psdr_cuda.HyperCubeDistribution3f)
    s = Vector3fC._wrap(_uniform(4096, 3, 7).cuda())
    pdf = grid.sample_reuse(s).t
    assert bool((pdf > 0).all()) and bool(((s.t >= 0) & (s.t <= 1)).all())
    back = grid.pdf(s).t
    w = s.t.cpu().numpy()
    ok = np.isclose(back.cpu().numpy(), pdf.cpu().numpy(), rtol=1e-6)
    assert np.all(ok | _on_face(w, grid.m_resolution))


# ------------------------------------------------------------------------------------------------------------ boundary segments
def _deciding(sc, k, p0, p2, n2):
    """fp64 cosTheta and the two sign-test dot products of scene.cpp:475-483 from the returned points and the drawn rows"""
    rows = sc.tables(0, capacity=True)["sec_edge"].detach().double().cpu().numpy()[k]
    e = p2.astype(np.float64) - p0.astype(np.float64)
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    cos = -(n2.astype(np.float64) * e).sum(1)
    d0, d1 = (rows[:, 6:9] * e).sum(1), (rows[:, 9:12] * e).sum(1)
    near = (np.abs(cos - EPS) < NEAR) | (np.abs(np.abs(d0) - EDGE_EPS) < NEAR) | ((rows[:, 15] == 0) & (np.abs(np.abs(d1) - EDGE_EPS) < NEAR))
    return rows, cos, near


@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_bunny"])
def test_boundary_segment_native_matches_the_torch_mirror(name):
    sc, _ = load_scene(name, res=16, spp=1, sppse=1)
    assert len(sc.m_emitters) == 1
    s3 = torch.rand(1 << 16, 3, generator=torch.Generator().manual_seed(11)).cuda()
    a = sc.sample_boundary_segment_direct(Vector3fC._wrap(s3))
    b = sc._sample_boundary_segment_direct_torch(Vector3fC._wrap(s3))
    k = a._edge_index.cpu().numpy()
    tb = sc.tables(0, capacity=True)
    x = s3[:, 0] * tb["sec_sum"]
    kb = torch.searchsorted(tb["sec_cmf"], x.contiguous(), right=False).clamp(max=tb["num_sec_edges"] - 1).cpu().numpy()
    assert np.array_equal(k, kb)                                               # the same edge rows
    # unit vectors to 1e-5; points to 1e-5 of the scene's extent (a coordinate near 0 keeps the rounding of the terms that cancelled in it)
    scale = float(tb["sec_edge"][:, 0:3].detach().abs().max())
    for f in ("edge", "n"):
        np.testing.assert_allclose(getattr(a, f).numpy(), getattr(b, f).numpy(), rtol=1e-5, atol=1e-5, err_msg=f)
    for f in ("p0", "edge2", "p2"):
        np.testing.assert_allclose(getattr(a, f).numpy(), getattr(b, f).numpy(), rtol=1e-5, atol=1e-5 * scale, err_msg=f)
    va, vb = a.is_valid.cpu().numpy(), b.is_valid.cpu().numpy()
    _, _, near = _deciding(sc, k, a.p0.numpy(), a.p2.numpy(), a.n.numpy())
    flip = va != vb
    assert np.all(near[flip]) and flip.mean() < 1e-3, (flip.sum(), near[flip].sum())
    both = va & vb
    assert both.sum() > 100
    # pdf to 1e-5; where the segment grazes the emitter the factor d^2 / cosTheta carries a few fp32 ulp of the direction as 1e-7 / cosTheta
    rel = np.abs(a.pdf.numpy()[both].astype(np.float64) - b.pdf.numpy()[both]) / b.pdf.numpy()[both]
    _, cos, _ = _deciding(sc, k, a.p0.numpy(), a.p2.numpy(), a.n.numpy())
    assert np.mean(rel <= 1e-5) > 0.999 and np.all(rel <= 1e-5 + 1e-6 / cos[both]), np.sort(rel)[-5:]
    assert np.all(a.pdf.numpy()[~va] == 0)


def _point_on_emitters(tb, p):
    """per point: the emitter index whose triangle holds it (fp64 barycentrics, distance < 1e-4 of the scene scale), -1 for none"""
    rows = tb["tri_info"].detach().double().cpu().numpy()
    ei = tb["emitter_i"].cpu().numpy().reshape(-1, 4)
    env = int(tb.get("env_emitter", -1))
    scale = max(1.0, float(np.abs(rows[:, 0:3]).max()))
    out = np.full(len(p), -1)
    p = p.astype(np.float64)
    for e in range(len(ei)):
        if e == env:
            continue
        for t in range(ei[e, 1], ei[e, 1] + ei[e, 2]):
            p0, e1, e2 = rows[t, 0:3], rows[t, 3:6], rows[t, 6:9]
            A = np.stack([e1, e2], 1)
            uv, *_ = np.linalg.lstsq(A, (p - p0).T, rcond=None)
            dist = np.linalg.norm(p - p0 - (A @ uv).T, axis=1)
            inside = (uv[0] >= -1e-4) & (uv[1] >= -1e-4) & (uv.sum(0) <= 1 + 1e-4) & (dist < 1e-4 * scale)
            out[inside & (out < 0)] = e
    return out


def _env_pdf64(tb, p0, p2, n2):
    """EnvironmentMap::__sample_position_pdf (envmap.cpp:124-143) in fp64, without the emitter pick"""
    f = tb["env_f"].detach().double().cpu().numpy()
    fw = f[0:9].reshape(3, 3)
    d = p2 - p0
    dist2 = (d * d).sum(1)
    d = d / np.sqrt(dist2)[:, None]
    Gv = np.abs((d * n2).sum(1)) / dist2
    dl = d @ fw.T
    factor = Gv / np.sqrt(np.maximum(dl[:, 0] ** 2 + dl[:, 2] ** 2, 1e-10)) * (0.5 / (math.pi ** 2))
    u = np.arctan2(dl[:, 0], -dl[:, 2]) / (2 * math.pi)
    v = np.arccos(np.clip(dl[:, 1], -1, 1)) / math.pi
    u -= np.floor(u); v -= np.floor(v)
    r0, r1 = int(tb["env_reso"][0]), int(tb["env_reso"][1])
    pmf = tb["env_pmf"].detach().double().cpu().numpy()
    i0, i1 = np.clip(np.floor(u * r0).astype(int), 0, r0 - 1), np.clip(np.floor(v * r1).astype(int), 0, r1 - 1)
    return pmf[i0 * r1 + i1] / float(tb["env_sum"]) * (r0 * r1) * factor


def _debug_secondary(tb, opts, n):
    L = oracle.lib()
    L.psdr_oracle_debug_secondary.argtypes = [C.POINTER(_abi.SceneDesc), C.POINTER(_abi.RenderOpts), C.c_void_p, C.c_int64] + [C.c_void_p] * 6
    L.psdr_oracle_debug_secondary.restype = C.c_int
    desc, keep = make_desc(oracle._cpu_tables(tb), None, device="cpu")
    st32, st64, px32, px64 = (np.zeros(n, np.int32) for _ in range(4))
    v32, v64 = np.zeros(n), np.zeros(n)
    assert L.psdr_oracle_debug_secondary(C.byref(desc), C.byref(opts), None, n, st32.ctypes.data, st64.ctypes.data, px32.ctypes.data,
                                         px64.ctypes.data, v32.ctypes.data, v64.ctypes.data) == 0
    return st32


@pytest.mark.parametrize("name", ["cbox_bunny_two_lights", "cbox_env", "bunny_env"])
def test_boundary_segment_every_emitter_kind(name):
    sc, _ = load_scene(name, res=16, spp=1, sppse=1)
    n = 1 << 16
    opts = _abi.make_opts(sppse=n, rng_offset=(0, 0, 5))
    s3 = np.stack([oracle.rng(i, opts.rng_offset[2], 3) for i in range(n)])
    r = sc.sample_boundary_segment_direct(Vector3fC._wrap(torch.as_tensor(s3).cuda()))
    valid = r.is_valid.cpu().numpy()
    k = r._edge_index.cpu().numpy()
    p0, p2, n2, pdf = (x.numpy().astype(np.float64) for x in (r.p0, r.p2, r.n, r.pdf))
    # the validity of the renderer's draw: psdr_oracle_debug_secondary's stage 1 is the sampling test of scene.cpp:475-483
    st32 = _debug_secondary(sc.tables(0), opts, n)
    rows, cos, near = _deciding(sc, k, p0, p2, n2)
    flip = valid != (st32 != 1)
    assert flip.mean() <= 1e-3 and np.all(near[flip]), (flip.sum(), near[flip].sum())
    if name == "cbox_env":
        # inside the closed box (nearly) every environment sample fails the test, in the oracle as well: the agreement above is the check
        return
    assert valid.sum() > 100
    # pdf: an fp64 recomputation from the returned rows and points
    tb = sc.tables(0, capacity=True)
    em = _point_on_emitters(tb, p2)
    env = int(tb.get("env_emitter", -1))
    ne = int(tb["num_emitters"])
    epmf = tb["emitter_pmf"].detach().double().cpu().numpy() / float(tb["emitter_sum"]) if ne > 1 else np.ones(1)
    ef = tb["emitter_f"].detach().double().cpu().numpy().reshape(ne, -1)
    sec_pmf = tb["sec_pmf"].detach().double().cpu().numpy()[k] / float(tb["sec_sum"])
    e1len = np.linalg.norm(rows[:, 3:6], axis=1)
    dist2 = ((p2 - p0) ** 2).sum(1)
    if env < 0:
        assert np.all(em[valid] >= 0)                                       # every valid p2 lies on an emitter triangle
    else:
        lo, hi = tb["env_f"][19:22].double().cpu().numpy(), tb["env_f"][22:25].double().cpu().numpy()
        on_box = np.any(np.isclose(p2, lo, rtol=1e-5, atol=1e-4) | np.isclose(p2, hi, rtol=1e-5, atol=1e-4), axis=1)
        assert np.all((em[valid] >= 0) | on_box[valid])                     # an area light's triangle, or the box the env directions end on
    area = valid & (em >= 0)
    pe = np.where(em >= 0, ef[np.maximum(em, 0), 4] * epmf[np.maximum(em, 0)] if ne > 1 else ef[np.maximum(em, 0), 4], 0.0)
    if env >= 0:
        envs = valid & (em < 0)
        pe = np.where(envs, _env_pdf64(tb, p0, p2, n2) * (epmf[env] if ne > 1 else 1.0), pe)
        area = area | envs
    want = sec_pmf / e1len * pe * dist2 / cos
    rel = np.abs(pdf[area] - want[area]) / np.abs(want[area])
    # (as in the mirror test: 1e-7 / cosTheta where the segment grazes the emitter; an env sample within an ulp of a cell face may read the
    #  neighbouring cell's pmf)
    slack = 1e-6 / cos[area] + (em[area] < 0) * 1.0
    assert np.mean(rel <= 1e-5) > 0.999 and np.all(rel <= 1e-5 + slack), np.sort(rel)[-5:]
    assert np.all(pdf[~valid] == 0)


def test_boundary_segment_active_mask():
    sc, _ = load_scene("cbox_bunny_two_lights", res=16, spp=1, sppse=1)
    s3 = Vector3fC._wrap(torch.rand(4096, 3, generator=torch.Generator().manual_seed(12)).cuda())
    off = sc.sample_boundary_segment_direct(s3, False)
    assert not bool(off.is_valid.any()) and bool((off.pdf.t == 0).all())
    on = sc.sample_boundary_segment_direct(s3)
    mask = torch.arange(4096, device="cuda") % 2 == 0
    half = sc.sample_boundary_segment_direct(s3, mask)
    assert torch.equal(half.is_valid, on.is_valid & mask)
    assert torch.equal(half.pdf.t, torch.where(mask, on.pdf.t, torch.zeros_like(on.pdf.t)))
    assert torch.equal(half.p0.t.detach(), on.p0.t.detach())


def _moved_mesh_setup(d):
    probe, _ = load_scene("cbox_bunny", res=16, spp=1, sppse=1)
    mid = max(range(len(probe.m_meshes)), key=lambda i: probe.m_meshes[i].num_vertices)
    sc, P = load_scene("cbox_bunny", res=16, spp=1, sppse=1, translate=(mid, d))
    return sc, P, mid


def _edge_mesh(sc, k):
    tb = sc.tables(0, capacity=True)
    f0 = tb["sec_edge_faces"][k.long(), 0].long()
    return tb["tri_mesh"][f0] & ~0x40000000          # PSDR_TRI_FACE_NORMALS


def test_boundary_segment_p0_forward_mode():
    d = (0.3, -1.0, 2.0)
    sc, P, mid = _moved_mesh_setup(d)
    s3 = torch.rand(1 << 15, 3, generator=torch.Generator().manual_seed(13)).cuda()
    r = sc.sample_boundary_segment_direct(Vector3fC._wrap(s3))
    moved = (_edge_mesh(sc, r._edge_index) == mid)
    valid = r.is_valid
    assert int((moved & valid).sum()) > 10 and int((~moved & valid).sum()) > 10
    want = torch.tensor(d, device="cuda").expand(len(s3), 3)
    ek.forward(P)
    g = ek.gradient(r.p0).t
    assert torch.allclose(g[moved], want[moved], rtol=0, atol=1e-6)
    assert bool((g[~moved] == 0).all())
    # forward again while the record lives: the first call freed its graph, so zeros -- and no exception
    ek.forward(P)
    g2 = ek.gradient(r.p0).t
    assert g2.shape == g.shape and int(torch.count_nonzero(g2)) == 0


def test_boundary_segment_p0_reverse_mode():
    d = (0.3, -1.0, 2.0)
    sc, P, mid = _moved_mesh_setup(d)
    s3 = torch.rand(1 << 15, 3, generator=torch.Generator().manual_seed(14)).cuda()
    r = sc.sample_boundary_segment_direct(Vector3fC._wrap(s3))
    w = torch.rand(1 << 15, 3, generator=torch.Generator().manual_seed(15)).cuda() * r.is_valid.unsqueeze(-1)
    loss = psdr_cuda.core.FloatD._wrap((w * r.p0.t).sum().reshape(1))
    ek.backward(loss)
    moved = (_edge_mesh(sc, r._edge_index) == mid)
    want = float((w[moved].double() * torch.tensor(d, device="cuda", dtype=torch.float64)).sum())
    got = float(ek.gradient(P).t.reshape(-1)[0])
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
