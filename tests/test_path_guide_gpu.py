"""Guiding grids of the PathTracer's secondary-edge term (csrc/psdr_path_sedge.hip) on the GPU: the two builds and the guided render
kernels through the C ABI against the host harness (same streams, same grids), against DirectIntegrator's guided term and build (depth 1) and against
themselves (one-cell grids, launch forms, shards, dropped grids), the error cases of psdr_path_guide_build, and the Python surface.
res 32, sppse 16, depth 3 unless stated: 16 384 slots."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from helpers import GpuScene, load_scene, rel_l2, same_rays, tangents_wrt
from path_guide_helpers import (gpu_path_guide_build, gpu_set_guides, gpu_set_path_guide, host_path_guide_fwd, host_path_guide_mass, host_path_guide_rev, make_grid,
                                one_cell_grid, synthetic_grid)
from path_sedge_helpers import path_opts, scenario_scene
from psdr_cuda import _abi

pytestmark = pytest.mark.gpu

TABLES = ["tri_info", "sec_edge", "cam_to_world"]
RES, SPPSE, DEPTH = 32, 16, 3
TOL = {"cbox_occluder": 1e-3, "cbox_bunny": 2e-2}          # test_gpu_parity's guiding tests / test_path_sedge_gpu.py on the tree scene
BUILD_RESO, BUILD_ROUNDS = [64, 4, 4, 2], 2


@functools.lru_cache(maxsize=None)
def _scene(name, res=RES, sppse=SPPSE):
    sc, P = load_scene(name, res=res, spp=0, sppe=0, sppse=sppse, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    return tb, tangents_wrt(tb, P), np.random.default_rng(4).random((res * res, 3)).astype(np.float32)


GA, GB = synthetic_grid(), synthetic_grid((4, 8, 2))          # positive everywhere, unlike anything built from a scene: every slot stays alive on both sides


@functools.lru_cache(maxsize=None)
def _host_mass(name, segment):
    return host_path_guide_mass(_scene(name)[0], path_opts(DEPTH, SPPSE), segment, BUILD_RESO, BUILD_ROUNDS)


@functools.lru_cache(maxsize=None)
def _host_render(name):
    tb, tan, adj = _scene(name)
    o = path_opts(DEPTH, SPPSE, (0, 0, 7))
    return host_path_guide_fwd(tb, o, tan, grid_a=GA, grid_b=GB), host_path_guide_rev(tb, o, adj, grid_a=GA, grid_b=GB, want=TABLES)


# ---------------------------------------------------------------- 1. / 2. the builds
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("segment", [1, 2])
@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_bunny"])
def test_mass_matches_host(name, segment, split):
    """psdr_path_guide_build against the host harness on the same streams: [64, 4, 4, 2] x 2 rounds, one kernel (sedge_split 0) and filter + survivors (1)"""
    ref = _host_mass(name, segment)
    g = GpuScene(_scene(name)[0], options={"sedge_split": split})
    mass = gpu_path_guide_build(g, path_opts(DEPTH, SPPSE), segment, BUILD_RESO, BUILD_ROUNDS)
    g.close()
    print(name, segment, split, rel_l2(mass, ref), float(ref.sum()))
    assert ref.sum() > 0 and np.isfinite(mass).all() and rel_l2(mass, ref) < TOL[name], rel_l2(mass, ref)


@pytest.mark.parametrize("split", [0, 1])
def test_depth_one_build_is_psdr_guide_build(split):
    tb = _scene("cbox_occluder")[0]
    g = GpuScene(tb, options={"sedge_split": split})
    ref = g.guide_build(_abi.make_opts(spp=0, sppe=0, sppse=SPPSE, bsdf_samples=1, light_samples=1), BUILD_RESO, BUILD_ROUNDS)
    mass = gpu_path_guide_build(g, path_opts(1, SPPSE), 1, BUILD_RESO, BUILD_ROUNDS)
    g.close()
    assert ref.sum() > 0 and rel_l2(mass, ref) < 1e-5, rel_l2(mass, ref)


# ---------------------------------------------------------------- 3. guided render against the host
@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_bunny"])
def test_guided_render_matches_host(name):
    """forward (K = 1) and reverse under both grids against the host harness on the same streams and grids, both launch forms"""
    tb, tan, adj = _scene(name)
    ref_d, ref_g = _host_render(name)
    o = path_opts(DEPTH, SPPSE, (0, 0, 7))
    assert np.abs(ref_d).max() > 0
    for split in (0, 1):
        g = GpuScene(tb, options={"sedge_split": split})
        gpu_set_guides(g, GA, GB)
        _, d = g.render_d_fwd(o, [tan])
        assert np.abs(d[0]).max() > 0 and rel_l2(d[0], ref_d) < TOL[name], (split, rel_l2(d[0], ref_d))
        _, grads = g.render_d_rev(o, adj, want=TABLES, with_image=False)
        for k in TABLES:
            assert np.abs(ref_g[k]).max() > 0 and np.abs(grads[k]).max() > 0 and rel_l2(grads[k], ref_g[k]) < TOL[name], (split, k, rel_l2(grads[k], ref_g[k]))
        g.close()


# ---------------------------------------------------------------- 4. one-cell grids
def test_one_cell_grids_are_no_grids():
    """rel_l2 < 2e-5 and the same rays (float atomics forbid bitwise equality), forward and reverse, both launch forms"""
    tb, tan, adj = _scene("cbox_occluder")
    o = path_opts(DEPTH, SPPSE)
    for split in (0, 1):
        g = GpuScene(tb, options={"sedge_split": split})
        _, d0 = g.render_d_fwd(o, [tan]); rays0 = g.counters()
        _, g0 = g.render_d_rev(o, adj, want=TABLES, with_image=False); rrays0 = g.counters()
        gpu_set_guides(g, one_cell_grid(), one_cell_grid())
        _, d1 = g.render_d_fwd(o, [tan]); rays1 = g.counters()
        _, g1 = g.render_d_rev(o, adj, want=TABLES, with_image=False); rrays1 = g.counters()
        g.close()
        assert rays0[3] == rays1[3] > 0 and same_rays(rays0[0], rays1[0]) and same_rays(rrays0[0], rrays1[0])
        assert np.abs(d0[0]).max() > 0 and rel_l2(d1[0], d0[0]) < 2e-5, (split, rel_l2(d1[0], d0[0]))
        for k in TABLES:
            assert np.abs(g0[k]).max() > 0 and rel_l2(g1[k], g0[k]) < 2e-5, (split, k, rel_l2(g1[k], g0[k]))


# ---------------------------------------------------------------- 5. depth 1
@pytest.mark.parametrize("split", [0, 1])
def test_depth_one_guided_is_the_guided_direct_integrator(split):
    tb, tan, adj = _scene("cbox_occluder")
    g = GpuScene(tb, options={"sedge_split": split})
    od = _abi.make_opts(spp=0, sppe=0, sppse=SPPSE, bsdf_samples=1, light_samples=1)
    op = path_opts(1, SPPSE)
    g.set_guide(make_grid(BUILD_RESO, g.guide_build(od, BUILD_RESO, 8)))
    _, d_d = g.render_d_fwd(od, [tan]); rays_d = g.counters()
    _, d_p = g.render_d_fwd(op, [tan]); rays_p = g.counters()
    assert rays_d[3] == rays_p[3] > 0 and same_rays(rays_d[0], rays_p[0])
    assert np.abs(d_d[0]).max() > 0 and rel_l2(d_p[0], d_d[0]) < 1e-5, rel_l2(d_p[0], d_d[0])
    _, g_d = g.render_d_rev(od, adj, want=TABLES, with_image=False); rays_d = g.counters()
    _, g_p = g.render_d_rev(op, adj, want=TABLES, with_image=False); rays_p = g.counters()
    g.close()
    assert same_rays(rays_d[0], rays_p[0])
    for k in TABLES:
        assert np.abs(g_d[k]).max() > 0 and rel_l2(g_p[k], g_d[k]) < 2e-5, (k, rel_l2(g_p[k], g_d[k]))


# ---------------------------------------------------------------- 6. launch forms and shards under the grids
def test_guided_split_launch_and_shards():
    """filter + survivor kernels against one kernel over all slots (rel_l2 < 2e-5, K = 1, K = 3 with three equal tangent sets, reverse), and sppse_range halves
    that sum to the whole (< 1e-5)"""
    tb, tan, adj = _scene("cbox_occluder")
    g = GpuScene(tb)
    gpu_set_guides(g, GA, GB)
    o = path_opts(DEPTH, SPPSE)
    out = {}
    for mode in (0, 1):
        g.set_option("sedge_split", mode)
        _, d = g.render_d_fwd(o, [tan]); rays_f = g.counters()[0]
        _, d3 = g.render_d_fwd(o, [tan, tan, tan])
        _, grads = g.render_d_rev(o, adj, want=TABLES, with_image=False); rays_r = g.counters()[0]
        out[mode] = (d[0], grads, rays_f, rays_r, d3)
    assert same_rays(out[0][2], out[1][2]) and same_rays(out[0][3], out[1][3])
    assert np.abs(out[0][0]).max() > 0 and rel_l2(out[1][0], out[0][0]) < 2e-5
    for k in range(3):
        assert rel_l2(out[0][4][k], out[0][0]) < 2e-5 and rel_l2(out[1][4][k], out[0][0]) < 2e-5
    for k in TABLES:
        a, b = out[0][1][k], out[1][1][k]
        assert np.abs(a).max() > 0 and rel_l2(b, a) < 2e-5, (k, rel_l2(b, a))
    half = SPPSE // 2
    parts_d = sum(g.render_d_fwd(path_opts(DEPTH, SPPSE, sppse_range=r), [tan])[1][0].astype(np.float64) for r in ((0, half), (half, SPPSE)))
    assert rel_l2(parts_d, out[1][0]) < 1e-5
    halves = [g.render_d_rev(path_opts(DEPTH, SPPSE, sppse_range=r), adj, want=TABLES, with_image=False)[1] for r in ((0, half), (half, SPPSE))]
    for k in TABLES:
        assert rel_l2(halves[0][k].astype(np.float64) + halves[1][k], out[1][1][k]) < 1e-5, k
    g.close()


# ---------------------------------------------------------------- 7. grid B belongs to the tables it was set after
def test_set_tables_drops_grid_b():
    tb, tan, _ = _scene("cbox_occluder")
    g = GpuScene(tb)
    o = path_opts(DEPTH, SPPSE)
    _, plain = g.render_d_fwd(o, [tan])
    gpu_set_path_guide(g, GB)
    _, guided = g.render_d_fwd(o, [tan])
    assert rel_l2(guided[0], plain[0]) > 1e-2                   # the grid is used
    g.set_guide(None)                                           # psdr_scene_set_tables, no psdr_scene_set_path_guide after it
    _, after = g.render_d_fwd(o, [tan])
    assert rel_l2(after[0], plain[0]) < 2e-5
    gpu_set_path_guide(g, GB)
    assert rel_l2(g.render_d_fwd(o, [tan])[1][0], guided[0]) < 2e-5
    gpu_set_path_guide(g, None)                                 # psdr_scene_set_path_guide(h, reso, NULL, NULL, 0)
    _, cleared = g.render_d_fwd(o, [tan])
    g.close()
    assert rel_l2(cleared[0], plain[0]) < 2e-5


# ---------------------------------------------------------------- 8. errors carry a message
def test_build_errors():
    tb = _scene("cbox_occluder")[0]
    g = GpuScene(tb)
    lib = g.lib
    mass = torch.zeros(64, dtype=torch.float32, device="cuda")
    r4 = lambda *r: (C.c_int32 * 4)(*r)

    def call(h, o, seg, reso, nrounds, out=mass):
        rc = lib.psdr_path_guide_build(h, C.byref(o) if o is not None else None, seg, reso, nrounds, out.data_ptr() if out is not None else None, None)
        return rc, (lib.psdr_last_error() or b"").decode()

    ok = path_opts(DEPTH, SPPSE)
    small = r4(4, 4, 4, 1)
    for args in ((None, ok, 1, small, 1), (g.h, None, 1, small, 1), (g.h, ok, 1, None, 1), (g.h, ok, 1, small, 1, None)):
        rc, msg = call(*args)
        assert rc != 0 and "null argument" in msg, msg
    for args, text in (((g.h, ok, 1, small, 0), "nrounds must be positive"),
                       ((g.h, _abi.make_opts(sppse=SPPSE), 1, small, 1), "PSDR_INTEGRATOR_PATH"),
                       ((g.h, path_opts(9, SPPSE), 1, small, 1), "max_depth > 8"),
                       ((g.h, path_opts(1, SPPSE), 2, small, 1), "segment 2 needs max_depth >= 2"),
                       ((g.h, ok, 0, small, 1), "segment must be 1"), ((g.h, ok, 3, small, 1), "segment must be 1"),
                       ((g.h, ok, 1, r4(2048, 1024, 1024, 1), 1), "2^31"), ((g.h, ok, 2, r4(1024, 1024, 512, 2), 4), "2^31")):
        rc, msg = call(*args)
        assert rc != 0 and text in msg, (text, msg)
    g.close()
    g = GpuScene(dict(tb, num_sec_edges=0))
    rc, msg = call(g.h, ok, 1, small, 1)
    assert rc != 0 and "no secondary edges" in msg, msg
    g.close()
    assert float(mass.abs().sum()) == 0.0          # no failed call wrote anything


# ---------------------------------------------------------------- 9. the Python surface
def test_surface():
    res, n = 32, 16
    w = torch.linspace(0.5, 1.5, res * res * 3, device="cuda").reshape(-1, 3)
    sc, P = scenario_scene("occluder", n, n, n, res=res)
    pt = psdr_cuda.PathTracer(3, secondary_edges=True)
    wa, wb = pt.preprocess_path_secondary_edges(sc, 0, np.array([64, 4, 4, 2]), np.array([64, 4, 4, 2]), nrounds=4)
    assert isinstance(wa, psdr_cuda.HyperCubeDistribution3f) and isinstance(wb, psdr_cuda.HyperCubeDistribution3f)
    assert wa.m_distrb.m_sum > 0 and wb.m_distrb.m_sum > 0
    assert sc._rng_offset[2] == 0
    sc._rng_offset = [0, 0, 0]
    for call in range(2):
        assert sc._rng_offset[2] == 24 * call          # 11 d - 9 draws per slot at depth 3, guided or not
        img = pt.renderD(sc)
        ek.forward(P)
        grad = ek.gradient(img).numpy().copy()
        if call == 0:
            first = grad
    ref = float((w.cpu().numpy().astype(np.float64) * first).sum())
    # backward = forward contracted with the same adjoint, under the grids
    sc, P = scenario_scene("occluder", n, n, n, res=res)
    sc._rng_offset = [0, 0, 0]
    img = pt.renderD(sc)
    (img.t * w).sum().backward()
    gP = float(ek.gradient(P).numpy().reshape(-1)[0])
    assert abs(gP - ref) < 5e-3 * max(abs(ref), 1e-3), (gP, ref)          # the forward / backward bound of tests/test_python_surface_gpu.py
    # the unguided gradient image on the same streams is another estimate: the grids were used
    sc, P = scenario_scene("occluder", n, n, n, res=res)
    sc._rng_offset = [0, 0, 0]
    img = psdr_cuda.PathTracer(3, secondary_edges=True).renderD(sc)
    ek.forward(P, free_graph=True)
    assert rel_l2(ek.gradient(img).numpy(), first) > 1e-2
    # one grid alone, and none
    wa, wb = pt.preprocess_path_secondary_edges(sc, 0, np.array([16, 2, 2, 1]))
    assert wa is not None and wb is None and pt._guide[0][1] is None
    with pytest.raises(RuntimeError, match="never evaluates the slots"):
        psdr_cuda.PathTracer(3).preprocess_path_secondary_edges(sc, 0, np.array([16, 2, 2, 1]))
    with pytest.raises(RuntimeError, match="max_depth > 8 is not supported for the secondary-edge term"):
        psdr_cuda.PathTracer(9, secondary_edges=True).preprocess_path_secondary_edges(sc, 0, np.array([16, 2, 2, 1]))
    with pytest.raises(RuntimeError, match="only DirectIntegrator builds a guiding grid"):
        pt.preprocess_secondary_edges(sc, 0, np.array([10, 2, 2, 1]), 1)
