"""The PathTracer's secondary-edge term (PSDR_FLAG_PATH_SEDGES; csrc/psdr_path_sedge.hip) on the GPU: through the C ABI against
DirectIntegrator's term (depth 1), against the host harness (same streams) and against itself (split launch, shards, no flag), and through the Python
surface against central finite differences of renderC -- the reference's own validation method, as tests/test_ad_vs_fd_gpu.py."""
import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from helpers import GpuScene, load_scene, rel_l2, same_rays, tangents_wrt
from path_sedge_helpers import SCENARIOS, host_path_sedge_fwd, host_path_sedge_rev, path_opts, scenario_scene
from psdr_cuda import _abi

pytestmark = pytest.mark.gpu

TABLES = ["tri_info", "sec_edge", "cam_to_world"]


# ---------------------------------------------------------------- 4. AD against FD, three scenarios
def _ad(name, secondary_edges, options=None, spp=8192):
    depth = SCENARIOS[name][1]
    sc, P = scenario_scene(name, spp, spp, spp)
    sc.native_options = dict(options or {})
    integ = psdr_cuda.PathTracer(depth, secondary_edges=secondary_edges)
    sc._rng_offset = [0, 0, 0]
    img = integ.renderD(sc)
    ek.forward(P, free_graph=True)
    return ek.gradient(img).numpy().astype(np.float64)


def _fd(name, M):
    """central difference (eps = 1) of renderC, both sides on the same streams (as test_object_translation_needs_all_three_terms: two fresh scenes), twice on
    independent streams: (mean of the two, their rel_l2 distance = the FD floor)"""
    depth = SCENARIOS[name][1]
    integ = psdr_cuda.PathTracer(depth)
    fds = []
    for seed in (0, 1):
        sides = []
        for s in (+1.0, -1.0):
            sc, _ = scenario_scene(name, M, offset=s)
            sc._rng_offset = [1000 * seed, 0, 0]
            sides.append(integ.renderC(sc).numpy().astype(np.float64))
        fds.append((sides[0] - sides[1]) / 2.0)
    return (fds[0] + fds[1]) / 2.0, rel_l2(fds[0], fds[1])


B, MARGIN = 0.08, 0.05          # tests/test_ad_vs_fd_gpu.py:134-135


@pytest.mark.parametrize("name,masked,fd_spp,ad_spp", [("occluder", None, 131072, 8192), ("uplight", {"pt_sedge": 1}, 524288, 8192), ("mirror", {"pt_sedge_walk": 0}, 524288, 65536)])
def test_ad_vs_fd(name, masked, fd_spp, ad_spp):
    """res 24, spp = sppe = sppse = ad_spp, FD from renderC at fd_spp (two independent FDs: their mean is the reference, their distance the FD floor; fd_spp is
    raised from 131072 until 2 * floor < B), an occluder translated, B = 0.08 and margin = 0.05 as test_object_translation_needs_all_three_terms.
      occluder  cbox_occluder, PathTracer(3), 8192 slots: e_all < B and e_all + margin < the error with secondary_edges=False;
      uplight   the floor is lit by the ceiling alone, PathTracer(2), 8192 slots: e_all < B, and without segment B (pt_sedge 1) worse by the margin;
      mirror    the floor is seen only in a rough-conductor quad, PathTracer(2): e_all < B, and with the walk cut (pt_sedge_walk 0) worse by the margin.  65536 slots:
                at 8192 the AD estimate's own noise is above B (tests/test_path_sedge_host.py::test_ad_vs_fd_mirror has the figures); the bound is unchanged.
    Measured figures: DESIGN.md section 10."""
    fd, floor = _fd(name, fd_spp)
    e_all = rel_l2(_ad(name, True, spp=ad_spp), fd)
    e_masked = rel_l2(_ad(name, False, spp=ad_spp) if masked is None else _ad(name, True, masked, spp=ad_spp), fd)
    print("%s: FD floor %.4f e_all %.4f e_masked %.4f" % (name, floor, e_all, e_masked))
    assert 2 * floor < B, floor
    assert e_all < B, (floor, e_all, e_masked)
    assert e_masked > e_all + MARGIN, (floor, e_all, e_masked)


# ---------------------------------------------------------------- 5. anchor, host parity, split launch
def _occluder(res, sppse, scene="cbox_occluder"):
    sc, P = load_scene(scene, res=res, spp=0, sppe=0, sppse=sppse, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    return tb, tangents_wrt(tb, P), np.random.default_rng(4).random((res * res, 3)).astype(np.float32)


@pytest.mark.parametrize("split", [0, 1])
def test_depth_one_is_the_direct_integrators_term(split):
    """PathTracer(1) with the flag against DirectIntegrator(1, 1): the same rays, the derivative image to 1e-5, the reverse gradients to 2e-5 (the bounds
    of test_secondary_edge_split_launch_equals_one_kernel: float atomics forbid bitwise equality)."""
    tb, tan, adj = _occluder(64, 32)
    g = GpuScene(tb, options={"sedge_split": split})
    od = _abi.make_opts(spp=0, sppe=0, sppse=32, bsdf_samples=1, light_samples=1)
    op = path_opts(1, 32)
    _, d_d = g.render_d_fwd(od, [tan]); rays_d = g.counters()
    _, d_p = g.render_d_fwd(op, [tan]); rays_p = g.counters()
    assert rays_d[3] == rays_p[3] > 0 and same_rays(rays_d[0], rays_p[0])
    assert np.abs(d_d[0]).max() > 0 and rel_l2(d_p[0], d_d[0]) < 1e-5
    _, g_d = g.render_d_rev(od, adj, want=TABLES, with_image=False); rays_d = g.counters()
    _, g_p = g.render_d_rev(op, adj, want=TABLES, with_image=False); rays_p = g.counters()
    assert same_rays(rays_d[0], rays_p[0])
    for k in TABLES:
        assert np.abs(g_d[k]).max() > 0 and rel_l2(g_p[k], g_d[k]) < 2e-5, (k, rel_l2(g_p[k], g_d[k]))


@pytest.mark.parametrize("scene,tol", [("cbox_occluder", 1e-3), ("cbox_bunny", 2e-2)])
def test_gpu_matches_host_at_depth_three(scene, tol):
    """forward derivative image and reverse gradients at depth 3 against the host harness on the same streams (rel_l2 < 1e-3 as
    test_gpu_reverse_matches_host_reverse; 2e-2 on the tree scene, that file's bound for bunny scenes), both launch forms"""
    tb, tan, adj = _occluder(32, 16, scene)
    o = path_opts(3, 16, (0, 0, 7))
    ref_d = host_path_sedge_fwd(tb, o, tan)
    ref_g = host_path_sedge_rev(tb, o, adj, want=TABLES)
    assert np.abs(ref_d).max() > 0
    for split in (0, 1):
        g = GpuScene(tb, options={"sedge_split": split})
        _, d = g.render_d_fwd(o, [tan])
        assert rel_l2(d[0], ref_d) < tol, (split, rel_l2(d[0], ref_d))
        _, grads = g.render_d_rev(o, adj, want=TABLES, with_image=False)
        for k in TABLES:
            assert np.abs(ref_g[k]).max() > 0 and rel_l2(grads[k], ref_g[k]) < tol, (split, k, rel_l2(grads[k], ref_g[k]))
        g.close()


def test_split_launch_equals_one_kernel():
    """filter kernels + survivor kernels against one kernel over all slots at depth 3: same rays, rel_l2 < 2e-5, forward (K = 1 and K = 3) and reverse"""
    tb, tan, adj = _occluder(64, 32)
    g = GpuScene(tb)
    o = path_opts(3, 32)
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


# ---------------------------------------------------------------- 6. nothing moves without the flag
def test_without_the_flag_sppse_is_ignored():
    tb, tan, _ = _occluder(32, 8)
    g = GpuScene(tb)
    kw = dict(integrator=_abi.INTEGRATOR_PATH, max_depth=3, spp=64, sppe=8, rng_offset=(1, 2, 3))          # (64 samples per pixel: the camera kernel stores its pixels, the primal is reproducible bit for bit)
    img0, d0 = g.render_d_fwd(_abi.make_opts(sppse=0, **kw), [tan])
    img1, d1 = g.render_d_fwd(_abi.make_opts(sppse=8, **kw), [tan])
    assert g.counters()[3] == 0
    assert np.array_equal(img0, img1) and rel_l2(d1[0], d0[0]) < 1e-6
    img2, d2 = g.render_d_fwd(_abi.make_opts(sppse=8, flags=_abi.FLAG_PATH_SEDGES, **kw), [tan])
    assert g.counters()[3] == 32 * 32 * 8 and np.array_equal(img0, img2) and rel_l2(d2[0], d0[0]) > 1e-2
    # the flag is ignored for the other integrators
    kd = dict(bsdf_samples=1, light_samples=1, spp=8, sppe=8, sppse=8, rng_offset=(1, 2, 3))
    _, da = g.render_d_fwd(_abi.make_opts(**kd), [tan])
    _, db = g.render_d_fwd(_abi.make_opts(flags=_abi.FLAG_PATH_SEDGES, **kd), [tan])
    assert rel_l2(db[0], da[0]) < 1e-6


def test_surface_default_streams_and_depth_limit():
    sc, P = scenario_scene("occluder", 4, 4, 4, res=16)
    pt = psdr_cuda.PathTracer(3)
    img = pt.renderD(sc); ek.forward(P, free_graph=True); ek.gradient(img).numpy()
    assert pt.last_counters[3] == 0 and sc._rng_offset[2] == 0
    sc, P = scenario_scene("occluder", 4, 4, 4, res=16)
    pt = psdr_cuda.PathTracer(3, secondary_edges=True)
    grads = []
    for call in range(2):
        assert sc._rng_offset[2] == call * _abi.draws_per_slot(path_opts(3, 4))[2] == call * 24
        img = pt.renderD(sc); ek.forward(P); grads.append(ek.gradient(img).numpy().copy())
        assert pt.last_counters[3] == 16 * 16 * 4
    assert rel_l2(grads[1], grads[0]) > 1e-2          # disjoint streams: another estimate
    with pytest.raises(RuntimeError, match="max_depth > 8 is not supported for the secondary-edge term"):
        psdr_cuda.PathTracer(9, secondary_edges=True).renderD(sc)
    tb, tan, _ = _occluder(16, 4)
    with pytest.raises(RuntimeError, match="max_depth > 8 is not supported for the secondary-edge term"):
        GpuScene(tb).render_d_fwd(path_opts(9, 4), [tan])
    with pytest.raises(RuntimeError, match="only DirectIntegrator builds a guiding grid"):
        pt.preprocess_secondary_edges(sc, 0, np.array([10, 2, 2, 1]), 1)


# ---------------------------------------------------------------- 7. shards are linear
def test_shards_are_linear():
    """sppse_range halves sum to the whole (rel_l2 < 1e-5, the bound of test_gpu_full_size::test_c2_shards_are_linear), forward and reverse"""
    tb, tan, adj = _occluder(64, 32)
    g = GpuScene(tb)
    full_d = g.render_d_fwd(path_opts(3, 32), [tan])[1][0]
    full_g = g.render_d_rev(path_opts(3, 32), adj, want=TABLES, with_image=False)[1]
    parts_d = sum(g.render_d_fwd(path_opts(3, 32, sppse_range=r), [tan])[1][0].astype(np.float64) for r in ((0, 16), (16, 32)))
    assert np.abs(full_d).max() > 0 and rel_l2(parts_d, full_d) < 1e-5
    halves = [g.render_d_rev(path_opts(3, 32, sppse_range=r), adj, want=TABLES, with_image=False)[1] for r in ((0, 16), (16, 32))]
    for k in TABLES:
        assert rel_l2(halves[0][k].astype(np.float64) + halves[1][k], full_g[k]) < 1e-5, k


# ---------------------------------------------------------------- 8. through the surface: backward = forward contracted with the same adjoint
def test_surface_backward_equals_forward():
    res, n = 32, 16
    w = torch.linspace(0.5, 1.5, res * res * 3, device="cuda").reshape(-1, 3)
    sc, P = scenario_scene("occluder", n, n, n, res=res)
    pt = psdr_cuda.PathTracer(3, secondary_edges=True)
    sc._rng_offset = [0, 0, 0]
    img = pt.renderD(sc)
    ek.forward(P, free_graph=True)
    ref = float((w.cpu().numpy().astype(np.float64) * ek.gradient(img).numpy()).sum())
    sc, P = scenario_scene("occluder", n, n, n, res=res)
    sc._rng_offset = [0, 0, 0]
    img = pt.renderD(sc)
    (img.t * w).sum().backward()
    gP = float(ek.gradient(P).numpy().reshape(-1)[0])
    # without the term the same contraction is another number: the backward call did run the new adjoint kernels
    sc, P = scenario_scene("occluder", n, n, n, res=res)
    sc._rng_offset = [0, 0, 0]
    img = psdr_cuda.PathTracer(3).renderD(sc)
    ek.forward(P, free_graph=True)
    ref_without = float((w.cpu().numpy().astype(np.float64) * ek.gradient(img).numpy()).sum())
    assert abs(gP - ref) < 5e-3 * max(abs(ref), 1e-3), (gP, ref)          # the forward / backward bound of tests/test_python_surface_gpu.py
    assert abs(ref_without - ref) > 0.05 * abs(ref), (ref, ref_without)
