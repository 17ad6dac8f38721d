"""The PathTracer's secondary-edge term (PSDR_FLAG_PATH_SEDGES, csrc/psdr_path_sedge.h) on the HOST: the product's PSDR_HD
functions run slot by slot by tests/hostcheck/hostcheck_path_sedge.cpp.  Three questions, none of which needs a GPU:
  1. depth 1 IS DirectIntegrator(1, 1)'s term, bit for bit (the anchor to the reference's eval_secondary_edge);
  2. reverse mode is the adjoint of forward mode, and the two segments add up;
  3. the estimator is the derivative: AD against central finite differences of the PathTracer's own renderC, with each new part
     (the sensor-side walk, the indirect-source segment) shown to be needed where a scene makes it carry the gradient."""
import numpy as np
import pytest

from helpers import dot_tables, host_render, load_scene, random_tangents, rel_l2, tangents_wrt
from path_sedge_helpers import SCENARIOS, host_path_sedge_fwd, host_path_sedge_rev, path_opts, scenario_scene
from psdr_cuda import _abi


@pytest.mark.parametrize("scene,mesh", [("cbox_occluder", 1), ("cbox_bunny", 1)])
def test_depth_one_is_the_direct_integrators_term(scene, mesh):
    """PathTracer(1) with the flag against hostcheck_render mode 1 of DirectIntegrator(1, 1): the difference of two runs with and without sppse (no camera and
    no primary-edge slots, so that the difference is exact).  The host's summation order is fixed: np.array_equal.  With segment A alone and the walk cut
    at its first vertex the term is that same image at every depth."""
    sc, P = load_scene(scene, res=24, spp=8, sppe=8, sppse=8, translate=(mesh, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    kw = dict(spp=0, sppe=0, rng_offset=(0, 5, 9), bsdf_samples=1, light_samples=1)
    ref = host_render(tb, _abi.make_opts(sppse=8, **kw), mode=1, tangents=tan)[1] - host_render(tb, _abi.make_opts(sppse=0, **kw), mode=1, tangents=tan)[1]
    assert np.abs(ref).max() > 0
    assert np.array_equal(host_path_sedge_fwd(tb, path_opts(1, 8, (0, 5, 9)), tan), ref)
    for depth in (2, 3, 8):
        assert np.array_equal(host_path_sedge_fwd(tb, path_opts(depth, 8, (0, 5, 9)), tan, seg=1, walk=0), ref), depth
    # ... and the full term at depth 3 is not that image
    assert rel_l2(host_path_sedge_fwd(tb, path_opts(3, 8, (0, 5, 9)), tan), ref) > 1e-2


def test_draws_per_slot():
    from path_sedge_helpers import path_sedge_lib
    H = path_sedge_lib()
    for d in range(1, 9):
        assert _abi.draws_per_slot(path_opts(d, 4))[2] == H.hostcheck_path_sedge_draws(d) == (3 if d == 1 else 11 * d - 9)
    # without the flag, and for the other integrators, a slot of sampler 2 keeps its three draws
    assert _abi.draws_per_slot(_abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=3, sppse=4))[2] == 3
    assert _abi.draws_per_slot(_abi.make_opts(sppse=4, flags=_abi.FLAG_PATH_SEDGES))[2] == 3


@pytest.mark.parametrize("scene", ["cbox_occluder", "cbox_bunny"])
def test_forward_equals_reverse_and_segments_add_up(scene):
    """<adj, J t> = <J^T adj, t> for the tables the term reaches (triangle rows, edge rows, the camera), at depth 3, per segment and for both;
    |lhs - rhs| <= 1e-4 * scale as test_reverse_mode.py::test_dot_product_identity_host.  pt_sedge 1 + pt_sedge 2 = pt_sedge 3 to the same bound."""
    res, sppse = 16, 16
    sc, _ = load_scene(scene, res=res, spp=4, sppe=0, sppse=sppse)
    tb = sc.tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = path_opts(3, sppse, (2, 3, 4))
    for n in ("tri_info", "sec_edge", "cam_to_world"):
        tan = random_tangents(tb, [n], seed=1)
        lhs_seg, grads_seg = {}, {}
        for seg in (1, 2, 3):
            dimg = host_path_sedge_fwd(tb, o, tan, seg=seg)
            grads = host_path_sedge_rev(tb, o, adj, want=[n], seg=seg)
            lhs, rhs = float((adj.astype(np.float64) * dimg).sum()), dot_tables(grads, tan)
            scale = float(np.abs(adj.astype(np.float64) * dimg).sum())       # the sum itself may cancel
            assert scale > 0, (n, seg)
            assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, seg, lhs, rhs, scale)
            lhs_seg[seg], grads_seg[seg] = (lhs, scale, dimg), grads[n].astype(np.float64)
        scale = lhs_seg[3][1]
        assert abs(lhs_seg[1][0] + lhs_seg[2][0] - lhs_seg[3][0]) <= 1e-4 * scale, n
        assert rel_l2(lhs_seg[1][2].astype(np.float64) + lhs_seg[2][2], lhs_seg[3][2]) < 1e-4, n
        assert rel_l2(grads_seg[1] + grads_seg[2], grads_seg[3]) < 1e-4, n


# ---------------------------------------------------------------- AD against finite differences
AD_SPP, BASE_SPP, FD_SPP, NT = 16384, 4096, 262144, 16


def _fd(name, depth):
    """central difference (eps = 1) of the PathTracer's renderC on the host, mean of two independent seeds; also the distance of the two (the FD floor)"""
    fds = []
    for seed in (0, 1):
        imgs = []
        for s in (+1.0, -1.0):
            sc, _ = scenario_scene(name, FD_SPP, offset=s)
            imgs.append(host_render(sc.tables(0), _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=FD_SPP, rng_offset=(1000 * seed, 0, 0)), nthreads=NT).astype(np.float64))
        fds.append((imgs[0] - imgs[1]) / 2.0)
    return (fds[0] + fds[1]) / 2.0, rel_l2(fds[0], fds[1])


def _ad_errors(name, variants, ad_spp=AD_SPP, base_spp=BASE_SPP):
    """rel_l2 against FD of interior + primary edges (the existing harness, ONE run shared by all variants, so that two errors differ by the new parts
    alone) + the new term per (pt_sedge, pt_sedge_walk)"""
    depth = SCENARIOS[name][1]
    fd, floor = _fd(name, depth)
    sc, P = scenario_scene(name, ad_spp, ad_spp, ad_spp)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    _, base = host_render(tb, _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=base_spp, sppe=base_spp, sppse=0), mode=1, tangents=tan, nthreads=NT)
    out = {"floor": floor, "without": rel_l2(base, fd)}
    for key, (seg, walk) in variants.items():
        out[key] = rel_l2(base.astype(np.float64) + host_path_sedge_fwd(tb, path_opts(depth, ad_spp), tan, seg=seg, walk=walk, nthreads=NT), fd)
    print(name, " ".join("%s=%.4f" % kv for kv in out.items()))
    return out


def test_ad_vs_fd_occluder():
    """cbox_occluder, res 24, Mesh[1] translated along (1, 0.5, 0), PathTracer(3): AD (16384 slots per pixel for the new term, 4096 for interior and primary
    edges) against FD (2 x 262144 spp, eps = 1).
    Bounds: e_all < 0.1 and e_without > e_all + 0.05 (test_oracle_estimators.py::test_geometry_derivative_interior_plus_edges_matches_fd); completeness:
    e_all < e_cut - 0.015, e_cut = the same run with segment A alone and the walk cut at y_0 (what DirectIntegrator's term would add).
    Measured: FD floor 0.0175, e_without 0.2014, e_cut 0.0637, segment A with its walk 0.0468, e_all 0.0456 (gap to e_cut 0.018)."""
    e = _ad_errors("occluder", {"cut": (1, 0), "all": (3, 1)})
    assert e["all"] < 0.1, e
    assert e["without"] > e["all"] + 0.05, e
    assert e["all"] < e["cut"] - 0.015, e


def test_ad_vs_fd_uplight():
    """The emitter faces the ceiling and the floor is lit by the ceiling alone: the occluder's shadow has no direct-source segment (segment A adds exactly
    nothing here), the indirect-source segment carries the whole boundary term.  PathTracer(2), the counts of the occluder test.
    Measured: FD floor 0.0297, e_without = e(segment A only) 0.5155, e_all 0.0877 (0.062 with eight times the AD slots)."""
    e = _ad_errors("uplight", {"a_only": (1, 1), "all": (3, 1)})
    assert e["all"] < 0.1, e
    assert e["a_only"] > e["all"] + 0.05, e


def test_ad_vs_fd_mirror():
    """The camera sees the floor under a rough-conductor quad (alpha 0.15), and the occluder's shadow on it, only in that quad: the boundary reaches the
    image through one bounce of the sensor-side walk (a cosine-sampled direction from the floor, then the GGX lobe evaluated towards the camera: about one
    walk in ten carries weight).  PathTracer(2).  At the counts of the occluder test the AD estimate itself is too noisy for the bound -- two AD seeds
    differ by 0.10 of the FD norm for the new term and by 0.10 for interior + primary edges, e_all = 0.145 -- so THIS scenario runs with eight times
    the AD slots (131072) and sixteen times the interior / primary-edge samples (65536); the bounds are unchanged.
    Measured there: FD floor 0.0276, e_without 1.8669, walk cut at y_0 1.5092, segment A only 0.51, e_all 0.0380."""
    e = _ad_errors("mirror", {"no_walk": (3, 0), "all": (3, 1)}, ad_spp=8 * AD_SPP, base_spp=16 * BASE_SPP)
    assert e["all"] < 0.1, e
    assert e["no_walk"] > e["all"] + 0.05, e
