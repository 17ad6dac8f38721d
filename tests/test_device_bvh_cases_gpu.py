"""The device tree builder (csrc/psdr_lbvh.h) on the inputs a radix-tree builder classically gets wrong (tests/lbvh_cases.py: runs of equal
Morton keys across the leaf limit, the two sides of the depth limit, a scene without extent in one axis, triangle counts around kLbvhLeaf and
kBlock, clusters, zero-area faces) -- structure against ref_depth, hits against the host-built tree and a float64 brute force, refit after the
geometry has left the Morton order, renders at the deepest traversal stack, and the state of a handle whose build failed.
tests/test_lbvh_cases.py holds the inputs and the references to their promises without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import lbvh_cases as L
import oracle
from helpers import GpuScene, rel_l2
from psdr_cuda import _abi

pytestmark = pytest.mark.gpu

ALL = sorted(L.FAMILIES)
DEVICE = [n for n in ALL if n != "ladder_R39"]          # ladder_R39 is one level too deep: the host builder's


def bvh_stats(g):
    out = (C.c_int32 * 4)()
    _abi.check(g.lib, g.lib.psdr_bvh_stats(g.h, out))
    return dict(builds=out[0], refits=out[1], nodes=out[2], depth=out[3])


def build_options(tb, device):
    """bvh_build = 1 / bvh_build = 0, two_level = 0.  A table of <= 16 triangles would travel in the kernel arguments and get no tree at all
    (kTinyTris): tiny_scene = 0 for those, on both handles -- the triangle counts around kLbvhLeaf are the point of one_cell(5 .. 10)."""
    o = {"bvh_build": 1} if device else {"bvh_build": 0, "two_level": 0}
    if tb["tri_info"].shape[0] <= 16:
        o["tiny_scene"] = 0
    return o


_handles = {}


def handles(name):
    """(device-built handle, host-built handle) of the family's table -- standing handles nobody writes to; the refit and failed-build tests make their own"""
    if name not in _handles:
        tb = L.case(name).tb
        _handles[name] = (GpuScene(tb, options=build_options(tb, True)), GpuScene(tb, options=build_options(tb, False)))
    return _handles[name]


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("name", DEVICE)
def test_structure_is_the_radix_tree_of_the_reference(name):
    c = L.case(name)
    gd, gh = handles(name)
    T = c.rows.shape[0]
    st = bvh_stats(gd)
    want = L.ref_depth(L.ref_keys(c.rows))
    print("%s: T = %d, device tree %s, reference depth %d; host tree %s" % (name, T, st, want, bvh_stats(gh)))
    assert _abi.scene_stats(gd.h)["device_built"] == 1 and _abi.scene_stats(gh.h)["device_built"] == 0
    assert st["nodes"] == T - 1 and st["builds"] == 1 and st["refits"] == 0, st
    assert st["depth"] == want, (st, want)


# ---------------------------------------------------------------- hits
def hit_t(rows, o, d, tri, u, v):
    """t of a reported hit, in float64 from the reported (triangle, u, v): the distance of that point of the triangle along the ray"""
    r = rows.astype(np.float64)
    p = r[tri, 0:3] + u[:, None].astype(np.float64) * r[tri, 3:6] + v[:, None].astype(np.float64) * r[tri, 6:9]
    return ((p - o.astype(np.float64)) * d.astype(np.float64)).sum(1) / (d.astype(np.float64) ** 2).sum(1)


def deviation(rows, rays, bf, got, clear):
    """largest |u|, |v|, |t| deviation of a handle's hits from the brute force on the clear rays it names the same triangle on"""
    o, d, _ = rays
    _, tri, u, v = got
    m = clear & (tri >= 0) & (tri == bf["tri"][:, 0])
    t = hit_t(rows, o[m], d[m], tri[m], u[m], v[m])
    return max(np.abs(u[m] - bf["u"][m, 0]).max(), np.abs(v[m] - bf["v"][m, 0]).max()), np.abs(t - bf["t"][m, 0]).max()


def check_against_brute_force(label, rows, rays, bf, dev, host):
    """A handle's answers (`dev`) against brute_force, with the slack measured on `host` (the host builder's handle, not under test).
    Outside the rays brute_force marks as near an edge or a near-tie (at most 0.2 %), the named triangle is THE float64 hit of minimal t and a miss is a
    float64 miss; barycentrics and t deviate by at most four times what the host-built handle's do on the same rays."""
    o, d, owner = rays
    excluded = bf["near_edge"] | bf["near_tie"]
    assert excluded.mean() <= 0.002, excluded.mean()
    clear = ~excluded
    assert np.array_equal(host[1][clear], bf["tri"][clear, 0]), "%s: the HOST tree disagrees with the brute force -- the reference of this test is broken" % label
    wrong = clear & (dev[1] != bf["tri"][:, 0])
    assert not wrong.any(), "%s: %d clear rays answered wrongly, e.g. ray %d: got triangle %d, float64 says %d" % (
        label, wrong.sum(), np.nonzero(wrong)[0][0], dev[1][wrong][0], bf["tri"][wrong, 0][0])
    (h_uv, h_t), (d_uv, d_t) = deviation(rows, rays, bf, host, clear), deviation(rows, rays, bf, dev, clear)
    print("%s: %d rays (%.3f %% excluded): host tree off the brute force by %.3e in (u, v), %.3e in t; device tree by %.3e, %.3e" % (
        label, o.shape[0], 100 * excluded.mean(), h_uv, h_t, d_uv, d_t))
    assert d_uv <= 4 * h_uv and d_t <= 4 * h_t, (d_uv, h_uv, d_t, h_t)
    dead = np.nonzero(rows[:, 21] == 0)[0]
    assert not np.isin(dev[1], dead).any()              # no zero-area face is ever returned


def check_device_against_host(label, rows, rays, dev, host):
    """Both handles run the same triangle test: they may differ only where two candidates tie in t to float32 resolution -- judged per differing ray by
    the float64 test of the two named triangles (lbvh_cases.pair_test); at most 0.2 % of the rays; agreeing hits agree in (u, v) to 1e-5."""
    o, d, _ = rays
    diff = np.nonzero(dev[1] != host[1])[0]
    assert diff.size <= 0.002 * o.shape[0], diff.size / o.shape[0]
    if diff.size:
        assert (dev[1][diff] >= 0).all() and (host[1][diff] >= 0).all(), "%s: one tree hits where the other misses" % label
        a, b = L.pair_test(rows, o[diff], d[diff], dev[1][diff]), L.pair_test(rows, o[diff], d[diff], host[1][diff])
        assert (a["possible"] & b["possible"]).all(), "%s: a differing ray names a triangle float64 rules out" % label
        assert (np.abs(a["t"] - b["t"]) <= a["tol_t"] + b["tol_t"]).all(), "%s: a differing ray is no tie: %s" % (label, np.abs(a["t"] - b["t"]).max())
    same = (dev[1] == host[1]) & (host[1] >= 0)
    assert same.sum() > 0.1 * o.shape[0]
    assert np.abs(dev[2][same] - host[2][same]).max() < 1e-5 and np.abs(dev[3][same] - host[3][same]).max() < 1e-5
    assert np.array_equal(dev[0][same], host[0][same])
    return diff.size


@pytest.mark.parametrize("name", ALL)
def test_hits_are_the_host_trees_and_the_brute_forces(name):
    """Probe rays (six per live triangle) + 20 000 random rays.  The slack on (u, v) and t is four times the deviation of the HOST-built handle from the
    float64 brute force on the same rays, measured in the run itself and printed per family.  Measured on an MI355X: the host-built handle is off by
    3.3e-6 (planar_y) to 4.0e-4 (with_degenerates) in (u, v) -- 1.3e-4 on ladder(R38), 5.6e-5 on two_clusters -- and by 3.7e-7 (planar_z) to 3.2e-4
    (uniform_1000, the longest edges) in t; the device-built handle by the same figures to all printed digits (same triangle test, same winner).
    The float32 test compiled for the host (tests/test_lbvh_cases.py) gives 5e-6 .. 3.5e-4 in (u, v)."""
    c = L.case(name)
    gd, gh = handles(name)
    o, d, owner = c.rays
    dev, host = gd.trace(o, d), gh.trace(o, d)
    n_diff = check_device_against_host(name, c.rows, c.rays, dev, host)
    check_against_brute_force(name, c.rows, c.rays, c.bf, dev, host)
    # every live triangle is the device tree's answer for at least one of its own probe rays
    probe = owner >= 0
    own = np.unique(owner[probe & (dev[1] == owner)])
    assert np.array_equal(own, np.nonzero(c.rows[:, 21] > 0)[0])
    print("%s: device and host tree differ on %d rays" % (name, n_diff))


def test_a_tree_one_level_too_deep_is_the_host_builders():
    """ladder(R39): the radix tree is 39 deep, lbvh_build hands over to the host builder -- device_built == 0, the host tree's hits (the test above
    runs the family against the brute force) and image, and the handle still follows moved vertices."""
    c = L.case("ladder_R39")
    assert L.ref_depth(L.ref_keys(c.rows)) == 39
    sc = L.make_scene(c.verts, c.faces, res=16, spp=4, eye=(0.5, 0.45, 2.5), target=(0.5, 0.5, 0.5))
    tb = sc.tables(0)
    gd, gh = GpuScene(tb, options=build_options(tb, True)), GpuScene(tb, options=build_options(tb, False))
    st = bvh_stats(gd)
    assert _abi.scene_stats(gd.h)["device_built"] == 0 and st["builds"] == 1 and 0 < st["depth"] <= 38, st
    o, d, _ = c.rays
    check_device_against_host("ladder_R39", c.rows, c.rays, gd.trace(o, d), gh.trace(o, d))
    for opt in (_abi.make_opts(spp=4, bsdf_samples=1, light_samples=1), _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=3, spp=4)):
        img, ref = gd.render_c(opt), gh.render_c(opt)
        assert np.isfinite(img).all() and img.mean() > 0 and rel_l2(img, ref) < 1e-4, rel_l2(img, ref)
    rows = gd.tb["tri_info"]
    rows[:, 0] += 0.5
    rows[::2, 1] += 5.0              # whole cells, and 2^j + 5 is no power of two: no moved triangle lands on (or in the plane of) one that stayed
    torch.cuda.synchronize()
    _abi.check(gd.lib, gd.lib.psdr_bvh_build(gd.h, None))
    st = bvh_stats(gd)
    assert st["builds"] + st["refits"] == 2, st              # refitted or rebuilt, either is right
    tb_moved = dict(tb); tb_moved["tri_info"] = rows.detach().cpu()
    fresh = GpuScene(tb_moved, options=build_options(tb, False))
    o2 = o + np.float32(0.5) * np.array([1, 0, 0], np.float32)
    a, b = gd.trace(o2, d), fresh.trace(o2, d)
    assert (b[1] >= 0).mean() > 0.1
    check_device_against_host("ladder_R39 (moved)", L.table_rows(tb_moved), (o2, d, None), a, b)


# ---------------------------------------------------------------- refit
@pytest.mark.parametrize("name", L.REFIT_FAMILIES)
def test_refit_after_the_geometry_has_left_the_morton_order(name):
    """Every triangle translated to the place of another (lbvh_cases.permuted_rows), rows [:, 0:3] written in place: the standing topology has
    nothing to do with the geometry any more.  The first refit after a build is always taken (the area check reads the PREVIOUS refit): the
    refitted tree must still return the brute force's hits on the moved table."""
    c = L.case(name)
    rows, rays, bf = L.moved(c)
    g = GpuScene(c.tb, options=build_options(c.tb, True))
    assert _abi.scene_stats(g.h)["device_built"] == 1
    g.tb["tri_info"][:, 0:3] = torch.as_tensor(rows[:, 0:3]).cuda()
    torch.cuda.synchronize()
    _abi.check(g.lib, g.lib.psdr_bvh_build(g.h, None))
    st = bvh_stats(g)
    assert st["refits"] == 1 and st["builds"] == 1, st
    tb_moved = dict(c.tb); tb_moved["tri_info"] = torch.as_tensor(rows)
    host = GpuScene(tb_moved, options=build_options(c.tb, False))
    o, d, _ = rays
    dev, ref = g.trace(o, d), host.trace(o, d)
    check_device_against_host(name + " (refitted)", rows, rays, dev, ref)
    check_against_brute_force(name + " (refitted)", rows, rays, bf, dev, ref)


# ---------------------------------------------------------------- render
VIEWS = {"ladder_R38": ((0.5, 0.45, 2.5), (0.5, 0.5, 0.5)), "one_cell_1001": ((0.5, 0.45, 2.5), (0.5, 0.5, 0.5)), "two_clusters": ((1.0, 0.9, 5.0), (1.0, 1.0, 1.0))}


@pytest.mark.parametrize("name", sorted(VIEWS))
def test_renders_through_the_deepest_stacks(name):
    """The soup as an emissive mesh seen from close to its cluster at cell 0, 24 x 24 at 4 spp, DirectIntegrator(1, 1) and PathTracer(3).  ladder(R38) is
    the deepest tree the kernels may be asked to walk: depth 38, min(kBvhStack, depth + 2) = 40 stack entries per lane."""
    c = L.case(name)
    sc = L.make_scene(c.verts, c.faces, res=24, spp=4, eye=VIEWS[name][0], target=VIEWS[name][1])
    tb = sc.tables(0)
    gd, gh = GpuScene(tb, options=build_options(tb, True)), GpuScene(tb, options=build_options(tb, False))
    assert _abi.scene_stats(gd.h)["device_built"] == 1
    want = L.ref_depth(L.ref_keys(L.table_rows(tb)))
    assert bvh_stats(gd)["depth"] == want and (name != "ladder_R38" or want == 38)
    for kw in (dict(bsdf_samples=1, light_samples=1), dict(integrator=_abi.INTEGRATOR_PATH, max_depth=3)):
        opt = _abi.make_opts(spp=4, **kw)
        img, img_h, ref = gd.render_c(opt), gh.render_c(opt), oracle.render(tb, opt)
        assert np.isfinite(img).all() and img.mean() > 0
        print("%s %s: device against host tree rel-L2 %.2e, mean %.3f" % (name, sorted(kw), rel_l2(img, img_h), img.mean()))
        assert rel_l2(img, img_h) < 1e-4, rel_l2(img, img_h)
        bad = (np.abs(img - ref).max(1) > 2e-3 * (1 + np.abs(ref).max(1))).mean()             # the criterion of test_render_fuzz_random_scenes
        assert bad < 0.03, (name, kw, bad)


# ---------------------------------------------------------------- a build that fails
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_a_failed_build_leaves_the_handle_without_a_tree(device):
    """A standing tree that has rendered; one NaN in a vertex; psdr_bvh_build (bvh_refit = 0: a full build) fails with `non-finite vertex`.  The device
    builder has by then overwritten the leaf records and the children of the old tree: the handle must refuse to launch (`Input scene must be
    configured!`) instead of walking new children with old boxes, and the next build -- vertex restored -- must be a full one whose hits are a fresh
    handle's.  The host builder's error exit (same message) leaves the same state."""
    c = L.case("runs")
    sc = L.make_scene(c.verts, c.faces, res=16, spp=4, eye=(0.5, 0.45, 2.5), target=(0.5, 0.5, 0.5))
    tb = sc.tables(0)
    g = GpuScene(tb, options=build_options(tb, device))
    assert _abi.scene_stats(g.h)["device_built"] == int(device)
    opt = _abi.make_opts(spp=4, bsdf_samples=1, light_samples=1)
    o, d, _ = c.rays
    img0, hits0 = g.render_c(opt), g.trace(o, d)
    assert np.isfinite(img0).all() and (hits0[1] >= 0).mean() > 0.1
    rows = g.tb["tri_info"]
    keep = float(rows[37, 1])
    rows[37, 1] = float("nan")
    torch.cuda.synchronize()
    g.set_option("bvh_refit", 0)
    assert g.lib.psdr_bvh_build(g.h, None) != 0 and b"non-finite vertex" in g.lib.psdr_last_error()
    with pytest.raises(RuntimeError, match="Input scene must be configured!"):
        g.render_c(opt)
    with pytest.raises(RuntimeError, match="Input scene must be configured!"):
        g.trace(o[:64], d[:64])
    # a second failing build changes nothing; nor does switching the refit back on (no tree to refit)
    g.set_option("bvh_refit", 1)
    assert g.lib.psdr_bvh_build(g.h, None) != 0 and b"non-finite vertex" in g.lib.psdr_last_error()
    with pytest.raises(RuntimeError, match="Input scene must be configured!"):
        g.trace(o[:64], d[:64])
    rows[37, 1] = keep
    torch.cuda.synchronize()
    before = bvh_stats(g)
    _abi.check(g.lib, g.lib.psdr_bvh_build(g.h, None))
    st = bvh_stats(g)
    assert st["builds"] == before["builds"] + 1 and st["refits"] == before["refits"], (before, st)
    assert _abi.scene_stats(g.h)["device_built"] == int(device)
    fresh = GpuScene(tb, options=build_options(tb, device))
    hits1, hits_f = g.trace(o, d), fresh.trace(o, d)
    assert all(np.array_equal(x, y) for x, y in zip(hits1, hits_f)) and all(np.array_equal(x, y) for x, y in zip(hits1, hits0))
    assert rel_l2(g.render_c(opt), fresh.render_c(opt)) < 1e-6 and rel_l2(g.render_c(opt), img0) < 1e-6
