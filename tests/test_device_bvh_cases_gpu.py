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
from bvh_checks import check_against_brute_force, check_device_against_host
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


# ---------------------------------------------------------------- hits (the criteria: tests/bvh_checks.py)
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
