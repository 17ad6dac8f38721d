"""Lean twin of the log-derivative camera kernel (option logd_park; csrc/psdr_logd_lean.h, psdr_logd_lean.hip): the K = 1 forward-mode PathTracer launches with
tangents on albedo texels, on a plain diffuse scene without a tree, keep a path's idle state in per-lane LDS columns instead of scratch memory.

The twin evaluates the estimator of k_camera_logd with the same draws and the same arithmetic forms, so image and derivative image are the same BITS with the
option on and off, and with the seeds loaded from the handle's seed table or computed.  Every case runs two consecutive render calls: the second continues the
streams behind the first one's draws (a non-zero rng_offset).  Shapes: a wave on one pixel (pixels stored by the run's head lane), several pixels per wave,
and a launch that is no multiple of the workgroup, whose pixels straddle waves (at most two waves add to a pixel of a zeroed image: the sum does not depend on
their order).  psdr_scene_logd_info says which kernel a launch took."""
import functools

import numpy as np
import pytest
import torch

import psdr_cuda
from helpers import GpuScene, random_tangents
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32, 64), (24, 24, 8), (17, 13, 5)]


@functools.lru_cache(maxsize=None)
def tables(name, w, h):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(name), False)
    sc.opts.width, sc.opts.height = w, h
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 0, 0, 0
    sc.configure()
    return sc.tables(0)


def two_calls(spp, depth):
    o = _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=spp)
    return o, _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=spp, rng_offset=_abi.draws_per_slot(o))


def run(g, calls, tans):
    out = []
    for o in calls:
        img, d = g.render_d_fwd(o, tans)
        out.append((img, d, g.counters()[0]))
    return out


def same_bits(a, b):
    for (ia, da, ra), (ib, db, rb) in zip(a, b):
        assert np.isfinite(ia).all() and ia.max() > 0 and np.abs(da).max() > 0
        assert np.array_equal(ia, ib), np.abs(ia - ib).max()
        assert np.array_equal(da, db), np.abs(np.asarray(da) - np.asarray(db)).max()
        assert ra == rb and ra > 0
    assert not np.array_equal(a[0][0], a[1][0])          # the second call drew other numbers


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("w,h,spp", SHAPES)
def test_the_lean_twin_returns_the_bits_of_the_kernel_it_replaces(w, h, spp, depth):
    tb = tables("cbox", w, h)
    tan = random_tangents(tb, ["texels"], seed=11)
    g1, g0 = GpuScene(tb, options={"logd_park": 1}), GpuScene(tb, options={"logd_park": 0})
    same_bits(run(g1, two_calls(spp, depth), [tan]), run(g0, two_calls(spp, depth), [tan]))
    i1, i0 = _abi.logd_info(g1.h), _abi.logd_info(g0.h)
    print("lean launch: %d bytes of dynamic LDS per workgroup" % i1["lean_lds_bytes"])
    assert (i1["launches"], i1["lean"], i1["lean_seeded"]) == (2, 2, 2), i1
    assert 0 < 6 * i1["lean_lds_bytes"] <= 160 * 1024
    assert (i0["launches"], i0["lean"], i0["lean_seeded"], i0["lean_lds_bytes"]) == (2, 0, 0, 0), i0


@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("w,h,spp", SHAPES)
def test_the_seeded_lean_twin_returns_the_bits_of_the_unseeded_one(w, h, spp, depth):
    tb = tables("cbox", w, h)
    tan = random_tangents(tb, ["texels"], seed=5)
    g1, g0 = GpuScene(tb, options={"seed_cache": 1}), GpuScene(tb, options={"seed_cache": 0})
    same_bits(run(g1, two_calls(spp, depth), [tan]), run(g0, two_calls(spp, depth), [tan]))
    i1, i0 = _abi.logd_info(g1.h), _abi.logd_info(g0.h)
    assert (i1["lean"], i1["lean_seeded"]) == (2, 2), i1
    assert (i0["lean"], i0["lean_seeded"]) == (2, 0), i0
    s1 = _abi.seed_cache_info(g1.h)
    assert (s1["fills"], s1["slots"]) == (1, w * h * spp), s1          # one fill serves both calls


def test_three_tangent_sets_take_the_kernel_without_columns():
    tb = tables("cbox", 24, 24)
    t3 = []
    for c in range(3):
        t = torch.zeros_like(tb["texels"]); t[c] = 1.0
        t3.append({"texels": t})
    g1, g0 = GpuScene(tb, options={"logd_park": 1}), GpuScene(tb, options={"logd_park": 0})
    same_bits(run(g1, two_calls(8, 3), t3), run(g0, two_calls(8, 3), t3))
    i1 = _abi.logd_info(g1.h)
    assert (i1["launches"], i1["lean"]) == (2, 0), i1


def test_a_scene_with_a_tree_takes_the_kernel_without_columns():
    tb = tables("cbox_bunny", 16, 16)
    st = _abi.scene_stats(GpuScene(tb).h)
    assert st["n_blas"] > 0 or st["leaf_tris"] > 0
    tan = random_tangents(tb, ["texels"], seed=3)
    g1, g0 = GpuScene(tb, options={"logd_park": 1}), GpuScene(tb, options={"logd_park": 0})
    same_bits(run(g1, two_calls(4, 3), [tan]), run(g0, two_calls(4, 3), [tan]))
    i1 = _abi.logd_info(g1.h)
    assert (i1["launches"], i1["lean"]) == (2, 0), i1


def test_a_zero_albedo_under_a_tangent_still_takes_the_dual_number_kernel():
    tb = dict(tables("cbox", 24, 24))
    tex = tb["texels"].clone(); tex[1] = 0.0
    tb["texels"] = tex
    t = torch.zeros_like(tex); t[0:3] = 1.0
    calls = two_calls(8, 3)
    g1, gd = GpuScene(tb, options={"logd_park": 1}), GpuScene(tb, options={"logd": 0})
    a, b = run(g1, calls, [{"texels": t}]), run(gd, calls, [{"texels": t}])
    # the log-derivative estimator has no derivative for the zero channel: the gate hands the launch to the dual-number kernel, whose bits these are
    assert np.abs(b[0][1][0][:, 1]).max() > 0
    same_bits(a, b)
    i1, idn = _abi.logd_info(g1.h), _abi.logd_info(gd.h)
    assert (i1["launches"], i1["lean"]) == (2, 2), i1          # launched behind the gate, returned at once
    assert (idn["launches"], idn["lean"]) == (0, 0), idn


def test_an_lds_budget_too_small_for_the_columns_takes_the_kernel_without_columns():
    tb = tables("cbox", 24, 24)
    tan = random_tangents(tb, ["texels"], seed=7)
    g1 = GpuScene(tb, options={"logd_park": 1})
    a = run(g1, two_calls(8, 3), [tan])
    need = _abi.logd_info(g1.h)["lean_lds_bytes"]
    assert need > 0
    gs, gf = GpuScene(tb, options={"logd_park": 1, "lds_budget": need - 16}), GpuScene(tb, options={"logd_park": 1, "lds_budget": need})
    same_bits(run(gs, two_calls(8, 3), [tan]), a)
    same_bits(run(gf, two_calls(8, 3), [tan]), a)
    i_s, i_f = _abi.logd_info(gs.h), _abi.logd_info(gf.h)
    assert (i_s["launches"], i_s["lean"]) == (2, 0), i_s
    assert (i_f["launches"], i_f["lean"]) == (2, 2), i_f


def test_logd_info_rejects_null_arguments():
    import ctypes as C
    lib = _abi.load_hip()
    out = (C.c_int64 * 4)()
    assert lib.psdr_scene_logd_info(None, out) != 0 and b"null" in lib.psdr_last_error()
