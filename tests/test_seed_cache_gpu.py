"""Seed table of the scene handle (option seed_cache; csrc/psdr_kernels.h k_seed_fill / seed_table): the fused PathTracer renderC launches on a scene without a tree load
the seeded PCG32 state of their sample slots from a read-only table instead of running the two TEA mixes of Rng::seed, and apply the call's jump-ahead to what they loaded.

A seeded launch draws the numbers the unseeded launch draws, so wherever the unseeded launch is deterministic -- the pixels are STORED: samples per pixel divide 64,
`own` -- the images are the same BITS; where a pixel is added to by several waves (atomics) the two runs differ by the order of fp32 additions only, and the bound is
the one tests/test_logd_gpu.py uses for two launch forms of one estimator (rel-L2 < 2e-6).  Ray counters are equal everywhere.

Forward mode: no forward kernel has a seeded twin ("Seed table"), so the forward tests hold the results in place -- the same bits with the
option on and off, agreement with the dual-number kernel -- and say nothing about which kernel ran.

The published streams (tests/golden/rng_streams.npz: slots 7, 0 and 2^31 + 5) are not checked directly here: no draw of a PathTracer slot leaves the kernel, the table
pointer is not exposed, and slot 2^31 + 5 is out of reach of a launch of a few thousand slots.  The bit-equality tests below stand in for it: the unseeded kernels are
held to those streams by test_golden.py / test_gpu_parity.py, and an image that is bit-equal over every slot of a launch -- fresh, with a non-zero jump, on a second
rank's shard (slot ids that are not the launch-local index) and on a ragged tail -- needs every table entry to be the state Rng::seed computes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import psdr_cuda
from helpers import GpuScene, random_tangents, rel_l2
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def tables(name, w, h):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(name), False)
    sc.opts.width, sc.opts.height = w, h
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 0, 0, 0
    sc.configure()
    return sc.tables(0)


def path_opts(spp, depth=3, **kw):
    return _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=spp, **kw)


def info(g):
    return _abi.seed_cache_info(g.h)


def render(g, o):
    img = g.render_c(o)
    return img, g.counters()[0]


def retable(g, tb):
    """other tables (another film size) on the SAME handle"""
    g.tb = {k: (v.detach().cuda() if isinstance(v, torch.Tensor) else v) for k, v in tb.items()}
    g.set_guide(None)
    _abi.check(g.lib, g.lib.psdr_bvh_build(g.h, None))


def test_seeded_launches_return_the_same_bits_fresh_and_with_a_jump():
    tb = tables("cbox", 16, 16)
    g1, g0 = GpuScene(tb, options={"seed_cache": 1}), GpuScene(tb, options={"seed_cache": 0})
    o = path_opts(64)
    draws = _abi.draws_per_slot(o)
    o2 = path_opts(64, rng_offset=draws)          # the second call of a loop: every stream continues behind the first call's draws
    a1, r1 = render(g1, o)
    a0, r0 = render(g0, o)
    b1, s1 = render(g1, o2)                       # the table is reused: the jump is applied to cached seeds
    b0, s0 = render(g0, o2)
    assert a0.max() > 0 and not np.array_equal(a0, b0)
    assert np.array_equal(a1, a0) and np.array_equal(b1, b0)
    assert r1 == r0 and s1 == s0 and r0 > 0
    i1, i0 = info(g1), info(g0)
    assert (i1["fills"], i1["launches"], i1["slots"], i1["bytes"]) == (1, 2, 16 * 16 * 64, 16 * 16 * 64 * 16), i1
    assert (i0["fills"], i0["launches"], i0["slots"], i0["bytes"]) == (0, 0, 0, 0), i0


def test_forward_mode_log_derivative_launches():
    tb = tables("cbox", 16, 16)
    o = path_opts(64)
    tan = random_tangents(tb, ["texels"], seed=11)
    t3 = []
    for c in range(3):
        t = torch.zeros_like(tb["texels"]); t[c] = 1.0
        t3.append({"texels": t})
    g1, g0, gd = GpuScene(tb, options={"seed_cache": 1}), GpuScene(tb, options={"seed_cache": 0}), GpuScene(tb, options={"logd": 0})
    for tans in ([tan], t3):          # K = 1, K = 3
        img1, d1 = g1.render_d_fwd(o, tans)
        img0, d0 = g0.render_d_fwd(o, tans)
        imgd, dd = gd.render_d_fwd(o, tans)
        assert np.abs(d0).max() > 0
        assert np.array_equal(img1, img0) and np.array_equal(d1, d0)
        assert g1.counters()[0] == g0.counters()[0]
        # the dual-number kernel (not seeded): the bounds of tests/test_logd_gpu.py
        for img, d in ((img1, d1), (img0, d0)):
            assert rel_l2(img, imgd) < 2e-6, rel_l2(img, imgd)
            for k in range(len(tans)):
                assert np.abs(dd[k]).max() > 0 and rel_l2(d[k], dd[k]) < 2e-5, (k, rel_l2(d[k], dd[k]))


def test_a_key_change_refills_the_table():
    tb = tables("cbox", 16, 16)
    g1, g0 = GpuScene(tb, options={"seed_cache": 1}), GpuScene(tb, options={"seed_cache": 0})

    def pair(o):
        a1, r1 = render(g1, o)
        a0, r0 = render(g0, o)
        assert r1 == r0 and r0 > 0
        return a1, a0

    a1, a0 = pair(path_opts(64))
    assert np.array_equal(a1, a0) and info(g1)["fills"] == 1
    # 128 samples per pixel: two waves per pixel, atomics -- the order of the additions is free
    f1, f0 = pair(path_opts(128))
    print("spp 128 (atomics): rel-L2 seeded vs unseeded %.2e" % rel_l2(f1, f0))
    assert rel_l2(f1, f0) < 2e-6 and info(g1)["fills"] == 2 and info(g1)["slots"] == 16 * 16 * 128
    # a second rank's shard of those samples: spp_begin != 0, the slot ids are not the launch-local indices
    hi1, hi0 = pair(path_opts(128, spp_range=(64, 128)))
    assert np.array_equal(hi1, hi0) and info(g1)["fills"] == 3 and info(g1)["slots"] == 16 * 16 * 64
    lo1, lo0 = pair(path_opts(128, spp_range=(0, 64)))
    assert np.array_equal(lo1, lo0) and info(g1)["fills"] == 4
    assert not np.array_equal(lo1, hi1)
    # the two shards are the two halves of the unsharded image (global slot ids)
    print("shards vs unsharded: rel-L2 %.2e (seeded) %.2e (unseeded)" % (rel_l2(lo1 + hi1, f1), rel_l2(lo0 + hi0, f0)))
    assert rel_l2(lo1 + hi1, f1) < 2e-6
    # the same key again: no fill
    pair(path_opts(128, spp_range=(0, 64)))
    assert info(g1)["fills"] == 4
    # another film size on the same handle
    tb2 = tables("cbox", 24, 16)
    retable(g1, tb2); retable(g0, tb2)
    w1, w0 = pair(path_opts(64))
    assert w1.shape == (24 * 16, 3) and np.array_equal(w1, w0)
    assert info(g1)["fills"] == 5 and info(g1)["slots"] == 24 * 16 * 64 and info(g1)["launches"] == 6 and info(g0)["launches"] == 0


def test_ragged_tail():
    # 780 slots: not a multiple of the workgroup (256) nor of the wave (64); 16 pixels share a wave.  The table holds exactly 780 entries.
    tb = tables("cbox", 15, 13)
    g1, g0 = GpuScene(tb, options={"seed_cache": 1}), GpuScene(tb, options={"seed_cache": 0})
    o = path_opts(4)
    a1, r1 = render(g1, o)
    a0, r0 = render(g0, o)
    assert a0.max() > 0 and np.array_equal(a1, a0) and r1 == r0
    i = info(g1)
    assert (i["slots"], i["bytes"], i["fills"], i["launches"]) == (780, 780 * 16, 1, 1), i
    tan = random_tangents(tb, ["texels"], seed=5)
    img1, d1 = g1.render_d_fwd(o, [tan])
    img0, d0 = g0.render_d_fwd(o, [tan])
    assert np.abs(d0).max() > 0 and np.array_equal(img1, img0) and np.array_equal(d1, d0)


def test_launches_the_table_does_not_serve():
    tb = tables("cbox", 16, 16)
    o = path_opts(64)
    ref, rays = render(GpuScene(tb, options={"seed_cache": 0}), o)
    # above the cap: 16 384 slots > 2^10
    g = GpuScene(tb, options={"seed_cache_log2": 10})
    a, r = render(g, o)
    assert np.array_equal(a, ref) and r == rays
    assert (info(g)["fills"], info(g)["launches"], info(g)["bytes"]) == (0, 0, 0)
    # DirectIntegrator on the same scene
    od = _abi.make_opts(spp=64)
    g1, g0 = GpuScene(tb, options={"seed_cache": 1}), GpuScene(tb, options={"seed_cache": 0})
    d1, q1 = render(g1, od)
    d0, q0 = render(g0, od)
    assert d0.max() > 0 and np.array_equal(d1, d0) and q1 == q0
    assert (info(g1)["fills"], info(g1)["launches"]) == (0, 0)
    # a scene with a tree (1 024 slots: the fused kernel, pixels stored)
    tbb = tables("cbox_bunny", 16, 16)
    ob = path_opts(4)
    g1, g0 = GpuScene(tbb, options={"seed_cache": 1}), GpuScene(tbb, options={"seed_cache": 0})
    assert _abi.scene_stats(g1.h)["n_blas"] > 0 or _abi.scene_stats(g1.h)["leaf_tris"] > 0
    t1, p1 = render(g1, ob)
    t0, p0 = render(g0, ob)
    assert t0.max() > 0 and np.array_equal(t1, t0) and p1 == p0
    assert (info(g1)["fills"], info(g1)["launches"]) == (0, 0)


def test_seed_info_rejects_null_arguments():
    lib = _abi.load_hip()
    out = (C.c_int64 * 4)()
    assert lib.psdr_scene_seed_info(None, out) != 0 and b"null" in lib.psdr_last_error()
