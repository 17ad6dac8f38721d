"""The lean PathTracer twins of flag set 8 (option path_lean; csrc/psdr_path_lean.h, psdr_path_lean.hip, psdr_logd_lean.hip): renderC and the K = 1 forward mode on
albedo texels of a plain diffuse scene without a tree, where every wave of the launch sits on one pixel (64 samples per pixel in the call) and every primitive is an
axis-aligned rectangle.  The twins evaluate the estimator of the kernels they replace with the same draws and the same arithmetic forms, so every comparison with
path_lean = 0 (exactly the launches of before the twins) is bit for bit: image, derivative image, ray counter.  psdr_scene_path_lean_info says which kernel a launch
took -- the selection rule itself is tests/test_path_lean_plan_host.py's.  One case runs against the CPU oracle at the tolerance tests/test_gpu_parity.py uses."""
import functools

import numpy as np
import pytest
import torch

import oracle
import psdr_cuda
import texture_cases as tc
from helpers import GpuScene, rel_l2
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def tables(name, w, h, rotate_occluder=False):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(name), False)
    sc.opts.width, sc.opts.height = w, h
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 0, 0, 0
    if rotate_occluder:
        # the occluder quad turned 25 degrees about the z axis through its own centre: a parallelogram no slab form holds
        m = sc.param_map["Mesh[id=occluder]"]
        T = m._to_world_raw.detach().cpu().numpy().astype(np.float64).reshape(4, 4)
        a = np.deg2rad(25.0)
        R, to, back = np.eye(4), np.eye(4), np.eye(4)
        R[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        to[:3, 3], back[:3, 3] = -T[:3, 3], T[:3, 3]
        m._to_world_raw = torch.as_tensor(back @ R @ to @ T, dtype=torch.float32, device=m._to_world_raw.device).reshape(m._to_world_raw.shape)
    sc.configure()
    return sc.tables(0)


def two_calls(spp, depth, hide=False):
    o = _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=spp, hide_emitters=hide)
    return o, _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=spp, hide_emitters=hide, rng_offset=_abi.draws_per_slot(o))


def one_channel(tb, c=1):
    t = torch.zeros_like(tb["texels"]); t[c] = 1.0
    return {"texels": t}


def all_channels(tb):
    t = torch.zeros_like(tb["texels"]); t[0:3] = torch.tensor([1.0, -0.5, 0.25])
    return {"texels": t}


def run(g, calls, tan):
    """per call: renderC image and rays, then K = 1 forward image, derivative image and rays"""
    out = []
    for o in calls:
        c = g.render_c(o)
        rc = g.counters()[0]
        img, d = g.render_d_fwd(o, [tan])
        out.append((c, rc, img, d, g.counters()[0]))
    return out


def same_bits(a, b):
    for (ca, rca, ia, da, ra), (cb, rcb, ib, db, rb) in zip(a, b):
        assert np.isfinite(ca).all() and np.isfinite(ia).all() and np.isfinite(da).all()
        assert ca.max() > 0 and np.abs(da).max() > 0
        assert np.array_equal(ca, cb), np.abs(ca - cb).max()
        assert np.array_equal(ia, ib), np.abs(ia - ib).max()
        assert np.array_equal(da, db), np.abs(np.asarray(da) - np.asarray(db)).max()
        assert rca == rcb and ra == rb and rca > 0 and ra > 0
    assert not np.array_equal(a[0][0], a[1][0])          # the second call drew other numbers


def forms(g):
    i = _abi.path_lean_info(g.h)
    return i["render_c"], i["logd"], i["render_c_fallback"], i["logd_fallback"]


# w, h, spp, the twins run: 64 samples per pixel = one wave per pixel; 128: two waves per pixel; 5 x 3: 960 slots, a partial last workgroup with whole waves absent;
# 32 and 96: several pixels per wave / a pixel across waves
SHAPES = [(8, 8, 64, True), (8, 8, 128, False), (5, 3, 64, True), (8, 8, 32, False), (8, 8, 96, False)]


@pytest.mark.parametrize("w,h,spp,twin", SHAPES)
def test_the_twins_return_the_bits_of_the_launches_they_replace(w, h, spp, twin):
    tb = tables("cbox", w, h)
    tan = one_channel(tb)
    for depth, hide in [(1, False), (3, False), (3, True), (5, False), (5, True)]:
        g1, g0 = GpuScene(tb, options={"path_lean": 1}), GpuScene(tb, options={"path_lean": 0})
        same_bits(run(g1, two_calls(spp, depth, hide), tan), run(g0, two_calls(spp, depth, hide), tan))
        assert forms(g1) == ((2, 2, 0, 0) if twin else (0, 0, 2, 2)), (depth, hide, forms(g1))
        assert forms(g0) == (0, 0, 2, 2), forms(g0)          # switched off: every launch is one the rule left alone
        l1, l0 = _abi.logd_info(g1.h), _abi.logd_info(g0.h)
        assert (l1["launches"], l1["lean"]) == (l0["launches"], l0["lean"]) == (2, 2)          # either way a lean launch of the log-derivative kernel
        g1.close(); g0.close()


def test_one_albedo_channel_and_all_three_under_the_tangent():
    tb = tables("cbox", 8, 8)
    for tan in (one_channel(tb, 0), one_channel(tb, 2), all_channels(tb), {"texels": (torch.rand(tb["texels"].shape, generator=torch.Generator().manual_seed(3)) - 0.5).float()}):
        g1, g0 = GpuScene(tb, options={"path_lean": 1}), GpuScene(tb, options={"path_lean": 0})
        a, b = run(g1, two_calls(64, 3), tan), run(g0, two_calls(64, 3), tan)
        same_bits(a, b)
        assert forms(g1) == (2, 2, 0, 0)
        # the derivative is not one plane copied: the channels the tangent leaves alone stay zero where only one moves
        nz = [bool(np.abs(a[0][3][0][:, c]).max() > 0) for c in range(3)]
        assert any(nz)


def test_a_forced_small_chunk_and_the_seed_table_on_and_off():
    tb = tables("cbox", 8, 8)
    tan = all_channels(tb)
    ref = run(GpuScene(tb, options={"path_lean": 0}), two_calls(64, 3), tan)
    for options, seeded in [({"chunk_log2": 8}, True), ({"seed_cache": 0}, False), ({"seed_cache": 1}, True), ({"chunk_log2": 7, "seed_cache": 0}, False)]:
        g = GpuScene(tb, options=dict(options, path_lean=1))
        same_bits(run(g, two_calls(64, 3), tan), ref)
        assert forms(g) == (2, 2, 0, 0), (options, forms(g))          # the fused camera launches are not chunked: the option leaves their form alone
        s, l = _abi.seed_cache_info(g.h), _abi.logd_info(g.h)
        assert (s["launches"], l["lean_seeded"]) == ((4, 2) if seeded else (0, 0)), (options, s, l)
        assert s["fills"] == (1 if seeded else 0)          # one table serves renderC and renderD of both calls


def test_a_budget_too_small_for_the_columns_leaves_the_launch_to_the_other_kernels():
    tb = tables("cbox", 8, 8)
    tan = one_channel(tb)
    g1 = GpuScene(tb, options={"path_lean": 1})
    ref = run(g1, two_calls(64, 3), tan)
    need = _abi.logd_info(g1.h)["lean_lds_bytes"]
    assert 0 < 6 * need <= 160 * 1024 and forms(g1) == (2, 2, 0, 0)
    gs, gf = GpuScene(tb, options={"path_lean": 1, "lds_budget": need - 16}), GpuScene(tb, options={"path_lean": 1, "lds_budget": need})
    same_bits(run(gs, two_calls(64, 3), tan), ref)
    same_bits(run(gf, two_calls(64, 3), tan), ref)
    assert forms(gf) == (2, 2, 0, 0), forms(gf)
    assert forms(gs) == (2, 0, 0, 2), forms(gs)          # renderC parks nothing and keeps its twin; the log-derivative launch falls back
    assert _abi.logd_info(gs.h)["launches"] == 2


def both_ways(tb, tan, spp=64, depth=3):
    g1, g0 = GpuScene(tb, options={"path_lean": 1}), GpuScene(tb, options={"path_lean": 0})
    a, b = run(g1, two_calls(spp, depth), tan), run(g0, two_calls(spp, depth), tan)
    same_bits(a, b)
    return g1, g0, a


def test_a_primitive_no_slab_form_holds_keeps_the_kernels_with_the_plane_form_loop():
    tb = tables("cbox_occluder", 8, 8, True)
    n = tb["tri_info"].reshape(tb["num_tris"], -1)[:, 18:21]
    assert int(((n.abs() > 1e-3).sum(1) > 1).sum()) == 2          # the occluder's two triangles are the tilted ones
    g1, g0, _ = both_ways(tb, one_channel(tb))
    assert forms(g1) == (0, 0, 2, 2) and forms(g0) == (0, 0, 2, 2), forms(g1)
    assert _abi.scene_stats(g1.h)["n_blas"] == 0


@pytest.mark.parametrize("fmap", ["2x2", "6x5"])
def test_a_bitmap_albedo_goes_through_the_twins_one_bilinear_lookup(fmap):
    tb = tc.scene_tables("tiny", fmap, res=8)
    assert tc.MAPS[fmap][:2] in [(w, h) for _, _, _, w, h, c in tc.bitmap_slots(tb) if c == 3] and tc.staged(tb)
    tan = {"texels": (torch.rand(tb["texels"].shape, generator=torch.Generator().manual_seed(9)) * 0.5 + 0.25).float()}
    g1, g0, a = both_ways(tb, tan)
    assert np.abs(a[0][3][0]).max() > 0
    # the twins keep the general lookup -- once per vertex -- and the launch-form rule does not read the maps: renderC parks nothing and takes its twin; the K = 1
    # twin runs where the staged scene (the value pool and three tangent pools of the map among it) leaves its 22 columns room in a sixth of the CU's LDS
    l0 = _abi.logd_info(g0.h)
    assert l0["lean"] == 2, l0          # (the 19 columns of k_camera_logd_lean fit either map: its bytes tell the staged scene's)
    scene = l0["lean_lds_bytes"] - 19 * 1024
    fits = scene + 22 * 1024 <= 160 * 1024 // 6
    print("%s: staged scene %d bytes, the K = 1 twin %s" % (fmap, scene, "runs" if fits else "does not fit"))
    assert forms(g1) == ((2, 2, 0, 0) if fits else (2, 0, 0, 2)), forms(g1)
    if fmap == "2x2":
        assert fits


def test_a_zero_albedo_under_the_tangent_leaves_the_work_to_the_dual_number_kernel():
    tb = dict(tables("cbox", 8, 8))
    tex = tb["texels"].clone(); tex[1] = 0.0
    tb["texels"] = tex
    t = torch.zeros_like(tex); t[0:3] = 1.0
    g1, g0, a = both_ways(tb, {"texels": t})
    gd = GpuScene(tb, options={"logd": 0})
    same_bits(a, run(gd, two_calls(64, 3), {"texels": t}))
    assert np.abs(a[0][3][0][:, 1]).max() > 0          # the zero channel's derivative: only the dual-number kernel has one
    assert forms(g1) == (2, 2, 0, 0)          # launched behind the gate, returned at once
    assert forms(gd) == (2, 0, 0, 0)


def test_the_twins_against_the_cpu_oracle():
    tb = tables("cbox", 16, 16)
    o = _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=3, spp=64)
    tan = one_channel(tb, 0)
    g = GpuScene(tb, options={"path_lean": 1})
    c = g.render_c(o)
    img, d = g.render_d_fwd(o, [tan])
    assert forms(g) == (1, 1, 0, 0)
    ref_c = oracle.render(tb, o)
    ref_img, ref_d = oracle.render(tb, o, mode=1, tangents=tan)
    print("renderC %.3e, renderD image %.3e, d image / d albedo %.3e" % (rel_l2(c, ref_c), rel_l2(img, ref_img), rel_l2(d[0], ref_d)))
    assert rel_l2(c, ref_c) < 1e-4 and rel_l2(img, ref_img) < 1e-4
    assert rel_l2(d[0], ref_d) < 1e-4, rel_l2(d[0], ref_d)


def test_path_lean_info_rejects_null_arguments():
    import ctypes as C
    lib = _abi.load_hip()
    out = (C.c_int64 * 4)()
    assert lib.psdr_scene_path_lean_info(None, out) != 0 and b"null" in lib.psdr_last_error()
