"""Reverse mode's gradient scatter, ENTRY BY ENTRY, across the layouts psdr_render_d_rev picks per launch (csrc/psdr_hip.hip make_sink_layout,
csrc/psdr_kernels.h DeviceSink / RegPrivSink / defer_row / PrimaryEdgeSink, render_rev): the LDS cache and its texel, radiance and hot-row arms, its
copies (sink_rep), the lane-private emitter rows (LDS or registers), the deferred row adjoints (rev_sorted), the primary-edge table copies.  None of it
exists in the host build of the estimators, and a defect in one arm moves a few entries only -- under any whole-table measure.

Every case asserts through psdr_scene_rev_layout (psdr_cuda._abi.rev_layout) that its launch took the arm it is named after, then checks every gradient
table it asks for in two ways, with S = the sum of the magnitudes of an entry's fp32 pieces from the double-precision host run (hostcheck_render_rev_f64):
  (a) layout invariance: two handles that differ only in a scatter option run the same samples through the same kernel instance -- the same rays,
      and every entry equal up to the order of the float adds,  |a - b| <= C_SAME eps32 S + FLOOR max S.  No outlier: no sample can flip here.
  (b) against the f64 reference: |gpu - sum| <= C_REF eps32 S + FLOOR max S for all but a bounded number of entries (the GPU kernels and the host are
      different instruction streams: a 1-ulp difference flips an isolated sample's branch); the excluded entries' signed error must look like random flips.
Not covered yet (follow-up work): scenes with more than 85 emitters (the radiance cache's global-atomics arm); emitter 0 with one or more than two
triangles (every scene here has a two-triangle area light); the adjoint kernel on records a psdr_render_c(PSDR_FLAG_KEEP_RECORDS) kept (rev_layout launch
"kept_records", covered by whole-table tests in test_reverse_mode.py) and the DirectIntegrator's probe launch on two-level scenes ("probe": only from
large launches); the split launch with the traced-wavefront value sweep ("split_wavefront": from 2^16 slots)."""
import numpy as np
import pytest
import torch

from helpers import GpuScene, entry_errors, excluded_entries_unbiased, host_render_rev_f64, load_scene, outlier_share
from psdr_cuda import _abi

EPS32 = float(np.finfo(np.float32).eps)
PATH, DIRECT = _abi.INTEGRATOR_PATH, _abi.INTEGRATOR_DIRECT
ALL = ["texels", "emitter_rad", "tri_info", "cam_to_world"]

# (a) measured on the MI355X: at most 33.5 eps32 S (cbox_bunny texels, the 2048-word LDS cache against global atomics: 29.1 and 33.5 in two runs, the
#     order of the atomics varies); cbox texels 16.3; the other arms 0.2 - 9.4 (primary-edge replicas against shards 9.4, sort order 3.9, copies /
#     private rows / deferral <= 3.8).  The cause: the order of the fp32 adds, LDS and global atomics of the workgroups.
C_SAME = 64.0
# (b) GPU against the host: different instruction streams, and an fp32 piece that is itself a small difference (an edge-on triangle's derivative) is off by
#     many of its own ulps -- hence the floor against the table's largest S.  With these two numbers the scenes without a tree have NO outlier entry.
C_REF = 512.0
FLOOR = 1e-7
# (b) no outlier entry may be off by more than this share of its own magnitude sum S.  Measured on the MI355X: at most 1.6e-3 (bunny triangle rows: a
#     flipped sample is one piece of a row many samples reach); an entry the sink drops or misplaces is off by |sum|, for one-signed pieces all of S (1.0)
MAX_SHARE = 0.01


def _tables(scene, res, spp, sppe=0, texels=None):
    sc, _ = load_scene(scene, res=res, spp=spp, sppe=sppe)
    tb = dict(sc.tables(0))
    if texels is not None:
        # words behind the pool that no BSDF reads: the image does not change, num_texels does (the texel cache holds <= 2048 words)
        n = tb["texels"].numel()
        assert n < texels, (scene, n)
        tb["texels"] = torch.cat([tb["texels"], torch.zeros(texels - n, dtype=tb["texels"].dtype, device=tb["texels"].device)]).contiguous()
    return tb


_SLOT_CHANNELS = {_abi.BSDF_DIFFUSE: (3,), _abi.BSDF_ROUGHCONDUCTOR: (3, 1, 1, 3, 3)}


def _live_texels_last(tb, total, live_end):
    """The texel pool as `total` words whose LAST word is live: unused zeros in front, then the pool rotated so that its blocks up to `live_end` (one past
    the last texel any sample reaches) come last; the BSDF records' texel offsets follow.  A cache that flushes one word short then loses a live texel."""
    pool = tb["texels"]
    n, k = pool.numel(), live_end
    assert n <= total and tb.get("env_emitter", -1) < 0, (n, total)
    rec = tb["bsdf_rec"].detach().cpu().clone()
    for r in rec.tolist():
        for slot, ch in enumerate(_SLOT_CHANNELS[r[0]]):
            o, w, h = r[1 + 3 * slot: 4 + 3 * slot]
            assert not (o < k < o + w * h * ch), ("the cut falls inside a texture", r, k)
    pad = total - n
    for b in range(rec.shape[0]):
        for slot in range(5):
            o = int(rec[b, 1 + 3 * slot])
            rec[b, 1 + 3 * slot] = pad + (o - k if o >= k else o + n - k)
    out = dict(tb)
    out["texels"] = torch.cat([torch.zeros(pad, dtype=pool.dtype, device=pool.device), pool[k:], pool[:k]]).contiguous()
    out["bsdf_rec"] = rec.to(tb["bsdf_rec"].device).contiguous()
    return out


def _adj(res, seed=11):
    return np.random.default_rng(seed).random((res * res, 3)).astype(np.float32)


def _gpu(tb, o, adj, names, options=None):
    g = GpuScene(tb, options=options)
    _, grads = g.render_d_rev(o, adj, want=names, with_image=False)
    out = (grads, g.counters()[0], _abi.rev_layout(g.h))
    g.close()
    return out


def _same(label, ga, gb, ref, names):
    """(a): every entry of two layouts of the same samples; returns the worst |a - b| / (eps32 S)."""
    worst = 0.0
    for n in names:
        a, b, (s, sa) = ga[n], gb[n], ref[n]
        assert a.shape == b.shape == s.shape, (label, n)
        r, bad = entry_errors(a, (b, sa), C_SAME, FLOOR)
        c = float((np.abs(a.astype(np.float64) - b) / (EPS32 * sa + 1e-30))[sa > 0].max(initial=0.0))
        assert (a[sa == 0] == 0).all() and (b[sa == 0] == 0).all(), (label, n, "an entry no piece reaches is not zero")
        worst = max(worst, c)
        print("  (a) %-34s %-13s max |a-b| = %6.1f eps32 S, entries above the bound: %d" % (label, n, c, int(bad.sum())))
        assert not bad.any(), (label, n, int(bad.sum()), r)
    return worst


def _ref(label, g, ref, names, k_max):
    """(b): every entry against the double-precision host sum, at most k_max outliers whose signed error nets out."""
    total = 0
    for n in names:
        s, sa = ref[n]
        r, bad = entry_errors(g[n], ref[n], C_REF, FLOOR)
        inb = ~bad.reshape(sa.shape)
        c = float((np.abs(g[n].astype(np.float64) - s) / (EPS32 * sa + 1e-30))[(sa > 0) & inb].max(initial=0.0))
        total += int(bad.sum())
        print("  (b) %-34s %-13s max |gpu-ref| = %7.1f eps32 S (inliers), outliers: %d of %d, largest outlier share of its S %.2e" % (
            label, n, c, int(bad.sum()), int((sa > 0).sum()), outlier_share(g[n], ref[n], bad)))
        excluded_entries_unbiased(g[n], ref[n], bad, "%s %s" % (label, n), max_share=MAX_SHARE)
    assert total <= k_max, (label, total, k_max)
    return total


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the LDS cache on a scene without a tree (every row cached, slot = triangle): copies, lane-private rows in LDS (DirectIntegrator) or registers
# (PathTracer geometry kernels), deferred rows with and without overflow, HBM path records
CAMERA_CASES = [
    # id, scene, integrator kwargs, base options, {variant id: options}, expected base layout, k_max of (b)
    ("cbox_direct", "cbox", dict(integrator=DIRECT, bsdf_samples=1, light_samples=1), {},
     {"rep1": dict(sink_rep=1), "rep2": dict(sink_rep=2), "nopriv": dict(sink_private=0)},
     dict(rep=4, priv_rows=2, priv_regs=0, pend_rows=0, hot_identity=1, rad_n=3, launch="fused"), 0),
    ("cbox_path3", "cbox", dict(integrator=PATH, max_depth=3), {},
     {"unsorted": dict(rev_sorted=0), "rep1": dict(sink_rep=1), "nopriv": dict(sink_private=0)},
     dict(priv_rows=2, priv_regs=1, pend_rows=3, hot_identity=1, deep_rec=0, launch="fused"), 0),
    # depth 6: the LDS budget leaves 2 deferred columns per lane (< 4), rows beyond them go out on the spot
    ("cbox_path6_overflow", "cbox", dict(integrator=PATH, max_depth=6), {},
     {"unsorted": dict(rev_sorted=0), "rep1": dict(sink_rep=1)},
     dict(priv_rows=2, priv_regs=1, pend_rows=2, deep_rec=0, launch="fused"), 0),
    # 34 texels (rough-conductor textures in the cache); the rough-conductor PathTracer kernel keeps its private rows in LDS and has room for one deferred
    # column.  k_max = 2x the 16 outlier entries measured (9 rows, 7 camera
    # words): GGX samples at 8 spp whose branch flips between the GPU and the host (test_gpu_parity.py says the same of renderC); texels: no outlier
    ("cbox_rough_path3", "cbox_rough", dict(integrator=PATH, max_depth=3), {},
     {"unsorted": dict(rev_sorted=0), "rep1": dict(sink_rep=1)},
     dict(tex_n=34, priv_rows=2, priv_regs=0, pend_rows=1, launch="fused"), 32),
    ("cbox_path10_hbm_records", "cbox", dict(integrator=PATH, max_depth=10), {},
     {"unsorted": dict(rev_sorted=0), "rep1": dict(sink_rep=1), "nopriv": dict(sink_private=0)},
     dict(priv_rows=2, priv_regs=1, pend_rows=4, deep_rec=1, launch="fused"), 0),
    ("cbox_path3_split", "cbox", dict(integrator=PATH, max_depth=3), dict(rev_split=1),
     {"unsorted": dict(rev_split=1, rev_sorted=0), "rep1": dict(rev_split=1, sink_rep=1)},
     dict(priv_rows=2, priv_regs=1, launch="split"), 0),
    # tree scenes: the 200 hot rows (emitter triangles, then by area), the rest through global atomics; a cache of 200 rows leaves no room for a copy (rep 1).
    # k_max of (b) = 2x the outlier entries measured on the MI355X (isolated samples whose branch flips between the GPU and the host): bunny_path3 27
    # (21 rows, 4 camera words -- every flipped sample moves all 16 -- 1 texel, 1 radiance), bunny_direct 31, the device-built tree 5
    ("bunny_path3", "cbox_bunny", dict(integrator=PATH, max_depth=3), {},
     {"unsorted": dict(rev_sorted=0), "nopriv": dict(sink_private=0)},
     dict(hot_identity=0, hot_rows=200, rep=1, priv_rows=2, priv_regs=1, pend_rows=2, launch="fused"), 54),
    # the DirectIntegrator's private rows live in LDS: behind the staged tree and the 200-row cache they would cost a resident workgroup, render_rev drops
    # them (priv_rows 0 with sink_private 1; a forced lds_budget of 32 - 96 KB leaves this unchanged)
    ("bunny_direct_private_dropped", "cbox_bunny", dict(integrator=DIRECT, bsdf_samples=1, light_samples=1), {},
     {},                                                                 # (no scatter option changes this layout: (b) only)
     dict(hot_identity=0, hot_rows=200, priv_rows=0, priv_regs=0, pend_rows=0), 62),
    ("bunny_path3_device_tree", "cbox_bunny", dict(integrator=PATH, max_depth=3), dict(bvh_build=1),
     {"nopriv": dict(bvh_build=1, sink_private=0), "unsorted": dict(bvh_build=1, rev_sorted=0)},
     dict(hot_identity=0, hot_rows=200, priv_rows=2, pend_rows=1), 10),
    # the split launch (value kernel + adjoint kernel) on the tree scene; k_max = 2x the 27 outlier entries measured (the flips of bunny_path3)
    ("bunny_path3_split", "cbox_bunny", dict(integrator=PATH, max_depth=3), dict(rev_split=1),
     {"unsorted": dict(rev_split=1, rev_sorted=0), "nopriv": dict(rev_split=1, sink_private=0)},
     dict(hot_identity=0, hot_rows=200, priv_rows=2, priv_regs=1, launch="split"), 54),
    # the environment map as emitter 0: no private rows, the map's record cached.  k_max = 2x the 12 outlier entries measured (all triangle rows: flipped
    # shadow tests against the bunny; texels, camera and map record none)
    ("bunny_env_direct", "bunny_env", dict(integrator=DIRECT, bsdf_samples=1, light_samples=1), {},
     {"nopriv": dict(sink_private=0)},
     dict(priv_rows=0, env_n=_abi.ENV_WORDS), 24),
]


def _names(tb):
    if tb.get("env_f") is not None and tb.get("env_emitter", -1) >= 0:
        return ["texels", "tri_info", "cam_to_world", "env_f"]           # (no area light: the radiance table gets nothing)
    return list(ALL)


def _check_layout(label, lay, want, tb):
    for k, v in want.items():
        if v is not None:
            assert lay[k] == v, (label, k, lay[k], v, lay)
    if lay["hot_identity"]:
        assert lay["hot_rows"] == tb["num_tris"], (label, lay)
    else:
        assert 0 < lay["hot_rows"] < tb["num_tris"], (label, lay)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,scene,kw,base,variants,want,k_max", CAMERA_CASES, ids=[c[0] for c in CAMERA_CASES])
def test_camera_term_per_entry(cid, scene, kw, base, variants, want, k_max):
    res, spp = 32, 8
    tb = _tables(scene, res, spp)
    names = _names(tb)
    o = _abi.make_opts(spp=spp, rng_offset=(2, 3, 4), **kw)
    adj = _adj(res)
    _, ref = host_render_rev_f64(tb, o, adj, want=names)
    g0, rays0, lay0 = _gpu(tb, o, adj, names, base)
    print("\n%s: layout %s" % (cid, lay0))
    _check_layout(cid, lay0, want, tb)
    for n in names:
        assert np.abs(g0[n]).max() > 0, (cid, n)
    _ref(cid, g0, ref, names, k_max)
    for vid, opts in variants.items():
        g1, rays1, lay1 = _gpu(tb, o, adj, names, opts)
        print("%s/%s: layout %s" % (cid, vid, lay1))
        # the variant took the other arm
        if "sink_rep" in opts:
            assert lay1["rep"] == opts["sink_rep"] and lay0["rep"] > opts["sink_rep"], (cid, vid, lay0["rep"], lay1["rep"])
        if opts.get("sink_private") == 0:
            assert lay1["priv_rows"] == 0, (cid, vid)
        if opts.get("rev_sorted") == 0:
            assert lay1["pend_rows"] == 0 and lay0["pend_rows"] > 0, (cid, vid)
        assert rays1 == rays0, (cid, vid, rays1, rays0)
        _same("%s/%s" % (cid, vid), g1, g0, ref, names)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the texel cache holds at most 2048 words: exactly 2048 (cached) against 2049 (global atomics), the same samples.  The pool is laid out so that the
# last word of the cache is a live texel (_live_texels_last: the 2049-word table is the 2048-word one behind one more unused word).  On the tree scene the
# 2048-word cache leaves room for fewer than 200 hot rows (the word cap, not the row cap)
@pytest.mark.gpu
@pytest.mark.parametrize("scene,kw", [("cbox", dict(integrator=PATH, max_depth=3)), ("cbox_bunny", dict(integrator=PATH, max_depth=3))], ids=["cbox", "bunny"])
def test_texel_cache_threshold_per_entry(scene, kw):
    res, spp = 32, 8
    o = _abi.make_opts(spp=spp, rng_offset=(2, 3, 4), **kw)
    adj = _adj(res)
    tb = _tables(scene, res, spp)
    _, base = host_render_rev_f64(tb, o, adj, want=["texels"])
    live_end = int(np.nonzero(base["texels"][1])[0].max()) + 1
    tb_in, tb_out = _live_texels_last(tb, 2048, live_end), _live_texels_last(tb, 2049, live_end)
    _, ref_out = host_render_rev_f64(tb_out, o, adj, want=ALL)
    _, ref = host_render_rev_f64(tb_in, o, adj, want=ALL)
    # the last cached word carries a real share of the texel gradient (the third albedo's blue channel)
    assert ref["texels"][1][-1] > 0.02 * ref["texels"][1].sum(), ref["texels"][1][-1] / ref["texels"][1].sum()
    assert np.array_equal(ref_out["texels"][0][1:], ref["texels"][0]) and ref_out["texels"][1][0] == 0
    for n in ALL[1:]:
        assert np.array_equal(ref_out[n][0], ref[n][0]), n          # the same samples
    g_in, rays_in, lay_in = _gpu(tb_in, o, adj, ALL)
    g_out, rays_out, lay_out = _gpu(tb_out, o, adj, ALL)
    print("\n%s texels 2048: %s\n%s texels 2049: %s" % (scene, lay_in, scene, lay_out))
    assert lay_in["tex_n"] == 2048 and lay_out["tex_n"] == 0
    if scene == "cbox_bunny":
        # 6144 words - 16 (camera) - 2048 (texels) - 3 (radiance) = 4077 words: 169 rows of TRI_STRIDE words, below the 200 of the tree build
        assert lay_in["hot_rows"] == (6144 - 16 - 2048 - 3) // _abi.TRI_STRIDE < min(200, lay_in["tree_hot_rows"]), lay_in
        assert lay_out["hot_rows"] == lay_out["tree_hot_rows"] == 200, lay_out
    assert rays_in == rays_out
    assert g_out["texels"][0] == 0
    g_out["texels"] = g_out["texels"][1:]
    _same("%s tex2048/2049" % scene, g_in, g_out, ref, ALL)
    # k_max: cbox none measured; cbox_bunny 27 outlier entries measured in either run (21 rows, 4 camera words, 1 texel, 1 radiance: the flips of bunny_path3)
    _ref("%s tex2048" % scene, g_in, ref, ALL, 0 if scene == "cbox" else 54)
    _ref("%s tex2049" % scene, g_out, ref, ALL, 0 if scene == "cbox" else 54)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# a partial tail wave (19 x 19 x 3 = 1 083 slots) per entry
@pytest.mark.gpu
def test_partial_tail_wave_per_entry():
    res, spp = 19, 3
    tb = _tables("cbox", res, spp)
    o = _abi.make_opts(spp=spp, rng_offset=(2, 3, 4), integrator=PATH, max_depth=3)
    adj = _adj(res, 7)
    _, ref = host_render_rev_f64(tb, o, adj, want=ALL)
    g, _, lay = _gpu(tb, o, adj, ALL)
    print("\ntail wave: layout %s" % lay)
    assert lay["launch"] == "fused" and lay["pend_rows"] == 3
    _ref("tail wave", g, ref, ALL, 0)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# primary edges: the table is replicated from 2^18 edge slots (128^2 x 16); the same samples as two sppe_range shards of 2^17 (one copy each), the
# natural against the pixel-sorted slot order, and the f64 host run
@pytest.mark.gpu
def test_primary_edge_replicas_per_entry():
    res, sppe = 128, 16
    tb = _tables("cbox_occluder", res, 0, sppe=sppe)
    adj = _adj(res, 5)
    kw = dict(spp=0, sppe=sppe, integrator=DIRECT, bsdf_samples=1, light_samples=1, rng_offset=(2, 3, 4))
    names = ["prim_edge"]
    _, ref = host_render_rev_f64(tb, _abi.make_opts(**kw), adj, want=names)
    full, rays_full, lay = _gpu(tb, _abi.make_opts(**kw), adj, names)
    print("\nprimary edges, one launch: %s" % lay)
    assert lay["pe_reps"] > 1 and lay["pe_sorted"] == 1 and lay["launch"] == "none", lay
    shards, rays_sh = np.zeros_like(full["prim_edge"]), 0
    for rng in ((0, 8), (8, 16)):
        g, r, l = _gpu(tb, _abi.make_opts(sppe_range=rng, **kw), adj, names)
        assert l["pe_reps"] == 1, l
        shards += g["prim_edge"]; rays_sh += r
    unsorted, rays_u, lay_u = _gpu(tb, _abi.make_opts(**kw), adj, names, dict(sort_edges=0))
    assert lay_u["pe_sorted"] == 0 and lay_u["pe_reps"] == lay["pe_reps"], lay_u
    assert rays_sh == rays_full == rays_u
    _same("prim_edge replicas/shards", full, {"prim_edge": shards}, ref, names)
    _same("prim_edge sorted/natural", full, unsorted, ref, names)
    _ref("prim_edge replicas", full, ref, names, 0)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the checks themselves, on the host: the fp32 host sink stands in for a perfect GPU; with one small live entry dropped (texel 33 of cbox_rough carries
# 6e-4 of its table's magnitude) check (b) must fail even with the outlier budget of the case, and check (a) against the undamaged run as well
def test_the_checks_catch_a_dropped_entry():
    from helpers import host_render_rev
    res, spp = 32, 8
    tb = _tables("cbox_rough", res, spp)
    o = _abi.make_opts(spp=spp, rng_offset=(2, 3, 4), integrator=PATH, max_depth=3)
    adj = _adj(res)
    _, ref = host_render_rev_f64(tb, o, adj, want=ALL)
    _, g = host_render_rev(tb, o, adj, want=ALL)
    _ref("host", g, ref, ALL, 0)
    bad = {k: v.copy() for k, v in g.items()}
    assert 0 < ref["texels"][1][-1] < 1e-3 * ref["texels"][1].sum()
    bad["texels"][-1] = 0.0
    with pytest.raises(AssertionError, match="own magnitude sum"):
        _ref("host, last texel dropped", bad, ref, ALL, 32)
    with pytest.raises(AssertionError):
        _same("host, last texel dropped", bad, g, ref, ALL)
