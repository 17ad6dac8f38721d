"""The launch planning of csrc/psdr_plan.h -- grids, LDS plans, launch forms: pure host functions -- run by tests/hostcheck/hostcheck_plan.cpp over hand-filled
scene handles.  No GPU and no sanitizer.  Every expected value below is worked out by hand from the rules as the launch drivers stated them before they moved
into that header (the arithmetic stands beside each case); the LDS-fit decisions are recomputed here from the byte formulas of csrc/psdr_host.h
(sink_bytes_base, sink_reserve_pending), never taken from the function under test."""
import ctypes as C

import pytest

import hostlibs
from psdr_cuda import _abi

K = 1024
BLOCK, NODE, HIT_ROW = 256, 64, 64          # kBlock; bytes of a staged node / of a kernel-argument primitive's hit row
CACHE_WORDS, PRIV_WORDS, PEND_WORDS, REC_WORDS = 6144, 29, 10, 8          # kSinkCacheWords, kPrivWords, kPendWords, kPathRecWords
FL_ROUGH, FL_FOREST, FL_TINY = 2, 4, 8
G_TEX, G_RAD, G_TRI, G_CAM, G_ENV = 1, 2, 4, 8, 16


class PlanHandle(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "n_tiny", "n_blas", "num_nodes", "num_btris", "bvh_depth", "num_nodes4", "num_tris", "num_meshes", "num_bsdfs", "num_emitters", "emitter_tri0", "emitter_tris",
        "num_texels", "has_rough", "env_emitter", "lds_budget", "lds_limit", "hot_rows", "hot_identity", "sink_rep", "sink_private", "rev_split", "rev_sorted",
        "own_pixels", "chunk_log2", "width", "height")]


def handle(**kw):
    d = dict(num_meshes=6, num_bsdfs=3, num_emitters=1, emitter_tri0=0, emitter_tris=2, env_emitter=-1, lds_limit=160 * K, sink_rep=4, sink_private=1, rev_split=-1,
             rev_sorted=1, own_pixels=1, width=64, height=64)
    d.update(kw)
    return PlanHandle(**d)


def no_tree(**kw):          # the 12-triangle box: every primitive in the kernel arguments, the small tables fit
    return handle(**dict(dict(n_tiny=12, num_nodes=7, num_btris=12, bvh_depth=3, num_tris=12, hot_rows=12, hot_identity=1), **kw))


def two_level(**kw):          # 6 inline primitives around two per-mesh trees, the 4-wide forest on the device
    return handle(**dict(dict(n_tiny=6, n_blas=2, num_nodes=1000, num_btris=900, bvh_depth=12, num_nodes4=400, num_tris=3000, hot_rows=40), **kw))


def one_tree(**kw):          # one plain tree, depth 20, 10 000 nodes
    return handle(**dict(dict(num_nodes=10000, num_btris=12000, bvh_depth=20, num_tris=12000, hot_rows=40), **kw))


@pytest.fixture(scope="module")
def H():
    lib = hostlibs.load("plan")
    lib.hostcheck_plan_error.restype = C.c_char_p
    lib.hostcheck_plan_filter_grid.restype = C.c_longlong
    lib.hostcheck_plan_filter_grid.argtypes = [C.c_longlong, C.c_int]
    lib.hostcheck_plan_replicas.argtypes = [C.c_longlong, C.c_longlong]
    lib.hostcheck_plan_owns.argtypes = [C.c_void_p, C.c_int, C.c_longlong]
    lib.hostcheck_plan_split.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p]
    return lib


LDS_NAMES = ("ret", "lds_bytes", "off_lnodes", "b_lnodes", "off_lbtris", "b_lbtris", "off_ltri", "b_ltri", "off_lprim", "b_lprim", "n_lnodes", "n_lbtris", "n_ltri", "lt_end",
             "off_stack", "lt_nfaces")
LT_NAMES = ("lt_trimesh", "lt_meshbsdf", "lt_meshemitter", "lt_bsdf", "lt_emf", "lt_emi", "lt_fcmf", "lt_fpmf", "lt_ecmf", "lt_epmf", "lt_uv", "lt_tex", "lt_occ")          # in the order plan_lds places them


def plan_lds(H, h, reserved=0):
    out = (C.c_int32 * 32)()
    assert H.hostcheck_plan_lds(C.byref(h), reserved, out) == 0
    return dict(zip(LDS_NAMES + LT_NAMES, out))


LAYOUT = ("cam_off", "env_off", "env_n", "tex_off", "tex_n", "rad_off", "rad_n", "hot_off", "hot_rows", "total", "rep", "stride", "priv_off", "priv_rows", "priv_regs",
          "pend_off", "pend_rows", "sink_bytes")


def sink_layout(H, h, mask):
    out = (C.c_int32 * len(LAYOUT))()
    assert H.hostcheck_plan_sink_layout(C.byref(h), mask, out) == 0
    return dict(zip(LAYOUT, out))


# csrc/psdr_host.h sink_bytes_base / sink_reserve_pending / sink_bytes, restated
def base_bytes(L, priv_rows, priv_regs):
    return (L["priv_off"] + PRIV_WORDS * BLOCK) * 4 if (priv_rows > 0 and not priv_regs) else (L["rep"] * L["stride"] * 4 + 15) // 16 * 16


def pending_bytes(base, rows):
    return ((base // 4 + 3) // 4 * 4 + rows * PEND_WORDS * BLOCK) * 4


# ---------------------------------------------------------------------------------------------------------------- plan_lds
@pytest.mark.parametrize("make", [no_tree, two_level, one_tree])
@pytest.mark.parametrize("reserved", [0, 5000, 1 << 30])
def test_plan_lds_blocks(H, make, reserved):
    h = make()
    p = plan_lds(H, h, reserved)
    end = 0
    for name in ("lnodes", "lbtris", "ltri", "lprim"):          # disjoint, in declared order
        assert p["off_" + name] == end, (name, p)
        end += p["b_" + name]
    for name in LT_NAMES:
        assert p[name] == -1 or (p[name] % 16 == 0 and p[name] >= end), (name, p)
        end = max(end, p[name] + 1)
    assert end <= p["lt_end"] == p["off_stack"] and p["ret"] == p["lds_bytes"] >= p["off_stack"]
    if reserved == 1 << 30 and make is not no_tree:
        assert p["n_lnodes"] == p["n_lbtris"] == p["n_ltri"] == 0
    if make is no_tree:          # a scene without a tree always stages every row, and has no stacks
        assert (p["n_lnodes"], p["n_lbtris"], p["n_ltri"]) == (7, 12, 12) and p["ret"] == p["off_stack"]


def test_plan_lds_values(H):
    # no tree: 7 nodes (448 B) | 12 leaf triangles x 48 (-> 1024) | 12 rows x 96 (-> 2176) | 12 hit rows x 64 (-> 2944) | tri_mesh 12 words (48 -> 2992) |
    # mesh_bsdf, mesh_emitter 6 words (32 each -> 3056) | 3 BSDF records x 16 words (192 -> 3248) | emitter_f 8 words (-> 3280) | emitter_i 4 words (-> 3296) |
    # face cmf / pmf 2 words (16 each -> 3328); one emitter: no emitter distribution; no uv table, no texels, no occluder rows
    p = plan_lds(H, no_tree())
    assert [p[n] for n in LT_NAMES] == [2944, 2992, 3024, 3056, 3248, 3280, 3296, 3312, -1, -1, -1, -1, -1] and p["ret"] == 3328 and p["lt_nfaces"] == 2
    # two-level, depth 12: stacks 14 x 1 KB; 28 KB budget -> 14336 B of room = 224 nodes, nothing else of the tree; 6 hit rows (-> 14720), then the mesh-level
    # tables only (no tri_mesh): 32 + 32 + 192 + 32 + 16 + 16 + 16 -> 15056; + stacks = 29392
    p = plan_lds(H, two_level())
    assert (p["n_lnodes"], p["n_lbtris"], p["n_ltri"], p["off_lprim"], p["lt_trimesh"], p["lt_meshbsdf"], p["off_stack"], p["ret"]) == (224, 0, 0, 14336, -1, 14720, 15056, 29392)
    # one tree of depth 20: stacks 22 KB, 6 KB of room = 96 nodes; the budget is 28 KB lean, 40 KB with a rough conductor or an environment map, or what is forced
    assert (plan_lds(H, one_tree())["n_lnodes"], plan_lds(H, one_tree())["ret"]) == (96, 28 * K)
    assert (plan_lds(H, one_tree(has_rough=1))["n_lnodes"], plan_lds(H, one_tree(has_rough=1))["ret"]) == (288, 40 * K)
    assert plan_lds(H, one_tree(env_emitter=0))["ret"] == 40 * K
    assert plan_lds(H, one_tree(has_rough=1, lds_budget=32 * K))["ret"] == 32 * K == plan_lds(H, one_tree(lds_budget=32 * K))["ret"]
    # 10 000 nodes would fit a forced 1 MB: then the leaf triangles follow, as many as fit
    p = plan_lds(H, one_tree(lds_budget=K * K))
    assert (p["n_lnodes"], p["n_lbtris"], p["n_ltri"]) == (10000, (K * K - 22 * K - 640000) // 48, 0)


# ---------------------------------------------------------------------------------------------------------------- small rules
def test_wave_owns_pixels(H):
    h = no_tree()
    for nsp in (1, 2, 4, 8, 16, 32, 64):
        assert H.hostcheck_plan_owns(C.byref(h), nsp, 1 << 14) == 1, nsp
    for nsp in (3, 48, 128):
        assert H.hostcheck_plan_owns(C.byref(h), nsp, 1 << 14) == 0, nsp
        assert H.hostcheck_plan_owns(C.byref(h), nsp, 4096 * nsp) == 0, nsp          # (an unchunked launch of 4096 pixels)
    assert H.hostcheck_plan_owns(C.byref(no_tree(own_pixels=0)), 4, 1 << 14) == 0
    assert H.hostcheck_plan_owns(C.byref(h), 32, 16) == 0          # a chunk of 16 slots ends inside a pixel of 32 samples
    assert H.hostcheck_plan_owns(C.byref(h), 4, 16) == 1


def test_scene_flag_set(H):
    # environment map 1, rough conductor 2, two-level tree 4, no tree (and the small tables fit) 8
    for h, fl in ((one_tree(), 0), (one_tree(env_emitter=0), 1), (one_tree(has_rough=1), 2), (one_tree(has_rough=1, env_emitter=0), 3), (two_level(), 4), (two_level(has_rough=1), 6),
                  (no_tree(), 8), (no_tree(has_rough=1), 10), (no_tree(num_meshes=65), 0), (no_tree(env_emitter=0), 1)):
        assert H.hostcheck_plan_flag_set(C.byref(h)) == fl


def test_primary_edge_replicas(H):
    # the largest power of two <= 64 whose copies fit 64 MB = 2^24 words
    for pe_words, reps in ((8 * 1000, 64), (8 * 100000, 16), (1 << 18, 64), ((1 << 18) + 1, 32), (8 * 2000000, 1), (1 << 23, 2), ((1 << 23) + 1, 1)):
        assert H.hostcheck_plan_replicas(pe_words, 1 << 18) == reps, pe_words
        assert H.hostcheck_plan_replicas(pe_words, (1 << 18) - 1) == 1, pe_words


def test_filter_grid_and_record_words(H):
    assert [H.hostcheck_plan_filter_grid(n, d) for n, d in ((1 << 24, 16), (1 << 24, 4), (1 << 19, 16), (1 << 18, 4), ((1 << 18) + 4, 4))] == [1 << 20, 1 << 22, 1 << 16, 1 << 16, (1 << 16) + 1]
    assert [H.hostcheck_plan_record_words(d, w) for d, w in ((1, 0), (3, 0), (8, 0), (3, 1), (8, 1))] == [7, 17, 42, 26, 66]          # 2 + 5 depth; 2 + 8 depth from the wavefront


D, P, F = _abi.INTEGRATOR_DIRECT, _abi.INTEGRATOR_PATH, _abi.INTEGRATOR_FIELD
M = 1 << 20
# (integrator, max_depth, (bsdf, light) samples, n, rev_split, handle) -> (split, the value sweep is the traced wavefront)
SPLIT_TABLE = [
    ((P, 3, (1, 1), M, -1, one_tree()), (1, 0)),
    ((P, 3, (1, 1), M - 1, -1, one_tree()), (0, 0)),
    ((P, 1, (1, 1), M, -1, one_tree()), (0, 0)),                     # one vertex: not worth it
    ((P, 2, (1, 1), M, -1, one_tree()), (1, 0)),
    ((P, 3, (1, 1), M, -1, no_tree()), (0, 0)),                      # no tree to walk
    ((P, 3, (1, 1), M, 0, one_tree()), (0, 0)),
    ((P, 3, (1, 1), 100, 1, no_tree()), (1, 0)),                     # forced
    ((P, 1, (1, 1), 100, 1, one_tree()), (1, 0)),
    ((P, 3, (1, 1), M, -1, two_level()), (1, 1)),
    ((P, 3, (1, 1), M - 1, -1, two_level()), (0, 0)),
    ((P, 8, (1, 1), M, -1, two_level()), (1, 1)),
    ((P, 9, (1, 1), M, -1, two_level()), (1, 0)),                    # deeper than the LDS record: the fused value kernel
    ((P, 3, (1, 1), M, -1, two_level(num_nodes4=0)), (1, 0)),        # no 4-wide forest on the device
    ((P, 3, (1, 1), 1 << 16, 1, two_level()), (1, 1)),
    ((P, 3, (1, 1), (1 << 16) - 1, 1, two_level()), (1, 0)),         # below 2^16 slots the PathTracer does not run as a wavefront
    ((P, 3, (1, 1), M, 0, two_level()), (0, 0)),
    ((D, 1, (1, 1), M, -1, one_tree(num_nodes=16384)), (1, 0)),      # the DirectIntegrator gains on a large tree only
    ((D, 1, (1, 1), M, -1, one_tree(num_nodes=16383)), (0, 0)),
    ((D, 1, (1, 1), M - 1, -1, one_tree(num_nodes=16384)), (0, 0)),
    ((D, 1, (1, 1), M, -1, two_level(num_nodes=16384)), (1, 0)),
    ((D, 1, (2, 1), M, 1, one_tree(num_nodes=16384)), (0, 0)),       # two BSDF samples: hits not replayable
    ((D, 1, (1, 2), M, 1, one_tree(num_nodes=16384)), (0, 0)),
    ((D, 1, (1, 1), 100, 1, no_tree()), (1, 0)),
    ((D, 1, (1, 1), M, 0, one_tree(num_nodes=16384)), (0, 0)),
    ((F, 1, (1, 1), M, 1, one_tree(num_nodes=16384)), (0, 0)),
]


@pytest.mark.parametrize("row,want", SPLIT_TABLE)
def test_split_rule(H, row, want):
    integ, depth, (nb, nl), n, rev_split, h = row
    h.rev_split, h.width, h.height = rev_split, n, 1          # (use_wavefront counts the handle's film x the spp range)
    o = _abi.make_opts(integrator=integ, max_depth=depth, bsdf_samples=nb, light_samples=nl, spp=1)
    out = (C.c_int32 * 2)()
    assert H.hostcheck_plan_split(C.byref(h), C.byref(o), n, out) == 0
    assert tuple(out) == want


# ---------------------------------------------------------------------------------------------------------------- make_sink_layout
@pytest.mark.parametrize("sink_rep", [1, 2, 3, 4, 16])
@pytest.mark.parametrize("make,mask,kw", [(no_tree, G_TRI | G_CAM, {}), (no_tree, G_TEX | G_RAD | G_TRI, dict(num_texels=100)), (one_tree, G_TEX | G_TRI, dict(num_texels=2048, hot_rows=300)),
                                          (one_tree, G_TEX | G_RAD | G_TRI, dict(num_texels=2048, hot_rows=300)), (one_tree, G_TEX, dict(num_texels=4096)),
                                          (one_tree, G_ENV | G_TRI, dict(env_emitter=0, hot_rows=10))])
def test_make_sink_layout(H, make, mask, kw, sink_rep):
    L = sink_layout(H, make(sink_rep=sink_rep, **kw), mask)
    assert L["rep"] in (1, 2, 4, 8, 16) and L["rep"] <= max(sink_rep, 1) and L["stride"] % 2 == 1 and L["stride"] >= L["total"]
    assert L["rep"] == 1 or L["rep"] * L["stride"] <= CACHE_WORDS
    assert L["rep"] == max(r for r in (1, 2, 4, 8, 16) if r == 1 or (r <= sink_rep and r * L["stride"] <= CACHE_WORDS))
    assert L["total"] <= CACHE_WORDS
    if kw.get("hot_rows") == 300:          # 16 camera words + 2048 texels (+ 3 radiance words), the rest in rows of 24 words: 170 (169) of the 300
        assert L["hot_rows"] == (170 if not (mask & G_RAD) else 169) and L["total"] == L["hot_off"] + L["hot_rows"] * _abi.TRI_STRIDE
    if kw.get("num_texels") == 4096:          # more than 2048 texels are not cached
        assert L["tex_n"] == 0 and L["total"] == 16
    if mask & G_ENV:
        assert L["env_n"] == 32 and L["priv_rows"] == 0          # the environment map is emitter 0: no area light's rows to keep private


# ---------------------------------------------------------------------------------------------------------------- reverse LDS plans
CAMERA = ("form", "depth", "rec_bytes", "cache_bytes", "dyn1", "dyn_bytes", "geo", "deep_rec", "split", "kept_fused", "no_tree")
FUSED, SPLIT, SPLIT_WF, PROBE = 0, 1, 2, 4


def rev_camera(H, h, o, mask, fl, reg_priv=0, value_only=0):
    out = (C.c_int32 * (len(CAMERA) + 16 + 6 + len(LAYOUT)))()
    rc = H.hostcheck_plan_rev_camera(C.byref(h), C.byref(o), mask, fl, reg_priv, value_only, out)
    v = list(out)
    p = dict(zip(CAMERA, v))
    p["rev_layout"] = v[len(CAMERA):len(CAMERA) + 16]
    p["cx"], p["cx2"] = v[len(CAMERA) + 16:len(CAMERA) + 19], v[len(CAMERA) + 19:len(CAMERA) + 22]
    p["L"] = dict(zip(LAYOUT, v[len(CAMERA) + 22:]))
    return rc, p


def path(depth, spp=4):
    return _abi.make_opts(integrator=P, max_depth=depth, spp=spp)


ALL = G_TEX | G_RAD | G_TRI | G_CAM
# name: (handle, options, gradient mask, flag set, reg_priv, value_only) -> form
CAMERA_CASES = {
    "fused_no_tree": ((no_tree(), path(3), ALL, FL_TINY, 1, 0), FUSED),
    "fused_no_tree_direct": ((no_tree(), _abi.make_opts(spp=4), G_RAD | G_TRI, FL_TINY, 0, 0), FUSED),          # 3 KB of scene + 8 KB of record: the private rows' 30 KB fit a third of 160 KB
    "fused_tree_direct": ((one_tree(), _abi.make_opts(spp=4), G_TRI, 0, 0, 0), FUSED),
    "fused_material_only": ((one_tree(), path(3), G_TEX, 0, 1, 0), FUSED),
    "fused_deep_record": ((one_tree(), path(12), ALL, 0, 1, 0), FUSED),
    "split_tree": ((one_tree(rev_split=1), path(3), ALL, 0, 1, 0), SPLIT),
    "split_no_tree": ((no_tree(rev_split=1), path(3), ALL, FL_TINY, 1, 0), SPLIT),
    "split_value_only": ((no_tree(), path(3), 0, FL_TINY, 1, 1), SPLIT),
    "split_rough_lds_rows": ((one_tree(rev_split=1, has_rough=1), path(6), ALL, FL_ROUGH, 0, 0), SPLIT),
    "split_wavefront": ((two_level(width=1024, height=1024), path(3, spp=1), ALL, FL_FOREST, 1, 0), SPLIT_WF),
    "probe": ((two_level(width=256, height=256), _abi.make_opts(spp=1), ALL, FL_FOREST, 0, 0), PROBE),
    "fused_two_level_small": ((two_level(width=128, height=128), _abi.make_opts(spp=1), ALL, FL_FOREST, 0, 0), FUSED),          # below 2^16 slots: no probe pass
}


@pytest.mark.parametrize("lds_limit", [160 * K, 96 * K, 64 * K])
@pytest.mark.parametrize("name", sorted(CAMERA_CASES))
def test_rev_camera_plan(H, name, lds_limit):
    (h, o, mask, fl, reg_priv, value_only), form = CAMERA_CASES[name]
    h = PlanHandle.from_buffer_copy(h)
    h.lds_limit = lds_limit
    rc, p = rev_camera(H, h, o, mask, fl, reg_priv, value_only)
    L, L0 = p["L"], sink_layout(H, h, mask)
    is_path = o.integrator == P
    depth = min(o.max_depth, 250) if is_path else 1
    rec = 0 if depth > 8 else depth * REC_WORDS * BLOCK * 4
    assert (p["depth"], p["rec_bytes"], p["deep_rec"]) == (depth, rec, int(depth > 8))
    geo = bool(value_only or (mask & (G_TRI | G_CAM)))
    split = form in (SPLIT, SPLIT_WF)
    # what the plan may keep: the floor is what the launch needs without any cache -- (hit rows and small tables +) stacks + record
    bare = plan_lds(H, h, 1 << 30)
    floor = (bare["off_stack"] if split else bare["ret"]) + rec
    share = lds_limit // (3 if (o.integrator == D and not (fl & FL_ROUGH)) else 2)
    priv_regs = int(geo and is_path and reg_priv)
    priv_rows = L0["priv_rows"] if (priv_regs or L0["priv_rows"] == 0 or floor + base_bytes(L0, L0["priv_rows"], 0) <= share) else 0
    base = base_bytes(L0, priv_rows, priv_regs)
    pend = 0
    if geo and (mask & G_TRI) and is_path:
        pend = next((r for r in range(min(depth, 4), 0, -1) if floor + pending_bytes(base, r) <= share), 0)
    cache = pending_bytes(base, pend) if pend else base
    assert (L["priv_rows"], L["priv_regs"], L["pend_rows"], L["sink_bytes"], p["cache_bytes"]) == (priv_rows, priv_regs, pend, cache, cache), (p, floor, share)
    if rc != 0:          # only the LDS limit refuses a plan
        assert max(p["dyn_bytes"], p["dyn1"] if split else 0) > lds_limit and b"bytes of LDS" in H.hostcheck_plan_error()
        return
    assert (p["form"], p["geo"], p["split"], p["rev_layout"][8]) == (form, int(geo), int(split), form)
    assert p["no_tree"] == int(h.n_tiny > 0 and h.n_blas == 0)
    assert p["rev_layout"][:8] == [L["tex_n"], L["rad_n"], L["env_n"], L["hot_rows"], L["rep"], priv_rows, priv_regs, pend] and p["rev_layout"][11] == int(depth > 8)
    for cx in (p["cx"], p["cx2"]):
        off_stack, off_pathrec, off_sink = cx
        assert off_stack <= off_pathrec <= off_sink and off_sink - off_pathrec == rec
    # cx: the scene staged in what the record (and, fused, the cache) leave of the budget, the stacks, then the record
    staged = plan_lds(H, h, rec if split else rec + cache)
    assert p["cx"][0] == staged["off_stack"] and p["cx"][1] == staged["ret"] and p["dyn1"] == p["cx"][1] + rec
    # cx2: the kernels that walk no tree -- record and cache right behind the hit rows and small tables; a scene without a tree has one layout only
    assert p["cx2"] == (p["cx"] if (split and p["no_tree"]) else [bare["off_stack"], bare["off_stack"], bare["off_stack"] + rec])
    with_cache = p["cx2"] if (split or form == PROBE) else p["cx"]
    assert p["dyn_bytes"] == with_cache[2] + cache


def test_rev_camera_plan_keeps_and_drops(H):
    """the cases above meet both sides of every fit decision"""
    seen = set()
    for name, ((h, o, mask, fl, reg_priv, value_only), _) in CAMERA_CASES.items():
        for lim in (160 * K, 96 * K, 64 * K):
            h = PlanHandle.from_buffer_copy(h)
            h.lds_limit = lim
            rc, p = rev_camera(H, h, o, mask, fl, reg_priv, value_only)
            L0 = sink_layout(H, h, mask)
            if L0["priv_rows"] and not p["L"]["priv_regs"]:
                seen.add(("priv", p["L"]["priv_rows"] > 0))
            if (mask & G_TRI) and o.integrator == P:
                seen.add(("pend", p["L"]["pend_rows"]))
            seen.add(("rc", rc != 0))
    assert {("priv", True), ("priv", False), ("rc", True), ("rc", False)} <= seen and {("pend", r) for r in (0, 3, 4)} <= seen, seen


@pytest.mark.parametrize("make,mask", [(no_tree, ALL), (two_level, ALL), (one_tree, G_TEX), (one_tree, ALL)])
def test_one_vertex_plan(H, make, mask):
    """the secondary-edge kernels of both integrators and the CollocatedIntegrator's camera kernel: [ staged scene | stacks | cache ], no private rows, nothing deferred"""
    h = make()
    out = (C.c_int32 * (4 + len(LAYOUT)))()
    assert H.hostcheck_plan_one_vertex(C.byref(h), mask, out) == 0
    dyn, (off_stack, _, off_sink), L = out[0], out[1:4], dict(zip(LAYOUT, out[4:]))
    L0 = sink_layout(H, h, mask)
    cache = base_bytes(L0, 0, 0)
    staged = plan_lds(H, h, cache)
    assert (L["priv_rows"], L["priv_regs"], L["pend_rows"], L["sink_bytes"]) == (0, 0, 0, cache)
    assert (off_stack, off_sink, dyn) == (staged["off_stack"], staged["ret"], staged["ret"] + cache)


def test_small_lds_limit_refuses_every_plan(H):
    for name, ((h, o, mask, fl, reg_priv, value_only), _) in CAMERA_CASES.items():
        h = PlanHandle.from_buffer_copy(h)
        h.lds_limit = 2 * K
        rc, _ = rev_camera(H, h, o, mask, fl, reg_priv, value_only)
        assert rc != 0 and b"bytes of LDS per workgroup" in H.hostcheck_plan_error() and b"the device offers 2048" in H.hostcheck_plan_error(), name
    out = (C.c_int32 * (4 + len(LAYOUT)))()
    for make in (no_tree, two_level, one_tree):          # ... the one-vertex plan of the DirectIntegrator's secondary-edge launch among them
        assert H.hostcheck_plan_one_vertex(C.byref(make(lds_limit=2 * K)), ALL, out) != 0
        assert b"bytes of LDS per workgroup (traversal stacks + gradient cache), the device offers 2048" in H.hostcheck_plan_error()
