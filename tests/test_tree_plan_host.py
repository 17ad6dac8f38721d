"""The tree build and trace planning of csrc/psdr_tree_plan.h -- which hot rows, which refit, which tree, where it is built, the plan of the dense trace kernel and
of its request buffers: pure host functions -- run through the one entry of tests/hostcheck/hostcheck_plan.cpp (hostcheck_tree: numbers in, numbers out).  No GPU.
Every expected value is worked out by hand from the rules as psdr_bvh_build, launch_wf_trace and probe_buffers stated them before they moved into that header (the
arithmetic stands beside each case); the hot rows are compared with transcriptions of BOTH algorithms the two build paths used to carry.  The last test runs every
case of this file again in the stand-alone program tests/hostcheck/tree_plan_san.cpp, built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import hostlibs
from psdr_cuda import _abi

K = 1024
STRIDE = _abi.EMITTER_I_STRIDE          # words per emitter record: [1] first triangle, [2] faces
MAX_HOT, TINY_TRIS, AUTO_TRIS = 200, 16, 1 << 18          # kMaxHotRows, kTinyTris, kLbvhAutoTris
MAX_REFITS, GROWTH = 64, np.float32(1.3)          # kMaxRefits, kRefitAreaGrowth
TRACE_BLOCK, TRACE_NODE, TRACE_STACK_MAX, WF_SUB = 1024, 80, 16, 64          # kTraceBlock, kTraceNodeStride, kTraceStackMax, kWfSub
NONE, DEVICE_TREE, HOST_TREE = 0, 1, 2          # RefitKind

HANDLE = ("refit_enabled", "tiny_enabled", "two_level_enabled", "refit_ok", "tree_tris", "num_nodes", "refits_since_build", "lbvh", "built_area", "bvh_device_mode",
          "num_meshes", "env_emitter", "forest_min_inline", "num_nodes4", "stack_need4", "lds_limit", "trace_wg2", "num_cus", "blocks_per_cu")          # TreeHandle
RECORDED = []          # (rule, numbers in, numbers out) of every call: what the sanitizer program repeats


def handle(**kw):          # a 1000-triangle scene on one host-built tree, never refitted; the 4-wide forest of the trace cases: 400 nodes, 6 stack entries
    d = dict(refit_enabled=1, tiny_enabled=1, two_level_enabled=1, refit_ok=1, tree_tris=1000, num_nodes=500, refits_since_build=0, lbvh=0, built_area=100.0,
             bvh_device_mode=-1, num_meshes=3, env_emitter=-1, forest_min_inline=0, num_nodes4=400, stack_need4=6, lds_limit=160 * K, trace_wg2=-1, num_cus=256,
             blocks_per_cu=0)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return [float(d[n]) for n in HANDLE]


@pytest.fixture(scope="module")
def H():
    lib = hostlibs.load("plan")
    lib.hostcheck_tree.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def tree(H, what, *nums):
    nums = [float(v) for v in nums]
    out = (C.c_double * (len(nums) * 4 + 256))()
    m = H.hostcheck_tree(what.encode(), (C.c_double * len(nums))(*nums), len(nums), out)
    assert m >= 0, what
    got = [float(v) for v in out[:m]]
    RECORDED.append((what, nums, got))
    return got


def ints(v):
    assert all(x == int(x) for x in v), v
    return [int(x) for x in v]


def emitter_words(emitters):
    w = []
    for first, faces in emitters:
        w += [0, first, faces, 0][:STRIDE] + [0] * (STRIDE - 4)
    return w


# ---------------------------------------------------------------------------------------------------------------- hot rows
def hot_rows_host(T, tiny, emitters, by_area):
    """the host build of the parent: duplicates met through the triangle -> slot map"""
    slot, tris = [-1] * T, []

    def add(t):
        if 0 <= t < T and slot[t] < 0 and len(tris) < MAX_HOT:
            slot[t] = len(tris)
            tris.append(t)
    if tiny:
        for t in range(T):
            add(t)
    for first, faces in emitters:
        for f in range(min(faces, 64)):
            add(first + f)
    for t in by_area[:min(T, MAX_HOT)]:
        add(t)
    return tris


def hot_rows_device(T, emitters, by_area):
    """the device build of the parent (never on a tiny scene): duplicates met by a search of the list"""
    tris = []

    def add(t):
        if t < 0 or t >= T or len(tris) >= MAX_HOT:
            return
        if t not in tris:
            tris.append(t)
    for first, faces in emitters:
        for f in range(min(faces, 64)):
            add(first + f)
    for t in by_area[:min(T, MAX_HOT)]:
        add(t)
    return tris


def hot_rows(H, T, tiny, emitters, by_area):
    w = emitter_words(emitters)
    return ints(tree(H, "hot", T, tiny, len(emitters), len(w), *w, len(by_area), *by_area))


R = lambda a, b: list(range(a, b))          # noqa: E731
HOT_CASES = [
    # (T, tiny, emitters (first triangle, faces), by_area) -> slot -> triangle
    ((5, 1, [(3, 2)], [4, 2, 0, 1, 3]), R(0, 5)),                                                    # a scene without a tree: every row, slot = triangle
    ((300, 0, [(10, 2), (250, 70)], [260, 10, 5, 7]), [10, 11] + R(250, 300) + [5, 7]),               # faces 250 .. 319: 64 at most (.. 313), none past T; 260 and 10 once
    ((300, 0, [(10, 2), (100, 70)], [120, 5]), [10, 11] + R(100, 164) + [5]),                          # the 64-face cap inside the table
    # 52 emitter rows, then by_area = 260, 10, 0 .. 9, 11 .. 198 (200 entries): 10 new + 148 of the rest would make 249 -- the list ends at 200 (.. 149)
    ((300, 0, [(10, 2), (250, 70)], [260, 10] + R(0, 10) + R(11, 199)), [10, 11] + R(250, 300) + R(0, 10) + R(12, 150)),
    ((1000, 0, [(0, 2)], list(range(999, 799, -1))), [0, 1] + list(range(999, 801, -1))),          # by_area alone would pass 200 rows: 2 + 198 of its 200
    ((50, 0, [], list(range(49, -1, -1))), list(range(49, -1, -1))),                                  # no emitters
    ((20, 0, [(-1, 3)], [19, 0]), [0, 1, 19]),                                                        # a face in front of the table is dropped
]


def test_hot_rows(H):
    for (T, tiny, emitters, by_area), want in HOT_CASES:
        got = hot_rows(H, T, tiny, emitters, by_area)
        assert got == want, (T, emitters)
        assert len(got) == len(set(got)) <= MAX_HOT and all(0 <= t < T for t in got)
        assert got == hot_rows_host(T, tiny, emitters, by_area)
        if not tiny:          # (the device build never met a scene whose triangles travel in the kernel arguments)
            assert got == hot_rows_device(T, emitters, by_area)
    assert len(HOT_CASES[3][1]) == MAX_HOT == len(HOT_CASES[4][1])


# ---------------------------------------------------------------------------------------------------------------- emitter mask, occluder rows, tree boxes
def emitter_mask(H, num_emitters, env_emitter, T, words):
    out = ints(tree(H, "mask", num_emitters, env_emitter, T, len(words), *words))
    return out[0], out[1:]


def test_emitter_mask(H):
    wanted, mask = emitter_mask(H, 2, -1, 10, emitter_words([(8, 5), (-2, 4)]))          # 8 .. 12 and -2 .. 1 against a table of 10
    assert wanted == 1 and mask == [1, 1, 0, 0, 0, 0, 0, 0, 1, 1]
    wanted, mask = emitter_mask(H, 1, -1, 6, emitter_words([(2, 3)]))
    assert wanted == 1 and mask == [0, 0, 1, 1, 1, 0]
    # an environment emitter: no emitter rows to pre-test, whichever record it is
    assert emitter_mask(H, 2, 1, 6, emitter_words([(2, 3), (0, 0)]))[0] == 0
    assert emitter_mask(H, 2, 0, 6, emitter_words([(0, 0), (2, 3)]))[0] == 0
    # the host copy holds one record of two (a stale copy): only that one counts, the environment record behind it is not seen
    wanted, mask = emitter_mask(H, 2, 1, 6, emitter_words([(2, 3)]) + [0, 0])
    assert wanted == 1 and mask == [0, 0, 1, 1, 1, 0]
    assert emitter_mask(H, 0, -1, 3, []) == (1, [0, 0, 0])


def test_occluder_max_rows(H):
    # T = 3, emitter triangle 2, five rows in use: only column 2 counts, only bits 0 .. 4 -- 0b10111 has four of them set (bit 5 and above are not rows)
    occ = [0xffffffff, 0xffffffff, 0b00011,
           0xffffffff, 0xffffffff, 0b1110111,
           0xffffffff, 0xffffffff, 0]
    assert ints(tree(H, "occ", 3, 5, 0, 0, 1, *occ)) == [4]
    assert ints(tree(H, "occ", 3, 5, 0, 0, 0, *occ)) == [0]          # no emitter triangle
    assert ints(tree(H, "occ", 3, 5, 1, 0, 0, *occ)) == [5]


def test_blas_boxes(H):
    # two trees: their roots in the 4-wide node array reach hi.w, the other boxes and every lo.w (the BVH2 root) travel as they are
    out = ints(tree(H, "boxes", 2, *[40 + k for k in range(16)]))
    rows = [out[4 * k:4 * k + 4] for k in range(16)]
    assert rows == [[100 + k, (40 + k) if k < 2 else -1, k, k + 1] for k in range(16)]


# ---------------------------------------------------------------------------------------------------------------- levels and area
def node(lo0, hi0, lo1, hi1, c0, c1):
    return [np.float32(v) for v in (*lo0, *hi0, *lo1, *hi1)] + [c0, c1]


def area64(nodes):
    s = 0.0
    for n in nodes:
        lo0, hi0, lo1, hi1 = (np.array(n[i:i + 3], np.float64) for i in (0, 3, 6, 9))
        d = np.maximum(hi0, hi1) - np.minimum(lo0, lo1)
        s += d[0] * d[1] + d[1] * d[2] + d[2] * d[0]
    return s


def levels(H, root, nodes):
    out = tree(H, "levels", root, len(nodes), *[float(v) for n in nodes for v in n])
    return out[0], ints(out[1:])


LEAF = -1          # any negative child is a leaf here


def test_levels_and_area(H):
    assert levels(H, -1, []) == (0.0, [])          # the whole tree is one leaf: nothing to refit
    # three levels, breadth first: 0 -> (1, 2); 1 -> (3, leaf); 2, 3 -> leaves
    t3 = [node((0, 0, 0), (1.1, 0.7, 0.3), (0.9, 0.1, 0.2), (2.3, 1.9, 1.7), 1, 2),
          node((0, 0, 0), (0.6, 0.7, 0.3), (0.5, 0.2, 0.1), (1.1, 0.6, 0.3), 3, LEAF),
          node((0.9, 0.1, 0.2), (1.7, 1.3, 0.9), (1.5, 0.8, 0.6), (2.3, 1.9, 1.7), LEAF, LEAF),
          node((0, 0, 0), (0.3, 0.7, 0.2), (0.2, 0.1, 0.1), (0.6, 0.5, 0.3), LEAF, LEAF)]
    area, lv = levels(H, 0, t3)
    assert lv == [0, 1, 3, 4]
    # node 0 spans 2.3 x 1.9 x 1.7: 4.37 + 3.23 + 3.91 = 11.51 of the sum
    assert abs(area - area64(t3)) <= 1e-6 * area64(t3) and area64(t3) > 11.51
    # a chain: every node has one inner child -- as many levels as nodes
    chain = [node((i, 0, 0), (i + 1.3, 1, 1), (i + 1, 0, 0), (7, 1.7, 0.9), i + 1 if i < 5 else LEAF, LEAF) for i in range(6)]
    area, lv = levels(H, 0, chain)
    assert lv == [0, 1, 2, 3, 4, 5, 6]
    assert abs(area - area64(chain)) <= 1e-6 * area64(chain)
    area, lv = levels(H, 0, t3[3:])          # one node over two leaves
    assert lv == [0, 1] and abs(area - area64(t3[3:])) <= 1e-6 * area64(t3[3:])


# ---------------------------------------------------------------------------------------------------------------- refit or build
def refit(H, h, T=1000, tiny=0, same=1, stands=1, prev_area=100.0):
    return tuple(ints(tree(H, "refit", *h, T, tiny, same, stands, prev_area)))          # (refit_candidate, refit_choice)


def test_refit_candidate(H):
    assert refit(H, handle())[0] == 1
    for flipped in (dict(refit_enabled=0), dict(refit_ok=0), dict(tree_tris=999), dict(num_nodes=0)):          # every term, one at a time
        assert refit(H, handle(**flipped))[0] == 0, flipped
    assert refit(H, handle(), tiny=1)[0] == 0
    assert refit(H, handle(), T=1001)[0] == 0


def test_refit_choice(H):
    for lbvh, kind in ((0, HOST_TREE), (1, DEVICE_TREE)):
        assert refit(H, handle(lbvh=lbvh))[1] == kind
        assert refit(H, handle(lbvh=lbvh, refits_since_build=MAX_REFITS - 1))[1] == kind
        assert refit(H, handle(lbvh=lbvh, refits_since_build=MAX_REFITS))[1] == NONE          # a full rebuild at least every 64 refits
        assert refit(H, handle(lbvh=lbvh), same=0)[1] == NONE                                   # the emitter layout changed
        assert refit(H, handle(lbvh=lbvh), stands=0)[1] == NONE                                 # the two-level tree's tables no longer fit its kernels
        for built in (100.0, 0.37):          # the summed box area may have grown by 30 %, in float32
            built = np.float32(built)
            limit = GROWTH * built
            assert limit.dtype == np.float32
            h = handle(lbvh=lbvh, built_area=float(built), refits_since_build=3)
            assert refit(H, h, prev_area=float(limit))[1] == kind
            assert refit(H, h, prev_area=float(np.nextafter(limit, np.float32(0))))[1] == kind
            assert refit(H, h, prev_area=float(np.nextafter(limit, np.float32(np.inf))))[1] == NONE
        assert refit(H, handle(lbvh=lbvh), prev_area=float("nan"))[1] == NONE
    assert ints(tree(H, "inline_fits", TINY_TRIS)) == [1] and ints(tree(H, "inline_fits", TINY_TRIS + 1)) == [0]


def test_forest_stands(H):
    # (trees, meshes, emitters, faces of emitter 0): the kernels of a two-level scene stage up to 64 meshes, 8 emitters and 64 emitter faces in LDS
    for args, want in (((2, 64, 1, 2), 1), ((2, 65, 1, 2), 0), ((2, 3, 9, 2), 0), ((2, 3, 1, 65), 0), ((2, 3, 1, 64), 1), ((0, 65, 9, 65), 1)):
        assert ints(tree(H, "forest_stands", *args)) == [want], args


def kind(H, h, T, n_top=0, n_inline=0):
    return tuple(ints(tree(H, "kind", *h, T, n_top, n_inline)))          # (tiny_scene, device_build_wanted, forest_candidate, forest_kept)


def test_tree_kind(H):
    # where: option bvh_build -1 by size, 0 never on the device, 1 always
    for mode, T, device in ((-1, AUTO_TRIS - 1, 0), (-1, AUTO_TRIS, 1), (0, AUTO_TRIS, 0), (0, AUTO_TRIS - 1, 0), (1, AUTO_TRIS - 1, 1), (1, AUTO_TRIS, 1), (1, TINY_TRIS + 1, 1)):
        assert kind(H, handle(bvh_device_mode=mode), T)[:2] == (0, device), (mode, T)
    for mode in (-1, 0, 1):          # a scene whose triangles travel in the kernel arguments is never built on the device
        assert kind(H, handle(bvh_device_mode=mode), TINY_TRIS)[:2] == (1, 0)
        assert kind(H, handle(bvh_device_mode=mode), 1)[:2] == (1, 0)
    assert kind(H, handle(bvh_device_mode=1, tiny_enabled=0), TINY_TRIS)[:2] == (0, 1)
    # which: a two-level tree is tried on more than 16 triangles in meshes, never under an environment map, never with two_level or tiny_scene off
    assert kind(H, handle(), 1000)[2] == 1 and kind(H, handle(), TINY_TRIS + 1)[2] == 1
    for flipped in (dict(env_emitter=0), dict(two_level_enabled=0), dict(tiny_enabled=0), dict(num_meshes=0)):
        assert kind(H, handle(**flipped), 1000)[2] == 0, flipped
    assert kind(H, handle(), TINY_TRIS)[2] == 0
    # kept: at most 16 packed inline primitives, at least forest_min_inline inline triangles
    assert kind(H, handle(), 1000, 16, 20)[3] == 1 and kind(H, handle(), 1000, 17, 20)[3] == 0
    assert kind(H, handle(forest_min_inline=0), 1000, 0, 0)[3] == 1          # the default keeps a forest without any inline triangle
    assert kind(H, handle(forest_min_inline=6), 1000, 3, 5)[3] == 0 and kind(H, handle(forest_min_inline=6), 1000, 3, 6)[3] == 1


# ---------------------------------------------------------------------------------------------------------------- dense trace kernel
TRACE = ("wg2", "ovf", "S", "n_lnodes", "off_stack", "stack_entries", "grid", "dyn", "ovf_stride", "ovf_bytes")
COL = TRACE_BLOCK * 4          # bytes of one stack column
SMALL, LARGE = 1000, 1 << 19          # sub_cap: a launch below / from 2^25 requests (64 sub-queues)
FITS, TOO_BIG = 400, 5000          # nodes of the 4-wide forest: 32 000 B / 400 000 B


def trace(H, sub_cap, **kw):
    return dict(zip(TRACE, ints(tree(H, "trace", *handle(**kw), sub_cap))))


def plan(wg2, ovf, S, n_lnodes, grid, ovf_levels=0):
    return dict(wg2=wg2, ovf=ovf, S=S, n_lnodes=n_lnodes, off_stack=n_lnodes * TRACE_NODE, stack_entries=S, grid=grid, dyn=n_lnodes * TRACE_NODE + (S + 1) * COL,
                ovf_stride=grid * TRACE_BLOCK if ovf else 0, ovf_bytes=grid * TRACE_BLOCK * ovf_levels * 4)


TRACE_CASES = [
    # 160 KB.  One workgroup per CU: 163 840 - 1 024 static - 7 columns (28 672) = 134 144 B of room = 1 676 nodes; two: 81 920 - 1 024 - 28 672 = 52 224 B = 652 nodes
    (dict(), SMALL, plan(0, 0, 6, 400, 256)),                                                    # 32 000 + 28 672 + 1 024 fit: one workgroup, the whole forest staged
    (dict(num_nodes4=TOO_BIG), SMALL, plan(1, 0, 6, 652, 512)),                                  # a forest that does not fit anyway: two workgroups per CU
    (dict(), LARGE - 1, plan(0, 0, 6, 400, 256)),                                                # 2^25 - 64 requests
    (dict(), LARGE, plan(1, 0, 6, 400, 512)),                                                    # 2^25
    (dict(num_nodes4=TOO_BIG, trace_wg2=0), LARGE, plan(0, 0, 6, 1676, 256)),                    # never
    (dict(trace_wg2=5), SMALL, plan(1, 1, 5, 400, 512, 1)),                                      # always, columns of 5: the sixth entry overflows (512 x 1024 lanes x 4 B)
    (dict(num_nodes4=TOO_BIG, stack_need4=8), SMALL, plan(1, 0, 8, (80 * K - K - 9 * COL) // 80, 512)),          # columns of 8 hold 8
    (dict(num_nodes4=TOO_BIG, stack_need4=9), SMALL, plan(1, 1, 8, (80 * K - K - 9 * COL) // 80, 512, 1)),
    (dict(num_nodes4=TOO_BIG, stack_need4=20), SMALL, plan(1, 1, 8, (80 * K - K - 9 * COL) // 80, 512, 12)),
    (dict(stack_need4=20), SMALL, plan(0, 1, 16, 400, 256, 4)),                                  # one workgroup: kTraceStackMax columns (32 000 + 69 632 + 1 024 still fit)
    (dict(stack_need4=16), SMALL, plan(0, 0, 16, 400, 256)),
    # 64 KB: never two workgroups; 65 536 - 1 024 - 28 672 = 35 840 B = 448 nodes
    (dict(lds_limit=64 * K), SMALL, plan(0, 0, 6, 400, 256)),
    (dict(lds_limit=64 * K), LARGE, plan(0, 0, 6, 400, 256)),
    (dict(lds_limit=64 * K, num_nodes4=TOO_BIG), SMALL, plan(0, 0, 6, 448, 256)),
    (dict(lds_limit=64 * K, trace_wg2=5), SMALL, plan(0, 0, 6, 400, 256)),
    (dict(lds_limit=64 * K, stack_need4=9), SMALL, plan(0, 0, 9, (63 * K - 10 * COL) // 80, 256)),
    # 64 512 B hold 15 columns: 14 entries + the one above the top, 3 072 B = 38 nodes beside them; entries 15 .. 20 overflow
    (dict(lds_limit=64 * K, stack_need4=20), SMALL, plan(0, 1, 14, 38, 256, 6)),
]


def test_trace_plan(H):
    for kw, sub_cap, want in TRACE_CASES:
        p = trace(H, sub_cap, **kw)
        assert p == want, (kw, sub_cap)
        h = dict(zip(HANDLE, handle(**kw)))
        share = (h["lds_limit"] // 2 if p["wg2"] else h["lds_limit"]) - K          # beside the kernel's 1 KB of static LDS
        assert p["off_stack"] + (p["S"] + 1) * TRACE_BLOCK * 4 == p["dyn"] <= share, (kw, p)
        assert p["n_lnodes"] <= h["num_nodes4"] and p["S"] <= min(h["stack_need4"], TRACE_STACK_MAX) and p["ovf"] == int(h["stack_need4"] > p["S"])
    assert trace(H, SMALL, trace_wg2=5, stack_need4=3)["S"] == 3          # no column beyond what the forest needs


# ---------------------------------------------------------------------------------------------------------------- probe buffers
PROBE = ("sub_cap", "cnt_bytes", "hit_bytes", "mask_bytes", "req_bytes", "total")


def test_probe_buffers(H):
    h = handle()          # 256 CUs
    seen = {}
    for slots in (1, 255, 256, (1 << 20) + 1):
        for rays in (1, 3):
            for per_cu in (6, 16):
                p = dict(zip(PROBE, ints(tree(H, "probe", *h, slots, rays, per_cu))))
                # the probe launch: ceil(slots / 256) workgroups, 256 x per_cu at most, rounded up to the 64 queues; block b appends to queue b % 64
                blocks = -(-min(-(-slots // 256), 256 * per_cu) // WF_SUB) * WF_SUB
                trips = -(-slots // (blocks * 256))
                assert p["sub_cap"] == blocks // WF_SUB * trips * 256 * rays and p["sub_cap"] * WF_SUB >= slots * rays
                assert p["cnt_bytes"] == WF_SUB * 32 * 4 and p["hit_bytes"] == slots * rays * 16 and p["req_bytes"] == 2 * p["sub_cap"] * WF_SUB * 16
                assert p["mask_bytes"] % 256 == 0 and 0 <= p["mask_bytes"] - slots * 4 < 256 and p["cnt_bytes"] % 256 == 0
                assert p["total"] == p["cnt_bytes"] + p["hit_bytes"] + p["mask_bytes"] + p["req_bytes"]
                seen[slots, rays, per_cu] = p
    # one workgroup of 64: one queue entry per thread and ray; 8 192 + 16 + 256 + 2 x 256 x 64 x 16
    assert seen[1, 1, 16] == dict(sub_cap=256, cnt_bytes=8192, hit_bytes=16, mask_bytes=256, req_bytes=524288, total=532752)
    assert (seen[255, 1, 6]["sub_cap"], seen[255, 1, 6]["mask_bytes"], seen[256, 3, 6]["sub_cap"], seen[256, 3, 6]["mask_bytes"]) == (256, 1024, 768, 1024)
    # 2^20 + 1 slots: 4096 workgroups make two trips (64 per queue x 2 x 256), 1536 make three (24 x 3 x 256)
    assert seen[(1 << 20) + 1, 1, 16]["sub_cap"] == 32768 and seen[(1 << 20) + 1, 3, 6]["sub_cap"] == 3 * 18432
    assert seen[(1 << 20) + 1, 3, 6]["mask_bytes"] == 4194560


# ---------------------------------------------------------------------------------------------------------------- the same cases under the sanitizers
def test_sanitizer_program(H, tmp_path):
    """tests/hostcheck/tree_plan_san.cpp (host code only, its own main, run as a child process) repeats every case above and writes what the library wrote"""
    del RECORDED[:]
    for t in (test_hot_rows, test_emitter_mask, test_occluder_max_rows, test_blas_boxes, test_levels_and_area, test_refit_candidate, test_refit_choice, test_forest_stands,
              test_tree_kind, test_trace_plan, test_probe_buffers):
        t(H)
    cases = list(RECORDED)
    assert len(cases) > 100
    exe = hostlibs.san_program("tree_plan_san", hostlibs.deps("plan"))
    path = tmp_path / "cases.txt"
    path.write_text("".join("%s %s\n" % (what, " ".join(float(v).hex() for v in nums)) for what, nums, _ in cases))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (what, nums, want) in zip(lines, cases):
        got = line.split()
        assert int(got[0]) == len(want) and [float.fromhex(v) for v in got[1:]] == want, (what, nums)
