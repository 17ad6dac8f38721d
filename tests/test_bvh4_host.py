"""The host side of the two-level trees and the 4-wide tree, without a GPU: ForestBuilder / Builder, collapse_bvh4 and quantise_bvh4
(csrc/psdr_bvh_build.h, run through tests/hostcheck hostcheck_bvh4) on the adversarial families of tests/lbvh_cases.py, judged by numpy references
written here -- topology, the traversal-stack need the dense trace kernel sizes its columns by, containment of the dequantised planes, the
forest builder's thresholds.  Also: the ray sets of the two-level inputs stay inside the exclusion cap by the reference alone, and the
same host functions run clean in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import lbvh_cases as L
from helpers import ROOT, hostcheck_lib

NO_CHILD = 0x7ffffffe
NODE2 = np.dtype([("lo0", "<f4", 3), ("hi0", "<f4", 3), ("lo1", "<f4", 3), ("hi1", "<f4", 3), ("c", "<i4", 2), ("pad", "<i4", 2)])
NODE4 = np.dtype([("org", "<f4", 3), ("exps", "<u4"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("child", "<i4", 4), ("pad", "<u4", 2)])
assert NODE2.itemsize == 64 and NODE4.itemsize == 64

# n4 / stack_need of the host builder + collapse_bvh4 per family and bvh_maxleaf (single tree): the values the GPU tests choose their inputs by --
# 15, 16, 17 and 19-22 around kTraceStackMax = 16 of the dense trace kernel.  A changed builder or collapse announces itself here.
TABLE = {"ladder_R38": {4: (167, 19), 1: (544, 22), 8: (87, 18)}, "one_cell_1001": {4: (161, 16), 1: (562, 19), 8: (122, 15)},
         "two_clusters": {4: (305, 16), 1: (473, 17), 8: (305, 16)}, "runs": {4: (35, 12), 1: (100, 15), 8: (24, 11)},
         "planar_x": {4: (77, 13), 1: (145, 16), 8: (77, 13)}, "with_degenerates": {4: (52, 13), 1: (144, 16), 8: (41, 12)},
         "uniform_5000": {4: (1325, 20), 1: (2436, 22), 8: (1325, 20)}, "one_cell_65": {4: (9, 9), 1: (29, 11), 8: (7, 7)}}
FAMILIES = sorted(TABLE)
FORESTS = ["overlap16", "overlap17", "room"] + ["single:" + n for n in ("runs", "two_clusters")]


def bvh4(rows, tri_mesh, num_meshes, max_leaf, forest, lib=None):
    """hostcheck_bvh4 as a dict of numpy arrays"""
    H = lib or hostcheck_lib()
    rows = np.ascontiguousarray(rows, np.float32)
    tri_mesh = np.ascontiguousarray(tri_mesh, np.int32)
    T = rows.shape[0]
    sizes = np.zeros(8, np.int32)
    nodes, nodes4 = np.zeros(T, NODE2), np.zeros(T, NODE4)
    btris, boxes = np.zeros((T, 12), np.float32), np.zeros((num_meshes + 1, 6), np.float32)
    roots2, roots4 = np.zeros(num_meshes + 1, np.int32), np.zeros(num_meshes + 1, np.int32)
    child, src, inl = np.zeros((T, 4), np.int32), np.zeros((T, 4), np.int32), np.zeros(T, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    rc = H.hostcheck_bvh4(ptr(rows), ptr(tri_mesh), T, num_meshes, max_leaf, int(forest), ptr(sizes), ptr(nodes), ptr(btris), ptr(roots2), ptr(roots4),
                          ptr(child), ptr(src), ptr(nodes4), ptr(inl), ptr(boxes))
    assert rc == 0, rc
    n2, nb, nr, n4, need, ni, is_forest, depth = (int(x) for x in sizes)
    return dict(nodes=nodes[:n2], btris=btris[:nb], roots2=roots2[:nr], roots4=roots4[:nr], child=child[:n4], src=src[:n4], nodes4=nodes4[:n4], n4=n4,
                stack_need=need, inline=inl[:ni], forest=bool(is_forest), boxes=boxes[:nr], depth=depth, T=T)


_built = {}


def built(name, max_leaf, forest=False):
    key = (name, max_leaf, forest)
    if key not in _built:
        if forest:
            c = L.forest_case(name)
            rows, mesh_of = c.rows, c.mesh_of
        else:
            rows = L.case(name).rows
            mesh_of = np.zeros(rows.shape[0], np.int32)
        _built[key] = (rows, mesh_of, bvh4(rows, mesh_of, int(mesh_of.max()) + 1, max_leaf, forest))
    return _built[key]


CASES = [(n, ml, False) for n in FAMILIES for ml in (1, 4, 8)] + [(n, ml, True) for n in FORESTS for ml in (1, 4, 8)]
IDS = ["%s-%d%s" % (n, ml, "-forest" if f else "") for n, ml, f in CASES]


# ---------------------------------------------------------------- topology
@pytest.mark.parametrize("name,max_leaf,forest", CASES, ids=IDS)
def test_topology(name, max_leaf, forest):
    rows, mesh_of, t = built(name, max_leaf, forest)
    nodes, child, src, n4 = t["nodes"], t["child"], t["src"], t["n4"]
    assert n4 > 0 and (t["roots2"] >= 0).all()              # (no family produces a single-leaf tree)
    c2 = nodes["c"]
    # every triangle of a tree mesh sits in exactly one BVH2 leaf of at most max_leaf triangles
    leaves2 = c2[c2 < 0]
    enc = ~leaves2
    first, cnt = enc >> 3, (enc & 7) + 1
    assert cnt.max() <= max_leaf and np.unique(leaves2).size == leaves2.size
    order = np.argsort(first)
    assert first[order][0] == 0 and np.array_equal(first[order][1:], (first + cnt)[order][:-1]) and (first + cnt).max() == t["btris"].shape[0]
    ids = np.ascontiguousarray(t["btris"][:, 3]).view(np.int32)
    in_tree = np.ones(t["T"], bool)
    in_tree[t["inline"]] = False
    assert np.array_equal(np.sort(ids), np.nonzero(in_tree)[0])
    assert np.array_equal(t["btris"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], rows[ids, 0:9])
    if forest and t["forest"]:
        c = L.forest_case(name)
        assert np.array_equal(in_tree, c.in_tree) and len(t["roots2"]) == len(c.tree_meshes)
    # every BVH2 leaf is the child of exactly one 4-wide slot
    leaves4 = child[(child < 0)]
    assert np.array_equal(np.sort(leaves4), np.sort(leaves2))
    # empty slots: kNoChild with src = -1, behind the used ones; at least two children per node
    empty = child == NO_CHILD
    assert np.array_equal(empty, src < 0) and (src[empty] == -1).all() and not empty[:, :2].any() and (np.diff(empty.astype(int), axis=1) >= 0).all()
    # child[i][c] is what src[i][c] points at; every 4-wide node has one parent, with a smaller index; its slots are a cut of its BVH2 node's subtree
    node2_of = np.full(n4, -1, np.int64)
    depth4 = np.full(n4, -1, np.int64)
    assert np.array_equal(t["roots4"], np.arange(len(t["roots4"])))          # the roots come first, in the order of the trees
    node2_of[t["roots4"]], depth4[t["roots4"]] = t["roots2"], 0
    for i in range(n4):
        assert node2_of[i] >= 0, "4-wide node %d has no parent in front of it" % i
        used = [int(s) for s in src[i] if s >= 0]
        frontier = [2 * int(node2_of[i]), 2 * int(node2_of[i]) + 1]
        while set(frontier) != set(used):
            opened = [s for s in frontier if s not in used]
            assert opened and len(frontier) < 4, (i, frontier, used)
            s = opened[0]
            c = int(c2[s >> 1, s & 1])
            assert c >= 0, (i, s)
            frontier = [x for x in frontier if x != s] + [2 * c, 2 * c + 1]
        for k, s in enumerate(used):
            c, ch = int(c2[s >> 1, s & 1]), int(child[i, k])
            if c < 0:
                assert ch == c
            else:
                assert i < ch < n4 and node2_of[ch] < 0, (i, k, ch)
                node2_of[ch], depth4[ch] = c, depth4[i] + 1
    # level order across all roots: a prefix of the array is the top of every tree (what the dense trace kernel stages in LDS)
    assert (np.diff(depth4) >= 0).all()


# ---------------------------------------------------------------- stack need
def ref_stack_need(child, roots4):
    """top-down: on each level the non-empty siblings minus one wait on the stack while the walk is below the deepest child"""
    sys.setrecursionlimit(10000)

    def need(i):
        kids = [int(c) for c in child[i] if c != NO_CHILD]
        return len(kids) - 1 + max([need(c) for c in kids if c >= 0], default=0)
    return max(need(int(r)) for r in roots4)


@pytest.mark.parametrize("name,max_leaf,forest", CASES, ids=IDS)
def test_stack_need(name, max_leaf, forest):
    _, _, t = built(name, max_leaf, forest)
    want = ref_stack_need(t["child"], t["roots4"])
    print("%s maxleaf %d: n4 = %d, stack_need = %d (reference %d), BVH2 depth %d" % (name, max_leaf, t["n4"], t["stack_need"], want, t["depth"]))
    assert t["stack_need"] == want
    if not forest:
        assert (t["n4"], t["stack_need"]) == TABLE[name][max_leaf]
    elif name.startswith("single:"):                         # one mesh as a forest: the same tree
        assert (t["n4"], t["stack_need"]) == TABLE[name[7:]][max_leaf]


# ---------------------------------------------------------------- containment
def round_f32(x):
    """a Fraction to the nearest float32 (ties to even)"""
    c = np.float32(float(x))
    cand = sorted({float(c), float(np.nextafter(c, np.float32(-np.inf))), float(np.nextafter(c, np.float32(np.inf)))})
    best = min(cand, key=lambda v: (abs(Fraction(v) - x), int(np.float32(v).view(np.uint32)) & 1))
    return np.float32(best)


def fma32(q, scale, org):
    """fmaf(q, scale, org) of float32 operands, correctly rounded: in float64 where that sum is exact, by rational arithmetic elsewhere"""
    x, o = q.astype(np.float64) * scale.astype(np.float64), org.astype(np.float64)
    s = o + x
    out = s.astype(np.float32)
    inexact = ((s - o) != x) | ((s - x) != o)
    for k in zip(*np.nonzero(inexact)):
        out[k] = round_f32(Fraction(float(x[k])) + Fraction(float(o[k])))
    return out


def dequantised(n4):
    """lower and upper planes [n, slot, axis] as the node layout promises them: fmaf(q, 2^(E - 127), org)"""
    E = np.stack([(n4["exps"] >> (8 * a)) & 0xff for a in range(3)], 1).astype(np.int64)               # [n, axis]
    scale = np.ldexp(1.0, E - 127).astype(np.float32)
    ql = np.stack([(n4["qlo"] >> (8 * c)) & 0xff for c in range(4)], 1).astype(np.float32)              # [n, slot, axis]
    qh = np.stack([(n4["qhi"] >> (8 * c)) & 0xff for c in range(4)], 1).astype(np.float32)
    org, sc = np.broadcast_to(n4["org"][:, None, :], ql.shape), np.broadcast_to(scale[:, None, :], ql.shape)
    return E, ql, qh, fma32(ql, sc, org), fma32(qh, sc, org)


@pytest.mark.parametrize("name,max_leaf,forest", CASES, ids=IDS)
def test_dequantised_planes_contain_the_child_boxes(name, max_leaf, forest):
    _, _, t = built(name, max_leaf, forest)
    nodes, src, n4 = t["nodes"], t["src"], t["nodes4"]
    assert np.array_equal(n4["child"], t["child"]) and not n4["pad"].any()
    E, ql, qh, lo_q, hi_q = dequantised(n4)
    assert E.min() >= 1 and E.max() <= 254
    used = src >= 0
    s = np.where(used, src, 0)
    lo = np.where((s & 1)[..., None] == 1, nodes["lo1"][s >> 1], nodes["lo0"][s >> 1])
    hi = np.where((s & 1)[..., None] == 1, nodes["hi1"][s >> 1], nodes["hi0"][s >> 1])
    assert (lo <= hi)[used].all()
    assert (lo_q <= lo)[used].all() and (hi_q >= hi)[used].all(), "a dequantised plane cuts into a child box"
    # the origin is the lower corner of the union; the planes are no further out than one step of the axis' scale (or the clamp at E = 1)
    assert np.array_equal(n4["org"], np.where(used[..., None], lo, np.inf).min(axis=1))
    # (floor / ceil are within one step; the fix-up loop moves a plane only while its ROUNDED value is inside the box: one step + one ulp of the plane)
    step = np.ldexp(1.0, E - 127)[:, None, :]
    assert ((lo - lo_q.astype(np.float64)) <= step + np.spacing(np.abs(lo)))[used].all() and ((hi_q.astype(np.float64) - hi) <= step + np.spacing(np.abs(hi)))[used].all()
    # an empty slot: lower plane above the upper one, in every axis
    assert (ql[~used] == 255).all() and (qh[~used] == 0).all() and (lo_q > hi_q)[~used].all()
    # axes without extent (planar_*): still a valid scale, both planes on the box
    flat = (lo == hi) & used[..., None]
    assert (lo_q <= lo)[flat].all() and (hi_q >= hi)[flat].all()


# ---------------------------------------------------------------- the forest builder's thresholds
def soup_tables(counts, rects=0):
    """meshes of the given triangle counts, cut from uniform_5000 in order; behind them one mesh of `rects` axis-aligned rectangles (two triangles
    each, fan-triangulated: the inline triangles of a forest pair into one primitive per rectangle)"""
    rows = L.case("uniform_5000").rows[:sum(counts)]
    mesh_of = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    if rects:
        r = np.zeros((2 * rects, rows.shape[1]), np.float32)
        z = 2.0 + np.arange(rects, dtype=np.float32)
        r[0::2, 0:9] = np.stack([z * 0, z * 0, z, z * 0 + 4, z * 0, z * 0, z * 0 + 4, z * 0 + 4, z * 0], 1)               # a, b - a, c - a
        r[1::2, 0:9] = np.stack([z * 0, z * 0, z, z * 0 + 4, z * 0 + 4, z * 0, z * 0, z * 0 + 4, z * 0], 1)               # a, c - a, d - a
        r[:, 21] = 8.0
        rows, mesh_of = np.concatenate([rows, r]), np.concatenate([mesh_of, np.full(2 * rects, len(counts), np.int32)])
    return rows, mesh_of


@pytest.mark.parametrize("counts,rects,trees", [((64, 16), 0, 1), ((64, 17), 0, 0), ((64, 64), 0, 2), ((63, 64), 0, 0), ((64, 63), 0, 0), ((64,), 16, 1), ((64,), 17, 0),
                                                ((100, 5, 200), 3, 2), ((12, 64, 4, 70), 0, 2), ((64,) * 16 + (5,), 0, 16), ((64,) * 17, 0, 0), ((64,) * 17, 2, 0)])
def test_forest_builder_thresholds(counts, rects, trees):
    """kMinBlasTris = 64 triangles is the smallest mesh that gets a tree, a smaller one goes inline (a 63-triangle mesh beside a tree is more inline
    triangles than a forest may have); more than 2 kTinyTris = 32 inline triangles (16 rectangles are the most), more than kTinyTris = 16 inline
    primitives after pairing (16 lone triangles are the most) or more than kMaxBlas = 16 trees: the single tree (trees = 0 here)."""
    rows, mesh_of = soup_tables(counts, rects)
    n_meshes = int(mesh_of.max()) + 1
    t = bvh4(rows, mesh_of, n_meshes, 4, True)
    assert t["forest"] == (trees > 0)
    if trees:
        small = [i for i in range(n_meshes) if (mesh_of == i).sum() < 64]
        assert len(t["roots2"]) == trees and np.array_equal(np.sort(t["inline"]), np.nonzero(np.isin(mesh_of, small))[0])
        assert t["btris"].shape[0] + t["inline"].size == rows.shape[0]
    else:
        assert len(t["roots2"]) == 1 and t["inline"].size == 0 and t["btris"].shape[0] == rows.shape[0]


TREE_FORESTS = [n for n in FORESTS if n != "overlap17"]          # (17 trees: the table gets the single tree, there is no tree box)


@pytest.mark.parametrize("name,max_leaf", [(n, ml) for n in TREE_FORESTS for ml in (1, 4, 8)])
def test_tree_boxes_are_inside_what_the_root_nodes_cover(name, max_leaf):
    """tree_box(k), the box a ray must enter to walk tree k, is the union box of the BVH2 root's children and holds every triangle of the mesh.  A ray
    that enters it must not be turned away at the root: in float64, 4 000 segments between points of the box (every one of them enters it) and 2 000
    rays from outside towards a point inside each pass the slab test of a dequantised child of the 4-wide root wherever they pass that of the BVH2 box
    the child stands for -- and the union box of the dequantised children contains tree_box(k)."""
    rows, mesh_of, t = built(name, max_leaf, True)
    c = L.forest_case(name)
    assert t["forest"]
    _, _, _, lo_q, hi_q = dequantised(t["nodes4"])
    rng = np.random.default_rng(3)

    def enters(lo, hi, o, d):
        """float64 slab test of rays (o, d) against boxes [k, 3]: [rays, k]"""
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo[None] - o[:, None]) / d[:, None], (hi[None] - o[:, None]) / d[:, None]
        tn, tf = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
        return np.maximum(tn, 0.0) <= tf
    for k, mesh in enumerate(c.tree_meshes):
        r2, r4 = t["nodes"][t["roots2"][k]], int(t["roots4"][k])
        lo, hi = t["boxes"][k, 0:3].astype(np.float64), t["boxes"][k, 3:6].astype(np.float64)
        assert np.array_equal(lo, np.minimum(r2["lo0"], r2["lo1"])) and np.array_equal(hi, np.maximum(r2["hi0"], r2["hi1"]))
        r = rows[mesh_of == mesh].astype(np.float64)
        p = np.concatenate([r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9]])
        assert (p.min(axis=0) >= lo).all() and (p.max(axis=0) <= hi).all()
        used = t["src"][r4] >= 0
        qlo, qhi = lo_q[r4][used].astype(np.float64), hi_q[r4][used].astype(np.float64)
        assert (qlo.min(axis=0) <= lo).all() and (qhi.max(axis=0) >= hi).all()
        ss = t["src"][r4][used]                               # the BVH2 boxes the 4-wide root's children stand for (children or grandchildren of the BVH2 root)
        blo = np.stack([t["nodes"]["lo%d" % (x & 1)][x >> 1] for x in ss]).astype(np.float64)
        bhi = np.stack([t["nodes"]["hi%d" % (x & 1)][x >> 1] for x in ss]).astype(np.float64)
        # rays: inside -> inside, and outside -> inside; every second one ends inside a child's box (two_clusters: the children are specks of the root's
        # box).  Directions without zero components: no 0 * inf in the reference.
        a, b = lo + rng.random((6000, 3)) * (hi - lo), lo + rng.random((6000, 3)) * (hi - lo)
        pick = rng.integers(0, len(ss), 3000)
        b[::2] = blo[pick] + rng.random((3000, 3)) * (bhi[pick] - blo[pick])
        a[4000:] = lo - 0.5 * (hi - lo) + 2.0 * rng.random((2000, 3)) * (hi - lo)
        d = b - a
        keep = (d != 0).all(axis=1)
        a, d = a[keep], d[keep]
        assert enters(lo[None], hi[None], a, d).all()
        kids2, kids4 = enters(blo, bhi, a, d), enters(qlo, qhi, a, d)
        assert kids2.any(axis=1).mean() > 0.3 and kids4[kids2].all(), "a ray that enters a child's box is turned away by the quantised root node"
    if name == "room":                                        # two trees with disjoint boxes
        assert (t["boxes"][0, 3:6] < t["boxes"][1, 0:3]).all() or (t["boxes"][1, 3:6] < t["boxes"][0, 0:3]).all()


# ---------------------------------------------------------------- the ray sets of the GPU tests, by the reference alone
@pytest.mark.parametrize("name", L.FOREST_INPUTS)
def test_forest_ray_sets_stay_inside_the_caps(name):
    """At most 0.2 % of a ray set may be excluded as near an edge or a near-tie -- over the whole table (what a closest-hit query over the scene is judged by) and over the
    tree triangles alone (the dense trace kernel) -- and the 2 000 rays with exactly zero direction components are part of it."""
    c = L.forest_case(name)
    o, d, owner = c.rays
    assert ((d[-2000:] == 0).sum(1) >= 1).all() and np.isfinite(o).all()
    for label, bf in (("whole table", c.bf), ("tree triangles", c.bf_tree)):
        if label == "tree triangles" and c.tree_meshes is None:
            continue
        excl = (bf["near_edge"] | bf["near_tie"])
        print("%s, %s: %d rays, excluded %.4f %% (axis rays %.4f %%), hits %.1f %% (axis rays %.1f %%)" % (
            name, label, o.shape[0], 100 * excl.mean(), 100 * excl[-2000:].mean(), 100 * (bf["tri"][:, 0] >= 0).mean(), 100 * (bf["tri"][-2000:, 0] >= 0).mean()))
        assert excl.mean() <= 0.002 and bf["near_tie"].mean() < 0.001
        assert (bf["tri"][:, 0] >= 0).mean() > 0.1
        assert not np.isin(bf["tri"], np.nonzero(c.rows[:, 21] == 0)[0]).any()
    if c.tree_meshes is not None and not c.in_tree.all():
        assert np.isin(c.bf_tree["tri"][:, 0], np.concatenate([[-1], np.nonzero(c.in_tree)[0]])).all()
        assert (c.bf["tri"][:, 0] != c.bf_tree["tri"][:, 0]).any()              # some rays do end on an inline triangle first


def test_edge_ray_set_stays_inside_the_caps():
    """The rays that start on secondary edges of the bunny, as the GPU test judges them: the first half ignores its edge's two faces, the second half
    (edge = -1) sees them.  (With the faces seen on BOTH halves the share doubles: a ray that leaves an edge at a grazing angle can meet an adjacent
    face again just above RayEpsilon in float32 -- the reason the library skips them; printed, not capped.)"""
    e = L.edges_case()
    for label, bf in (("adjacent faces seen", e["bf"]), ("adjacent faces ignored on the first half", e["bf_ign"])):
        excl = bf["near_edge"] | bf["near_tie"]
        print("edges, %s: %d rays, excluded %.4f %%, hits %.1f %%" % (label, excl.size, 100 * excl.mean(), 100 * (bf["tri"][:, 0] >= 0).mean()))
    excl = e["bf_ign"]["near_edge"] | e["bf_ign"]["near_tie"]
    assert excl.mean() <= 0.002 and (e["bf_ign"]["tri"][:, 0] >= 0).mean() > 0.1
    # the rays come in pairs (same origin and direction, edge set on the first): ignoring the two faces changes an answer only on the first half
    half = e["o"].shape[0] // 2
    assert (e["edge"][:half] >= 0).all() and (e["edge"][half:] == -1).all() and np.array_equal(e["o"][:half], e["o"][half:])
    assert np.array_equal(e["bf"]["tri"][half:], e["bf_ign"]["tri"][half:])
    assert e["in_tree"][e["faces"][e["faces"] >= 0]].all()              # the edges are the tree mesh's


def test_brute_force_exclude_hides_exactly_the_named_triangles():
    c = L.case("runs")
    o, d, _ = c.rays
    o, d = o[::7], d[::7]
    bf = L.brute_force(c.rows, o, d)
    first = bf["tri"][:, 0]
    ex = np.stack([first, np.full_like(first, -1)], 1)
    hidden = L.brute_force(c.rows, o, d, exclude=ex)
    hit2 = bf["tri"][:, 1] >= 0
    assert np.array_equal(hidden["tri"][hit2, 0], bf["tri"][hit2, 1]) and np.array_equal(hidden["t"][hit2, 0], bf["t"][hit2, 1])
    assert (hidden["tri"][(first >= 0) & ~hit2, 0] == -1).all() and not (hidden["tri"][first >= 0, 0] == first[first >= 0]).any()
    none = L.brute_force(c.rows, o, d, exclude=np.full((o.shape[0], 2), -1))
    assert all(np.array_equal(none[k], bf[k]) for k in bf)


# ---------------------------------------------------------------- the same host functions under the sanitizers
def test_host_builders_run_clean_under_the_sanitizers(tmp_path):
    """tests/hostcheck/bvh4_san.cpp: a stand-alone program (its own main, no Python) over the same tables, built with -fsanitize=address,undefined
    for the host; it must end clean and report the sizes the library call reports."""
    d = os.path.join(ROOT, "tests", "hostcheck")
    exe, src = os.path.join(d, "bvh4_san"), os.path.join(d, "bvh4_san.cpp")
    deps = [src, os.path.join(d, "bvh4_host.h")] + [os.path.join(ROOT, "psdr-cuda_amd", "csrc", f) for f in ("psdr_math.h", "psdr_device.h", "psdr_bvh_build.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", src, "-o", exe]
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        r = subprocess.run(cmd + san, capture_output=True, text=True)
        if r.returncode != 0 and ("libclang_rt" in r.stderr or "sanitizer" in r.stderr.lower()):
            # no host sanitizer runtime beside this compiler: the program still runs the same functions over the same tables, without the instrumentation
            print("bvh4_san: built WITHOUT the sanitizers, the compiler's host runtime for them is missing:\n" + r.stderr[-800:])
            r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, "bvh4_san does not compile:\n" + r.stderr[-3000:]
    tables = [(n, ml, False) for n in ("ladder_R38", "one_cell_1001", "planar_x", "with_degenerates", "one_cell_65") for ml in (1, 4, 8)]
    tables += [(n, 4, True) for n in FORESTS]
    path = str(tmp_path / "tables.bin")
    want = []
    with open(path, "wb") as f:
        f.write(np.int32(len(tables)).tobytes())
        for name, ml, forest in tables:
            rows, mesh_of, t = built(name, ml, forest)
            f.write(np.array([rows.shape[0], int(mesh_of.max()) + 1, ml, int(forest)], np.int32).tobytes())
            f.write(np.ascontiguousarray(rows, np.float32).tobytes())
            f.write(np.ascontiguousarray(mesh_of, np.int32).tobytes())
            want.append([len(t["nodes"]), len(t["btris"]), len(t["roots2"]), t["n4"], t["stack_need"], len(t["inline"]), int(t["forest"]), t["depth"]])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    got = [[int(x) for x in line.split()] for line in r.stdout.strip().splitlines()]
    assert [g[:8] for g in got] == want
