"""The inputs of tests/test_device_bvh_cases_gpu.py held to their promises (tests/lbvh_cases.py) by the references alone -- no GPU, no
product kernel: the tables psdr_cuda.Scene makes of every family carry the cells the generator meant, ref_depth agrees with hand counts
and with the depths a transcription of k_lbvh_hierarchy gave, the ray sets stay inside the caps the GPU tests allow for excluded rays."""
import numpy as np
import pytest

import lbvh_cases as L

ALL = sorted(L.FAMILIES)
FULL = (1 << 30) - 1             # the far corner's key


@pytest.mark.parametrize("name", ALL)
def test_tables_carry_the_intended_cells(name):
    c = L.case(name)
    v, f, rows = c.verts.astype(np.float64), c.faces, c.rows.astype(np.float64)
    # on the grid, inside the box, pinned by the two corners; the rows are the vertices, exactly
    assert np.array_equal(v * L.U, np.rint(v * L.U)) and v.min() >= 0 and v.max() <= 1024
    assert np.array_equal(rows[:, 0:3], v[f[:, 0]]) and np.array_equal(rows[:, 3:6], v[f[:, 1]] - v[f[:, 0]]) and np.array_equal(rows[:, 6:9], v[f[:, 2]] - v[f[:, 0]])
    ext = v.max(axis=0) - v.min(axis=0)
    assert [e for k, e in enumerate(ext) if k != c.planar_axis] == [1024.0] * (3 if c.planar_axis is None else 2)
    if c.planar_axis is not None:
        assert ext[c.planar_axis] == 0.0 and 290 <= f.shape[0] <= 310
    keys = L.ref_keys(c.rows)
    assert np.array_equal(keys, L.meant_keys(c.verts, c.faces, c.planar_axis))
    assert (rows[:, 21] == 0).sum() == L.degenerate_faces(c.verts, c.faces).sum()           # column 21: the area
    s = np.sort(keys)
    uniq, first, counts = np.unique(s, return_index=True, return_counts=True)
    if name.startswith("ladder"):
        R = {"ladder_1": 1, "ladder_5": 5, "ladder_R38": L.R38, "ladder_R39": L.R39}[name]
        assert s.tolist() == [0] * R + [1 << b for b in range(30)] + [FULL]
    elif name.startswith("one_cell"):
        T = int(name.split("_")[-1])
        assert s.tolist() == [0] * (T - 1) + [FULL]
    elif name == "runs":
        assert counts.tolist() == L.RUN_LENGTHS and f.shape[0] == 200
        follows = {(a, b) for a, b in zip(L.RUN_LENGTHS, L.RUN_LENGTHS[1:])}
        assert (4, 5) in follows and (8, 9) in follows and set(counts.tolist()) == set(range(1, 10))
        for length in (5, 9):                             # runs across the leaf limit begin at even AND at odd positions
            assert {int(p) % 2 for p, n in zip(first, counts) if n == length} == {0, 1}
        assert not np.array_equal(keys, s)                # the table is not in Morton order
    elif name == "two_clusters":
        assert f.shape[0] == 1000 and uniq.size <= 16 and (keys < 64).sum() == 500 and (keys >= FULL - 63).sum() == 500
        edge = np.linalg.norm(rows[:, 3:6], axis=1)
        assert np.median(edge) == 2.0 ** -5
    elif name == "with_degenerates":
        dead = rows[:, 21] == 0
        assert f.shape[0] == 300 and dead.sum() == 30
        assert set(keys[dead].tolist()) <= set(keys[~dead].tolist())        # in cells that live triangles occupy
        pts = ~rows[dead][:, 3:9].any(axis=1)
        assert 10 <= pts.sum() <= 20                      # point faces and collinear faces
    elif name.startswith("uniform"):
        assert f.shape[0] == int(name.split("_")[-1]) and uniq.size > 0.99 * f.shape[0]


@pytest.mark.parametrize("T,depth", [(5, 1), (6, 2), (9, 2), (10, 3), (17, 3), (65, 5), (255, 7), (256, 7), (257, 7), (1001, 9)])
def test_ref_depth_agrees_with_a_hand_count_on_one_cell(T, depth):
    """T - 1 equal keys at positions 0 .. T - 2, one key above them.  By hand: the root splits the far corner off (1 node).  A run of n equal keys
    at positions 0 .. n - 1 is a leaf for n <= 4; otherwise the highest bit in which 0 and n - 1 differ is k = floor(log2(n - 1)), the left part is the
    full block of 2^k positions -- which halves k - 2 times before its parts hold 4 -- and the right part is no larger: 1 + (k - 2) nodes deep.
    T = 5: 1.  T = 6: n = 5, k = 2: 2.  T = 9: n = 8, k = 2: 2.  T = 10: n = 9, k = 3: 3.  T = 17: n = 16, k = 3: 3.  T = 65: n = 64, k = 5: 5.
    T = 255, 256, 257: n = 254, 255, 256, k = 7: 7.  T = 1001: n = 1000, k = 9: 9."""
    keys = np.array([0] * (T - 1) + [FULL])
    assert L.ref_depth(keys) == depth
    n = T - 1
    assert depth == 1 + (0 if n <= 4 else int(np.floor(np.log2(n - 1))) - 1)
    v, f = L.one_cell(T)
    assert L.ref_depth(L.meant_keys(v, f)) == depth
    # a run that does not start at position 0 is split by OTHER bits: the same five keys one place further on
    assert L.ref_depth(np.array([0] * 5 + [FULL])) == 2 and L.ref_depth(np.array([0] * 3 + [1] * 5 + [FULL])) == 3


def ladder_keys(R):
    return np.array([0] * R + [1 << b for b in range(30)] + [FULL])


def test_ladder_depths_and_the_two_sides_of_the_depth_limit():
    """A transcription of k_lbvh_hierarchy run in Python gave 27 at R = 1, 30 at R = 4, 31 at R = 5, 38 at R = 1024, 39 at R = 1025: the independent
    reference agrees.  R38 = 1024 is the LARGEST R of depth 38 (the depth does not decrease with R: a longer run of zeros only adds positions), so
    ladder(R38) is the deepest tree the device builder keeps (kBvhStack - 2 = 38) and ladder(R39) the first it hands to the host builder."""
    got = {R: L.ref_depth(ladder_keys(R)) for R in (1, 4, 5, 512, 513, 1023, 1024, 1025, 1026, 1400, 2049)}
    assert [got[R] for R in (1, 4, 5, 1024, 1025)] == [27, 30, 31, 38, 39], got
    assert list(got.values()) == sorted(got.values()) and got[513] == 38 and got[512] == 37 and got[2049] == 40, got
    assert (L.R38, L.R39) == (1024, 1025)
    for R in (L.R38, L.R39):
        v, f = L.ladder(R)
        assert f.shape[0] == R + 31 and L.ref_depth(L.meant_keys(v, f)) == got[R]


def test_ref_depth_rejects_nothing_and_loses_nothing():
    """every triangle in exactly one leaf (checked inside ref_depth) on random keys with many ties; the depth of distinct keys 0 .. 2^k - 1 is k - 2"""
    rng = np.random.default_rng(0)
    for n in (5, 6, 33, 1000):
        L.ref_depth(rng.integers(0, 7, n))
    assert L.ref_depth(np.arange(256)) == 6 and L.ref_depth(np.arange(256)[::-1]) == 6


def check_caps(name, rows, rays, bf, own_probes=True):
    """the caps of the GPU tests, by brute_force alone"""
    o, d, owner = rays
    tie, excl = bf["near_tie"].mean(), (bf["near_tie"] | bf["near_edge"]).mean()
    print("%s: %d rays, near ties %.4f %%, excluded %.4f %%, hits %.1f %%" % (name, o.shape[0], 100 * tie, 100 * excl, 100 * (bf["tri"][:, 0] >= 0).mean()))
    assert tie < 0.001, tie                             # half of the 0.2 % the device-against-host comparison allows
    assert excl <= 0.002, excl
    # every probe ray's answer is its own triangle, and each live triangle keeps at least one probe ray outside the exclusions
    probe = owner >= 0
    clean = probe & ~bf["near_tie"] & ~bf["near_edge"]
    if own_probes:
        assert np.array_equal(bf["tri"][clean, 0], owner[clean])
        live = np.nonzero(rows[:, 21] > 0)[0]
        assert np.array_equal(np.unique(owner[clean]), live)
    assert (bf["tri"][~probe, 0] >= 0).mean() > 0.1      # the random rays do go through the occupied region
    dead = np.nonzero(rows[:, 21] == 0)[0]
    assert not np.isin(bf["tri"], dead).any()


@pytest.mark.parametrize("name", ALL)
def test_ray_sets_stay_inside_the_caps(name):
    c = L.case(name)
    check_caps(name, c.rows, c.rays, c.bf)


@pytest.mark.parametrize("name", L.REFIT_FAMILIES)
def test_ray_sets_of_the_moved_tables_stay_inside_the_caps(name):
    c = L.case(name)
    rows, rays, bf = L.moved(c)
    assert not np.array_equal(rows[:, 0:3], c.rows[:, 0:3]) and np.array_equal(rows[:, 3:], c.rows[:, 3:])
    assert rows[:, 0:3].min() >= 0 and (rows[:, 0:3] + np.maximum(0, np.maximum(rows[:, 3:6], rows[:, 6:9]))).max() <= 1024
    assert np.array_equal(rows[:, 0:3] * L.U, np.rint(rows[:, 0:3] * L.U))
    # the topology of the standing tree is unrelated to the moved geometry: hardly a triangle keeps its cell
    if name in ("runs", "two_clusters"):
        assert (L.ref_keys(rows) == L.ref_keys(c.rows)).mean() < 0.2
    # (a moved triangle may come to lie right in front of another one's probe ray: the probes are ordinary rays here)
    check_caps(name + " (moved)", rows, rays, bf, own_probes=False)


def test_brute_force_against_one_triangle_at_a_time():
    """brute_force drops most pairs by a first pass of matrix products and sorts the rest per ray; here the textbook loop, one triangle at a time, on a
    family near the origin and on one whose second half sits at 1024: same hits, same (t, u, v) to 1e-9 (float32 resolves 1e-7 of them at best)."""
    for name in ("one_cell_65", "two_clusters"):
        c = L.case(name)
        o, d = (x[::11].astype(np.float64) for x in c.rays[:2])
        r = c.rows.astype(np.float64)
        best = np.full((o.shape[0], 4), np.inf)                 # t, tri, u, v
        for i in range(r.shape[0]):
            p0, e1, e2 = r[i, 0:3], r[i, 3:6], r[i, 6:9]
            h = np.cross(d, e2)
            det = h @ e1
            s = o - p0
            q = np.cross(s, e1)
            with np.errstate(divide="ignore", invalid="ignore"):
                u, v, t = (s * h).sum(1) / det, (d * q).sum(1) / det, (q @ e2) / det
            hit = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= L.RAY_EPSILON) & (t < best[:, 0])
            best[hit] = np.stack([t, np.full_like(t, i), u, v], 1)[hit]
        bf = L.brute_force(c.rows, o, d)
        clear = ~bf["near_edge"] & ~bf["near_tie"]
        assert clear.mean() > 0.99
        tri = np.where(np.isfinite(best[:, 0]), best[:, 1], -1).astype(np.int64)
        assert np.array_equal(tri[clear], bf["tri"][clear, 0])
        hit = clear & (tri >= 0)
        assert hit.sum() > 300
        for k, col in (("t", 0), ("u", 2), ("v", 3)):
            assert np.abs(bf[k][hit, 0] - best[hit, col]).max() < 1e-9, k


@pytest.mark.parametrize("name", [n for n in ALL if not (n.startswith("one_cell") and int(n.split("_")[-1]) <= 16)])
def test_the_float32_triangle_test_on_the_host_answers_every_clear_ray_as_brute_force_does(name):
    """The error model behind near_edge / near_tie, held against the product's own float32 triangle test without a GPU: closest_hit compiled for
    the host (tests/hostcheck) over the host builder's tree names brute_force's triangle on every ray brute_force does not exclude, and misses where
    it misses.  (This is also the host builder on these inputs: the GPU tests use its tree as the yardstick of the device builder's.)"""
    import ctypes as C
    import torch
    from helpers import hostcheck_lib, make_desc
    c = L.case(name)
    o, d, owner = c.rays
    H = hostcheck_lib()
    tbc = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in c.tb.items()}
    desc, keep = make_desc(tbc, None, device="cpu")
    m = o.shape[0]
    tri, u, v = np.zeros(m, np.int32), np.zeros(m, np.float32), np.zeros(m, np.float32)
    oo, dd = np.ascontiguousarray(o), np.ascontiguousarray(d)
    assert H.hostcheck_trace(C.byref(desc), m, C.c_void_p(oo.ctypes.data), C.c_void_p(dd.ctypes.data), C.c_void_p(tri.ctypes.data),
                             C.c_void_p(u.ctypes.data), C.c_void_p(v.ctypes.data)) == 0
    clear = ~(c.bf["near_edge"] | c.bf["near_tie"])
    wrong = clear & (tri != c.bf["tri"][:, 0])
    assert not wrong.any(), (int(wrong.sum()), np.nonzero(wrong)[0][:5])
    hit = clear & (tri >= 0)
    du, dv = np.abs(u[hit] - c.bf["u"][hit, 0]).max(), np.abs(v[hit] - c.bf["v"][hit, 0]).max()
    print("%s: float32 on the host off the brute force by %.2e in u, %.2e in v" % (name, du, dv))
    # on the excluded rays float32 still names one of the float64 candidates or a triangle the model calls possible
    odd = np.nonzero(~clear & (tri >= 0) & (tri != c.bf["tri"][:, 0]) & (tri != c.bf["tri"][:, 1]))[0]
    if odd.size:
        assert L.pair_test(c.rows, o[odd], d[odd], tri[odd])["possible"].all()
