"""Adversarial inputs for the device tree builder (csrc/psdr_lbvh.h) and plain references to judge it by.  No tests in here:
tests/test_lbvh_cases.py holds the inputs to their promises on the CPU, tests/test_device_bvh_cases_gpu.py runs the builder on them.

THE GRID.  Every coordinate is a multiple of 2^-6 inside [0, 1024]^3 (the generators work in integer UNITS of 2^-6 and divide once), so
p0 + (p1 - p0) is exact in float32.  Two corner triangles, one touching (0, 0, 0) and one touching (1024, 1024, 1024), pin the scene bounds:
the quantised cell of a triangle is the integer part of its box centre, exactly -- (c - 0) / 1024 * 1024 has no rounding for the builder
to disagree about.  A cell is a unit cube; what shares a cell shares a Morton key, and the tree under equal keys is decided by the
positions in the sorted array alone (lbvh_delta's tie term).

Triangles are well shaped (legs of 8 units with a small tilt; 2 units in two_clusters), and no two are coplanar and overlapping:
triangles that share a cell are parallel layers one unit apart, or sit in disjoint slots of the cell's footprint."""
import numpy as np

U = 64                       # units per 1.0
BOX = 1024 * U               # the far corner, in units
LEAF = 4                     # kLbvhLeaf


# ---------------------------------------------------------------- pieces
def _corner_pair():
    near = np.array([[0, 0, 0], [6, 0, 1], [0, 6, 2]], np.int64)
    return near, BOX - near


def _stack(cell, n, first=0):
    """n triangles (numbers first .. first + n - 1) inside the unit cell `cell`: 25 slots of the footprint (pitch 10, from 8: clear of a
    corner triangle, which keeps to [0, 6] / [58, 64]), 58 parallel layers per slot one unit apart.  Box centres stay inside the cell."""
    k = np.arange(first, first + n, dtype=np.int64)
    assert k.size == 0 or k.max() < 25 * 58
    layer, slot = k % 58, k // 58
    a0, b0, h0 = 8 + 10 * (slot % 5), 8 + 10 * (slot // 5), 2 + layer
    base = np.asarray(cell, np.int64) * U
    tri = np.stack([np.stack([a0, b0, h0], 1), np.stack([a0 + 8, b0, h0 + 1], 1), np.stack([a0, b0 + 8, h0 + 2], 1)], 1)
    return tri + base


def _finish(tris):
    tris = np.concatenate([np.asarray(t, np.int64).reshape(-1, 3, 3) for t in tris])
    assert tris.min() >= 0 and tris.max() <= BOX
    verts = (tris.reshape(-1, 3).astype(np.float64) / U).astype(np.float32)
    assert np.array_equal(verts.astype(np.float64) * U, tris.reshape(-1, 3))          # on the grid, exactly
    return verts, np.arange(verts.shape[0], dtype=np.int32).reshape(-1, 3)


def morton3(q):
    """30-bit key of integer cells q[:, 3] (10 bits per axis, interleaved x y z: x holds the highest bit)"""
    q = np.asarray(q, np.int64)
    key = np.zeros(q.shape[0], np.int64)
    for b in range(10):
        for k in range(3):
            key |= ((q[:, k] >> b) & 1) << (3 * b + 2 - k)
    return key


def cell_of_key(key):
    q = [0, 0, 0]
    for b in range(30):
        if (int(key) >> b) & 1:
            q[2 - b % 3] |= 1 << (b // 3)
    return q


def meant_keys(verts, faces, planar_axis=None):
    """The keys a family is MEANT to have, in integer arithmetic on the grid (no float32, none of ref_keys' steps): cell = floor of the box
    centre, the far corner's 1024 clamped to 1023; an axis without extent quantises to cell 0."""
    tri = np.rint(np.asarray(verts, np.float64)[np.asarray(faces)] * U).astype(np.int64)          # [T, 3, 3] units
    twice = tri.min(axis=1) + tri.max(axis=1)
    q = np.minimum(twice // (2 * U), 1023)
    if planar_axis is not None:
        q[:, planar_axis] = 0
    return morton3(q)


def degenerate_faces(verts, faces):
    tri = np.rint(np.asarray(verts, np.float64)[np.asarray(faces)] * U).astype(np.int64)
    return ~np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).any(axis=1)


# ---------------------------------------------------------------- the families
def ladder(R):
    """One triangle in the cell of key 1 << (29 - m) for m = 0..29, R triangles in cell 0 (the near corner among them), the far corner.
    Every level of the radix tree peels one key off: 30 levels before the run of equal keys even starts."""
    near, far = _corner_pair()
    tris = [near, _stack((0, 0, 0), R - 1)]
    for m in range(30):
        tris.append(_stack(cell_of_key(1 << (29 - m)), 1))
    tris.append(far)
    return _finish(tris)


ONE_CELL_SIZES = (5, 6, 9, 10, 17, 65, 255, 256, 257, 1001)


def one_cell(T):
    """T - 1 layered triangles in cell 0 (the near corner among them) + the far corner: T - 1 equal keys."""
    near, far = _corner_pair()
    return _finish([near, _stack((0, 0, 0), T - 2), far])


RUN_LENGTHS = ([1, 2, 3, 4, 5, 6, 7, 8, 9] + [9, 8, 7, 6, 5, 4, 3, 2, 1] + [4, 5, 8, 9, 1, 8, 9, 4, 5, 2, 7, 3, 6] + [5, 4, 9, 8] + [3, 1, 6, 2] + [1])


def runs():
    """200 triangles whose sorted keys form runs of the lengths RUN_LENGTHS, in that order: the first run is cell 0 (the near corner alone), the
    last the far corner alone, the others sit in random cells and in groups of neighbouring cells.  Runs of 5 and 9 follow runs of 4 and 8, at even and at odd positions."""
    rng = np.random.default_rng(41)
    n = len(RUN_LENGTHS) - 2
    # six groups of five cells with CONSECUTIVE keys (neighbouring keys share up to 29 bits: more than two positions of a run share), the rest anywhere
    keys = set()
    for base in rng.integers(1, 1 << 27, 6) * 8:
        keys.update(int(base) + k for k in range(5))
    while len(keys) < n:
        k = int(rng.integers(1, (1 << 30) - 1))
        if not any(abs(k - x) < 8 for x in keys):
            keys.add(k)
    cells = [tuple(cell_of_key(k)) for k in sorted(keys)]
    near, far = _corner_pair()
    tris = [near]
    for c, length in zip(cells, RUN_LENGTHS[1:-1]):
        tris.append(_stack(c, length))
    tris.append(far)
    # (shuffled: the table order must not be the Morton order)
    verts, faces = _finish(tris)
    return verts, faces[rng.permutation(faces.shape[0])]


def planar(axis):
    """About 300 triangles in ONE plane normal to `axis` (coordinate 512), the corner triangles moved into it: the scene extent in that axis is
    exactly 0.  Random cells of the plane hold 1..7 triangles each, in disjoint slots."""
    rng = np.random.default_rng(50 + axis)
    a, b = [k for k in range(3) if k != axis]

    def lift(flat):                                  # [n, 3, 2] in-plane units -> [n, 3, 3]
        out = np.full(flat.shape[:2] + (3,), 512 * U, np.int64)
        out[..., a], out[..., b] = flat[..., 0], flat[..., 1]
        return out
    corner = np.array([[0, 0], [6, 0], [0, 6]], np.int64)
    tris = [lift(corner[None]), lift((BOX - corner)[None])]
    cells, total = set(), 2
    while total < 300:
        c = tuple(int(x) for x in rng.integers(0, 1024, 2))
        if c in cells:
            continue
        cells.add(c)
        n = int(rng.integers(1, 8))
        slot = rng.permutation(25)[:n]
        a0, b0 = 8 + 10 * (slot % 5) + c[0] * U, 8 + 10 * (slot // 5) + c[1] * U
        tris.append(lift(np.stack([np.stack([a0, b0], 1), np.stack([a0 + 8, b0], 1), np.stack([a0, b0 + 8], 1)], 1)))
        total += n
    verts, faces = _finish(tris)
    return verts, faces[rng.permutation(faces.shape[0])]


def two_clusters():
    """500 triangles of size 2^-5 in each of two opposite corners of the box (the second cluster is the point reflection of the first): each
    cluster falls into the eight cells around its corner."""
    rng = np.random.default_rng(60)
    seen, tri = set(), []
    while len(tri) < 499:
        sa, sb, h = (int(x) for x in (rng.integers(0, 32), rng.integers(0, 32), rng.integers(0, 127)))
        if (sa < 2 and sb < 2) or (sa, sb, h) in seen:          # the corner triangle's footprint; one triangle per (slot, layer)
            continue
        seen.add((sa, sb, h))
        a0, b0 = 4 * sa, 4 * sb
        tri.append([[a0, b0, h], [a0 + 2, b0, h], [a0, b0 + 2, h + 1]])
    near, far = _corner_pair()
    tri = np.asarray(tri, np.int64)
    verts, faces = _finish([near, tri, BOX - tri, far])
    return verts, faces[rng.permutation(faces.shape[0])]


def with_degenerates():
    """A 300-triangle soup of small stacks in random cells; 30 of its faces have zero area (15 points, 15 collinear triples) and sit in cells
    that live triangles occupy."""
    rng = np.random.default_rng(70)
    near, far = _corner_pair()
    tris, cells, total = [near, far], [(0, 0, 0)], 2
    while total < 270:
        c = tuple(int(x) for x in rng.integers(0, 1023, 3))
        if c in cells:
            continue
        n = min(int(rng.integers(1, 10)), 270 - total)
        cells.append(c)
        tris.append(_stack(c, n))
        total += n
    for i in range(30):
        base = np.asarray(cells[int(rng.integers(0, len(cells)))], np.int64) * U
        p = base + rng.integers(1, 40, 3)
        step = np.array([1, 2, 1], np.int64) * int(rng.integers(1, 10))
        tris.append(np.stack([p, p, p]) if i % 2 == 0 else np.stack([p, p + step, p + 2 * step]))
    verts, faces = _finish(tris)
    return verts, faces[rng.permutation(faces.shape[0])]


def uniform(T):
    """The control: T - 2 random well-shaped triangles of ~10 units of length across the box + the corners."""
    rng = np.random.default_rng(80 + T)
    near, far = _corner_pair()
    out = []
    while len(out) < T - 2:
        c = rng.integers(20 * U, 1004 * U, 3)
        t = c + rng.integers(-12 * U, 12 * U + 1, (3, 3))
        e = np.stack([t[1] - t[0], t[2] - t[1], t[0] - t[2]]).astype(np.float64)
        if np.linalg.norm(np.cross(e[0], e[1])) > 0.3 * (np.linalg.norm(e, axis=1).max() ** 2):          # no slivers
            out.append(t)
    return _finish([near, np.asarray(out, np.int64), far])


PLANAR_AXIS = {"planar_x": 0, "planar_y": 1, "planar_z": 2}
R38, R39 = 1024, 1025           # ladder: the deepest tree the device builder keeps / the shallowest it hands to the host (tests/test_lbvh_cases.py)
FAMILIES = {"ladder_1": lambda: ladder(1), "ladder_5": lambda: ladder(5), "ladder_R38": lambda: ladder(R38), "ladder_R39": lambda: ladder(R39),
            "runs": runs, "planar_x": lambda: planar(0), "planar_y": lambda: planar(1), "planar_z": lambda: planar(2),
            "two_clusters": two_clusters, "with_degenerates": with_degenerates, "uniform_1000": lambda: uniform(1000), "uniform_5000": lambda: uniform(5000)}
FAMILIES.update({"one_cell_%d" % T: (lambda T=T: one_cell(T)) for T in ONE_CELL_SIZES})


# ---------------------------------------------------------------- scenes and tables
def make_scene(verts, faces, res=8, spp=1, eye=(6.0, 5.0, 9.0), target=(0.5, 0.5, 0.5), fov=40.0, quad=None):
    """The soup as ONE mesh of a psdr_cuda.Scene (face normals, no edge lists: a soup is no manifold).  Without `quad` the soup itself
    emits; with quad = (verts, faces) that second mesh is the emitter and the soup a diffuse receiver."""
    import psdr_cuda
    from psdr_cuda.scene import look_at
    sc = psdr_cuda.Scene()
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, 0, 0, 0
    cam = psdr_cuda.PerspectiveCamera(fov, 0.01, 1e4)
    cam.to_world = look_at(list(eye), list(target), [0, 1, 0])
    sc.add_sensor(cam)
    grey = psdr_cuda.Diffuse([0.5, 0.6, 0.7]); grey.id = "grey"
    sc.add_bsdf(grey)
    m = psdr_cuda.Mesh()
    m.use_face_normals = True
    m.enable_edges = False
    m.set_geometry(np.asarray(verts, np.float32), np.asarray(faces, np.int32))
    sc.add_mesh(m, grey, emitter_radiance=None if quad is not None else [3.0, 2.0, 1.0])
    if quad is not None:
        black = psdr_cuda.Diffuse([0.0, 0.0, 0.0]); black.id = "black"
        sc.add_bsdf(black)
        m2 = psdr_cuda.Mesh()
        m2.use_face_normals = True
        m2.enable_edges = False
        m2.set_geometry(np.asarray(quad[0], np.float32), np.asarray(quad[1], np.int32))
        sc.add_mesh(m2, black, emitter_radiance=[40.0, 30.0, 20.0])
    sc.finalize()
    sc.configure()
    return sc


def table_rows(tb):
    return tb["tri_info"].detach().cpu().numpy()


# ---------------------------------------------------------------- references
def ref_keys(tri_info):
    """The builder's 30-bit keys from the table rows (p0, e1, e2 in columns 0:9), as the header of csrc/psdr_lbvh.h describes them, in float32:
    box of p0, p0 + e1, p0 + e2; scene bounds; centre of the box relative to the scene box, 10 bits per axis (an axis without extent: 0),
    interleaved x y z."""
    r = np.asarray(tri_info, np.float32)
    p, q, w = r[:, 0:3], r[:, 0:3] + r[:, 3:6], r[:, 0:3] + r[:, 6:9]
    lo, hi = np.minimum(p, np.minimum(q, w)), np.maximum(p, np.maximum(q, w))
    slo, ext = lo.min(axis=0), hi.max(axis=0) - lo.min(axis=0)
    c = np.float32(0.5) * (lo + hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ext > 0, (c - slo) / ext, np.float32(0)).astype(np.float32)
    cell = np.minimum(np.maximum(t * np.float32(1024), np.float32(0)), np.float32(1023)).astype(np.int64)
    return morton3(cell)


def ref_depth(keys):
    """Depth of the radix tree over the keys, top-down: stable-sort; a range of <= 4 triangles is a leaf, any other range is an inner node that
    splits where the highest bit in which its first and last augmented keys (key << 32) | position differ changes.  Depth = inner nodes on
    the longest root-to-leaf path.  Checks that every triangle ends up in exactly one leaf."""
    keys = np.asarray(keys, np.int64)
    order = np.argsort(keys, kind="stable")
    aug = [(int(k) << 32) | i for i, k in enumerate(keys[order])]
    T = len(aug)
    in_leaf = np.zeros(T, np.int64)

    def walk(a, b):                                  # [a, b)
        if b - a <= LEAF:
            in_leaf[order[a:b]] += 1
            return 0
        bit = (aug[a] ^ aug[b - 1]).bit_length() - 1
        s = a
        while not (aug[s] >> bit) & 1:               # sorted, and equal above `bit`: zeros, then ones
            s += 1
        assert a < s < b and all((aug[i] >> bit) & 1 for i in range(s, b))
        return 1 + max(walk(a, s), walk(s, b))
    depth = walk(0, T)
    assert (in_leaf == 1).all(), "a triangle is in %s leaves" % sorted(set(in_leaf.tolist()))
    return depth


RAY_EPSILON = 1e-3              # csrc/psdr_math.h kRayEpsilon: hits start here
EPS32 = float(np.finfo(np.float32).eps)


def _pairs(o, d, p0, e1, e2):
    """The Moeller-Trumbore numerators of ray k against triangle k, float64, D made positive (signs flipped along), and the float32 error bounds
    of each (see brute_force)."""
    s = o - p0
    h, q = np.cross(d, e2), np.cross(s, e1)
    D = (e1 * h).sum(1)
    sg = np.where(D < 0, -1.0, 1.0)
    D, Nu, Nv, Nt = D * sg, (s * h).sum(1) * sg, (d * q).sum(1) * sg, (e2 * q).sum(1) * sg
    nh, nq = np.linalg.norm(h, axis=1), np.linalg.norm(q, axis=1)
    k8 = 8 * EPS32
    return (D, Nu, Nv, Nt, k8 * np.linalg.norm(e1, axis=1) * nh, k8 * np.linalg.norm(s, axis=1) * nh, k8 * np.linalg.norm(d, axis=1) * nq,
            k8 * np.linalg.norm(e2, axis=1) * nq)


def pair_test(tri_info, o, d, tri):
    """ray k against triangle tri[k] alone: t, its tolerance, and whether a float32 evaluation could call it a hit at all (brute_force's error model)"""
    r = np.asarray(tri_info, np.float64)[np.asarray(tri)]
    D, Nu, Nv, Nt, b, au, av, at = _pairs(np.asarray(o, np.float64), np.asarray(d, np.float64), r[:, 0:3], r[:, 3:6], r[:, 6:9])
    pos = (Nu + au >= 0) & (Nv + av >= 0) & ((Nu - au) + (Nv - av) <= D + b) & (Nt + at >= RAY_EPSILON * np.maximum(D - b, 0.0))
    neg = (D - b <= 0) & (Nu - au <= 0) & (Nv - av <= 0) & ((Nu + au) + (Nv + av) >= D - b) & (Nt - at <= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = Nt / D
        return dict(t=t, tol_t=(at + np.abs(t) * b) / D, possible=(pos | neg) & (r[:, 21] > 0))


def brute_force(tri_info, o, d, chunk=None, exclude=None):
    """Float64 Moeller-Trumbore of every ray against every triangle: per ray the two smallest t >= RayEpsilon with their triangle ids and
    barycentrics (id -1, t inf where there is none); zero-area faces never hit.  exclude: [m, 2] triangle ids (or -1) ray k does not see at all
    (a ray that starts on a secondary edge and ignores the edge's two faces).

    The test, with s = o - p0, h = d x e2, q = s x e1:  D = e1.h,  Nu = s.h,  Nv = d.q,  Nt = e2.q,  (u, v, t) = (Nu, Nv, Nt) / D.
    Two passes per chunk of rays.  (1) ALL pairs: D, Nu, Nv as matrix products (each triple product is linear in s = o - p0: D = -d.n with
    n = e1 x e2, Nu = e2.(o x d) - d.(e2 x p0), Nv = d.(e1 x p0) - e1.(o x d)), only to DROP the pairs whose (u, v) is outside the triangle by more
    than any tolerance below could bridge.  (2) The pairs that are left: the test as written above, in float64, and its float32 error model.

    Which rays may a FLOAT32 evaluation answer differently?  Each of D, Nu, Nv, Nt is a sum of six products; float32 gets them to within
        b = 8 eps32 |e1||h|,  au = 8 eps32 |s||h|,  av = 8 eps32 |d||q|,  at = 8 eps32 |e2||q|        (about ten roundings of half an ulp each, first order;
    s itself is exact or relatively exact: o and p0 share the grid of the larger of them).  With D made positive (signs flipped along), a pair is a
        SURE hit  when D - b > 0 and u, v, 1 - u - v > 0, t > RayEpsilon hold for EVERY value inside those intervals,
        POSSIBLE  when they hold for SOME value (a D whose interval contains 0 may take either sign),  UNSURE = possible, not sure.
    t of a sure hit is known to tol_t = (at + t b) / D.
        near_edge: an unsure pair could lie in front of the ray's first sure hit (t < t1 + tol_t1 for some value in the intervals)
        near_tie:  the first two sure hits are closer in t than their tolerances together
    On every other ray float32 has one answer, whatever the order the triangles are tested in: the first sure hit."""
    r = np.asarray(tri_info, np.float64)
    p0, e1, e2 = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    T = r.shape[0]
    nrm = np.cross(e1, e2)
    live = nrm.any(axis=1)
    ne1, ne2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    e2p0, e1p0 = np.cross(e2, p0), np.cross(e1, p0)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    m = o.shape[0]
    chunk = chunk or max(1, 2_000_000 // max(T, 1))
    out = dict(t=np.full((m, 2), np.inf), tri=np.full((m, 2), -1, np.int64), u=np.zeros((m, 2)), v=np.zeros((m, 2)),
               near_edge=np.zeros(m, bool), near_tie=np.zeros(m, bool))
    k8 = 8 * EPS32
    # pass 1 keeps a pair unless it is outside by more than the LARGEST tolerance any pair of this call can have (|s| <= reach)
    reach = np.abs(o).max() + np.abs(p0).max() + np.abs(e1).max() + np.abs(e2).max()
    amax = k8 * np.sqrt(3.0) * reach * np.linalg.norm(d, axis=1).max() * max(ne1.max(), ne2.max())
    for i0 in range(0, m, chunk):
        oo, dd = o[i0:i0 + chunk], d[i0:i0 + chunk]
        od = np.cross(oo, dd)
        D = -(dd @ nrm.T)
        sg = np.sign(D)
        Nu = (od @ e2.T - dd @ e2p0.T) * sg
        Nv = (dd @ e1p0.T - od @ e1.T) * sg
        np.abs(D, out=D)
        keep = (Nu >= -amax) & (Nv >= -amax) & (Nu + Nv <= D + 3.0 * amax) & live[None]
        ri, ti = np.nonzero(keep)
        del D, Nu, Nv, sg, keep
        if exclude is not None:
            ex = np.asarray(exclude, np.int64)[i0:i0 + chunk]
            seen = (ti != ex[ri, 0]) & (ti != ex[ri, 1])
            ri, ti = ri[seen], ti[seen]
        # pass 2: the test itself on what is left
        D, Nu, Nv, Nt, b, au, av, at = _pairs(oo[ri], dd[ri], p0[ti], e1[ti], e2[ti])
        sure = (D - b > 0) & (Nu - au > 0) & (Nv - av > 0) & ((D - b) - (Nu + au) - (Nv + av) > 0) & ((Nt - at) - RAY_EPSILON * (D + b) > 0)
        Ds = np.where(sure, D, 1.0)
        t, tol = np.where(sure, Nt / Ds, np.inf), np.where(sure, (at + np.abs(Nt / Ds) * b) / Ds, 0.0)
        # first and second sure hit per ray
        n = oo.shape[0]
        order = np.lexsort((t, ri))
        order = order[sure[order]]
        rs = ri[order]
        is1 = np.ones(rs.size, bool); is1[1:] = rs[1:] != rs[:-1]
        is2 = np.zeros(rs.size, bool); is2[1:] = is1[:-1] & ~is1[1:]
        t1, tol1, t2, tol2 = np.full(n, np.inf), np.zeros(n), np.full(n, np.inf), np.zeros(n)
        for c, pick in enumerate((order[is1], order[is2])):
            rr = ri[pick] + i0
            out["t"][rr, c], out["tri"][rr, c] = t[pick], ti[pick]
            out["u"][rr, c], out["v"][rr, c] = Nu[pick] / D[pick], Nv[pick] / D[pick]
            if c == 0:
                t1[ri[pick]], tol1[ri[pick]] = t[pick], tol[pick]
            else:
                t2[ri[pick]], tol2[ri[pick]] = t[pick], tol[pick]
        with np.errstate(invalid="ignore"):
            out["near_tie"][i0:i0 + n] = np.isfinite(t2) & (t2 - t1 <= tol1 + tol2)
        # unsure pairs that could come first
        lim = (t1 + tol1)[ri]
        with np.errstate(invalid="ignore"):
            front_pos = np.where(np.isfinite(lim), Nt - at <= lim * (D + b), True)
            front_neg = np.where(np.isfinite(lim), Nt + at >= lim * (D - b), True)
        pos = (Nu + au >= 0) & (Nv + av >= 0) & ((Nu - au) + (Nv - av) <= D + b) & (Nt + at >= RAY_EPSILON * np.maximum(D - b, 0.0)) & front_pos
        neg = (D - b <= 0) & (Nu - au <= 0) & (Nv - av <= 0) & ((Nu + au) + (Nv + av) >= D - b) & (Nt - at <= 0) & front_neg
        unsure = ~sure & (pos | neg)
        out["near_edge"][np.unique(ri[unsure]) + i0] = True
    return out


# ---------------------------------------------------------------- rays
def probe_rays(tri_info):
    """Six rays per non-degenerate triangle: from 2^-7 off the triangle, on either side, straight at three interior points of it."""
    r = np.asarray(tri_info, np.float64)
    p0, e1, e2 = r[:, 0:3], r[:, 3:6], r[:, 6:9]
    n = np.cross(e1, e2)
    ids = np.nonzero(n.any(axis=1))[0]
    n = n[ids] / np.linalg.norm(n[ids], axis=1, keepdims=True)
    o, d, owner = [], [], []
    for (bu, bv) in ((0.25, 0.25), (0.5, 0.2), (0.15, 0.6)):
        p = p0[ids] + bu * e1[ids] + bv * e2[ids]
        for side in (1.0, -1.0):
            o.append(p + side * 2.0 ** -7 * n); d.append(-side * n); owner.append(ids)
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32), np.concatenate(owner)


def random_rays(tri_info, m, seed):
    """m rays through the occupied region: each aims at a point within ~0.02 of a random live triangle and starts 0.5 .. 8 away from it."""
    rng = np.random.default_rng(seed)
    r = np.asarray(tri_info, np.float64)
    ids = np.nonzero(np.cross(r[:, 3:6], r[:, 6:9]).any(axis=1))[0]
    k = ids[rng.integers(0, ids.size, m)]
    b = rng.dirichlet((1.0, 1.0, 1.0), m)
    target = r[k, 0:3] + b[:, 1:2] * r[k, 3:6] + b[:, 2:3] * r[k, 6:9] + rng.normal(scale=0.02, size=(m, 3))
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = (target - d * rng.uniform(0.5, 8.0, (m, 1))).astype(np.float32)
    return o, d.astype(np.float32)


def ray_set(tri_info, seed=0, m=20_000):
    """probe rays + m random rays: (o, d, owner) with owner = the probed triangle, -1 for a random ray"""
    po, pd, owner = probe_rays(tri_info)
    ro, rd = random_rays(tri_info, m, seed)
    return np.concatenate([po, ro]), np.concatenate([pd, rd]), np.concatenate([owner, np.full(m, -1, np.int64)])


def axis_rays(tri_info, m, seed):
    """m rays with direction components that are EXACTLY zero (the first half along an axis: two zeros; the second half inside an axis plane: one) and
    origins that are exact in float32: the reciprocal direction holds infinities, and a slab test multiplies them with (plane - origin), which is
    0 * inf = NaN wherever a plane passes through the origin's coordinate.  Each ray aims at a grid point a few units beside an interior point of a
    random live triangle -- never 0 units beside it along an axis the direction is zero in, so that no ray runs inside the plane of a planar
    family.  Along those axes the origin sits OFF the unit lattice by (13, 29, 7) / 64 of a unit in (x, y, z): the legs of the families' triangles
    lie on lattice lines, their hypotenuses on x + y = integer, a wall's diagonal on x = y, and the planes of a stack rise by 1/8 and 1/4 per unit -- a ray
    on the lattice (or a simple fraction off it) would meet an edge every other time."""
    rng = np.random.default_rng(seed)
    r = np.asarray(tri_info, np.float64)
    ids = np.nonzero(np.cross(r[:, 3:6], r[:, 6:9]).any(axis=1))[0]
    k = ids[rng.integers(0, ids.size, m)]
    b = rng.dirichlet((1.0, 1.0, 1.0), m)
    p = np.rint((r[k, 0:3] + b[:, 1:2] * r[k, 3:6] + b[:, 2:3] * r[k, 6:9]) * U)                     # units
    d = rng.normal(size=(m, 3))
    axis = rng.integers(0, 3, m)
    zero = np.zeros((m, 3), bool)
    half = m // 2
    zero[:half] = True
    zero[np.arange(half), axis[:half]] = False                   # along `axis`
    zero[np.arange(half, m), axis[half:]] = True                 # inside the plane normal to `axis`
    d[zero] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    beside = rng.integers(1, 4, (m, 3)) * rng.choice([-1, 1], (m, 3))
    aim = p + np.where(zero, beside, rng.integers(-3, 4, (m, 3)))
    o = np.rint(aim - d * (rng.uniform(0.5, 8.0, (m, 1)) * U))
    o[zero] = (aim + np.array([13.0, 29.0, 7.0]) / 64)[zero]
    o, d = (o / U).astype(np.float32), d.astype(np.float32)
    assert np.array_equal(o.astype(np.float64) * U * 64, np.rint(o.astype(np.float64) * U * 64)) and ((d == 0).sum(1) >= 1).all() and ((d == 0).sum(1)[:half] == 2).all()
    return o, d


def permuted_rows(tri_info, seed):
    """The refit input: every triangle translated to the place of another (a random permutation of the centroids), on the grid -- the
    translation is rounded to whole units, so the moved rows are still exact.  Returns the new p0 columns."""
    r = np.asarray(tri_info, np.float64)
    cen = r[:, 0:3] + (r[:, 3:6] + r[:, 6:9]) / 3.0
    perm = np.random.default_rng(seed).permutation(r.shape[0])
    shift = np.rint((cen[perm] - cen) * U) / U
    lo = np.minimum(0.0, np.minimum(r[:, 3:6], r[:, 6:9]))
    hi = np.maximum(0.0, np.maximum(r[:, 3:6], r[:, 6:9]))
    p = np.clip(r[:, 0:3] + shift, -lo, 1024.0 - hi)                  # (a rounded shift must not leave the box)
    return p.astype(np.float32)


# ---------------------------------------------------------------- one of everything per family, computed once per process
_cases = {}


class Case:
    """verts, faces, the scene's tables (tb), the table rows (numpy), and -- on first use -- the ray set and its brute-force answer"""
    def __init__(self, name):
        self.name = name
        self.planar_axis = PLANAR_AXIS.get(name)
        self.verts, self.faces = FAMILIES[name]()
        self.tb = make_scene(self.verts, self.faces).tables(0)
        self.rows = table_rows(self.tb)
        self._rays = self._bf = None

    @property
    def rays(self):
        if self._rays is None:
            self._rays = ray_set(self.rows, seed=len(self.name))
        return self._rays

    @property
    def bf(self):
        if self._bf is None:
            self._bf = brute_force(self.rows, self.rays[0], self.rays[1])
        return self._bf


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


REFIT_FAMILIES = ("ladder_R38", "one_cell_257", "runs", "two_clusters")
_moved = {}


def moved(c):
    """(rows, rays, brute force) of the family's table after permuted_rows: what the refit tests write into the standing handle"""
    if c.name not in _moved:
        rows = c.rows.copy()
        rows[:, 0:3] = permuted_rows(c.rows, seed=7)
        rays = ray_set(rows, seed=100 + len(c.name))
        _moved[c.name] = (rows, rays, brute_force(rows, rays[0], rays[1]))
    return _moved[c.name]


# ---------------------------------------------------------------- two-level scenes (forests): tests/test_bvh4_host.py
def make_forest_scene(meshes):
    """Several soups as the meshes of one psdr_cuda.Scene (face normals, no edge lists), all diffuse grey; nothing emits (the tables serve tree
    builds and ray queries, not renders)."""
    import psdr_cuda
    from psdr_cuda.scene import look_at
    sc = psdr_cuda.Scene()
    sc.opts.width = sc.opts.height = 8
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 0, 0, 0
    cam = psdr_cuda.PerspectiveCamera(40.0, 0.01, 1e4)
    cam.to_world = look_at([6.0, 5.0, 9.0], [0.5, 0.5, 0.5], [0, 1, 0])
    sc.add_sensor(cam)
    grey = psdr_cuda.Diffuse([0.5, 0.6, 0.7]); grey.id = "grey"
    sc.add_bsdf(grey)
    for verts, faces in meshes:
        m = psdr_cuda.Mesh()
        m.use_face_normals = True
        m.enable_edges = False
        m.set_geometry(np.asarray(verts, np.float32), np.asarray(faces, np.int32))
        sc.add_mesh(m, grey)
    sc.finalize()
    sc.configure()
    return sc


def _submesh(verts, faces):
    """the faces as a mesh of their own (its own vertex array, in face order)"""
    return np.asarray(verts)[np.asarray(faces).reshape(-1)], np.arange(3 * len(faces), dtype=np.int32).reshape(-1, 3)


ROOM_LO, ROOM_HI = -1.0, 1025.0


def _room_walls():
    """six axis-aligned rectangles (12 triangles, fan-triangulated) on the faces of [ROOM_LO, ROOM_HI]^3"""
    verts, faces = [], []
    for axis in range(3):
        a, b = [k for k in range(3) if k != axis]
        for side in (ROOM_LO, ROOM_HI):
            c = np.full((4, 3), side)
            c[:, a] = [ROOM_LO, ROOM_HI, ROOM_HI, ROOM_LO]
            c[:, b] = [ROOM_LO, ROOM_LO, ROOM_HI, ROOM_HI]
            n = len(verts)
            verts.extend(c)
            faces.extend([[n, n + 1, n + 2], [n, n + 2, n + 3]])
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def forest_meshes(name):
    """The meshes of a forest input, and which of them the forest builder is meant to give a tree (None: a single tree serves the table).
      single:<family>  the family as one mesh: one tree, nothing inline
      overlap16        the first 1034 triangles of uniform_5000: triangle i < 1024 in mesh i % 16 (16 overlapping trees of exactly 64 triangles:
                       kMaxBlas and kMinBlasTris at once), the last 10 a 17th, inline mesh
      overlap17        17 x 64 likewise: one tree too many, the table gets the single tree
      room             12 wall triangles around two_clusters, each cluster a mesh: two trees with disjoint boxes, the walls inline"""
    if name.startswith("single:"):
        return [FAMILIES[name[7:]]()], [0]
    if name in ("overlap16", "overlap17"):
        k = 16 if name == "overlap16" else 17
        verts, faces = uniform(5000)
        meshes = [_submesh(verts, faces[i:64 * k:k]) for i in range(k)]
        if k == 16:
            meshes.append(_submesh(verts, faces[1024:1034]))
        return meshes, (list(range(16)) if k == 16 else None)
    if name == "room":
        verts, faces = two_clusters()
        near = verts[faces].mean(axis=1).max(axis=1) < 512
        return [_room_walls(), _submesh(verts, faces[near]), _submesh(verts, faces[~near])], [1, 2]
    raise KeyError(name)


FOREST_INPUTS = ["single:" + n for n in ("ladder_R38", "one_cell_1001", "two_clusters", "runs", "planar_x", "planar_y", "planar_z", "with_degenerates",
                                         "uniform_5000")] + ["overlap16", "overlap17", "room"]
_forest = {}


class ForestCase:
    """meshes, the tables of the scene (tb), the table rows, the
    mask of the triangles that are meant to sit in a tree, and -- on first use -- the ray set (the family's own + axis_rays), its brute force over the
    whole table (bf) and over the tree triangles alone (bf_tree: what a walk of the trees alone, such as the dense trace kernel's, answers)."""
    def __init__(self, name):
        self.name = name
        self.meshes, self.tree_meshes = forest_meshes(name)
        self._tb = None
        self.family = case(name[7:]) if name.startswith("single:") else None
        if self.family is not None:
            self._tb = self.family.tb
        self.rows = table_rows(self.tb)
        mesh_of = (self.tb["tri_mesh"].detach().cpu().numpy() & ~0x40000000)
        self.mesh_of = mesh_of
        self.in_tree = np.isin(mesh_of, self.tree_meshes) if self.tree_meshes is not None else np.zeros(mesh_of.shape, bool)
        self._rays = self._bf = self._bf_tree = None

    @property
    def tb(self):
        if self._tb is None:
            self._tb = make_forest_scene(self.meshes).tables(0)
        return self._tb

    @property
    def rays(self):
        if self._rays is None:
            seed = len(self.name)
            ao, ad = axis_rays(self.rows, 2000, seed + 500)
            if self.family is not None:
                o, d, owner = self.family.rays
            else:
                o, d, owner = ray_set(self.rows, seed=seed)
            o, d, owner = np.concatenate([o, ao]), np.concatenate([d, ad]), np.concatenate([owner, np.full(2000, -1, np.int64)])
            if self.name == "room":                                  # rays start inside the room
                o = np.clip(o, ROOM_LO + 0.25, ROOM_HI - 0.25)
            self._rays = (o, d, owner)
        return self._rays

    @property
    def bf(self):
        if self._bf is None:
            o, d, _ = self.rays
            if self.family is not None:                              # the family's own rays have their answer already
                tail = brute_force(self.rows, o[-2000:], d[-2000:])
                self._bf = {k: np.concatenate([self.family.bf[k], tail[k]]) for k in tail}
            else:
                self._bf = brute_force(self.rows, o, d)
        return self._bf

    def tree_rows(self, rows=None):
        """the table with every triangle outside the trees shrunk to a point (zero area: brute_force never hits it); ids stay global"""
        rows = (self.rows if rows is None else rows).copy()
        rows[~self.in_tree, 3:9] = 0
        return rows

    @property
    def bf_tree(self):
        if self._bf_tree is None:
            if self.in_tree.all():
                self._bf_tree = self.bf
            else:
                self._bf_tree = brute_force(self.tree_rows(), self.rays[0], self.rays[1])
        return self._bf_tree


def forest_case(name):
    if name not in _forest:
        _forest[name] = ForestCase(name)
    return _forest[name]


_edges = None


def edges_case(n_edges=2000):
    """cbox_bunny's own tables, the only input with sec_edge_faces: rays that start ON n_edges of its secondary edges (midpoint + a random direction),
    each twice -- first half with its edge index (a walk that ignores the edge's two faces, as the dense trace kernel's IGN instances do), second half with -1 -- and the
    brute force over the tree triangles with (bf_ign) and without (bf) the two faces removed on the first half."""
    global _edges
    if _edges is None:
        from helpers import load_scene
        sc, _ = load_scene("cbox_bunny", res=8, spp=1, sppse=1)
        tb = sc.tables(0)
        rows = table_rows(tb)
        mesh_of = tb["tri_mesh"].detach().cpu().numpy() & ~0x40000000
        in_tree = np.bincount(mesh_of)[mesh_of] >= 64
        se = tb["sec_edge"].detach().cpu().numpy().astype(np.float64)
        faces = tb["sec_edge_faces"].detach().cpu().numpy().astype(np.int64)
        rng = np.random.default_rng(91)
        own = np.nonzero(in_tree[faces[:, 0]])[0]                    # the bunny's edges, not the walls'
        pick = own[rng.choice(own.size, min(n_edges, own.size), replace=False)]
        d = rng.normal(size=(pick.size, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        o = (se[pick, 0:3] + 0.5 * se[pick, 3:6]).astype(np.float32)
        o, d = np.concatenate([o, o]), np.concatenate([d, d]).astype(np.float32)
        edge = np.concatenate([pick, np.full(pick.size, -1)]).astype(np.int32)
        ex = np.concatenate([faces[pick], np.full((pick.size, 2), -1)])
        tree_rows = rows.copy()
        tree_rows[~in_tree, 3:9] = 0
        _edges = dict(tb=tb, rows=rows, in_tree=in_tree, o=o, d=d, edge=edge, faces=faces[pick], bf=brute_force(tree_rows, o, d),
                      bf_ign=brute_force(tree_rows, o, d, exclude=ex))
    return _edges
