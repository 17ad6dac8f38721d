"""Meshes, cameras and the float64 references of the table-chain tests (tests/test_tables_cases.py, tests/test_tables_cases_gpu.py).

Every mesh is built here from fixed seeds at unit scale, its positions rounded to float32, and comes with its [E, 5] edge list (v0, v1, face0, face1 or -1,
opposite vertex of face0) from a plain dictionary over the sorted vertex pairs.  The references are the project's own definitions (psdr_cuda.scene
process_mesh / secondary_edge_records / primary_edge_records) evaluated in torch.float64 on the CPU, their adjoints from torch.autograd.grad and their tangents
from torch.func.jvp; the keep flags are written out here from mesh.cpp:251-270 and perspective.cpp:39-111.

process_mesh_guarded is process_mesh with the guards the native forward-mode kernel documents (csrc/psdr_tables.hip k_tri_rows_jvp): the normal and the area of
a face with |c| = 0 and the normal of a vertex whose normal sum is zero are CONSTANT (value 0 here, where process_mesh gives NaN), so their derivatives are zero
and autograd never sees a division by zero.

The error bound of a GPU case is max(FACTOR * r, FLOOR) with r = rel_l2(the float32 torch formulation on the CPU, the float64 reference): r measures what
float32 costs on THESE inputs and never looks at the kernel; FACTOR covers another order of the sums and the device's division and square root, FLOOR the cases
where the float32 chain happens to be exact."""
import functools

import numpy as np
import torch

from psdr_cuda.scene import Epsilon, EdgeEpsilon, primary_edge_records, process_mesh, secondary_edge_records

FACTOR, FLOOR = 4.0, 2e-6
MIN_MARGIN = 1e-4
GRID_T = (255, 256, 257)
FAMILIES = ("one", "tetra", "grid_255", "grid_256", "grid_257", "hub1000", "isolated", "sliver", "folded", "coplanar")
MANIFOLD = ("tetra", "grid_256", "hub1000")                       # compared with the product's host edge list
DEGENERATE = ("sliver", "folded")
EDGE_FAMILIES = ("tetra", "grid_255", "grid_256", "grid_257", "hub1000", "coplanar", "sliver")


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def bound(r, factor=FACTOR):
    return max(factor * r, FLOOR)


# ---------------------------------------------------------------- meshes
def edge_list(faces):
    """[E, 5] int32 in the order of the sorted vertex pairs; an edge of three faces raises"""
    d = {}
    for f, (a, b, c) in enumerate(np.asarray(faces).tolist()):
        for p, q, o in ((a, b, c), (b, c, a), (c, a, b)):
            key = (min(p, q), max(p, q))
            if key not in d:
                d[key] = [key[0], key[1], f, -1, o]
            else:
                assert d[key][3] == -1 and d[key][2] != f, "edge %s of more than two faces" % (key,)
                d[key][3] = f
    return np.array([d[k] for k in sorted(d)], dtype=np.int32).reshape(-1, 5)


def _grid(nx, ny, jitter_xy, jitter_z, seed, take=None, spacing=None):
    """(nx x ny) cells, two faces each, wound towards +z; the first `take` faces and the vertices they use"""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    sx, sy = (2.0 / nx, 2.0 / ny) if spacing is None else (spacing, spacing)
    v = np.stack([xs.ravel() * sx - 0.5 * nx * sx, ys.ravel() * sy - 0.5 * ny * sy, np.zeros(xs.size)], axis=1)
    v[:, :2] += rng.uniform(-1, 1, (len(v), 2)) * jitter_xy
    v[:, 2] += rng.uniform(-1, 1, len(v)) * jitter_z
    a = (ys[:-1, :-1] * (nx + 1) + xs[:-1, :-1]).ravel()
    f = np.stack([np.stack([a, a + 1, a + nx + 2], 1), np.stack([a, a + nx + 2, a + nx + 1], 1)], axis=1).reshape(-1, 3)
    if take is not None:
        f = f[:take]
        used = np.unique(f)
        remap = -np.ones(len(v), np.int64)
        remap[used] = np.arange(len(used))
        v, f = v[used], remap[f]
    return v, f.astype(np.int32)


def _spread(v, f, jitter_z, seed):
    """The angle between the two faces of an edge is a one-parameter family, so plain jitter leaves a few per cent of the edges within 1e-4 of the coplanar
    threshold: draw the height of the opposite vertex of every such edge again (seeded) until no interior edge has dot(n0, n1) above 1 - 1e-3"""
    rng = np.random.default_rng(seed + 7919)
    v = v.astype(np.float32).astype(np.float64)
    edges = edge_list(f)
    inner = edges[edges[:, 3] >= 0]
    for _ in range(1000):
        c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        n = c / np.linalg.norm(c, axis=1, keepdims=True)
        bad = inner[(n[inner[:, 2]] * n[inner[:, 3]]).sum(-1) > 1.0 - 1e-3]
        if len(bad) == 0:
            return v, f
        for i in np.unique(bad[:, 4]):
            v[i, 2] = np.float32(rng.uniform(-1, 1) * jitter_z)
    raise RuntimeError("no spread found")


SEEDS = {"grid_255": 1, "grid_256": 2, "grid_257": 3, "hub1000": 1}      # test_tables_cases.py holds every margin of these above MIN_MARGIN
_TETRA = (np.array([[0.9, 0.1, -0.4], [-0.6, 0.8, -0.5], [-0.5, -0.7, -0.3], [0.1, 0.05, 0.9]]), np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32))


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices [V, 3] float64 holding float32 values, faces [T, 3] int32, edges [E, 5] int32)"""
    if name == "one":
        v, f = np.array([[-0.7, -0.5, 0.1], [0.8, -0.4, -0.2], [0.1, 0.9, 0.3]]), np.array([[0, 1, 2]], np.int32)
    elif name == "tetra":
        v, f = _TETRA
    elif name.startswith("grid_"):
        v, f = _spread(*_grid(16, 9, 0.02, 0.04, seed=SEEDS[name], take=int(name[5:])), 0.04, SEEDS[name])
    elif name == "hub1000":
        rng = np.random.default_rng(SEEDS[name])
        n = 1000
        ang = 2 * np.pi * np.arange(n) / n
        rad = 1.0 + rng.uniform(-0.05, 0.05, n)
        rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.05, 0.05, n)], axis=1)
        v = np.concatenate([np.array([[0.02, -0.01, 0.6]]), rim])
        i = np.arange(n)
        f = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1).astype(np.int32)
        v, f = _spread(v, f, 0.05, SEEDS[name])
    elif name == "isolated":
        v = np.concatenate([_TETRA[0], np.random.default_rng(7).uniform(-1, 1, (100, 3))])
        f = _TETRA[1]
    elif name == "sliver":
        # faces 0, 1 live; face 2 has collinear corners (vertex 4 is the midpoint of 0 and 3: dyadic coordinates, so that cross(e1, e2) is exactly zero with
        # or without fused multiply-adds) and shares vertices 0 and 3 with the live faces; face 3 is a point on vertices of its own
        v = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.25], [-0.5, 0.5, 0.25], [0.5, 0.5, -0.5], [0.0, 0.0, -0.25], [0.75, 0.75, 0.5], [0.75, 0.75, 0.5], [0.75, 0.75, 0.5]])
        f = np.array([[0, 1, 2], [1, 3, 2], [0, 3, 4], [5, 6, 7]], np.int32)
    elif name == "folded":
        # faces 0 and 1 coincide with opposite winding: the normal sums of vertices 0 and 1 cancel exactly; face 2 keeps vertex 2 alive
        v = np.array([[-0.5, -0.25, 0.125], [0.75, -0.5, 0.0], [0.0, 0.5, 0.25], [0.5, 0.75, -0.25], [-0.5, 0.75, 0.5]])
        f = np.array([[0, 1, 2], [0, 2, 1], [2, 3, 4]], np.int32)
    elif name == "coplanar":
        # a flat 4 x 4 grid of spacing 1/4 on z = 0 (every face normal is (0, 0, 1) to the bit) and a wall of 4 cells standing on its edge x = 1/2
        v, f = _grid(4, 4, 0.0, 0.0, seed=0, spacing=0.25)
        edge = [int(np.nonzero((v[:, 0] == 0.5) & (v[:, 1] == y))[0][0]) for y in (-0.5, -0.25, 0.0, 0.25, 0.5)]
        top = len(v) + np.arange(5)
        v = np.concatenate([v, np.stack([np.full(5, 0.5), np.linspace(-0.5, 0.5, 5), np.full(5, 0.25)], axis=1)])
        wall = []
        for k in range(4):
            wall += [[edge[k + 1], edge[k], top[k]], [edge[k + 1], top[k], top[k + 1]]]
        f = np.concatenate([f, np.array(wall, np.int32)])
    else:
        raise KeyError(name)
    v = np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    f = np.ascontiguousarray(f, np.int32)
    return v, f, edge_list(f)


def degenerate_elements(name):
    """(faces with |c| = 0 [T] bool, vertices whose normal sum is zero [V] bool) in float64 -- exact on these dyadic families"""
    v, f, _ = case(name)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    s = np.zeros_like(v)
    for k in range(3):
        np.add.at(s, f[:, k], c)
    used = np.zeros(len(v), bool)
    used[f.ravel()] = True
    return (c == 0).all(1), (s == 0).all(1) & used


def live_row_mask(name, width=22):
    """[T, width] bool: the row words that no degenerate element makes non-finite (the normal of a degenerate face -- its area is a plain 0 --, the normal of a vertex of zero sum)"""
    v, f, _ = case(name)
    dead_f, dead_v = degenerate_elements(name)
    m = np.ones((len(f), width), bool)
    m[dead_f, 18:21] = False
    for k in range(3):
        m[dead_v[f[:, k]], 9 + 3 * k:12 + 3 * k] = False
    return m


# ---------------------------------------------------------------- cameras
def _look_at(pos, target, up):
    pos, target, up = (np.asarray(x, np.float64) for x in (pos, target, up))
    d = (target - pos) / np.linalg.norm(target - pos)
    left = np.cross(up, d); left /= np.linalg.norm(left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, np.cross(d, left), d, pos
    return m, d


def camera(k):
    """22 words world_to_sample | position | direction of a pinhole camera (float32 values in float64).  0: from outside, above the meshes; 1: from the
    side and low, so that the faces of an open sheet partly face it and partly turn away"""
    pos = ([0.4, -0.7, 3.5], [2.7, 0.9, 0.33])[k]
    to_world, d = _look_at(pos, [0.0, 0.0, 0.0], [0.0, 0.0, 1.0] if k else [0.0, 1.0, 0.0])
    f = 1.0 / np.tan(np.radians(40.0) / 2)
    persp = np.array([[-0.5 * f, 0, 0.5, 0], [0, -0.5 * f, 0.5, 0], [0, 0, 1000.1 / 999.9, -200.0 / 999.9], [0, 0, 1, 0]])
    w2s = persp @ np.linalg.inv(to_world)
    return np.concatenate([w2s.ravel(), pos, d]).astype(np.float32).astype(np.float64)


def face_normal_flags(name, mode):
    """[E] uint8 per edge: all 0, all 1 or mixed (seeded)"""
    E = len(case(name)[2])
    if mode == "mixed":
        return (np.random.default_rng(E).random(E) < 0.5).astype(np.uint8)
    return np.full(E, int(mode), np.uint8)


FLAG_MODES = (0, 1, "mixed")


# ---------------------------------------------------------------- references
def _t(x, dtype=torch.float64):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def process_mesh_guarded(verts, faces):
    """process_mesh with constant (zero) normal and area for a face with |c| = 0 and a constant (zero) normal for a vertex whose normal sum is zero: the same
    values everywhere else, finite derivatives everywhere.  The vertex normal is normalize(sum c): the same direction as process_mesh's sum c / sum |c|."""
    f0, f1, f2 = faces[:, 0].long(), faces[:, 1].long(), faces[:, 2].long()
    p0 = verts.index_select(0, f0)
    e1 = verts.index_select(0, f1) - p0
    e2 = verts.index_select(0, f2) - p0
    c = torch.cross(e1, e2, dim=-1)
    s = torch.zeros_like(verts)
    for fi in (f0, f1, f2):
        s = s.index_add(0, fi, c)

    def unit(x):
        l2 = (x * x).sum(-1, keepdim=True)
        ok = l2 > 0
        ln = torch.sqrt(torch.where(ok, l2, torch.ones_like(l2)))
        return torch.where(ok, x / ln, torch.zeros_like(x)), torch.where(ok, ln, torch.zeros_like(ln))
    vn, _ = unit(s)
    fn, fa = unit(c)
    return torch.cat([p0, e1, e2, vn.index_select(0, f0), vn.index_select(0, f1), vn.index_select(0, f2), fn, 0.5 * fa], dim=-1), vn


def tri_fn(name, guarded=None):
    """f(v) -> rows [T, 22] of the family: process_mesh, or the guarded formulation on the degenerate families"""
    faces = torch.as_tensor(case(name)[1]).long()
    g = name in DEGENERATE if guarded is None else guarded
    return (lambda v: process_mesh_guarded(v, faces)[0]) if g else (lambda v: process_mesh(v, faces)[0])


def sec_fn(name):
    edges = torch.as_tensor(case(name)[2]).long()
    return lambda v, rows: secondary_edge_records(v, rows, edges)


def prim_fn(name):
    edges = torch.as_tensor(case(name)[2]).long()
    return lambda v, w2s: primary_edge_records(v, w2s, edges)


def rows_input(name):
    """the row table the edge entries read, [T, 22] float32 values in float64: process_mesh in float64 rounded once (NaN where it divides by zero)"""
    v, f, _ = case(name)
    return process_mesh(_t(v), torch.as_tensor(f).long())[0].float().double()


def forward(f, inputs, dtype=torch.float64):
    return f(*[_t(x, dtype) for x in inputs]).detach()


def adjoint(f, inputs, cot, dtype=torch.float64):
    """J^T cot for every input, by torch.autograd.grad"""
    xs = [_t(x, dtype).clone().requires_grad_(True) for x in inputs]
    gs = torch.autograd.grad(f(*xs), xs, grad_outputs=_t(cot, dtype), allow_unused=True)
    return [torch.zeros_like(x) if g is None else g.detach() for g, x in zip(gs, xs)]


def tangent(f, inputs, tans, dtype=torch.float64):
    """J tans, by torch.func.jvp"""
    return torch.func.jvp(f, tuple(_t(x, dtype) for x in inputs), tuple(_t(t, dtype) for t in tans))[1].detach()


def float32_error(kind, f, inputs, other=None, mask=None):
    """r of the module docstring for one case: the float32 evaluation of f (forward / adjoint / tangent) on the CPU against the float64 one.  A list of
    outputs (the adjoint of several inputs) gives one r per output."""
    run = {"fwd": lambda dt: [forward(f, inputs, dt)], "rev": lambda dt: adjoint(f, inputs, other, dt), "jvp": lambda dt: [tangent(f, inputs, other, dt)]}[kind]
    a32, a64 = run(torch.float32), run(torch.float64)
    out = []
    for x, y in zip(a32, a64):
        x, y = x.double().numpy(), y.numpy()
        m = np.isfinite(y) if mask is None else (mask & np.isfinite(y))
        out.append(rel_l2(x[m], y[m]) if np.abs(y[m]).sum() > 0 else 0.0)
    return out, a64


# ---------------------------------------------------------------- keep flags (mesh.cpp:251-270, perspective.cpp:39-111) and their margins
def _edge_normals(rows, edges):
    valid = edges[:, 3] >= 0
    f1 = np.where(valid, edges[:, 3], 0)
    n0 = rows[edges[:, 2], 18:21]
    n1 = rows[f1, 18:21] * valid[:, None]
    return valid, f1, n0, n1


def sec_keep(rows, edges):
    """(keep [E] bool, margin [E]): the two face normals are not parallel; a boundary edge has n1 = 0.  Two kinds of edge are outside the margin condition: one
    constructed to sit exactly on dn = 1 (margin inf: both formulations drop it) and one of a face without a normal (margin NaN: a comparison with NaN is false in
    any precision)"""
    rows, edges = np.asarray(rows, np.float64), np.asarray(edges)
    _, _, n0, n1 = _edge_normals(rows, edges)
    dn = (n0 * n1).sum(-1)
    with np.errstate(invalid="ignore"):
        return dn < 1.0 - EdgeEpsilon, np.where(dn == 1.0, np.inf, np.abs(dn - (1.0 - EdgeEpsilon)))


def prim_keep(rows, edges, cam22, face_normals):
    """(keep [E] bool, margin [E]) as seen from the camera: a face-normal mesh drops an edge whose faces both turn away or are coplanar, a smooth mesh keeps an edge with
    exactly one face turned towards the camera; a boundary edge always stays.  margin = the least distance of a dot product from a threshold it is compared with."""
    rows, edges, cam22 = np.asarray(rows, np.float64), np.asarray(edges), np.asarray(cam22, np.float64)
    valid, f1, n0, n1 = _edge_normals(rows, edges)
    cp = cam22[16:19]
    unit = lambda x: x / np.sqrt((x * x).sum(-1, keepdims=True))
    e0 = unit(cp - rows[edges[:, 2], 0:3])
    e1 = unit(cp - rows[f1, 0:3] * valid[:, None])
    d0, d1, dn = (e0 * n0).sum(-1), (e1 * n1).sum(-1), (n0 * n1).sum(-1)
    fnm = np.asarray(face_normals).astype(bool)
    with np.errstate(invalid="ignore"):
        keep_face = ~(valid & (((d0 < Epsilon) & (d1 < Epsilon)) | (dn > 1.0 - Epsilon)))
        keep_smooth = (~valid) | ((d0 > Epsilon) ^ (d1 > Epsilon))
        margin = np.minimum(np.abs(d0 - Epsilon), np.abs(d1 - Epsilon))
        margin = np.where(fnm & (dn != 1.0), np.minimum(margin, np.abs(dn - (1.0 - Epsilon))), margin)
    return np.where(fnm, keep_face, keep_smooth), np.where(valid, margin, np.inf)


def prim_z4(v, edges, cam22):
    """(1 / depth of the two end points along the viewing direction [E, 2], the adjacent faces [E, 2] int32; a boundary edge repeats face0)"""
    v, edges, cam22 = np.asarray(v, np.float64), np.asarray(edges), np.asarray(cam22, np.float64)
    cp, cd = cam22[16:19], cam22[19:22] / np.linalg.norm(cam22[19:22])
    z = np.stack([1.0 / ((v[edges[:, 0]] - cp) @ cd), 1.0 / ((v[edges[:, 1]] - cp) @ cd)], axis=1)
    return z, np.stack([edges[:, 2], np.where(edges[:, 3] >= 0, edges[:, 3], edges[:, 2])], axis=1).astype(np.int32)
