"""Meshes, the float64 reference and the host-harness bindings of the LargeSteps tests (tests/test_smooth_host.py, tests/test_smooth_gpu.py).

The reference of every solve is scipy.sparse.linalg.spsolve of I + lambda L in float64, L assembled here from the unique undirected edges in numpy -- a restatement
that shares no code with csrc/psdr_smooth.h.  BOUND is the relative L2 error the product's float32 CG is held to at tol = 1e-6: a float32 numpy CG measured at most
5.5e-6 on these meshes at lambda in {1, 10, 100}; ten times that covers another summation order, and a wrong or missing neighbour gives errors of order one."""
import ctypes as C
import functools
import os

import numpy as np

import hostlibs
from hostlibs import HC_DIR, ROOT

SMOOTH_H = os.path.join(hostlibs.CSRC, "psdr_smooth.h")
BOUND = 5e-5
TOL = 1e-6
LAMBDAS = (1.0, 10.0, 100.0)


# ---------------------------------------------------------------- meshes
@functools.lru_cache(maxsize=None)
def icosphere(level):
    """(vertices [V, 3] float64 on the unit sphere, faces [F, 3] int32): 12 * 4^level - ... = 42 / 162 / 642 / 2562 / 10242 / 40962 vertices at level 1 .. 6"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []
        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float64), np.array(f, np.int32)


def planar_grid(n):
    """n x n vertices on z = 0"""
    ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([xs.ravel() / (n - 1.0), ys.ravel() / (n - 1.0), np.zeros(n * n)], axis=1)
    a = (ys[:-1, :-1] * n + xs[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([a, a + 1, a + n], 1), np.stack([a + 1, a + n + 1, a + n], 1)]).astype(np.int32)
    return v, f


def components():
    """two disjoint icospheres (levels 2 and 1) and one isolated vertex between them"""
    v1, f1 = icosphere(2)
    v2, f2 = icosphere(1)
    v = np.concatenate([v1, np.array([[5.0, 5.0, 5.0]]), v2 * 0.5 + 3.0])
    f = np.concatenate([f1, f2 + len(v1) + 1]).astype(np.int32)
    return v, f


def hub_fan(m=1000):
    """a fan: vertex 0 with m neighbours on a circle"""
    a = 2.0 * np.pi * np.arange(m) / m
    v = np.concatenate([np.array([[0.0, 0.0, 0.3]]), np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(3 * a)], 1)])
    k = np.arange(m)
    f = np.stack([np.zeros(m, np.int64), 1 + k, 1 + (k + 1) % m], 1).astype(np.int32)
    return v, f


def odd_faces():
    """a duplicated face, an edge (0, 1) of three faces, a face with a repeated vertex, a face that is one vertex; vertex 6 is unused"""
    v = np.random.default_rng(7).standard_normal((7, 3))
    f = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 3], [1, 0, 4], [2, 2, 3], [5, 5, 5]], np.int32)
    return v, f


def padded(v, f, V):
    """the mesh with isolated vertices appended (or the unused tail cut) so that it has exactly V vertices"""
    assert V >= int(f.max()) + 1 if len(f) else True
    if V <= len(v):
        return v[:V].copy(), f
    extra = np.random.default_rng(V).standard_normal((V - len(v), 3))
    return np.concatenate([v, extra]), f


CASES = {
    "ico1": lambda: icosphere(1), "ico3": lambda: icosphere(3), "ico4": lambda: icosphere(4), "ico6": lambda: icosphere(6),
    "grid40": lambda: planar_grid(40), "components": components, "hub1000": hub_fan, "odd": odd_faces,
}
SMALL_CASES = ("ico1", "ico3", "ico4", "grid40", "components", "hub1000", "odd")


@functools.lru_cache(maxsize=None)
def case(name):
    v, f = CASES[name]()
    v.setflags(write=False); f.setflags(write=False)
    return v, f


# ---------------------------------------------------------------- the float64 reference
def unique_edges(V, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.sort(e, axis=1), axis=0) if len(e) else e.reshape(0, 2)
    return e


def system_matrix(V, faces, lam):
    """I + lam L as scipy CSR float64 (sorted indices)"""
    import scipy.sparse as sp
    e = unique_edges(V, faces)
    i, j = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    A = sp.coo_matrix((np.ones(len(i)), (i, j)), shape=(V, V)).tocsr()
    A.sum_duplicates(); A.sort_indices()
    deg = np.asarray(A.sum(axis=1)).ravel()
    return (sp.identity(V, format="csr") + lam * (sp.diags(deg) - A)).tocsr(), A, deg


@functools.lru_cache(maxsize=None)
def _factor(name, lam):
    import scipy.sparse.linalg as spl
    v, f = case(name)
    M, _, _ = system_matrix(len(v), f, lam)
    return M, spl.splu(M.tocsc())


def reference_apply(name, lam, x):
    return _factor(name, lam)[0] @ np.asarray(x, np.float64)


def reference_solve(name, lam, b):
    """float64 sparse direct solve of the case's system (LU of the SPD matrix; the factor is cached per case and lambda)"""
    return _factor(name, lam)[1].solve(np.asarray(b, np.float64))


def reference_solve_mesh(V, faces, lam, b):
    import scipy.sparse.linalg as spl
    M, _, _ = system_matrix(V, faces, lam)
    return spl.spsolve(M.tocsc(), np.asarray(b, np.float64))


def rel_l2(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-300))


def rhs(name, lam):
    """the right-hand side of the case: M x for the case's vertex positions, in float32 (what to_differential hands to from_differential)"""
    v, _ = case(name)
    return reference_apply(name, lam, v).astype(np.float32)


# ---------------------------------------------------------------- the host harness
def host_lib():
    lib = hostlibs.load("smooth")
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    lib.hostcheck_smooth_csr.argtypes = [i32, i32, vp, vp, vp, i32, vp, C.c_char_p, i32]
    lib.hostcheck_smooth_apply.argtypes = [i32, i32, vp, f32, vp, vp]
    lib.hostcheck_smooth_solve.argtypes = [i32, i32, vp, f32, vp, vp, vp, f32, i32, vp, vp]
    return lib


def _faces(faces):
    return np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def host_csr(V, faces):
    """(rowptr [V + 1], cols [nnz]) of the harness, or RuntimeError with its message"""
    lib, f = host_lib(), _faces(faces)
    rowptr, nnz, err = np.zeros(V + 1, np.int32), np.zeros(1, np.int32), C.create_string_buffer(256)
    rc = lib.hostcheck_smooth_csr(V, len(f), _p(f), rowptr.ctypes.data, None, 0, nnz.ctypes.data, err, 256)
    if rc:
        raise RuntimeError(err.value.decode())
    cols = np.zeros(max(int(nnz[0]), 1), np.int32)
    rc = lib.hostcheck_smooth_csr(V, len(f), _p(f), rowptr.ctypes.data, cols.ctypes.data, len(cols), nnz.ctypes.data, err, 256)
    assert rc == 0
    return rowptr, cols[:int(nnz[0])]


def host_apply(V, faces, lam, x):
    lib, f = host_lib(), _faces(faces)
    x = np.ascontiguousarray(x, np.float32)
    u = np.empty_like(x)
    assert lib.hostcheck_smooth_apply(V, len(f), _p(f), lam, x.ctypes.data, u.ctypes.data) == 0
    return u


def host_solve(V, faces, lam, b, x0=None, tol=TOL, max_iter=1000):
    """(x [V, 3] float32, info dict) of the harness' CG"""
    lib, f = host_lib(), _faces(faces)
    b = np.ascontiguousarray(b, np.float32)
    x0 = None if x0 is None else np.ascontiguousarray(x0, np.float32)
    x, info, res = np.empty_like(b), np.zeros(3, np.int32), np.zeros(3, np.float32)
    assert lib.hostcheck_smooth_solve(V, len(f), _p(f), lam, b.ctypes.data, None if x0 is None else x0.ctypes.data, x.ctypes.data, tol, max_iter,
                                      info.ctypes.data, res.ctypes.data) == 0
    return x, {"iterations": int(info[0]), "converged": bool(info[1]), "rel_residual": tuple(float(r) for r in res)}
