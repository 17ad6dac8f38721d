"""LargeSteps: the parameterisation of "Large Steps in Inverse Rendering" (Nicolet, Jacobson, Jakob 2021) for per-vertex shape optimisation, on the
HIP library (csrc/psdr_smooth.hip, include/psdr_hip.h psdr_smooth_*).  Raw per-vertex gradients of a Monte Carlo boundary estimator tangle a mesh within
a few Adam steps; instead one optimises u = M x with M = I + lambda L (L: the combinatorial Laplacian of the mesh) and recovers x = M^-1 u every step, so
that the chain rule turns the vertex gradient g into M^-1 g.

    ls = psdr_cuda.LargeSteps(mesh)                    # or (faces, num_vertices)
    u = ls.to_differential(mesh.vertex_positions)      # M x
    ek.set_requires_gradient(u)
    mesh.vertex_positions = ls.from_differential(u)    # M^-1 u, differentiable: the backward of a solve is a solve (M is symmetric)

or, keeping x as the parameter, g = ls.precondition(x.grad).  Every call is enqueued on torch.cuda.current_stream() and returns without waiting;
info() is the one call that waits.  There is no CPU fallback: a tensor that is not on the GPU raises."""
import ctypes as C

import numpy as np
import torch

import enoki as ek
from enoki.cuda import Vector3f as Vector3fC

from . import _abi

# The smallest power of two above the largest iteration count measured (189 .. 192: a 40962-vertex sphere, cold, lambda = 100).  The multi-launch form enqueues
# its iterations in chunks and stops when it sees the solve's `done` word, so a solve that needs fewer does not pay for max_iter of them.
DEFAULT_MAX_ITER = 256


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Apply(torch.autograd.Function):
    """u = M x; the backward is M again (M is symmetric), written as an application of this Function so that it can be differentiated once more
    (enoki.forward: double backward, enoki/_array.py _jvp_wrt)."""

    @staticmethod
    def forward(ctx, x, ls):
        ctx.ls = ls
        return ls._apply(x.detach())

    @staticmethod
    def backward(ctx, a):
        return _Apply.apply(a, ctx.ls), None


class _Solve(torch.autograd.Function):
    """x = M^-1 b from the initial guess x0 (no gradient flows to the guess); the backward is a solve of the adjoint, an application of this Function."""

    @staticmethod
    def forward(ctx, b, x0, ls):
        ctx.ls = ls
        return ls._solve(b.detach(), x0)

    @staticmethod
    def backward(ctx, a):
        return _Solve.apply(a, None, ctx.ls), None, None


class LargeSteps:
    def __init__(self, mesh_or_faces, num_vertices=None, lmbda=19.0, tol=1e-6, max_iter=DEFAULT_MAX_ITER, one_workgroup=-1):
        faces = getattr(mesh_or_faces, "face_indices", mesh_or_faces)
        if num_vertices is None and hasattr(mesh_or_faces, "num_vertices"):
            num_vertices = mesh_or_faces.num_vertices
        if isinstance(faces, torch.Tensor):
            faces = faces.detach().cpu().numpy()
        faces = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3).astype(np.int32))
        if num_vertices is None:
            num_vertices = int(faces.max()) + 1 if faces.size else 0
        self.num_vertices, self.faces = int(num_vertices), faces
        self.lmbda, self.tol, self.max_iter, self.one_workgroup = float(lmbda), float(tol), int(max_iter), int(one_workgroup)
        if self.num_vertices <= 0:
            raise RuntimeError("LargeSteps: the mesh has no vertices")
        if faces.size and (faces.min() < 0 or faces.max() >= self.num_vertices):
            raise RuntimeError("LargeSteps: a face names a vertex outside [0, %d)" % self.num_vertices)
        if not (self.lmbda >= 0.0) or not (self.tol > 0.0) or self.max_iter < 1:
            raise RuntimeError("LargeSteps: lmbda must not be negative, tol must be positive and max_iter at least 1")
        self._handle = None

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            try:
                _abi.load_hip().psdr_smooth_destroy(h)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass

    # ------------------------------------------------------------ the library calls
    def _lib_handle(self):
        lib = _abi.load_hip()
        if self._handle is None:
            h = C.c_void_p()
            _abi.check(lib, lib.psdr_smooth_create(self.num_vertices, len(self.faces), self.faces.ctypes.data if self.faces.size else None, C.byref(h)))
            try:
                _abi.check(lib, lib.psdr_smooth_set_option(h, b"one_workgroup", self.one_workgroup))
            except RuntimeError:
                lib.psdr_smooth_destroy(h)          # the option was refused (one_workgroup = 1 past the limit): no handle is kept, the next call raises again
                raise
            self._handle = h
        return lib, self._handle

    def set_option(self, name, value):
        """psdr_smooth_set_option: "one_workgroup" 1 (always) / 0 (never) / -1 (by the vertex count)"""
        if name == "one_workgroup":
            old, self.one_workgroup = self.one_workgroup, int(value)
            try:
                lib, h = self._lib_handle()
                _abi.check(lib, lib.psdr_smooth_set_option(h, name.encode(), int(value)))
            except RuntimeError:
                self.one_workgroup = old
                raise
            return
        lib, h = self._lib_handle()
        _abi.check(lib, lib.psdr_smooth_set_option(h, name.encode(), int(value)))

    def _table(self, t, what):
        if not isinstance(t, torch.Tensor):
            raise TypeError("LargeSteps.%s: expected an enoki Vector3f or a torch tensor, got %s" % (what, type(t).__name__))
        if not t.is_cuda:
            raise RuntimeError("LargeSteps.%s: the table is on '%s'; the solves are HIP kernels and there is no CPU fallback -- move it to the GPU" % (what, t.device))
        if tuple(t.shape) != (self.num_vertices, 3):
            raise RuntimeError("LargeSteps.%s: expected a [%d, 3] table, got %s" % (what, self.num_vertices, tuple(t.shape)))
        return t.contiguous().float()

    def _apply(self, x):
        x = self._table(x, "to_differential")
        lib, h = self._lib_handle()
        u = torch.empty_like(x)
        _abi.check(lib, lib.psdr_smooth_apply(h, self.lmbda, x.data_ptr(), u.data_ptr(), _stream()))
        return u

    def _solve(self, b, x0=None, what="from_differential"):
        b = self._table(b, what)
        x0 = None if x0 is None else self._table(x0.detach(), what + " (x0)")
        lib, h = self._lib_handle()
        x = torch.empty_like(b)
        _abi.check(lib, lib.psdr_smooth_solve(h, self.lmbda, b.data_ptr(), None if x0 is None else x0.data_ptr(), x.data_ptr(), self.tol, self.max_iter, _stream()))
        return x

    # ------------------------------------------------------------ the surface
    @staticmethod
    def _unwrap(v):
        return (v.t, type(v)) if isinstance(v, ek.ArrayBase) else (v, None)

    @staticmethod
    def _rewrap(t, cls):
        return t if cls is None else cls._wrap(t)

    def to_differential(self, x):
        """u = (I + lambda L) x; an enoki Vector3f or a torch tensor [V, 3] in, the same kind out; differentiable."""
        t, cls = self._unwrap(x)
        self._table(t, "to_differential")
        return self._rewrap(_Apply.apply(t, self), cls)

    def from_differential(self, u, x0=None):
        """x = (I + lambda L)^-1 u by conjugate gradients from x0 (e.g. the previous step's positions; None: zero); differentiable in u."""
        t, cls = self._unwrap(u)
        self._table(t, "from_differential")
        t0 = None if x0 is None else self._unwrap(x0)[0]
        return self._rewrap(_Solve.apply(t, t0, self), cls)

    def precondition(self, grad):
        """(I + lambda L)^-1 grad without autograd: for keeping x as the parameter and preconditioning its gradient."""
        t, cls = self._unwrap(grad)
        with torch.no_grad():
            out = self._solve(self._table(t, "precondition").detach(), what="precondition")
        if cls is not None and cls._ad:
            cls = Vector3fC          # a gradient table carries no graph: the detached flavour of the class that came in
        return self._rewrap(out, cls)

    def info(self):
        """What the last solve did (psdr_smooth_info) -- the only call that waits for it."""
        lib, h = self._lib_handle()
        s = _abi.SmoothInfo()
        _abi.check(lib, lib.psdr_smooth_info(h, C.byref(s)))
        return {"iterations": s.iterations, "converged": bool(s.converged), "form": _abi.SMOOTH_FORMS.get(s.form, "none"), "launches": s.launches,
                "rel_residual": tuple(float(v) for v in s.rel_residual), "one_workgroup_limit": s.one_workgroup_limit,
                "one_workgroup_default": s.one_workgroup_default, "num_vertices": s.num_vertices, "num_entries": s.num_entries, "long_rows": s.long_rows}
