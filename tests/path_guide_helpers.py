"""Front-end of tests/hostcheck/hostcheck_path_guide.cpp: the guided secondary-edge term of the PathTracer and the guiding-grid build of either segment
(csrc/psdr_path_sedge.h) run on the host, and what the CPU and GPU tests of the grids share."""
import ctypes as C

import numpy as np
import torch

import hostlibs
from helpers import _grad_buffers, AD_KEYS
from hostlibs import HC_DIR, cpu_desc, host_threads, tangents_struct
from psdr_cuda import _abi

HC_SRC = hostlibs.source("path_guide")
HC_DEPS = hostlibs.deps("path_guide")          # (what tests/test_path_guide_host.py's stand-alone program is stale against)


def path_guide_lib():
    return hostlibs.load("path_guide")


def make_grid(reso, mass):
    """(reso[:3], cmf, pmf, sum) as DiscreteDistribution holds them (inclusive prefix sum, unnormalised), on the host"""
    pmf = torch.as_tensor(np.asarray(mass, dtype=np.float32).reshape(-1))
    assert pmf.numel() == int(reso[0]) * int(reso[1]) * int(reso[2])
    return ([int(r) for r in reso[:3]], torch.cumsum(pmf, 0).contiguous(), pmf.contiguous(), float(pmf.sum().item()))


def one_cell_grid():
    return make_grid([1, 1, 1], [1.0])


def synthetic_grid(reso=(8, 4, 4)):
    """a positive grid that knows nothing of the scene: mass 1 + 3 ((c0 + c1 + c2) % 2) -- pdf 0.4 / 1.6"""
    c = np.indices(reso).sum(axis=0)
    return make_grid(reso, 1.0 + 3.0 * (c % 2))


def _grid_b_args(grid_b, keep):
    if grid_b is None:
        return None, None, None, C.c_float(0.0)
    reso, cmf, pmf, s = grid_b
    cmf, pmf = cmf.cpu().float().contiguous(), pmf.cpu().float().contiguous()
    keep += [cmf, pmf]
    return (C.c_int32 * 3)(*reso), C.c_void_p(cmf.data_ptr()), C.c_void_p(pmf.data_ptr()), C.c_float(s)


def host_path_guide_fwd(tb, opts, tangents, grid_a=None, grid_b=None, seg=3, walk=1, nthreads=None):
    """Forward mode (K = 1) on the host: the derivative image of the guided secondary-edge term alone."""
    tbc, desc, keep = cpu_desc(tb, grid_a)
    dimg = np.zeros(tb["width"] * tb["height"] * 3, np.float32)
    tan = tangents_struct(tangents, keep)
    rc = path_guide_lib().hostcheck_path_guide_fwd(C.byref(desc), C.byref(opts), int(seg), int(walk), *_grid_b_args(grid_b, keep), C.byref(tan), C.c_void_p(dimg.ctypes.data),
                                                   nthreads or host_threads())
    assert rc == 0, rc
    return dimg.reshape(-1, 3)


def host_path_guide_rev(tb, opts, adj, grid_a=None, grid_b=None, want=AD_KEYS, seg=3, walk=1):
    """Reverse mode on the host: {table: gradient} of the guided secondary-edge term alone."""
    tbc, desc, keep = cpu_desc(tb, grid_a)
    bufs, g = _grad_buffers(tbc, want)
    adj = np.ascontiguousarray(adj, dtype=np.float32).reshape(-1)
    rc = path_guide_lib().hostcheck_path_guide_rev(C.byref(desc), C.byref(opts), int(seg), int(walk), *_grid_b_args(grid_b, keep), C.c_void_p(adj.ctypes.data), C.byref(g))
    assert rc == 0, rc
    return bufs


def host_path_guide_survivors(tb, opts, grid_a=None, grid_b=None):
    """(survivors of segment A's filter, of segment B's, slots) under the grids, on the host"""
    tbc, desc, keep = cpu_desc(tb, grid_a)
    out = (C.c_longlong * 3)()
    rc = path_guide_lib().hostcheck_path_guide_survivors(C.byref(desc), C.byref(opts), *_grid_b_args(grid_b, keep), out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


def host_path_guide_mass(tb, opts, segment, reso, nrounds, walk=1, nthreads=None):
    """psdr_path_guide_build on the host: the mass of segment 1 (A) or 2 (B) on reso [4]"""
    tbc, desc, keep = cpu_desc(tb)
    mass = np.zeros(int(reso[0]) * int(reso[1]) * int(reso[2]), np.float32)
    rc = path_guide_lib().hostcheck_path_guide_mass(C.byref(desc), C.byref(opts), int(segment), int(walk), (C.c_int32 * 4)(*[int(r) for r in reso]), int(nrounds),
                                                    C.c_void_p(mass.ctypes.data), nthreads or host_threads())
    assert rc == 0, rc
    return mass


# ---------------------------------------------------------------- GPU through the C ABI (a GpuScene of helpers.py)
def gpu_set_path_guide(g, grid_b):
    """psdr_scene_set_path_guide on a GpuScene; None clears.  The device tables stay alive on the GpuScene."""
    if grid_b is None:
        _abi.check(g.lib, g.lib.psdr_scene_set_path_guide(g.h, (C.c_int32 * 3)(1, 1, 1), None, None, 0.0))
        g.keep_b = None
        return
    reso, cmf, pmf, s = grid_b
    g.keep_b = (cmf.cuda().float().contiguous(), pmf.cuda().float().contiguous())
    _abi.check(g.lib, g.lib.psdr_scene_set_path_guide(g.h, (C.c_int32 * 3)(*reso), g.keep_b[0].data_ptr(), g.keep_b[1].data_ptr(), float(s)))


def gpu_set_guides(g, grid_a, grid_b):
    """both grids, in the order the Python layer sets them: the tables (with grid A), then grid B"""
    g.set_guide(grid_a)
    gpu_set_path_guide(g, grid_b)


def gpu_path_guide_build(g, opts, segment, reso, nrounds):
    cells = int(reso[0]) * int(reso[1]) * int(reso[2])
    mass = torch.zeros(cells, dtype=torch.float32, device="cuda")
    _abi.check(g.lib, g.lib.psdr_path_guide_build(g.h, C.byref(opts), int(segment), (C.c_int32 * 4)(*[int(x) for x in reso]), int(nrounds), mass.data_ptr(), None))
    torch.cuda.synchronize()
    return mass.cpu().numpy()
