"""The native test libraries (tests/hostcheck/*.cpp: the product's PSDR_HD code run on the host; tests/poison/poison.hip) for the front ends: the build table
and its one staleness rule -- those of __graft_entry__.build(), taken from there, so that the lazy loader and build() cannot disagree --, the loader, and the
marshalling every front end of a host-check library needs.  Only the standard library (and __graft_entry__, which imports no more) is imported here; torch and the
package are imported by the functions that hand tables over."""
import ctypes as C
import os
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if ROOT not in sys.path:
    sys.path.append(ROOT)
from __graft_entry__ import CSRC, HC_DIR, TEST_LIBS as LIBS, build_testlib as build, testlib_deps as deps  # noqa: E402,F401

_loaded = {}


def source(name):
    return os.path.join(TESTS, LIBS[name][0])


def load(name):
    if name not in _loaded:
        _loaded[name] = C.CDLL(build(name))
    return _loaded[name]


def host_threads():
    """the default of every nthreads=None: a command on the shared GPU machines has 16 CPUs, whatever os.cpu_count() says of the machine"""
    return min(16, os.cpu_count() or 1)


def cpu_desc(tb, guide=None):
    """(tables on the CPU, their scene descriptor, what keeps its pointers alive)"""
    import torch
    from psdr_cuda.scene import make_desc
    tbc = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in tb.items()}
    if guide is not None:
        guide = (guide[0], guide[1].cpu(), guide[2].cpu(), guide[3])
    desc, keep = make_desc(tbc, guide, device="cpu")
    return tbc, desc, keep


def tangents_struct(tangents, keep):
    """psdr_tangents of {table: tensor or None}; the CPU copies go to `keep`"""
    from psdr_cuda import _abi
    tan = _abi.Tangents()
    for k, t in (tangents or {}).items():
        if t is not None:
            t = t.detach().cpu().float().contiguous()
            keep.append(t)
            setattr(tan, "d_" + k, t.data_ptr())
    return tan


def write_tables_file(path, desc, keep, opts, *arrays):
    """the input of the stand-alone programs (tests/hostcheck/host_common.h TablesFile):
    int64 sizeof(desc) | desc | int64 m | m x (int64 offset of a pointer member of desc, int64 bytes, data) | opts | each of `arrays` as it lies in memory"""
    import numpy as np
    by_ptr = {t.data_ptr(): t for t in keep}
    recs = [(getattr(type(desc), fname).offset, by_ptr[getattr(desc, fname)].numpy().tobytes())
            for fname, ftype in desc._fields_ if ftype is C.c_void_p and getattr(desc, fname)]
    with open(path, "wb") as f:
        f.write(np.int64(C.sizeof(desc)).tobytes() + bytes(desc) + np.int64(len(recs)).tobytes())
        for off, raw in recs:
            f.write(np.array([off, len(raw)], np.int64).tobytes() + raw)
        f.write(bytes(opts))
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
