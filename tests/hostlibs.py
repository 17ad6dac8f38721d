"""The native test libraries (tests/hostcheck/*.cpp: the product's PSDR_HD code run on the host; tests/poison/poison.hip) for the front ends: the build table
and its one staleness rule -- those of __graft_entry__.build(), taken from there, so that the lazy loader and build() cannot disagree --, the loader, and the
marshalling every front end of a host-check library needs.  Only the standard library (and __graft_entry__, which imports no more) is imported here; torch and the
package are imported by the functions that hand tables over."""
import ctypes as C
import os
import subprocess
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


def san_program(name, extra_deps):
    """The stand-alone program tests/hostcheck/<name>.cpp (its own main, run as a child process, never loaded into Python) built with the host sanitizers;
    rebuilt when its source or one of `extra_deps` is newer than the executable.  Returns the executable's path."""
    exe, src = os.path.join(HC_DIR, name), os.path.join(HC_DIR, name + ".cpp")
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in list(extra_deps) + [src]):
        tmp = "%s.%d.tmp" % (exe, os.getpid())          # the test files that share the program may run in several processes: each builds its own file, the rename is atomic
        cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-pthread", src, "-o", tmp]
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        r = subprocess.run(cmd + san, capture_output=True, text=True)
        if r.returncode != 0 and ("libclang_rt" in r.stderr or "sanitizer" in r.stderr.lower()):
            # no host sanitizer runtime beside this compiler: the program still runs the same functions over the same tables, without the instrumentation
            print("%s: built WITHOUT the sanitizers, the compiler's host runtime for them is missing:\n" % name + r.stderr[-800:])
            r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, "%s does not compile:\n" % name + r.stderr[-3000:]
        os.replace(tmp, exe)
    return exe


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
