"""The LargeSteps operator M = I + lambda L and its guarded conjugate-gradient loop (csrc/psdr_smooth.h) on the HOST, through tests/hostcheck/hostcheck_smooth.cpp:
the adjacency build, the row operator and the CG step the kernels compile from.  The reference of every number is a float64 sparse direct solve of M assembled
in numpy from the unique edges (tests/smooth_cases.py).

Right-hand sides are Gaussian (seeded): what a gradient table looks like, and the kind of right-hand side the bound of smooth_cases.BOUND was measured with.
Measured with this harness at tol = 1e-6: relative L2 error at most 7.3e-6 (the 40962-vertex sphere at lambda = 100, 189 iterations), 1.8e-6 on the hub fan.
One thing the stopping test ||r|| <= tol ||b|| does NOT bound: with b = M v for the hub fan's own positions at lambda = 100 the hub's diagonal is 1e5, b is
that one entry to six digits, and CG stops after 3 steps at a relative error of 3e-4 in x -- the condition number times the tolerance, met by any solver that
stops on the residual; test_residual_stop_on_the_hub pins what the solve does promise there."""
import os
import subprocess

import numpy as np
import pytest
import torch

import smooth_cases as sc

ALL = tuple(sc.CASES)


def _b(name, seed=11):
    v, _ = sc.case(name)
    b = np.random.default_rng(seed).standard_normal((len(v), 3)).astype(np.float32)
    if name == "grid40":
        b[:, 2] = 0.0          # a floor mesh: the z column of positions and of gradients is zero
    return b


@pytest.mark.parametrize("name", ALL)
def test_adjacency_equals_scipy_pattern(name):
    """rowptr and cols of the harness = indptr and indices of scipy's CSR of the unique edges (sorted columns), byte for byte; the degrees follow"""
    v, f = sc.case(name)
    rowptr, cols = sc.host_csr(len(v), f)
    _, A, deg = sc.system_matrix(len(v), f, 1.0)
    assert np.array_equal(rowptr, A.indptr.astype(np.int32))
    assert np.array_equal(cols, A.indices.astype(np.int32))
    assert np.array_equal(np.diff(rowptr), deg.astype(np.int64))


def test_adjacency_of_the_odd_face_list():
    """a duplicated face, an edge of three faces and two degenerate faces: 7 unique edges, the unused vertices have empty rows"""
    v, f = sc.case("odd")
    rowptr, cols = sc.host_csr(len(v), f)
    edges = {(0, 1), (0, 2), (1, 2), (0, 3), (1, 3), (0, 4), (1, 4), (2, 3)}
    got = {(i, int(j)) for i in range(len(v)) for j in cols[rowptr[i]:rowptr[i + 1]]}
    assert got == edges | {(b, a) for a, b in edges}
    assert rowptr[5] == rowptr[6] == rowptr[7]          # vertices 5 (a face that is one vertex) and 6 (unused)


@pytest.mark.parametrize("bad", [[0, 1, 7], [0, -1, 2], [2 ** 31 - 1, 0, 1]])
def test_out_of_range_index_is_an_error(bad):
    with pytest.raises(RuntimeError, match="outside"):
        sc.host_csr(7, np.array([[0, 1, 2], bad], np.int32))


def test_isolated_vertex_rows_are_the_identity():
    v, f = sc.case("components")
    x = _b("components")
    u = sc.host_apply(len(v), f, 100.0, x)
    assert np.array_equal(u[162], x[162])          # the vertex between the two spheres
    y, info = sc.host_solve(len(v), f, 100.0, x)
    assert info["converged"] and abs(y[162] - x[162]).max() <= 1e-6 * abs(x[162]).max()


@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", ALL)
def test_apply_against_float64(name, lam):
    v, f = sc.case(name)
    x = _b(name, seed=5)
    e = sc.rel_l2(sc.host_apply(len(v), f, lam, x), sc.reference_apply(name, lam, x))
    assert e <= 1e-6, e


@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", ALL)
def test_solve_against_direct_solve(name, lam):
    v, f = sc.case(name)
    b = _b(name)
    x, info = sc.host_solve(len(v), f, lam, b)
    e = sc.rel_l2(x, sc.reference_solve(name, lam, b))
    print("%s lambda %g: %d iterations, rel-L2 %.2e" % (name, lam, info["iterations"], e))
    assert info["converged"] and max(info["rel_residual"]) <= sc.TOL
    assert np.isfinite(x).all() and e <= sc.BOUND, e


def test_residual_stop_on_the_hub():
    """b = M v for the hub fan's positions at lambda = 100 (module docstring): the solve converges by its own test and the TRUE residual is within a few
    float roundings of the tolerance -- that, and not an error in x of tol, is what a residual test promises at a condition number of 1e5."""
    v, f = sc.case("hub1000")
    b = sc.rhs("hub1000", 100.0)
    x, info = sc.host_solve(len(v), f, 100.0, b)
    assert info["converged"]
    res = np.linalg.norm(sc.reference_apply("hub1000", 100.0, x) - b, axis=0) / np.linalg.norm(b.astype(np.float64), axis=0)
    assert res.max() <= 4 * sc.TOL, res


@pytest.mark.parametrize("lam", sc.LAMBDAS)
def test_planar_grid_zero_column_is_exact(lam):
    """the floor mesh that made a naive float CG return NaN in all three columns: the z column is exactly zero and nothing is non-finite"""
    v, f = sc.case("grid40")
    b = sc.rhs("grid40", lam)
    assert (b[:, 2] == 0).all()
    for x0 in (None, v.astype(np.float32), np.ones((len(v), 3), np.float32)):
        x, info = sc.host_solve(len(v), f, lam, b, x0=x0)
        assert np.isfinite(x).all() and info["converged"]
        assert (x[:, 2] == 0).all() and not np.signbit(x[:, 2]).any()
        assert sc.rel_l2(x, sc.reference_solve("grid40", lam, b)) <= sc.BOUND


@pytest.mark.parametrize("name", ["ico3", "grid40", "odd"])
def test_zero_right_hand_side(name):
    v, f = sc.case(name)
    z = np.zeros((len(v), 3), np.float32)
    for x0 in (None, v.astype(np.float32)):
        x, info = sc.host_solve(len(v), f, 100.0, z, x0=x0)
        assert (x == 0).all() and info["converged"] and info["iterations"] == 0


@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", ALL)
def test_warm_start_from_the_solution(name, lam):
    v, f = sc.case(name)
    b = _b(name)
    ref = sc.reference_solve(name, lam, b)
    x, info = sc.host_solve(len(v), f, lam, b, x0=ref.astype(np.float32))
    assert info["converged"] and info["iterations"] <= 1, info
    assert sc.rel_l2(x, ref) <= sc.BOUND


@pytest.mark.parametrize("name", ["ico4", "grid40", "ico6"])
def test_iteration_limit(name):
    v, f = sc.case(name)
    b = _b(name)
    x, info = sc.host_solve(len(v), f, 100.0, b, max_iter=3)
    assert not info["converged"] and info["iterations"] == 3
    assert np.isfinite(x).all() and max(info["rel_residual"]) > sc.TOL


def test_non_finite_input_ends_non_finite():
    """a NaN or an infinity in b: the solve runs to max_iter (never loops, never reports convergence) and the column comes back non-finite"""
    v, f = sc.case("ico1")
    for bad in (np.nan, np.inf):
        b = _b("ico1")
        b[3, 1] = bad
        x, info = sc.host_solve(len(v), f, 10.0, b, max_iter=20)
        assert info["iterations"] == 20 and not info["converged"]
        assert not np.isfinite(x[:, 1]).any()
        assert np.isfinite(x[:, 0]).all() and np.isfinite(x[:, 2]).all()          # the columns are independent


@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", ["ico3", "components", "hub1000", "odd"])
def test_solve_is_symmetric(name, lam):
    """<solve(a), b> = <a, solve(b)> per column, to 1e-4 relative: |lhs - rhs| <= 1e-4 max(|lhs|, |rhs|).  Measured: at most 1.0e-5 over these cases."""
    v, f = sc.case(name)
    a, b = _b(name, seed=1), _b(name, seed=2)
    xa, _ = sc.host_solve(len(v), f, lam, a)
    xb, _ = sc.host_solve(len(v), f, lam, b)
    for c in range(3):
        lhs, rhs = float(xa[:, c].astype(np.float64) @ b[:, c]), float(a[:, c].astype(np.float64) @ xb[:, c])
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print("%s lambda %g column %d: %.2e" % (name, lam, c, rel))
        assert rel <= 1e-4, (c, lhs, rhs)


# ---------------------------------------------------------------- the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers():
    """tests/hostcheck/smooth_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_smooth.cpp, built with -fsanitize=address,undefined for the
    host: adjacency, operator, cold, warm and cut solves on a planar grid, a fan with a long row, an odd face list and a single vertex; it must end clean."""
    exe, src = os.path.join(sc.HC_DIR, "smooth_san"), os.path.join(sc.HC_DIR, "smooth_san.cpp")
    deps = [src, os.path.join(sc.HC_DIR, "hostcheck_smooth.cpp"), sc.SMOOTH_H]
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in deps):
        cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-pthread", src, "-o", exe]
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        r = subprocess.run(cmd + san, capture_output=True, text=True)          # (no build without the instrumentation: that would not be this test)
        assert r.returncode == 0, "smooth_san does not compile with the host sanitizers:\n" + r.stderr[-3000:]
    # the program that runs carries the instrumentation: the sanitizer runtime's entry points are in its symbol table
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "tests/hostcheck/smooth_san was built without the sanitizers"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    names = [line.split()[0] for line in r.stdout.splitlines()]
    assert names == ["grid", "fan", "odd", "single"], r.stdout


# ---------------------------------------------------------------- the Python surface without a GPU
def test_largesteps_refuses_cpu_tensors():
    """no CPU fallback: a CPU tensor (or an enoki array over one) raises with a message that says so, as the render path does without a GPU"""
    import psdr_cuda
    v, f = sc.case("ico1")
    ls = psdr_cuda.LargeSteps(f, len(v))
    x = torch.from_numpy(v.astype(np.float32))
    for call in (ls.to_differential, ls.from_differential, ls.precondition):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(x)
    with pytest.raises(RuntimeError, match="outside"):
        psdr_cuda.LargeSteps(np.array([[0, 1, 42]], np.int32), 42)
    with pytest.raises(RuntimeError):
        psdr_cuda.LargeSteps(f, len(v), lmbda=-1.0)


def test_abi_mirror_of_the_info_struct():
    """psdr_cuda/_abi.py SmoothInfo against the header's psdr_smooth_info_t: the same fields in the same order, all 4-byte"""
    import ctypes as C
    import re
    from psdr_cuda import _abi
    src = open(os.path.join(sc.ROOT, "include", "psdr_hip.h")).read()
    body = re.search(r"typedef struct psdr_smooth_info_s \{(.*?)\} psdr_smooth_info_t;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:int32_t|float)\s+([a-z_]+)(?:\[(\d+)\])?;", body)
    assert [n for n, _ in fields] == [n for n, _ in _abi.SmoothInfo._fields_]
    assert C.sizeof(_abi.SmoothInfo) == 4 * sum(int(k) if k else 1 for _, k in fields)
