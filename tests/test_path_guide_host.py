"""Guiding grids of the PathTracer's secondary-edge term (csrc/psdr_path_sedge.h) on the HOST: the product's PSDR_HD functions run slot by
slot by tests/hostcheck/hostcheck_path_guide.cpp.  None of this needs a GPU:
  1. one-cell grids are no grids, bit for bit, and the two grids are independent;
  2. depth 1 is DirectIntegrator's guided term and its guiding-grid build;
  3. guided reverse mode is the adjoint of guided forward mode;
  4. the estimator stays unbiased under ANY positive grid (the pdf factor sits where it belongs);
  5. grids from the build reduce the error at equal slot count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
from helpers import dot_tables, host_render, hostcheck_lib, load_scene, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, write_tables_file
from path_guide_helpers import (HC_DEPS, HC_DIR, HC_SRC, host_path_guide_fwd, host_path_guide_mass, host_path_guide_rev, host_path_guide_survivors, make_grid,
                                one_cell_grid, synthetic_grid)
from path_sedge_helpers import SCENARIOS, host_path_sedge_fwd, host_path_sedge_rev, host_path_sedge_survivors, path_opts, scenario_scene
from psdr_cuda import _abi
from psdr_cuda.scene import make_desc

TABLES = ["tri_info", "sec_edge", "cam_to_world"]
NT = 16


def _occluder(res, sppse):
    sc, P = load_scene("cbox_occluder", res=res, spp=0, sppe=0, sppse=sppse, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    return tb, tangents_wrt(tb, P), np.random.default_rng(4).random((res * res, 3)).astype(np.float32)


# ---------------------------------------------------------------- 1. one-cell grids, independence
def test_one_cell_grids_are_no_grids_and_the_grids_are_independent():
    tb, tan, adj = _occluder(16, 16)
    o = path_opts(3, 16, (0, 0, 3))
    one, syn = one_cell_grid(), synthetic_grid()
    ref = host_path_sedge_fwd(tb, o, tan)
    assert np.abs(ref).max() > 0
    assert np.array_equal(host_path_guide_fwd(tb, o, tan), ref)                                    # the guided harness without grids is the unguided one
    assert np.array_equal(host_path_guide_fwd(tb, o, tan, grid_a=one, grid_b=one), ref)
    ref_g = host_path_sedge_rev(tb, o, adj, want=TABLES)
    got_g = host_path_guide_rev(tb, o, adj, grid_a=one, grid_b=one, want=TABLES)
    for k in TABLES:
        assert np.abs(ref_g[k]).max() > 0 and np.array_equal(got_g[k], ref_g[k]), k
    assert host_path_guide_survivors(tb, o, one, one) == host_path_sedge_survivors(tb, o)
    # a grid on one segment leaves the other segment's image alone, bit for bit -- and moves its own
    ref_a, ref_b = host_path_sedge_fwd(tb, o, tan, seg=1), host_path_sedge_fwd(tb, o, tan, seg=2)
    assert np.abs(ref_a).max() > 0 and np.abs(ref_b).max() > 0
    assert np.array_equal(host_path_guide_fwd(tb, o, tan, grid_a=syn, seg=2), ref_b)
    assert np.array_equal(host_path_guide_fwd(tb, o, tan, grid_b=syn, seg=1), ref_a)
    assert rel_l2(host_path_guide_fwd(tb, o, tan, grid_a=syn, seg=1), ref_a) > 1e-2
    assert rel_l2(host_path_guide_fwd(tb, o, tan, grid_b=syn, seg=2), ref_b) > 1e-2
    # ... and segment B warps the RAW s3[0]: with both grids it is what it is with grid B alone
    assert np.array_equal(host_path_guide_fwd(tb, o, tan, grid_a=syn, grid_b=syn, seg=2), host_path_guide_fwd(tb, o, tan, grid_b=syn, seg=2))


# ---------------------------------------------------------------- 2. depth 1
def test_depth_one_is_the_direct_integrators_build_and_guided_term():
    """segment 1's mass at depth 1 against hostcheck_guide on the same resolution (rel_l2 < 1e-6: only the summation order may differ), and the image
    guided by that grid against hostcheck_render of DirectIntegrator(1, 1) with the same grid (< 1e-5)"""
    tb, tan, _ = _occluder(24, 8)
    reso, nrounds = [16, 4, 4, 2], 3
    od = _abi.make_opts(spp=0, sppe=0, sppse=8, bsdf_samples=1, light_samples=1, rng_offset=(0, 5, 9))
    tbc = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in tb.items()}
    desc, keep = make_desc(tbc, None, device="cpu")
    ref_mass = np.zeros(reso[0] * reso[1] * reso[2], np.float32)
    assert hostcheck_lib().hostcheck_guide(C.byref(desc), (C.c_int32 * 4)(*reso), nrounds, C.c_void_p(ref_mass.ctypes.data), 4) == 0          # the product's k_guide arithmetic on the host
    assert rel_l2(oracle.guide_build(tb, od, reso, nrounds), ref_mass) < 1e-4          # (which the oracle confirms to the bound of test_hostcheck_parity.py)
    mass = host_path_guide_mass(tb, path_opts(1, 8, (0, 5, 9)), 1, reso, nrounds)
    assert ref_mass.sum() > 0 and rel_l2(mass, ref_mass) < 1e-6, rel_l2(mass, ref_mass)
    grid = make_grid(reso, mass)
    kw = dict(spp=0, sppe=0, rng_offset=(0, 5, 9), bsdf_samples=1, light_samples=1)
    ref = host_render(tb, _abi.make_opts(sppse=8, **kw), mode=1, tangents=tan, guide=grid)[1] - host_render(tb, _abi.make_opts(sppse=0, **kw), mode=1, tangents=tan, guide=grid)[1]
    got = host_path_guide_fwd(tb, path_opts(1, 8, (0, 5, 9)), tan, grid_a=grid)
    assert np.abs(ref).max() > 0 and rel_l2(got, ref) < 1e-5, rel_l2(got, ref)
    assert rel_l2(host_path_sedge_fwd(tb, path_opts(1, 8, (0, 5, 9)), tan), ref) > 1e-2          # (the grid did move the slots)


# ---------------------------------------------------------------- 3. forward = reverse
def test_guided_forward_equals_reverse():
    """<adj, J t> = <J^T adj, t> under both grids at depth 3: |lhs - rhs| <= 1e-4 * scale, the bound of test_path_sedge_host.py for the same identity"""
    res, sppse = 16, 16
    sc, _ = load_scene("cbox_occluder", res=res, spp=4, sppe=0, sppse=sppse)
    tb = sc.tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = path_opts(3, sppse, (2, 3, 4))
    ga, gb = synthetic_grid(), synthetic_grid((4, 8, 2))
    for n in TABLES:
        tan = random_tangents(tb, [n], seed=1)
        dimg = host_path_guide_fwd(tb, o, tan, grid_a=ga, grid_b=gb)
        grads = host_path_guide_rev(tb, o, adj, grid_a=ga, grid_b=gb, want=[n])
        lhs, rhs = float((adj.astype(np.float64) * dimg).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)


# ---------------------------------------------------------------- 4. / 5. errors at equal slot count
N_SLOTS, M_SLOTS = 256, 4096          # per pixel; M = 16 N: the floor (distance of two M-slot runs) is sqrt(2) e(N) / 4, so 2 * floor ~ 0.71 e(N) < e(N)


def _errors(name, res, grids):
    """rel_l2 of the term's derivative image at N_SLOTS against R = the mean of two independent unguided M_SLOTS runs, unguided ("u") and per grid pair; "floor" = the
    distance of the two runs"""
    depth = SCENARIOS[name][1]
    sc, P = scenario_scene(name, 0, 0, N_SLOTS, res=res)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    draws = _abi.draws_per_slot(path_opts(depth, 1))[2]
    big = [host_path_sedge_fwd(tb, path_opts(depth, M_SLOTS, (0, 0, 1000000 * (1 + k))), tan, nthreads=NT).astype(np.float64) for k in (0, 1)]
    R = (big[0] + big[1]) / 2.0
    o = path_opts(depth, N_SLOTS, (0, 0, 0))
    assert draws * N_SLOTS < 1000000          # the three runs use disjoint stretches of the streams
    out = {"floor": rel_l2(big[0], big[1]), "u": rel_l2(host_path_sedge_fwd(tb, o, tan, nthreads=NT), R)}
    for key, make in grids.items():
        ga, gb = make(tb, depth)
        out[key] = rel_l2(host_path_guide_fwd(tb, o, tan, grid_a=ga, grid_b=gb, nthreads=NT), R)
    print(name, " ".join("%s=%.4f" % kv for kv in out.items()))
    return out


def test_unbiased_under_a_synthetic_grid():
    """A grid that is not built from the scene (mass 1 + 3 ((c0 + c1 + c2) % 2) on 8 x 4 x 4 cells, on both segments): the pdf stays within [0.4, 1.6], so the
    variance stays of the same order -- e_s < 1.5 e_u -- while a missing or misplaced pdf factor gives an error of order 1.  2 * floor < e_u holds for the
    unguided code alone."""
    e = _errors("occluder", 16, {"s": lambda tb, d: (synthetic_grid(), synthetic_grid())})
    assert 2 * e["floor"] < e["u"], e
    assert e["s"] < 1.5 * e["u"], e


BUILD_RESO, BUILD_ROUNDS = [64, 4, 4, 4], 64          # fine along the edge axis, coarse in the other two; 256 evaluations per cell: a cell with the average
#                                                       survival rate of segment A (2 %) still sees five survivors


def _built(tb, depth):
    o = path_opts(depth, 1)
    return tuple(make_grid(BUILD_RESO, host_path_guide_mass(tb, o, seg, BUILD_RESO, BUILD_ROUNDS, nthreads=NT)) for seg in (1, 2))


@pytest.mark.parametrize("name", ["occluder", "mirror"])
def test_built_grids_help(name):
    """grids from the build (BUILD_RESO, BUILD_ROUNDS) on both segments: e_g < e_u at the same slot count.  Measured figures: DESIGN.md section 11."""
    e = _errors(name, 16, {"g": _built})
    assert 2 * e["floor"] < e["u"], e
    assert e["g"] < e["u"], e


# ---------------------------------------------------------------- the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers(tmp_path):
    """hostcheck_path_guide.cpp as a stand-alone program (its own main, -DPATH_GUIDE_MAIN, no Python), built with -fsanitize=address,undefined for the host: guided
    forward and reverse, the survivor counts and both builds on the smallest case; it must end clean and report what the library reports."""
    exe = os.path.join(HC_DIR, "path_guide_san")
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in HC_DEPS):
        cmd = ["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-pthread", "-DPATH_GUIDE_MAIN", HC_SRC, "-o", exe]
        san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
        r = subprocess.run(cmd + san, capture_output=True, text=True)
        if r.returncode != 0 and ("libclang_rt" in r.stderr or "sanitizer" in r.stderr.lower()):
            # no host sanitizer runtime beside this compiler: the program still runs the same functions over the same tables, without the instrumentation
            print("path_guide_san: built WITHOUT the sanitizers, the compiler's host runtime for them is missing:\n" + r.stderr[-800:])
            r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, "path_guide_san does not compile:\n" + r.stderr[-3000:]
    res, sppse = 8, 4
    tb, tan, adj = _occluder(res, sppse)
    o = path_opts(3, sppse, (0, 0, 2))
    ga, gb = synthetic_grid(), synthetic_grid((4, 8, 2))
    mass_reso, nrounds = [8, 2, 2, 2], 2
    tbc, desc, keep = cpu_desc(tb, ga)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, np.array(gb[0], np.int32), np.float32(gb[3]), gb[1].numpy().astype(np.float32), gb[2].numpy().astype(np.float32),
                      np.array(mass_reso + [nrounds], np.int32), tan["sec_edge"].detach().cpu().numpy().astype(np.float32), adj.astype(np.float32))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    tan1 = {"sec_edge": tan["sec_edge"]}
    want = [np.abs(host_path_guide_fwd(tb, o, tan1, grid_a=ga, grid_b=gb, nthreads=2).astype(np.float64)).sum(),
            np.abs(host_path_guide_rev(tb, o, adj, grid_a=ga, grid_b=gb, want=["sec_edge"])["sec_edge"].astype(np.float64)).sum(),
            *host_path_guide_survivors(tb, o, ga, gb),
            host_path_guide_mass(tb, o, 1, mass_reso, nrounds, nthreads=2).astype(np.float64).sum(), host_path_guide_mass(tb, o, 2, mass_reso, nrounds, nthreads=2).astype(np.float64).sum()]
    assert want[0] > 0 and want[1] > 0 and want[5] > 0 and want[6] > 0, want
    assert got[2:5] == want[2:5] and np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
