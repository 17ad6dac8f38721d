"""The selection rule of the lean PathTracer twins (csrc/psdr_plan.h path_lean_form: which kernel a fused PathTracer camera launch on a scene without a tree runs),
run by tests/hostcheck/hostcheck_path_lean.cpp.  No GPU and no sanitizer.  The expected form is restated here from the rule's wording, never taken from the function:

  the twin runs  <=>  option path_lean on, flag set 8 (plain diffuse, no tree), PathTracer,
                      K = 0, or K = 1 with every tangent on albedo texels and option logd_park on,
                      every wave on one pixel: option own_pixels on, 64 samples per pixel in the launch, the chunk a multiple of them,
                      every kernel-argument primitive a slab-form rectangle: slab slots in use, no row behind the 9 slab slots, no tree,
                      and (where the twin parks: K = 1, 22 columns of 256 lanes x 4 bytes) staged scene + columns within a sixth of the CU's 160 KiB and a forced budget."""
import ctypes as C
import itertools

import pytest

import hostlibs
from psdr_cuda import _abi

FL_TINY, FL_ROUGH, FL_FOREST = 8, 2, 4
NONE, OWN_SLAB = 0, 1
COLS = {0: 0, 1: 22, 3: 34}          # LeanLayout<K>::cols = 16 + 6 K; K = 0 holds everything in registers
SIXTH = 160 * 1024 // 6
AA_BOX = 2 | (3 << 8) | (1 << 16)          # the Cornell box: two walls across x, floor / ceiling / light across y, the back wall across z


class Case(C.Structure):
    _fields_ = [("flags", C.c_int), ("K", C.c_int), ("integrator", C.c_int), ("texels_only", C.c_int), ("nsp", C.c_int), ("chunk", C.c_longlong),
                ("n_tiny", C.c_int), ("aa_cnt", C.c_int), ("n_blas", C.c_int), ("lds_scene", C.c_int), ("lds_budget", C.c_int),
                ("own_pixels", C.c_int), ("path_lean", C.c_int), ("logd_park", C.c_int)]


def case(**kw):
    d = dict(flags=FL_TINY, K=0, integrator=_abi.INTEGRATOR_PATH, texels_only=1, nsp=64, chunk=64 * 64 * 64, n_tiny=9, aa_cnt=AA_BOX, n_blas=0, lds_scene=3584, lds_budget=0,
             own_pixels=1, path_lean=1, logd_park=1)
    d.update(kw)
    return Case(**d)


@pytest.fixture(scope="module")
def H():
    lib = hostlibs.load("path_lean")
    lib.hostcheck_path_lean_wave_is_pixel.argtypes = [C.c_int, C.c_int, C.c_longlong]
    lib.hostcheck_path_lean_owns.argtypes = [C.c_int, C.c_int, C.c_longlong]
    return lib


def both(H, c):
    a, b = H.hostcheck_path_lean_form(C.byref(c)), H.hostcheck_path_lean_form_handle(C.byref(c))
    assert a == b, (a, b)
    return a


def expected(c):
    own = c.own_pixels != 0 and c.nsp == 64 and c.chunk % c.nsp == 0
    slab = c.n_blas == 0 and c.aa_cnt != 0 and 0 < c.n_tiny <= 9
    k_ok = c.K == 0 or (c.K == 1 and c.texels_only != 0 and c.logd_park != 0)
    limit = min(c.lds_budget, SIXTH) if c.lds_budget > 0 else SIXTH
    fits = COLS.get(c.K, 0) == 0 or c.lds_scene + COLS[c.K] * 256 * 4 <= limit
    return OWN_SLAB if (c.path_lean != 0 and c.flags == FL_TINY and c.integrator == _abi.INTEGRATOR_PATH and k_ok and own and slab and fits) else NONE


def test_the_columns_per_tangent_count(H):
    assert [H.hostcheck_path_lean_cols(k) for k in (0, 1, 3)] == [COLS[0], COLS[1], COLS[3]]


def test_the_headline_launch_takes_the_twins(H):
    assert both(H, case(K=0, chunk=512 * 512 * 64)) == OWN_SLAB
    assert both(H, case(K=1, chunk=512 * 512 * 64)) == OWN_SLAB


# own: (samples per pixel, chunk); slab: (rows, slab slots, trees); fit: staged scene bytes, forced budget
OWN_CASES = [(64, 8 * 8 * 64, True), (64, 5 * 3 * 64, True), (128, 8 * 8 * 128, False), (32, 8 * 8 * 32, False), (96, 8 * 8 * 96, False), (64, 1 << 5, False), (64, 96, False), (1, 64, False)]
SLAB_CASES = [(9, AA_BOX, 0, True), (10, AA_BOX, 0, False), (12, 0, 0, False), (9, AA_BOX, 1, False), (0, 0, 0, False)]
FIT_CASES = [(3584, 0), (SIXTH - 22 * 1024, 0), (SIXTH - 22 * 1024 + 16, 0), (3584, 3584 + 22 * 1024), (3584, 3584 + 22 * 1024 - 16)]


@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("option", [1, 0])
def test_every_combination_of_own_slab_fit_and_option(H, K, option):
    seen = set()
    for (nsp, chunk, own), (n_tiny, aa, n_blas, slab), (scene, budget) in itertools.product(OWN_CASES, SLAB_CASES, FIT_CASES):
        c = case(K=K, path_lean=option, nsp=nsp, chunk=chunk, n_tiny=n_tiny, aa_cnt=aa, n_blas=n_blas, lds_scene=scene, lds_budget=budget)
        want = expected(c)
        assert both(H, c) == want, (K, option, nsp, chunk, n_tiny, aa, n_blas, scene, budget)
        if not (own and slab) or option == 0 or K == 3:
            assert want == NONE
        seen.add(want)
    assert seen == ({NONE, OWN_SLAB} if (option == 1 and K != 3) else {NONE})


def test_the_columns_must_fit_a_sixth_of_the_cu_and_a_forced_budget(H):
    park = 22 * 1024
    assert both(H, case(K=1, lds_scene=SIXTH - park - (SIXTH - park) % 16)) == OWN_SLAB
    assert both(H, case(K=1, lds_scene=SIXTH - park + 16)) == NONE
    assert both(H, case(K=1, lds_scene=3584, lds_budget=3584 + park)) == OWN_SLAB
    assert both(H, case(K=1, lds_scene=3584, lds_budget=3584 + park - 16)) == NONE
    # renderC parks nothing: no budget stands in its way
    assert both(H, case(K=0, lds_scene=3584, lds_budget=1024)) == OWN_SLAB


def test_other_flag_sets_integrators_and_tangent_kinds_keep_their_kernels(H):
    for fl in (0, FL_ROUGH, FL_FOREST, FL_TINY | FL_ROUGH):
        assert both(H, case(flags=fl)) == NONE
    assert both(H, case(integrator=_abi.INTEGRATOR_DIRECT)) == NONE
    assert both(H, case(K=1, texels_only=0)) == NONE
    assert both(H, case(K=1, logd_park=0)) == NONE
    assert both(H, case(K=0, logd_park=0)) == OWN_SLAB          # logd_park speaks of the log-derivative launches only
    assert both(H, case(K=2)) == NONE


def test_own_is_never_chosen_for_a_chunk_off_the_pixel_boundary_or_a_sample_count_64_does_not_divide(H):
    for own_pixels, nsp, chunk in itertools.product((0, 1), (1, 2, 3, 8, 32, 48, 63, 64, 65, 96, 128, 192, 256), (1, 32, 63, 64, 96, 128, 960, 4096, 1 << 20, 3 * 64 * 5, 12345)):
        got = H.hostcheck_path_lean_wave_is_pixel(own_pixels, nsp, chunk)
        if chunk % nsp != 0 or nsp % 64 != 0 or own_pixels == 0:
            assert got == 0, (own_pixels, nsp, chunk)
        assert got == (1 if (own_pixels and nsp == 64 and chunk % 64 == 0) else 0)
        # the twin's form implies the kernels' `own`: a launch that stores its pixels
        if got:
            assert H.hostcheck_path_lean_owns(own_pixels, nsp, chunk) == 1
        for K in (0, 1):
            assert both(H, case(K=K, own_pixels=own_pixels, nsp=nsp, chunk=chunk)) == (OWN_SLAB if got else NONE)


def test_slab_only_means_no_row_behind_the_slab_slots(H):
    assert H.hostcheck_path_lean_slab_only(9, AA_BOX, 0) == 1
    assert H.hostcheck_path_lean_slab_only(9, 1, 0) == 1          # one rectangle: the slots of the other axes stay empty
    assert H.hostcheck_path_lean_slab_only(10, AA_BOX, 0) == 0    # a lone triangle or a rotated quad behind them
    assert H.hostcheck_path_lean_slab_only(12, 0, 0) == 0         # no slab form at all (option aa off): twelve plane-form rows
    assert H.hostcheck_path_lean_slab_only(9, AA_BOX, 2) == 0     # a two-level scene
    assert H.hostcheck_path_lean_slab_only(0, 0, 0) == 0
