"""The LightStageIntegrator's estimator (csrc/psdr_lightstage.h) on the host, against the PointLightIntegrator's host harness light by light: the stack shares
one hit among its lights, and plane l must be what the single-light estimator gives for light l (tests/test_pointlight_host.py pins that one on closed forms,
an analytic shadow and AD against finite differences).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from collocated_helpers import xml_scene
from helpers import dot_tables, load_scene, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, san_program, write_tables_file
from lightstage_helpers import BELOW_FLOOR, HC_DEPS, KIND, LIGHTS_MAX, OCCLUDER_LIGHTS, host_stack_render, host_stack_rev, lights_of, stack_opts
from pointlight_helpers import floor_occluder_xml, host_point_render, host_point_render_k3, host_point_rev, point_opts
from psdr_cuda import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
RES, SPP, SPPE, SPPSE = 16, 4, 4, 8
OFF = (2, 3, 4)
# the quad with an occluder (pointlight_helpers.floor_occluder_xml: the receiver at z = 0 faces +z, the occluder hangs at z = 150): lights in front of it, a
# coincident pair, one behind the receiver
QUAD_LIGHTS = np.array([(60.3, 180.7, 600.0), (-80.9, 100.3, 450.0), (60.3, 180.7, 600.0), (10.0, 120.0, -200.0), (5.1, 130.2, 300.0), (140.7, 60.1, 700.0)], np.float32)
BOUND = 1e-6          # test_pointlight_host's "K = 3 equals three K = 1 launches": same slots, same arithmetic per plane


@pytest.fixture(scope="module")
def occluder():
    sc, P = load_scene("cbox_occluder", res=RES, spp=SPP, sppe=SPPE, sppse=SPPSE, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    return tb, tangents_wrt(tb, P)


def _worst(worst, a, b):
    """the running worst rel-L2; a reference that is all zero asks for a result that is all zero"""
    if not np.any(b):
        assert not np.any(a)
        return worst
    return max(worst, rel_l2(a, b))


def test_kind():
    assert KIND == 5 and LIGHTS_MAX == 256 and _abi.INTEGRATOR_POINT == 4


@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_rough", "bunny_light", "cbox_bunny", "cbox_env"])
def test_light_sets_give_lit_and_dark_pixels(name):
    """every light of the shared sets except the one below the floor gives a plane with both lit and zero pixels (the single-light harness); that one is all zero"""
    sc, _ = load_scene(name, res=19, spp=3)
    tb = sc.tables(0)
    for l, p in enumerate(lights_of(name, tb)):
        img = host_point_render(tb, point_opts(3, rng_offset=(7, 0, 0)), p)
        if name == "cbox_occluder" and l == BELOW_FLOOR:
            assert (img == 0).all()
        else:
            assert img.max() > 0 and (img.max(axis=1) == 0).any(), (name, l)


@pytest.mark.parametrize("L", [1, 2, 3, 6])
def test_stack_equals_single_lights(occluder, L):
    """renderC, forward K = 1 (a texel set; the occluder's translation with all three terms; one light's translation; every light's tangent at once) and K = 3
    of the stack against host_point_render per light: rel-L2 1e-6.  Coincident lights give identical planes, the plane of the light below the floor is exactly 0."""
    tb, tan = occluder
    pos = OCCLUDER_LIGHTS[:L]
    oc, op = stack_opts(SPP, rng_offset=OFF), point_opts(SPP, rng_offset=OFF)
    o3, p3 = stack_opts(SPP, SPPE, SPPSE, rng_offset=OFF), point_opts(SPP, SPPE, SPPSE, rng_offset=OFF)
    worst = 0.0
    img = host_stack_render(tb, oc, pos)
    assert img.shape[0] == L
    ref = [host_point_render(tb, op, p) for p in pos]
    for l in range(L):
        if l == BELOW_FLOOR:
            assert (img[l] == 0).all() and (ref[l] == 0).all()
            continue
        worst = _worst(worst, img[l], ref[l])
    if L > 2:
        assert np.array_equal(img[0], img[2])
    # a texel set (material duals)
    ts = random_tangents(tb, ["texels"], seed=2)
    simg, sd = host_stack_render(tb, oc, pos, mode=1, tangent_sets=[ts])
    for l in range(L):
        rimg, rd = host_point_render(tb, op, pos[l], mode=1, tangents=ts)
        assert l == BELOW_FLOOR or np.abs(rd).max() > 0
        worst = max(_worst(worst, simg[l], rimg), _worst(worst, sd[0, l], rd))
    # the occluder's translation, interior + primary edges + shadow boundary
    simg, sd = host_stack_render(tb, o3, pos, mode=1, tangent_sets=[tan])
    for l in range(L):
        rimg, rd = host_point_render(tb, p3, pos[l], mode=1, tangents=tan)
        worst = _worst(worst, sd[0, l], rd)
    if L > 2:
        assert np.array_equal(sd[0, 0], sd[0, 2])
    # one light's translation: every other plane's derivative is exactly 0
    m = L - 1 if L != BELOW_FLOOR + 1 else 0
    dl = np.zeros((1, L, 3), np.float32)
    dl[0, m] = (1.0, 0.5, 0.0)
    _, sd = host_stack_render(tb, o3, pos, mode=1, d_pos=dl)
    _, rd = host_point_render(tb, p3, pos[m], mode=1, d_pos=dl[0, m])
    assert np.abs(rd).max() > 0
    worst = _worst(worst, sd[0, m], rd)
    for l in range(L):
        assert l == m or (sd[0, l] == 0).all(), l
    # every light's tangent at once
    rng = np.random.default_rng(9)
    dl = (rng.random((1, L, 3)) - 0.5).astype(np.float32)
    _, sd = host_stack_render(tb, o3, pos, mode=1, d_pos=dl)
    for l in range(L):
        _, rd = host_point_render(tb, p3, pos[l], mode=1, d_pos=dl[0, l])
        worst = _worst(worst, sd[0, l], rd)
    # K = 3: (geometry, texels, the lights)
    none = {}
    d3 = np.zeros((3, L, 3), np.float32)
    d3[2] = dl[0]
    simg, sd = host_stack_render(tb, o3, pos, mode=1, tangent_sets=[tan, ts, none], d_pos=d3)
    for l in range(L):
        rimg, rd = host_point_render_k3(tb, p3, pos[l], [tan, ts, none], d_pos=d3[:, l])
        worst = _worst(worst, simg[l], rimg)
        for k in range(3):
            worst = _worst(worst, sd[k, l], rd[k])
    print("L = %d: worst rel-L2 of a stack plane against the single-light harness %.2e" % (L, worst))
    assert worst < BOUND, worst


@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_rough"])
def test_forward_equals_reverse_and_the_sum_over_the_lights(name):
    """<A, J t> = <J^T A, t> per table with a random adjoint stack and all three terms on: |lhs - rhs| <= 1e-4 * scale (test_pointlight_host's
    test_forward_equals_reverse), the lights' positions included; the stack's gradient tables equal the sum of host_point_rev over the lights with A_l, and row l
    of g_pos is host_point_rev's of light l (rel-L2 1e-4: the hit's adjoint chain runs once on fp32 sums where the single-light runs add fp32 results)."""
    sc, _ = load_scene(name, res=12, spp=SPP, sppe=SPPE, sppse=SPPSE)
    tb = sc.tables(0)
    pos = lights_of(name, tb)
    L = len(pos)
    o, po = stack_opts(SPP, SPPE, SPPSE, rng_offset=OFF), point_opts(SPP, SPPE, SPPSE, rng_offset=OFF)
    A = np.random.default_rng(5).random((L, 12 * 12, 3)).astype(np.float32)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge"]
    img_r, grads, g_pos = host_stack_rev(tb, o, pos, A, want=names)
    A64 = A.astype(np.float64)
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = host_stack_render(tb, o, pos, mode=1, tangent_sets=[tan])
        assert rel_l2(img_r, img) < 1e-6
        lhs, rhs, scale = float((A64 * dimg[0]).sum()), dot_tables(grads, tan), float(np.abs(A64 * dimg[0]).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
    dl = (np.random.default_rng(6).random((1, L, 3)) - 0.5).astype(np.float32)
    _, dimg = host_stack_render(tb, o, pos, mode=1, d_pos=dl)
    lhs, rhs, scale = float((A64 * dimg[0]).sum()), float((g_pos.astype(np.float64) * dl[0]).sum()), float(np.abs(A64 * dimg[0]).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    # the sum of single-light reverse runs
    total = {n: np.zeros_like(grads[n], np.float64) for n in grads}
    for l in range(L):
        _, g1, gp1 = host_point_rev(tb, po, pos[l], A[l], want=names)
        for n in g1:
            total[n] += g1[n]
        if np.abs(gp1).max() > 0:
            assert rel_l2(g_pos[l], gp1) < 1e-4, (l, g_pos[l], gp1)
        else:
            assert (g_pos[l] == 0).all()
    for n in total:
        assert np.abs(total[n]).max() > 0 and rel_l2(grads[n], total[n]) < 1e-4, (n, rel_l2(grads[n], total[n]))


def test_constructor_checks():
    """the Python class's argument checks that need no library"""
    import psdr_cuda
    integ = psdr_cuda.LightStageIntegrator(OCCLUDER_LIGHTS, 2.0)
    assert integ._kind == KIND and tuple(integ.m_positions.t.shape) == (6, 3) and tuple(integ.m_intensities.t.shape) == (6, 3)
    assert float(integ.m_intensities.t[3, 1]) == 2.0 and integ.combine is False
    assert tuple(psdr_cuda.LightStageIntegrator(OCCLUDER_LIGHTS[:2], (1.0, 0.5, 0.25)).m_intensities.t[1].tolist()) == (1.0, 0.5, 0.25)
    assert psdr_cuda.LightStageIntegrator(OCCLUDER_LIGHTS[:2], [[1, 2, 3], [4, 5, 6]], combine=True).combine is True
    for bad in ([], [[0.0, 1.0]], [[0.0, float("nan"), 1.0]], np.zeros((257, 3))):
        with pytest.raises(Exception):
            psdr_cuda.LightStageIntegrator(bad)
    with pytest.raises(Exception):
        psdr_cuda.LightStageIntegrator(OCCLUDER_LIGHTS[:2], [[1, 2, 3]] * 3)


@pytest.mark.parametrize("L", [1, 6])
def test_host_functions_run_clean_under_the_sanitizers(tmp_path, L):
    """tests/hostcheck/lightstage_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_lightstage.cpp, built with -fsanitize=address,undefined
    for the host (hostlibs.san_program): render, forward and reverse with all three terms on the quad with an occluder, L = 1 and L = 6; it must end clean and
    report what the library reports."""
    exe = san_program("lightstage_san", HC_DEPS)
    res, spp, sppe, sppse = 8, 2, 2, 8

    def prep(sc):
        sc.opts.sppse = sppse
    tb = xml_scene(floor_occluder_xml(), res, spp, sppe, prepare=prep).tables(0)
    o = stack_opts(spp, sppe, sppse, rng_offset=(1, 2, 3))
    names = ("tri_info", "texels", "prim_edge", "sec_edge")
    tan = random_tangents(tb, list(names), seed=3)
    pos = QUAD_LIGHTS[:L]
    adj = np.random.default_rng(4).random((L, res * res, 3)).astype(np.float32)
    d_pos = (np.random.default_rng(5).random((1, L, 3)) - 0.5).astype(np.float32)
    tbc, desc, keep = cpu_desc(tb)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in names], adj, pos, d_pos)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path, str(L)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_stack_render(tb, o, pos, mode=1, tangent_sets=[tan], d_pos=d_pos, nthreads=2)
    _, grads, g_pos = host_stack_rev(tb, o, pos, adj, want=list(names))
    want = [np.abs(host_stack_render(tb, o, pos, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + \
           [np.abs(grads[n].astype(np.float64)).sum() for n in names] + [np.abs(g_pos.astype(np.float64)).sum()]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
