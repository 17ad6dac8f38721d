"""The CollocatedIntegrator's estimator (csrc/psdr_collocated.h: a point light at the camera, Li = f(wi, wi) / r^2) on the HOST: the product's PSDR_HD functions
run slot by slot by tests/hostcheck/hostcheck_collocated.cpp.  The reference snapshot has no such integrator and the oracle is not extended, so the estimator is
pinned on closed forms, on the second oracle's BSDF values, on forward = reverse and on AD against finite differences of its own renderC."""
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle
import torch_oracle as to
from collocated_helpers import (DIFFUSE, HC_DEPS, ROUGH, colloc_opts, host_colloc_render, host_colloc_rev, host_film_samples, quad_xml, xml_scene)
from helpers import dot_tables, load_scene, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, san_program, write_tables_file
from psdr_cuda import _abi

RES, SPP = 16, 4


def _film_samples_from_oracle_rng(W, H, spp, offset):
    """(sx, sy) of every camera slot from oracle.rng (two draws per slot), in the kernel's fp32 arithmetic"""
    out = np.zeros((W * H * spp, 2), np.float32)
    for pixel in range(W * H):
        for s in range(spp):
            j = oracle.rng(pixel * spp + s, offset, 2)
            out[pixel * spp + s, 0] = (np.float32(pixel % W) + j[0]) / np.float32(W)
            out[pixel * spp + s, 1] = (np.float32(pixel // W) + j[1]) / np.float32(H)
    return out


def test_draws_per_slot():
    """two draws per camera slot, one per primary-edge slot: what _abi.draws_per_slot returns for a kind that is neither Direct nor Path"""
    assert _abi.INTEGRATOR_COLLOCATED == 3
    assert _abi.draws_per_slot(colloc_opts(4, 4))[:2] == (2, 1)


def test_diffuse_quad_closed_form():
    """A diffuse quad facing the camera: per pixel, the harness' renderC against rho / pi * cos(theta) / r^2 evaluated in float64 numpy at the same film samples
    (jitter from oracle.rng).  Bound 1e-5 relative per pixel: fp32 rounding of about twenty operations per sample."""
    sc = xml_scene(quad_xml(DIFFUSE, 0.0), RES, SPP)
    tb = sc.tables(0)
    o = colloc_opts(SPP, rng_offset=(3, 0, 0))
    img = host_colloc_render(tb, o).astype(np.float64)
    sxy = _film_samples_from_oracle_rng(RES, RES, SPP, 3)
    assert np.array_equal(sxy, host_film_samples(tb, o))          # the harness draws what oracle.rng draws
    cam = tb["cam"].detach().cpu().numpy().astype(np.float64)
    s2c, tw = cam[0:16].reshape(4, 4), cam[16:32].reshape(4, 4)
    v = np.concatenate([sxy.astype(np.float64), np.zeros((len(sxy), 1)), np.ones((len(sxy), 1))], axis=1) @ s2c.T
    d = v[:, :3] / v[:, 3:4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ tw[:3, :3].T
    org = tw[:3, 3] / tw[3, 3]
    T = tb["tri_info"].detach().cpu().numpy().astype(np.float64)
    rho = np.array([0.7, 0.5, 0.3], np.float32).astype(np.float64)
    val = np.zeros((len(sxy), 3))
    for row in T:          # Moeller-Trumbore against both triangles of the quad (no sample lies on the shared diagonal to 1e-12)
        p0, e1, e2, fn = row[0:3], row[3:6], row[6:9], row[18:21]
        h = np.cross(d, e2)
        f = 1.0 / (h @ e1)
        s = org - p0
        u = f * (h @ s)
        q = np.cross(s, e1)
        w = f * (d @ q)
        t = f * (q @ e2)
        hit = (u >= 0) & (w >= 0) & (u + w <= 1) & (t > 0)
        p = org + d * t[:, None]
        r2 = ((p - org) ** 2).sum(1)
        cos = -(d @ fn)          # the quad faces the camera
        val[hit] = (rho[None, :] / np.pi * (cos / r2)[:, None])[hit]
    ref = val.reshape(RES * RES, SPP, 3).mean(axis=1)
    assert (ref > 0).any() and (ref == 0).any()          # the quad and the background are both seen
    assert (img[ref[:, 0] == 0] == 0).all()
    err = np.abs(img - ref)[ref[:, 0] > 0] / ref[ref[:, 0] > 0]
    print("diffuse closed form: worst per-pixel relative error %.2e" % err.max())
    assert err.max() <= 1e-5, err.max()


def _f64_tables(tb):
    return {k: (v.detach().cpu().double() if isinstance(v, torch.Tensor) and v.is_floating_point() else (v.detach().cpu() if isinstance(v, torch.Tensor) else v)) for k, v in tb.items()}


@pytest.mark.parametrize("alpha", [(0.2, 0.2), (0.1, 0.4)], ids=["isotropic", "anisotropic"])
@pytest.mark.parametrize("tilt", [0.0, 30.0, 70.0])
def test_rough_conductor_retro_reflection(alpha, tilt):
    """The quad with a RoughConductor, tilted: the harness' renderC against the BSDF evaluation of oracle/torch_oracle.py (fp64, an independent restatement) called
    with wo = wi at the same film samples, divided by r^2.  Bound 2e-6 (image rel-L2): what the two restatements agree to."""
    def prepare(sc):
        b = sc.m_bsdfs[0]
        b.alpha_u.fill(alpha[0]); b.alpha_v.fill(alpha[1])
    sc = xml_scene(quad_xml(ROUGH % alpha[0], tilt), RES, SPP, prepare=prepare)
    tb = sc.tables(0)
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(tb, o)
    tt = _f64_tables(tb)
    sxy = torch.from_numpy(host_film_samples(tb, o).astype(np.float64))
    org, d = to.primary_ray(tt, sxy[:, 0], sxy[:, 1], False)
    its = to.intersect(tt, org, d, torch.ones(len(sxy), dtype=torch.bool), "C")
    f = to.bsdf_eval(tt, its, its.wi, False)
    r2 = ((its.p - org) ** 2).sum(-1)
    val = torch.where(its.valid.unsqueeze(-1), f / r2.unsqueeze(-1), torch.zeros_like(f))
    ref = val.reshape(RES * RES, SPP, 3).mean(dim=1).numpy()
    assert (ref > 0).any()
    print("rough conductor alpha %s tilt %g: rel-L2 %.2e" % (alpha, tilt, rel_l2(img, ref)))
    assert rel_l2(img, ref) <= 2e-6, rel_l2(img, ref)


@pytest.mark.parametrize("scene", ["cbox_uv", "cbox_rough", "bunny_light"])
def test_forward_equals_reverse(scene):
    """<adj, J t> = <J^T adj, t> for every gradient table the term reaches -- triangle rows, texels (albedo and alpha), the camera pose, primary-edge rows -- with
    random tangents and a random adjoint image; |lhs - rhs| <= 1e-4 * scale as test_reverse_mode.py::test_dot_product_identity_host.  bunny_light: two meshes,
    one tree."""
    res, spp, sppe = 16, 4, 4
    sc, _ = load_scene(scene, res=res, spp=spp, sppe=sppe)
    tb = sc.tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    for n in ("tri_info", "texels", "cam_to_world", "prim_edge"):
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan)
        img_r, grads = host_colloc_rev(tb, o, adj, want=[n])
        assert rel_l2(img_r, img) < 1e-6
        lhs, rhs = float((adj.astype(np.float64) * dimg).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg).sum())          # the sum itself may cancel
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)


# ---------------------------------------------------------------- AD against finite differences
AD_SPP, AD_SPPE, FD_SPP, NT = 1024, 4096, 16384, 8
DIRECTION = (1.0, 0.5, 0.0)


def _occluder(spp, sppe=0, offset=None):
    """cbox_occluder at res 24, Mesh[1] (the occluder) translated along DIRECTION: by P (offset None) or by a number"""
    import enoki as ek
    import psdr_cuda
    from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD, Matrix4f as Matrix4fD
    from psdr_cuda.fixtures import scene_path
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_occluder"), False)
    sc.opts.width = sc.opts.height = 24
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, 0, 0
    P = None
    if offset is None:
        P = FloatD(0.)
        ek.set_requires_gradient(P)
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * P))
    else:
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * FloatD(float(offset))))
    sc.configure()
    return sc, P


def test_ad_vs_fd_occluder():
    """cbox_occluder, res 24, the occluder translated: AD (interior + primary edges, forward mode) against the central difference (eps = 1) of the integrator's own
    renderC, both sides on the same streams -- the method of DESIGN.md section 10.  FD floor = distance of two independent FDs, AD seed distance = distance of two
    AD seeds (both relative to the FD's norm); bound: e_all <= 1.5 (floor + AD seed distance).  The same comparison with sppe = 0 must exceed that bound by a
    factor of two at least: the primary-edge term carries the silhouette, and nothing else is missing -- no secondary-edge term exists for this integrator.
    Measured: FD floor 0.0319, AD seed distance 0.0205, e_all 0.0175 (bound 0.0787), e(sppe = 0) 0.9992."""
    fds = []
    for seed in (0, 1):
        imgs = []
        for s in (+1.0, -1.0):
            sc, _ = _occluder(FD_SPP, offset=s)
            imgs.append(host_colloc_render(sc.tables(0), colloc_opts(FD_SPP, rng_offset=(1000 * seed, 0, 0)), nthreads=NT).astype(np.float64))
        fds.append((imgs[0] - imgs[1]) / 2.0)
    fd, floor = (fds[0] + fds[1]) / 2.0, rel_l2(fds[0], fds[1])
    sc, P = _occluder(AD_SPP, AD_SPPE)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    ads = [host_colloc_render(tb, colloc_opts(AD_SPP, AD_SPPE, rng_offset=(77 * seed, 55 * seed, 0)), mode=1, tangents=tan, nthreads=NT)[1].astype(np.float64) for seed in (0, 1)]
    ad_dist = float(np.linalg.norm(ads[0] - ads[1]) / np.linalg.norm(fd))
    e_all = rel_l2(ads[0], fd)
    e_no_edges = rel_l2(host_colloc_render(tb, colloc_opts(AD_SPP, 0), mode=1, tangents=tan, nthreads=NT)[1], fd)
    bound = 1.5 * (floor + ad_dist)
    print("collocated AD vs FD: floor %.4f, AD seed distance %.4f, e_all %.4f (bound %.4f), e without primary edges %.4f" % (floor, ad_dist, e_all, bound, e_no_edges))
    assert np.linalg.norm(fd) > 0
    assert e_all <= bound, (e_all, bound)
    assert e_no_edges >= 2.0 * bound, (e_no_edges, bound)


def test_scene_without_an_emitter():
    """A scene without any emitter is valid for this integrator: it configures (num_emitters = 0) and the harness renders it.  (That DirectIntegrator still fails
    on it with "No Emitter!" is the library's check: tests/test_collocated_gpu.py::test_scene_without_an_emitter.)"""
    sc = xml_scene(quad_xml(DIFFUSE, 30.0), RES, SPP)
    tb = sc.tables(0)
    assert tb["num_emitters"] == 0
    img = host_colloc_render(tb, colloc_opts(SPP))
    assert np.isfinite(img).all() and img.max() > 0
    # ... and an emitter in the scene adds nothing: the same quad as an area light renders the same image
    sc_e = xml_scene(quad_xml(DIFFUSE, 30.0, emitter=True), RES, SPP)
    assert sc_e.tables(0)["num_emitters"] == 1
    assert np.array_equal(host_colloc_render(sc_e.tables(0), colloc_opts(SPP)), img)


# ---------------------------------------------------------------- the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers(tmp_path):
    """tests/hostcheck/colloc_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_collocated.cpp, built with -fsanitize=address,undefined for
    the host (hostlibs.san_program): render, forward and reverse on one tiny scene; it must end clean and report what the library reports."""
    exe = san_program("colloc_san", HC_DEPS)
    res, spp, sppe = 8, 2, 2
    sc, _ = load_scene("cbox_rough", res=res, spp=spp, sppe=sppe)
    tb = sc.tables(0)
    o = colloc_opts(spp, sppe, rng_offset=(1, 2, 0))
    tan = random_tangents(tb, ["tri_info", "texels", "prim_edge"], seed=3)
    adj = np.random.default_rng(4).random((res * res, 3)).astype(np.float32)
    tbc, desc, keep = cpu_desc(tb)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in ("tri_info", "texels", "prim_edge")], adj)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan, nthreads=2)
    _, grads = host_colloc_rev(tb, o, adj, want=["tri_info", "texels", "prim_edge"])
    want = [np.abs(host_colloc_render(tb, o, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + [np.abs(grads[n].astype(np.float64)).sum() for n in ("tri_info", "texels", "prim_edge")]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
