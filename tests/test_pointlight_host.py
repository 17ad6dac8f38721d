"""The PointLightIntegrator's estimator (csrc/psdr_pointlight.h: a point light anywhere, Li = f(wi, wo) V / r^2, and the boundary term of the moving shadow
outline) on the HOST: the product's PSDR_HD functions run slot by slot by tests/hostcheck/hostcheck_pointlight.cpp.  The reference snapshot has no such
integrator, so the estimator is pinned on closed forms written out in float64, on the collocated harness in the limit pL = camera, on an analytic hard shadow,
on forward = reverse and on AD against finite differences of its own renderC."""
import os
import subprocess

import numpy as np
import pytest

import enoki as ek
import psdr_cuda
from collocated_helpers import DIFFUSE, colloc_opts, host_colloc_render, host_film_samples, quad_xml, xml_scene
from colloc_microfacet_helpers import ROUGH_MAT, height_xml, microfacet_xml, normal_xml, scene, uv_quad_xml
from enoki.cuda_autodiff import Float32 as FloatD, Matrix4f as Matrix4fD, Vector3f as Vector3fD
from helpers import dot_tables, load_scene, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, san_program, write_tables_file
from pointlight_helpers import (HC_DEPS, HIDDEN_LIGHT, cam_pos, camera_rays64, floor_occluder_xml, hidden_occluder_xml, host_point_render, host_point_rev,
                                point_closed_form, point_opts)
from psdr_cuda import _abi

RES, SPP = 16, 4
OFF_AXIS = (60.0, 180.0, 600.0)


def test_kind_and_draws_per_slot():
    """kind 4; two draws per camera slot, one per primary-edge slot, three per shadow-boundary slot: _abi.draws_per_slot for a kind that is neither Direct nor Path"""
    assert _abi.INTEGRATOR_POINT == 4
    assert _abi.draws_per_slot(point_opts(4, 4, 4)) == (2, 1, 3)
    assert "psdr_scene_set_point_light" in _abi.HIP_SYMBOLS


# ---------------------------------------------------------------- 1. diffuse closed form
def test_diffuse_closed_form():
    """A diffuse quad facing the camera, the light off-axis, no occluder: per pixel, the harness' renderC against rho / pi cos(theta_L) / r_L^2 in float64 at the
    harness' own film samples.  Bound 1e-5 relative per pixel (tests/test_collocated_host.py's bound for the same arithmetic).  Measured worst pixel: 1.6e-7."""
    sc = xml_scene(quad_xml(DIFFUSE, 0.0), RES, SPP)
    tb = sc.tables(0)
    o = point_opts(SPP, rng_offset=(3, 0, 0))
    img = host_point_render(tb, o, OFF_AXIS).astype(np.float64)
    val, hit, _ = point_closed_form(tb, host_film_samples(tb, colloc_opts(SPP, rng_offset=(3, 0, 0))), OFF_AXIS)
    ref = val.reshape(RES * RES, SPP, 3).mean(axis=1)
    assert (ref > 0).any() and (ref == 0).any()
    assert (img[ref[:, 0] == 0] == 0).all()
    err = np.abs(img - ref)[ref[:, 0] > 0] / ref[ref[:, 0] > 0]
    print("point light, diffuse closed form: worst per-pixel relative error %.2e" % err.max())
    assert err.max() <= 1e-5, err.max()


# ---------------------------------------------------------------- 2. the collocated limit
@pytest.mark.parametrize("name", ["quad", "cbox_rough", "bunny_light"])
def test_collocated_limit(name):
    """With the light at the camera position the image is the collocated harness': rel-L2 <= 2e-6 (the bound of the collocated BSDF checks).  A shadow ray that
    re-hits its own surface would darken the image.  Measured: 0 on all three (the same fp32 operations)."""
    if name == "quad":
        sc = xml_scene(quad_xml(DIFFUSE, 30.0), RES, SPP)
    else:
        sc, _ = load_scene(name, res=RES, spp=SPP)
    tb = sc.tables(0)
    ref = host_colloc_render(tb, colloc_opts(SPP, rng_offset=(2, 0, 0)))
    img = host_point_render(tb, point_opts(SPP, rng_offset=(2, 0, 0)), cam_pos(tb))
    assert ref.max() > 0
    print("collocated limit %s: rel-L2 %.2e" % (name, rel_l2(img, ref)))
    assert rel_l2(img, ref) <= 2e-6, rel_l2(img, ref)


# ---------------------------------------------------------------- 3. general wo
# Two light directions.  "grazing" comes in almost along the quad's plane from +y (the tilts turn the quad about y, so it stays grazing at every tilt): part of a
# mapped quad has wo below n'.  Neither puts the half vector near a mapped quad's normal: at the GGX peak the relative condition number of D in h.z is
# 2 (1 / alpha^2 - 1) h.z^2 / q (some hundreds at the maps' roughness 0.2), so fp32 rounding of h alone is 5e-6 there (measured with the light at
# (500, 125, 60), tilt 30: 2.8e-6 image rel-L2, 7e-6 on the peak's pixels) -- the collocated bound 2e-6 holds where wi = wo = h needs no normalisation.
LIGHTS = {"front": (150.0, 200.0, 500.0), "grazing": (0.0, 625.0, 60.0)}
# The maps lean n' by up to about 12 degrees (normal texels with a tangential part within +-0.15; heights in [0, 1] at a scale of 2 world units).  At the 70 degree
# tilt the view is 20 degrees above the face, and the specular lobe's G1(wi') / wi'.z has relative condition number 1 / wi'.z in the rounded direction: with
# wi'.z >= sin(8 deg) = 0.14 an fp32 direction (6e-8) stays under 1e-6.  (Maps that lean 26 degrees, colloc_microfacet_helpers' random ones, put wi'.z through
# zero on the quad: measured 2.3e-6 .. 7.8e-6 at 70 degrees, all of it on the samples next to that line.)
def _gentle_normals():
    from colloc_microfacet_helpers import encode
    rng = np.random.default_rng(7)
    return encode(np.concatenate([rng.uniform(-0.15, 0.15, (16, 2)), np.ones((16, 1))], axis=1)).astype(np.float32)


_KIND_XML = {"plain": lambda: (microfacet_xml(0.3), dict(textured=True)), "normal": lambda: (normal_xml(0.3), dict(textured=True, normal=_gentle_normals())),
             "height": lambda: (height_xml(0.3, scale=2.0), dict(textured=True, height="random", scale=2.0))}


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("tilt", [0.0, 30.0, 70.0])
@pytest.mark.parametrize("kind", ["plain", "normal", "height"])
def test_general_wo_closed_form(kind, tilt, light):
    """MicrofacetBSDF types 2, 3 and 4 with wo != wi: the harness' renderC of the tilted textured quad against the closed forms of DESIGN.md sections 14 - 16
    written out in float64 (colloc_microfacet_helpers.microfacet64 and the kinds' perturbed normals, wi and wo in a frame about n').  Where the closed form is zero
    -- the light below the face or below n' -- the harness' pixel is EXACTLY zero.  Bound 2e-6 image rel-L2, as in the test_colloc_* host files.
    Measured: 1.9e-7 .. 7.5e-7 under the front light, up to 1.7e-6 under the grazing light at 70 degrees."""
    xml, kw = _KIND_XML[kind]()
    sc = scene(uv_quad_xml(xml, tilt), RES, SPP, **kw)
    tb = sc.tables(0)
    o = point_opts(SPP, rng_offset=(5, 0, 0))
    img = host_point_render(tb, o, LIGHTS[light])
    sxy = host_film_samples(tb, colloc_opts(SPP, rng_offset=(5, 0, 0)))
    val, hit, _ = point_closed_form(tb, sxy, LIGHTS[light], kind)
    ref = val.reshape(RES * RES, SPP, 3).mean(axis=1)
    dark = (val == 0).all(axis=1).reshape(RES * RES, SPP).all(axis=1)
    assert (img[dark] == 0).all()
    if not (ref > 0).any():
        return          # the light is behind the face: all of the image is exactly zero
    e = rel_l2(img, ref)
    print("general wo %s tilt %g light %s: rel-L2 %.2e, %d of %d quad samples dark" % (kind, tilt, light, e, int(((val == 0).all(axis=1) & hit).sum()), int(hit.sum())))
    assert e <= 2e-6, e


def test_grazing_light_darkens_part_of_the_mapped_quad():
    """the case of test_general_wo_closed_form that the issue asks for by name: under the grazing light some samples of the normal-mapped quad have wo below n'
    and some do not (so the exact zeros above are not vacuous)"""
    xml, kw = _KIND_XML["normal"]()
    tb = scene(uv_quad_xml(xml, 0.0), RES, SPP, **kw).tables(0)
    val, hit, _ = point_closed_form(tb, host_film_samples(tb, colloc_opts(SPP, rng_offset=(5, 0, 0))), LIGHTS["grazing"], "normal")
    darkq = (val == 0).all(axis=1) & hit
    assert darkq.any() and (~darkq & hit).any(), (int(darkq.sum()), int(hit.sum()))


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("tilt", [0.0, 30.0, 70.0])
def test_rough_conductor_general_wo(tilt, light):
    """RoughConductor with wo != wi against the BSDF evaluation of oracle/torch_oracle.py (fp64, an independent restatement) at the harness' film samples, with
    wo = the direction to the light in the hit's frame, over r_L^2.  Bound 2e-6 image rel-L2 (test_collocated_host.py::test_rough_conductor_retro_reflection).  Measured: 1.2e-7 .. 2.8e-7."""
    import torch
    import torch_oracle as to
    sc = xml_scene(quad_xml(ROUGH_MAT % ("m", 0.2), tilt), RES, SPP)
    tb = sc.tables(0)
    img = host_point_render(tb, point_opts(SPP, rng_offset=(5, 0, 0)), LIGHTS[light])
    tt = {k: (v.detach().cpu().double() if isinstance(v, torch.Tensor) and v.is_floating_point() else (v.detach().cpu() if isinstance(v, torch.Tensor) else v)) for k, v in tb.items()}
    sxy = torch.from_numpy(host_film_samples(tb, colloc_opts(SPP, rng_offset=(5, 0, 0))).astype(np.float64))
    org, d = to.primary_ray(tt, sxy[:, 0], sxy[:, 1], False)
    its = to.intersect(tt, org, d, torch.ones(len(sxy), dtype=torch.bool), "C")
    dv = torch.tensor(LIGHTS[light], dtype=torch.float64) - its.p
    r2 = (dv * dv).sum(-1)
    l = dv / r2.sqrt().unsqueeze(-1)
    wo = torch.stack([(l * its.sh_s).sum(-1), (l * its.sh_t).sum(-1), (l * its.sh_n).sum(-1)], dim=-1)
    f = to.bsdf_eval(tt, its, wo, False)
    val = torch.where(its.valid.unsqueeze(-1), f / r2.unsqueeze(-1), torch.zeros_like(f))
    ref = val.reshape(RES * RES, SPP, 3).mean(dim=1).numpy()
    assert (img[(ref == 0).all(axis=1)] == 0).all()
    if (ref > 0).any():
        print("rough conductor general wo tilt %g light %s: rel-L2 %.2e" % (tilt, light, rel_l2(img, ref)))
        assert rel_l2(img, ref) <= 2e-6, rel_l2(img, ref)


# ---------------------------------------------------------------- 4. hard shadow
def test_hard_shadow():
    """A 40 x 40 occluder (outside the camera's view) between the light and the receiver quad: its shadow on the receiver is the square of side 160 / 3 about
    (0, 125).  Pixels whose footprint (the receiver points of the pixel's four corners, and hence of every sample in it) lies wholly inside the shadow are exactly 0,
    pixels wholly outside equal the unoccluded closed form (1e-5 per pixel, as test_diffuse_closed_form); the pixels the outline cuts are the only ones left out:
    under 15 % of the pixels that see the receiver (asserted).  Measured: 28 of 528 = 5.3 %, 36 pixels wholly inside."""
    res = 32
    sc = xml_scene(hidden_occluder_xml(), res, SPP)
    tb = sc.tables(0)
    o = point_opts(SPP, rng_offset=(9, 0, 0))
    img = host_point_render(tb, o, HIDDEN_LIGHT).astype(np.float64)
    sxy = host_film_samples(tb, colloc_opts(SPP, rng_offset=(9, 0, 0)))
    val, hit, _ = point_closed_form(tb, sxy, HIDDEN_LIGHT, rows=(0, 1))          # (rows 0, 1: the receiver; the occluder is not in view: asserted below)
    vall, hitall, _ = point_closed_form(tb, sxy, HIDDEN_LIGHT)
    assert np.array_equal(hit, hitall) and np.array_equal(val, vall)
    ref = val.reshape(res * res, SPP, 3).mean(axis=1)
    # the pixel corners on the receiver plane z = 0
    gx, gy = np.meshgrid(np.arange(res + 1) / res, np.arange(res + 1) / res)
    org, d = camera_rays64(tb, np.stack([gx.ravel(), gy.ravel()], axis=1))
    p = org + d * (-org[2] / d[:, 2])[:, None]
    px, py = p[:, 0].reshape(res + 1, res + 1), p[:, 1].reshape(res + 1, res + 1)
    corners = lambda a: np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]], axis=-1).reshape(res * res, 4)          # noqa: E731
    cx, cy = corners(px), corners(py)
    L = np.asarray(HIDDEN_LIGHT)
    k = L[2] / (L[2] - 150.0)
    lo = L[:2] + (np.array([130.0, 105.0]) - L[:2]) * k
    hi = L[:2] + (np.array([170.0, 145.0]) - L[:2]) * k
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    assert np.allclose(hi - lo, 160.0 / 3.0) and np.allclose((lo + hi) / 2, (0.0, 125.0))
    m = 1e-3          # (ShadowEpsilon-sized margin about the outline)
    inside = ((cx > lo[0] + m) & (cx < hi[0] - m) & (cy > lo[1] + m) & (cy < hi[1] - m)).all(axis=1)
    outside = (cx.max(1) < lo[0] - m) | (cx.min(1) > hi[0] + m) | (cy.max(1) < lo[1] - m) | (cy.min(1) > hi[1] + m)
    on_receiver = hit.reshape(res * res, SPP).any(axis=1)
    cut = on_receiver & ~inside & ~outside
    share = cut.sum() / on_receiver.sum()
    print("hard shadow: %d pixels inside, %d cut by the outline of %d on the receiver (%.1f %%)" % (inside.sum(), cut.sum(), on_receiver.sum(), 100 * share))
    assert inside.sum() >= 16 and share < 0.15, (inside.sum(), share)
    assert (img[inside] == 0).all()
    lit = outside & (ref[:, 0] > 0)
    err = np.abs(img - ref)[lit] / ref[lit]
    assert err.max() <= 1e-5, err.max()
    assert (img[outside & (ref[:, 0] == 0)] == 0).all()


# ---------------------------------------------------------------- 5. forward = reverse
def _occluder_scene(name, res, spp, sppe, sppse):
    if name == "quad":
        def prep(sc):
            sc.opts.sppse = sppse
        return xml_scene(floor_occluder_xml(), res, spp, sppe, prepare=prep), np.array(OFF_AXIS, np.float32)
    sc, _ = load_scene(name, res=res, spp=spp, sppe=sppe, sppse=sppse)
    return sc, np.array({"cbox_occluder": (30.0, 180.0, 50.0), "bunny_light": (0.0, 0.0, 0.0)}[name], np.float32)


@pytest.mark.parametrize("name", ["quad", "cbox_occluder", "bunny_light"])
def test_forward_equals_reverse(name):
    """<adj, J t> = <J^T adj, t> per table -- triangle rows, texels, the camera pose, primary-edge rows, secondary-edge rows, the light position -- with random
    tangents and a random adjoint image, all three terms on: |lhs - rhs| <= 1e-4 * scale (scale = sum |adj x dimg|: the sum itself may cancel).  bunny_light: the
    light halfway between the camera and the scene's centre (two meshes, one tree)."""
    res, spp, sppe, sppse = 16, 4, 4, 8
    sc, pos = _occluder_scene(name, res, spp, sppe, sppse)
    tb = sc.tables(0)
    if name == "bunny_light":
        T = tb["tri_info"].detach().cpu().numpy()
        pos = (0.5 * (cam_pos(tb) + T[:, 0:3].mean(axis=0)) + np.array([40.0, 60.0, 0.0])).astype(np.float32)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    for n in ("tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge", "light"):
        tan = random_tangents(tb, [n], seed=1) if n != "light" else {}
        d_pos = np.array([0.3, -0.2, 0.4], np.float32) if n == "light" else None
        img, dimg = host_point_render(tb, o, pos, mode=1, tangents=tan, d_pos=d_pos)
        img_r, grads, g_pos = host_point_rev(tb, o, pos, adj, want=[n] if n != "light" else [], light=n == "light")
        assert rel_l2(img_r, img) < 1e-6
        lhs = float((adj.astype(np.float64) * dimg).sum())
        rhs = dot_tables(grads, tan) if n != "light" else float(g_pos.astype(np.float64) @ d_pos)
        scale = float(np.abs(adj.astype(np.float64) * dimg).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
    # the shadow boundary reaches the secondary-edge rows, the receiver's triangle rows and the light
    o_se = point_opts(0, 0, sppse, rng_offset=(2, 3, 4))
    o_se.spp = spp          # (check_counts-style: spp stays the divisor of nothing here; no camera slot is in the shard)
    o_se.spp_begin = o_se.spp_end = 0
    _, g, g_pos = host_point_rev(tb, o_se, pos, adj, want=["sec_edge", "tri_info"])
    assert np.abs(g["sec_edge"]).sum() > 0 and np.abs(g["tri_info"]).sum() > 0 and np.abs(g_pos).sum() > 0


# ---------------------------------------------------------------- 7. AD against finite differences
AD_SPP, AD_SPPE, AD_SPPSE, FD_SPP, NT = 1024, 4096, 4096, 16384, 8
DIRECTION = (1.0, 0.5, 0.0)
CBOX_LIGHT = np.array([30.0, 180.0, 50.0])


def _cbox_occluder(spp, sppe=0, sppse=0, offset=None):
    """cbox_occluder at res 24, Mesh[1] (the occluder) translated along DIRECTION: by P (offset None) or by a number"""
    from psdr_cuda.fixtures import scene_path
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_occluder"), False)
    sc.opts.width = sc.opts.height = 24
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    P = None
    if offset is None:
        P = FloatD(0.)
        ek.set_requires_gradient(P)
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * P))
    else:
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * FloatD(float(offset))))
    sc.configure()
    return sc, P


def _fd(render):
    """central difference (step 1) from two seeds: (mean, distance of the two relative to it)"""
    fds = []
    for seed in (0, 1):
        im = [render(s, point_opts(FD_SPP, rng_offset=(1000 * seed, 0, 0))).astype(np.float64) for s in (+1.0, -1.0)]
        fds.append((im[0] - im[1]) / 2.0)
    return (fds[0] + fds[1]) / 2.0, rel_l2(fds[0], fds[1])


def _ad_check(label, fd, floor, ad_of):
    """the section-12 recipe: e_all <= 1.5 (FD floor + AD seed distance); returns the bound"""
    ads = [ad_of(point_opts(AD_SPP, AD_SPPE, AD_SPPSE, rng_offset=(77 * seed, 55 * seed, 33 * seed))).astype(np.float64) for seed in (0, 1)]
    ad_dist = float(np.linalg.norm(ads[0] - ads[1]) / np.linalg.norm(fd))
    e_all, bound = rel_l2(ads[0], fd), 1.5 * (floor + ad_dist)
    print("point light AD vs FD, %s: floor %.4f, AD seed distance %.4f, e_all %.4f (bound %.4f)" % (label, floor, ad_dist, e_all, bound))
    assert np.linalg.norm(fd) > 0
    assert e_all <= bound, (label, e_all, bound)
    return bound


def test_ad_vs_fd_occluder_translation():
    """cbox_occluder, res 24, the occluder translated, the light under the ceiling beside it: AD with all three terms on against the central difference of the
    integrator's own renderC.  Without the shadow-boundary term the error must be at least twice the bound: the occluder's shadow on the floor moves.
    Measured: floor 0.0316, AD seed distance 0.0598, e_all 0.0787 (bound 0.1371), e(sppse = 0) 0.4545."""
    fd, floor = _fd(lambda s, o: host_point_render(_cbox_occluder(FD_SPP, offset=s)[0].tables(0), o, CBOX_LIGHT, nthreads=NT))
    sc, P = _cbox_occluder(AD_SPP, AD_SPPE, AD_SPPSE)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    bound = _ad_check("occluder", fd, floor, lambda o: host_point_render(tb, o, CBOX_LIGHT, mode=1, tangents=tan, nthreads=NT)[1])
    e_no_se = rel_l2(host_point_render(tb, point_opts(AD_SPP, AD_SPPE, 0), CBOX_LIGHT, mode=1, tangents=tan, nthreads=NT)[1], fd)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se >= 2.0 * bound, (e_no_se, bound)


def test_ad_vs_fd_light_translation():
    """the same scene, the LIGHT translated along DIRECTION: interior (r^2, wo) + shadow boundary against the central difference.
    Measured: floor 0.0312, AD seed distance 0.1037, e_all 0.1910 (bound 0.2023)."""
    tb = _cbox_occluder(FD_SPP, offset=0.0)[0].tables(0)
    dl = np.asarray(DIRECTION)
    fd, floor = _fd(lambda s, o: host_point_render(tb, o, CBOX_LIGHT + s * dl, nthreads=NT))
    tba = _cbox_occluder(AD_SPP, AD_SPPE, AD_SPPSE, offset=0.0)[0].tables(0)
    _ad_check("light", fd, floor, lambda o: host_point_render(tba, o, CBOX_LIGHT, mode=1, d_pos=dl, nthreads=NT)[1])


def test_hidden_occluder_boundary_term_carries_the_derivative():
    """The occluder outside the camera's view, only its shadow visible (the scene of test_hard_shadow): the primary-edge term is zero, the interior term sees
    nothing of the translation, so with sppse = 0 the relative error against the central difference must exceed 0.9, and with the term on it meets the bound of
    the recipe.  Measured: floor 0.0160, AD seed distance 0.0096, e_all 0.0136 (bound 0.0384), e(sppse = 0) 1.0000."""
    def moved(spp, sppe, sppse, offset):
        P = [None]

        def prep(sc):
            sc.opts.sppse = sppse
            if offset is None:
                P[0] = FloatD(0.)
                ek.set_requires_gradient(P[0])
                sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * P[0]))
            else:
                sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * FloatD(float(offset))))
        return xml_scene(hidden_occluder_xml(), 24, spp, sppe, prepare=prep), P[0]
    fd, floor = _fd(lambda s, o: host_point_render(moved(FD_SPP, 0, 0, s)[0].tables(0), o, HIDDEN_LIGHT, nthreads=NT))
    sc, P = moved(AD_SPP, AD_SPPE, AD_SPPSE, None)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    _ad_check("hidden occluder", fd, floor, lambda o: host_point_render(tb, o, HIDDEN_LIGHT, mode=1, tangents=tan, nthreads=NT)[1])
    e_no_se = rel_l2(host_point_render(tb, point_opts(AD_SPP, AD_SPPE, 0), HIDDEN_LIGHT, mode=1, tangents=tan, nthreads=NT)[1], fd)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se > 0.9, e_no_se


# ---------------------------------------------------------------- 8. surface (what needs no GPU)
def test_constructor_checks():
    integ = psdr_cuda.PointLightIntegrator((1.0, 2.0, 3.0), (0.5, 1.0, 2.0))
    assert integ.m_position.numpy().tolist() == [[1.0, 2.0, 3.0]] and integ.m_intensity.numpy().tolist() == [[0.5, 1.0, 2.0]]
    assert psdr_cuda.PointLightIntegrator(Vector3fD([4.0, 5.0, 6.0])).m_intensity.numpy().tolist() == [[1.0, 1.0, 1.0]]
    for bad in ((1.0, 2.0), (1.0, 2.0, float("nan")), 3.0):
        with pytest.raises(Exception):
            psdr_cuda.PointLightIntegrator(bad)
    with pytest.raises(Exception):
        psdr_cuda.PointLightIntegrator((0.0, 0.0, 0.0), (1.0, 2.0))
    assert "PointLightIntegrator" in psdr_cuda.__all__


def test_scene_without_an_emitter_and_emitters_add_nothing():
    sc = xml_scene(quad_xml(DIFFUSE, 30.0), RES, SPP)
    tb = sc.tables(0)
    assert tb["num_emitters"] == 0
    img = host_point_render(tb, point_opts(SPP), OFF_AXIS)
    assert np.isfinite(img).all() and img.max() > 0
    sc_e = xml_scene(quad_xml(DIFFUSE, 30.0, emitter=True), RES, SPP)
    assert sc_e.tables(0)["num_emitters"] == 1
    assert np.array_equal(host_point_render(sc_e.tables(0), point_opts(SPP), OFF_AXIS), img)


# ---------------------------------------------------------------- 9. the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers(tmp_path):
    """tests/hostcheck/pointlight_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_pointlight.cpp, built with -fsanitize=address,undefined
    for the host (hostlibs.san_program): render, forward and reverse with all three terms on one tiny scene; it must end clean and report what the library reports."""
    exe = san_program("pointlight_san", HC_DEPS)
    res, spp, sppe, sppse = 8, 2, 2, 8
    sc, _ = load_scene("cbox_occluder", res=res, spp=spp, sppe=sppe, sppse=sppse)
    tb = sc.tables(0)
    o = point_opts(spp, sppe, sppse, rng_offset=(1, 2, 3))
    names = ("tri_info", "texels", "prim_edge", "sec_edge")
    tan = random_tangents(tb, list(names), seed=3)
    adj = np.random.default_rng(4).random((res * res, 3)).astype(np.float32)
    pos, d_pos = CBOX_LIGHT.astype(np.float32), np.array([0.3, -0.2, 0.4], np.float32)
    tbc, desc, keep = cpu_desc(tb)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in names], adj, pos, d_pos)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_point_render(tb, o, pos, mode=1, tangents=tan, d_pos=d_pos, nthreads=2)
    _, grads, g_pos = host_point_rev(tb, o, pos, adj, want=list(names))
    want = [np.abs(host_point_render(tb, o, pos, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + \
           [np.abs(grads[n].astype(np.float64)).sum() for n in names] + [np.abs(g_pos.astype(np.float64)).sum()]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)


# ---------------------------------------------------------------- 6. the independent boundary reference
def _hidden(spp, sppe, sppse, moving):
    """hidden_occluder_xml at res 24; moving: the occluder translated by DIRECTION * P (returns P), otherwise at rest"""
    P = [None]

    def prep(sc):
        sc.opts.sppse = sppse
        if moving:
            P[0] = FloatD(0.)
            ek.set_requires_gradient(P[0])
            sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(DIRECTION)) * P[0]))
    return xml_scene(hidden_occluder_xml(), 24, spp, sppe, prepare=prep), P[0]


def _against_reference(label, ref, ad_of):
    """rel-L2 of the AD derivative image against the float64 reference; bound 1.5 x the rel-L2 distance of two AD seeds at the test's sample counts"""
    ads = [ad_of(point_opts(AD_SPP, AD_SPPE, AD_SPPSE, rng_offset=(77 * seed, 55 * seed, 33 * seed))).astype(np.float64) for seed in (0, 1)]
    dist, e = rel_l2(ads[0], ads[1]), rel_l2(ads[0], ref)
    print("point light, line-integral reference, %s: AD seed distance %.4f, error %.4f (bound %.4f)" % (label, dist, e, 1.5 * dist))
    assert np.linalg.norm(ref) > 0
    assert e <= 1.5 * dist, (label, e, 1.5 * dist)


def test_boundary_reference_occluder_translation():
    """The occluder outside the camera's view, only its shadow on the Lambertian receiver seen (the primary-edge term is zero, the interior term sees nothing of
    the occluder).  Translate the occluder along DIRECTION: its shadow, the square of shadow_square, moves rigidly with velocity k DIRECTION, k = L.z / (L.z - 150),
    and the per-pixel derivative image is minus the line integral of the unoccluded closed form times the film's area density along the outline
    (pointlight_helpers.outline_line_integral: float64 numpy, no project code).  The harness' forward mode with all three terms against it: 1.5 x the distance of two
    AD seeds; with sppse = 0 the relative error exceeds 0.9 -- the shadow-boundary term carries the derivative.  This pins the Jacobian (rD / rB)(sinphi / sinphi2),
    the sign rule and the cosine that turns sensor_val into a density per receiver area.
    Measured: AD seed distance 0.0096, error 0.0072 (bound 0.0144); with sppse = 0: 1.0000."""
    from pointlight_helpers import outline_line_integral, shadow_square
    sc, P = _hidden(AD_SPP, AD_SPPE, AD_SPPSE, True)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    lo, hi, k = shadow_square(HIDDEN_LIGHT, (130.0, 105.0), (170.0, 145.0), 150.0)
    ref = outline_line_integral(tb, HIDDEN_LIGHT, lo, hi, k * np.asarray(DIRECTION[:2]))
    _against_reference("occluder", ref, lambda o: host_point_render(tb, o, HIDDEN_LIGHT, mode=1, tangents=tan, nthreads=NT)[1])
    e_no_se = rel_l2(host_point_render(tb, point_opts(AD_SPP, AD_SPPE, 0), HIDDEN_LIGHT, mode=1, tangents=tan, nthreads=NT)[1], ref)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se > 0.9, e_no_se


def test_boundary_reference_light_translation():
    """The same scene, the LIGHT translated along DIRECTION (in its plane z = 600, so k stays): the outline moves with velocity (1 - k) DIRECTION -- the line integral
    as above -- and the lit part changes through cos(theta_L) / r_L^2 (pointlight_helpers.interior_light_derivative: the closed form's float64 central difference
    over 32 x 32 film points per pixel).  Interior + boundary of the harness against their sum: 1.5 x the distance of two AD seeds.
    Measured: AD seed distance 0.0091, error 0.0072 (bound 0.0137)."""
    from pointlight_helpers import interior_light_derivative, outline_line_integral, shadow_square
    tb = _hidden(AD_SPP, AD_SPPE, AD_SPPSE, False)[0].tables(0)
    dl = np.asarray(DIRECTION)
    lo, hi, k = shadow_square(HIDDEN_LIGHT, (130.0, 105.0), (170.0, 145.0), 150.0)
    ref = outline_line_integral(tb, HIDDEN_LIGHT, lo, hi, (1.0 - k) * dl[:2]) + interior_light_derivative(tb, HIDDEN_LIGHT, dl, lo, hi, (-80.0, 45.0), (80.0, 205.0))
    _against_reference("light", ref, lambda o: host_point_render(tb, o, HIDDEN_LIGHT, mode=1, d_pos=dl, nthreads=NT)[1])


# ---------------------------------------------------------------- 7c. AD against FD: a roughness texel under off-axis light
def test_ad_vs_fd_roughness_texel():
    """A MicrofacetBSDF quad with 4 x 4 maps, tilted 30 degrees, the light off-axis (wo != wi): d image / d (one roughness texel) in forward mode -- the material
    adjoint's forward twin, colloc_bsdf_eval with dual texels -- against the central difference (step 0.02) of the harness' own renderC, by the recipe of the cases
    above: e_all <= 1.5 (FD floor + AD seed distance).  Reverse mode reaches the same texel: <adj, column> = gradient entry (1e-4 of the scale).
    Measured: floor 0.0030, AD seed distance 0.0140, e_all 0.0102 (bound 0.0255)."""
    import torch
    from colloc_microfacet_helpers import record
    light, eps = LIGHTS["front"], 0.02
    tb = scene(uv_quad_xml(microfacet_xml(0.3), 30.0), 24, 4, textured=True).tables(0)
    idx = record(tb, "plain")[1]["roughness"] + 5          # an inner texel of the 4 x 4 map
    onehot = torch.zeros(tb["texels"].numel())
    onehot[idx] = 1.0

    def moved(s):
        t = dict(tb)
        t["texels"] = tb["texels"].detach().clone()
        t["texels"].reshape(-1)[idx] += s * eps
        return t
    fds = []
    for seed in (0, 1):
        im = [host_point_render(moved(s), point_opts(FD_SPP, rng_offset=(1000 * seed, 0, 0)), light, nthreads=NT).astype(np.float64) for s in (+1.0, -1.0)]
        fds.append((im[0] - im[1]) / (2.0 * eps))
    fd, floor = (fds[0] + fds[1]) / 2.0, rel_l2(fds[0], fds[1])
    _ad_check("roughness texel", fd, floor, lambda o: host_point_render(tb, o, light, mode=1, tangents={"texels": onehot.reshape(tb["texels"].shape)}, nthreads=NT)[1])
    adj = np.random.default_rng(8).random((24 * 24, 3)).astype(np.float32)
    o = point_opts(16, rng_offset=(4, 0, 0))
    col = host_point_render(tb, o, light, mode=1, tangents={"texels": onehot.reshape(tb["texels"].shape)})[1].astype(np.float64)
    _, g, _ = host_point_rev(tb, o, light, adj, want=["texels"], light=False)
    lhs, scale = float((adj * col).sum()), float(np.abs(adj * col).sum())
    assert scale > 0 and abs(lhs - float(g["texels"].reshape(-1)[idx])) <= 1e-4 * scale, (lhs, g["texels"].reshape(-1)[idx], scale)


def test_k3_equals_three_k1_launches():
    """forward mode with K = 3 (three tangent sets and three light tangents in one pass over the slots) gives the columns of three K = 1 runs, all three terms on:
    a geometry set, a texel set and the light alone, on cbox_occluder.  Same slots, same arithmetic per column: 1e-6."""
    from pointlight_helpers import host_point_render_k3
    sc, _ = load_scene("cbox_occluder", res=16, spp=4, sppe=4, sppse=8)
    tb = sc.tables(0)
    o = point_opts(4, 4, 8, rng_offset=(2, 3, 4))
    sets = [random_tangents(tb, ["tri_info", "prim_edge", "sec_edge"], seed=1), random_tangents(tb, ["texels"], seed=2), {}]
    d_pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.3, -0.2, 0.4]], np.float32)
    img3, d3 = host_point_render_k3(tb, o, CBOX_LIGHT, sets, d_pos)
    for k in range(3):
        # (the K = 3 run is a geometry run for every column; a K = 1 run of the texel set alone takes the on-surface form of the hit: same value and derivative)
        img1, d1 = host_point_render(tb, o, CBOX_LIGHT, mode=1, tangents=sets[k], d_pos=d_pos[k] if k == 2 else None)
        assert np.abs(d1).max() > 0
        assert rel_l2(img3, img1) < 1e-6 and rel_l2(d3[k], d1) < (1e-5 if k == 1 else 1e-6), (k, rel_l2(img3, img1), rel_l2(d3[k], d1))


def test_ad_vs_fd_light_translation_smooth_normals():
    """bunny_light at res 24 (a bunny with interpolated shading normals in front of a backdrop, one tree), the light between the camera and the bunny, off the axis,
    translated along DIRECTION: interior + shadow boundary against the central difference by the recipe above.  The bunny shadows itself and the backdrop, so the
    boundary term's receiver carries shading normals that differ from the geometric ones -- the case in which the term's cosine factor (geometric, towards the
    camera) and the shading cosine inside f are not the same number.  Without the boundary term the error is at least twice the bound.
    Measured: floor 0.0345, AD seed distance 0.0517, e_all 0.0462 (bound 0.1294), e(sppse = 0) 0.6965."""
    sc, _ = load_scene("bunny_light", res=24, spp=4, sppe=4, sppse=4)
    tb = sc.tables(0)
    T = tb["tri_info"].detach().cpu().numpy()
    assert np.abs(T[:, 9:12] - T[:, 18:21]).max() > 0.1          # vertex normals that are not the face's
    pos = (0.5 * (cam_pos(tb) + T[:, 0:3].mean(axis=0)) + np.array([40.0, 60.0, 0.0])).astype(np.float64)
    dl = np.asarray(DIRECTION)
    fd, floor = _fd(lambda s, o: host_point_render(tb, o, pos + s * dl, nthreads=NT))
    bound = _ad_check("light, smooth normals", fd, floor, lambda o: host_point_render(tb, o, pos, mode=1, d_pos=dl, nthreads=NT)[1])
    e_no_se = rel_l2(host_point_render(tb, point_opts(AD_SPP, AD_SPPE, 0), pos, mode=1, d_pos=dl, nthreads=NT)[1], fd)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se >= 2.0 * bound, (e_no_se, bound)
