"""The distant (directional) light model of the PointLightIntegrator and the LightStageIntegrator (csrc/psdr_pointlight.h, csrc/psdr_lightstage.h with
LK = PSDR_LIGHT_DISTANT: Li = f(wi, wo = to_local(d / |d|)) V(p, d / |d|), no falloff, and the boundary term of the shadow outline under PARALLEL projection) on
the HOST: the product's PSDR_HD functions run slot by slot by tests/hostcheck/hostcheck_distantlight.cpp.  Pinned on closed forms written out in float64, on
the point light far away (the convention), on an analytic hard shadow, on float64 line integrals of the moving outline, on forward = reverse, on AD against
finite differences of its own renderC, and -- the stacks -- on the single-light harness plane by plane."""
import os
import subprocess

import numpy as np
import pytest

import enoki as ek
import psdr_cuda
from collocated_helpers import DIFFUSE, colloc_opts, host_film_samples, quad_xml, xml_scene
from colloc_microfacet_helpers import ROUGH_MAT, height_xml, microfacet_xml, normal_xml, scene, uv_quad_xml
from distantlight_helpers import (DISTANT, ENV_MESSAGE, HC_DEPS, POINT, distant_closed_form, host_light_render, host_light_rev, host_lights_render, host_lights_rev,
                                  interior_direction_derivative, outline_line_integral_distant, shadow_square_distant, unit)
from enoki.cuda_autodiff import Float32 as FloatD, Matrix4f as Matrix4fD, Vector3f as Vector3fD
from helpers import dot_tables, load_scene, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, san_program, write_tables_file
from lightstage_helpers import stack_opts
from pointlight_helpers import camera_rays64, hidden_occluder_xml, host_point_render, point_closed_form, point_opts
from psdr_cuda import _abi

RES, SPP = 16, 4
# directions TOWARDS the light, not unit length.  The quad's centre is the camera's target (0, 125, 0): these are the section-17 lights seen from there
DIRS = {"front": (150.0, 75.0, 500.0), "grazing": (0.0, 500.0, 60.0)}
HIDDEN_DIR = (1.0, 0.0, 1.0)          # hidden_occluder_xml: the shadow of the occluder [130, 170] x [105, 145] at z = 150 is [-20, 20] x [105, 145] on the receiver


def test_kinds_and_symbols():
    assert (_abi.LIGHT_POINT, _abi.LIGHT_DISTANT) == (0, 1)
    assert "psdr_scene_set_light" in _abi.HIP_SYMBOLS and "psdr_scene_set_lights" in _abi.HIP_SYMBOLS
    assert "DistantLightIntegrator" in psdr_cuda.__all__


# ---------------------------------------------------------------- 1. diffuse closed form
@pytest.mark.parametrize("direction", [(150.0, 75.0, 500.0), (0.0, 400.0, 300.0)])
@pytest.mark.parametrize("tilt", [0.0, 30.0, 70.0])
def test_diffuse_closed_form(tilt, direction):
    """A diffuse quad, no occluder: per pixel, the harness' renderC against rho / pi max(0, n . u) in float64 at the harness' own film samples.  Bound 1e-5
    relative per pixel (section 17's bound for the same arithmetic).  Measured worst pixel: 1.2e-7."""
    tb = xml_scene(quad_xml(DIFFUSE, tilt), RES, SPP).tables(0)
    o = point_opts(SPP, rng_offset=(3, 0, 0))
    img = host_light_render(tb, o, direction).astype(np.float64)
    val, hit, _ = distant_closed_form(tb, host_film_samples(tb, colloc_opts(SPP, rng_offset=(3, 0, 0))), direction)
    ref = val.reshape(RES * RES, SPP, 3).mean(axis=1)
    assert (ref > 0).any() and (ref == 0).any()
    assert (img[ref[:, 0] == 0] == 0).all()
    err = np.abs(img - ref)[ref[:, 0] > 0] / ref[ref[:, 0] > 0]
    print("distant light, diffuse closed form, tilt %g: worst per-pixel relative error %.2e" % (tilt, err.max()))
    assert err.max() <= 1e-5, err.max()


# ---------------------------------------------------------------- 2. general wo
def _gentle_normals():
    from colloc_microfacet_helpers import encode
    rng = np.random.default_rng(7)
    return encode(np.concatenate([rng.uniform(-0.15, 0.15, (16, 2)), np.ones((16, 1))], axis=1)).astype(np.float32)


_KIND_XML = {"plain": lambda: (microfacet_xml(0.3), dict(textured=True)), "normal": lambda: (normal_xml(0.3), dict(textured=True, normal=_gentle_normals())),
             "height": lambda: (height_xml(0.3, scale=2.0), dict(textured=True, height="random", scale=2.0))}


@pytest.mark.parametrize("light", sorted(DIRS))
@pytest.mark.parametrize("tilt", [0.0, 30.0, 70.0])
@pytest.mark.parametrize("kind", ["plain", "normal", "height"])
def test_general_wo_closed_form(kind, tilt, light):
    """MicrofacetBSDF types 2, 3 and 4 with wo = the light's direction: the harness' renderC of the tilted textured quad against the closed forms of DESIGN.md
    sections 14 - 16 in float64.  Where the closed form is zero the harness' pixel is EXACTLY zero.  Bound 2e-6 image rel-L2 (section 17's); the directions are
    section 17's lights seen from the quad's centre, gentle maps: the same clearance from the GGX peak and from wi'.z = 0."""
    xml, kw = _KIND_XML[kind]()
    tb = scene(uv_quad_xml(xml, tilt), RES, SPP, **kw).tables(0)
    o = point_opts(SPP, rng_offset=(5, 0, 0))
    img = host_light_render(tb, o, DIRS[light])
    val, hit, _ = distant_closed_form(tb, host_film_samples(tb, colloc_opts(SPP, rng_offset=(5, 0, 0))), DIRS[light], kind)
    ref = val.reshape(RES * RES, SPP, 3).mean(axis=1)
    dark = (val == 0).all(axis=1).reshape(RES * RES, SPP).all(axis=1)
    assert (img[dark] == 0).all()
    if not (ref > 0).any():
        return          # the light is behind the face: all of the image is exactly zero
    e = rel_l2(img, ref)
    print("distant, general wo %s tilt %g light %s: rel-L2 %.2e" % (kind, tilt, light, e))
    assert e <= 2e-6, e


@pytest.mark.parametrize("light", sorted(DIRS))
@pytest.mark.parametrize("tilt", [0.0, 30.0, 70.0])
def test_rough_conductor_general_wo(tilt, light):
    """RoughConductor against the BSDF evaluation of oracle/torch_oracle.py (fp64) at the harness' film samples with wo = the light's direction in the hit's
    frame, no falloff.  Bound 2e-6 image rel-L2 (section 17's)."""
    import torch
    import torch_oracle as to
    tb = xml_scene(quad_xml(ROUGH_MAT % ("m", 0.2), tilt), RES, SPP).tables(0)
    img = host_light_render(tb, point_opts(SPP, rng_offset=(5, 0, 0)), DIRS[light])
    tt = {k: (v.detach().cpu().double() if isinstance(v, torch.Tensor) and v.is_floating_point() else (v.detach().cpu() if isinstance(v, torch.Tensor) else v)) for k, v in tb.items()}
    sxy = torch.from_numpy(host_film_samples(tb, colloc_opts(SPP, rng_offset=(5, 0, 0))).astype(np.float64))
    org, d = to.primary_ray(tt, sxy[:, 0], sxy[:, 1], False)
    its = to.intersect(tt, org, d, torch.ones(len(sxy), dtype=torch.bool), "C")
    l = torch.from_numpy(unit(DIRS[light])).expand_as(its.p)
    wo = torch.stack([(l * its.sh_s).sum(-1), (l * its.sh_t).sum(-1), (l * its.sh_n).sum(-1)], dim=-1)
    f = to.bsdf_eval(tt, its, wo, False)
    val = torch.where(its.valid.unsqueeze(-1), f, torch.zeros_like(f))
    ref = val.reshape(RES * RES, SPP, 3).mean(dim=1).numpy()
    assert (img[(ref == 0).all(axis=1)] == 0).all()
    if (ref > 0).any():
        print("distant, rough conductor tilt %g light %s: rel-L2 %.2e" % (tilt, light, rel_l2(img, ref)))
        assert rel_l2(img, ref) <= 2e-6, rel_l2(img, ref)


# ---------------------------------------------------------------- 3. the convention, against the point light
def test_point_light_far_away_tends_to_the_distant_light():
    """The harness' point light at c + R u with intensity R^2 against the harness' distant light of direction u, R = 100 scene radii about the quad's centre c.
    delta(R): the per-pixel relative distance of the two float64 closed forms at the same film samples, computed here; the two images may differ by delta(R)
    plus twice section 17's closed-form bound (1e-5 per pixel).  Pins the sign of d, the missing 1 / r^2 and the irradiance normalisation; no precision claim.
    Measured: delta(R) 7.4e-3, distance of the images 7.4e-3."""
    tb = xml_scene(quad_xml(DIFFUSE, 30.0), RES, SPP).tables(0)
    T = tb["tri_info"].detach().cpu().numpy().astype(np.float64)
    c = np.array([0.0, 125.0, 0.0])
    verts = np.concatenate([T[:, 0:3], T[:, 0:3] + T[:, 3:6], T[:, 0:3] + T[:, 6:9]])
    R = 100.0 * np.linalg.norm(verts - c, axis=1).max()
    d = np.array(DIRS["front"])
    pL = c + R * unit(d)
    o = point_opts(SPP, rng_offset=(3, 0, 0))
    sxy = host_film_samples(tb, colloc_opts(SPP, rng_offset=(3, 0, 0)))
    mean = lambda v: v.reshape(RES * RES, SPP, 3).mean(axis=1)          # noqa: E731
    cf_d, cf_p = mean(distant_closed_form(tb, sxy, d)[0]), mean(point_closed_form(tb, sxy, pL)[0]) * R * R
    lit = cf_d[:, 0] > 0
    assert lit.any() and np.array_equal(lit, cf_p[:, 0] > 0)
    delta = (np.abs(cf_p - cf_d)[lit] / cf_d[lit]).max()
    img_d = host_light_render(tb, o, d).astype(np.float64)
    img_p = host_point_render(tb, o, pL).astype(np.float64) * R * R
    assert (img_d[~lit] == 0).all() and (img_p[~lit] == 0).all()
    dist = (np.abs(img_p - img_d)[lit] / cf_d[lit]).max()
    print("point light at %g scene radii against the distant light: delta(R) %.3e, distance of the harness images %.3e" % (100.0, delta, dist))
    assert delta < 0.1          # (the limit is near: a wrong sign or a kept falloff is off by far more)
    assert dist <= delta + 2e-5, (dist, delta)
    # ... and -d is a different light: the quad faces away from it
    assert (host_light_render(tb, o, -d) == 0).all()


# ---------------------------------------------------------------- 4. the scale of d
def test_scale_of_the_direction():
    """d and 4 d give the same image and the same table gradients bit for bit, and g_dir(4 d) = g_dir(d) / 4 exactly: powers of two commute with the
    normalisation.  All three terms on (cbox_occluder through its open front)."""
    res, spp, sppe, sppse = 16, 4, 4, 8
    tb = load_scene("cbox_occluder", res=res, spp=spp, sppe=sppe, sppse=sppse)[0].tables(0)
    d = np.array(CBOX_DIR, np.float32)
    o = point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    names = ["tri_info", "texels", "prim_edge", "sec_edge"]
    img1, g1, gd1 = host_light_rev(tb, o, d, adj, want=names)
    img4, g4, gd4 = host_light_rev(tb, o, 4.0 * d, adj, want=names)
    assert np.abs(img1).max() > 0 and np.array_equal(img1, img4)
    assert np.array_equal(host_light_render(tb, o, d), host_light_render(tb, o, 4.0 * d))
    for n in names:
        assert np.abs(g1[n]).max() > 0 and np.array_equal(g1[n], g4[n]), n
    assert np.abs(gd1).max() > 0 and np.array_equal(gd4 * np.float32(4.0), gd1), (gd1, gd4)


# ---------------------------------------------------------------- 5. hard shadow
def test_hard_shadow():
    """hidden_occluder_xml under d = (1, 0, 1): the shadow of the occluder (outside the camera's view) is the square [-20, 20] x [105, 145] on the receiver.
    Pixels whose footprint lies wholly inside it are exactly 0, pixels wholly outside equal the unoccluded closed form (1e-5 per pixel); the pixels the outline
    cuts are the only ones left out (under 15 % of the receiver's, asserted).  Measured: 16 pixels inside, 20 of 528 cut (3.8 %)."""
    res = 32
    tb = xml_scene(hidden_occluder_xml(), res, SPP).tables(0)
    o = point_opts(SPP, rng_offset=(9, 0, 0))
    img = host_light_render(tb, o, HIDDEN_DIR).astype(np.float64)
    sxy = host_film_samples(tb, colloc_opts(SPP, rng_offset=(9, 0, 0)))
    val, hit, _ = distant_closed_form(tb, sxy, HIDDEN_DIR, rows=(0, 1))          # (rows 0, 1: the receiver; the occluder is not in view: asserted below)
    vall, hitall, _ = distant_closed_form(tb, sxy, HIDDEN_DIR)
    assert np.array_equal(hit, hitall) and np.array_equal(val, vall)
    ref = val.reshape(res * res, SPP, 3).mean(axis=1)
    gx, gy = np.meshgrid(np.arange(res + 1) / res, np.arange(res + 1) / res)
    org, dd = camera_rays64(tb, np.stack([gx.ravel(), gy.ravel()], axis=1))
    p = org + dd * (-org[2] / dd[:, 2])[:, None]
    px, py = p[:, 0].reshape(res + 1, res + 1), p[:, 1].reshape(res + 1, res + 1)
    corners = lambda a: np.stack([a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]], axis=-1).reshape(res * res, 4)          # noqa: E731
    cx, cy = corners(px), corners(py)
    lo, hi = shadow_square_distant(HIDDEN_DIR, (130.0, 105.0), (170.0, 145.0), 150.0)
    assert np.allclose(lo, (-20.0, 105.0)) and np.allclose(hi, (20.0, 145.0))
    m = 1e-3          # (ShadowEpsilon-sized margin about the outline)
    inside = ((cx > lo[0] + m) & (cx < hi[0] - m) & (cy > lo[1] + m) & (cy < hi[1] - m)).all(axis=1)
    outside = (cx.max(1) < lo[0] - m) | (cx.min(1) > hi[0] + m) | (cy.max(1) < lo[1] - m) | (cy.min(1) > hi[1] + m)
    on_receiver = hit.reshape(res * res, SPP).any(axis=1)
    cut = on_receiver & ~inside & ~outside
    share = cut.sum() / on_receiver.sum()
    print("distant hard shadow: %d pixels inside, %d cut by the outline of %d on the receiver (%.1f %%)" % (inside.sum(), cut.sum(), on_receiver.sum(), 100 * share))
    assert inside.sum() >= 9 and share < 0.15, (inside.sum(), share)
    assert (img[inside] == 0).all()
    lit = outside & (ref[:, 0] > 0)
    err = np.abs(img - ref)[lit] / ref[lit]
    assert lit.any() and err.max() <= 1e-5, err.max()
    assert (img[outside & (ref[:, 0] == 0)] == 0).all()


# ---------------------------------------------------------------- 6. the independent boundary reference
AD_SPP, AD_SPPE, AD_SPPSE, FD_SPP, NT = 1024, 4096, 4096, 16384, 8


def _hidden(spp, sppe, sppse, along=None):
    """hidden_occluder_xml at res 24; along: the occluder translated by along * P (returns P), otherwise at rest"""
    P = [None]

    def prep(sc):
        sc.opts.sppse = sppse
        if along is not None:
            P[0] = FloatD(0.)
            ek.set_requires_gradient(P[0])
            sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(along)) * P[0]))
    return xml_scene(hidden_occluder_xml(), 24, spp, sppe, prepare=prep), P[0]


def _against_reference(label, ref, ad_of):
    """rel-L2 of the AD derivative image against the float64 reference; bound 1.5 x the rel-L2 distance of two AD seeds at the test's sample counts; also the
    error with sppse = 0, which must be the whole signal (> 0.9): the occluder is hidden, only its shadow is seen"""
    ads = [ad_of(point_opts(AD_SPP, AD_SPPE, AD_SPPSE, rng_offset=(77 * seed, 55 * seed, 33 * seed))).astype(np.float64) for seed in (0, 1)]
    dist, e = rel_l2(ads[0], ads[1]), rel_l2(ads[0], ref)
    print("distant light, line-integral reference, %s: AD seed distance %.4f, error %.4f (bound %.4f)" % (label, dist, e, 1.5 * dist))
    assert np.linalg.norm(ref) > 0
    assert e <= 1.5 * dist, (label, e, 1.5 * dist)
    return ads[0]


LO, HI = shadow_square_distant(HIDDEN_DIR, (130.0, 105.0), (170.0, 145.0), 150.0)


def test_boundary_reference_occluder_translation_parallel():
    """(a) The occluder translated parallel to the receiver, along (1, 0.5, 0): under parallel projection the outline moves WITH the occluder (k = 1; the point
    light's k = L.z / (L.z - 150) is a different number), and the derivative image is minus the line integral of the unoccluded closed form times the film's
    area density along the outline (distantlight_helpers.outline_line_integral_distant: float64 numpy).  Pins the Jacobian sinphi / sinphi2 alone.
    Measured: AD seed distance 0.0073, error 0.0060 (bound 0.0109); with sppse = 0: 1.0000."""
    along = (1.0, 0.5, 0.0)
    sc, P = _hidden(AD_SPP, AD_SPPE, AD_SPPSE, along)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    ref = outline_line_integral_distant(tb, HIDDEN_DIR, LO, HI, np.asarray(along[:2]))
    _against_reference("occluder, parallel", ref, lambda o: host_light_render(tb, o, HIDDEN_DIR, mode=1, tangent_sets=[tan], nthreads=NT)[1][0])
    e_no_se = rel_l2(host_light_render(tb, point_opts(AD_SPP, AD_SPPE, 0), HIDDEN_DIR, mode=1, tangent_sets=[tan], nthreads=NT)[1][0], ref)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se > 0.9, e_no_se


def test_boundary_reference_occluder_translation_along_the_normal():
    """(b) The occluder translated along the receiver's normal (0, 0, 1): the outline moves by -(u_xy / u_z) dz = (-1, 0) dz -- the motion term of the ray's
    ORIGIN (the edge row) under a fixed direction, which the point light does not have.
    Measured: AD seed distance 0.0069, error 0.0055 (bound 0.0104); with sppse = 0: 1.0000."""
    along = (0.0, 0.0, 1.0)
    sc, P = _hidden(AD_SPP, AD_SPPE, AD_SPPSE, along)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    u = unit(HIDDEN_DIR)
    ref = outline_line_integral_distant(tb, HIDDEN_DIR, LO, HI, -u[:2] / u[2])
    _against_reference("occluder, normal", ref, lambda o: host_light_render(tb, o, HIDDEN_DIR, mode=1, tangent_sets=[tan], nthreads=NT)[1][0])
    e_no_se = rel_l2(host_light_render(tb, point_opts(AD_SPP, AD_SPPE, 0), HIDDEN_DIR, mode=1, tangent_sets=[tan], nthreads=NT)[1][0], ref)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se > 0.9, e_no_se


def test_boundary_reference_direction_tangent():
    """(c) A tangent t on d (with a radial part, which must not matter): the outline moves by -z_occ d(d_xy / d_z)[t], and the lit part changes by
    rho / pi n . du (distantlight_helpers.interior_direction_derivative).  Interior + boundary of the harness against their sum.
    Measured: AD seed distance 0.0080, error 0.0067 (bound 0.0121); with sppse = 0: 0.9890."""
    tb = _hidden(AD_SPP, AD_SPPE, AD_SPPSE)[0].tables(0)
    d, t = np.asarray(HIDDEN_DIR), np.array([0.3, 0.5, -0.2])
    vel = -150.0 * (t[:2] * d[2] - d[:2] * t[2]) / d[2] ** 2
    ref = outline_line_integral_distant(tb, d, LO, HI, vel) + interior_direction_derivative(tb, d, t, LO, HI, (-80.0, 45.0), (80.0, 205.0))
    _against_reference("direction", ref, lambda o: host_light_render(tb, o, d, mode=1, d_v=t[None, :], nthreads=NT)[1][0])
    e_no_se = rel_l2(host_light_render(tb, point_opts(AD_SPP, AD_SPPE, 0), d, mode=1, d_v=t[None, :], nthreads=NT)[1][0], ref)
    print("   without the shadow boundary: %.4f" % e_no_se)
    assert e_no_se > 0.9, e_no_se


# ---------------------------------------------------------------- 7. AD identities
CBOX_DIR = (0.2, 0.5, 1.0)          # cbox_occluder is lit through its open front (+z), from above: the occluder's shadow falls on the back wall


def _scene_and_direction(name, res, spp, sppe, sppse):
    if name == "quad":
        from pointlight_helpers import floor_occluder_xml

        def prep(sc):
            sc.opts.sppse = sppse
        return xml_scene(floor_occluder_xml(), res, spp, sppe, prepare=prep), np.array((60.0, 55.0, 600.0), np.float32)
    sc, _ = load_scene(name, res=res, spp=spp, sppe=sppe, sppse=sppse)
    return sc, np.array({"cbox_occluder": CBOX_DIR, "bunny_light": (0.4, 0.6, -1.0)}[name], np.float32)


@pytest.mark.parametrize("name", ["quad", "cbox_occluder", "bunny_light"])
def test_forward_equals_reverse(name):
    """<adj, J t> = <J^T adj, t> per table -- triangle rows, texels, the camera pose, primary-edge rows, secondary-edge rows -- and for the direction, with a
    tangential and a radial tangent: |lhs - rhs| <= 1e-4 * scale (scale = sum |adj x dimg|).  The radial tangent's column and its inner product with g_dir are
    both zero to that scale: the gradient is tangential by construction."""
    res, spp, sppe, sppse = 16, 4, 4, 8
    sc, d = _scene_and_direction(name, res, spp, sppe, sppse)
    tb = sc.tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    u = unit(d)
    t_tan = np.cross(u, (0.3, -0.2, 0.4))
    scale_dir = None
    for n in ("tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge", "direction", "radial"):
        table = n not in ("direction", "radial")
        tan = random_tangents(tb, [n], seed=1) if table else {}
        d_v = None if table else (t_tan if n == "direction" else 0.7 * np.asarray(d, np.float64)).astype(np.float32)[None, :]
        img, dimg = host_light_render(tb, o, d, mode=1, tangent_sets=[tan], d_v=d_v)
        img_r, grads, g_dir = host_light_rev(tb, o, d, adj, want=[n] if table else [], light=not table)
        assert rel_l2(img_r, img) < 1e-6
        lhs = float((adj.astype(np.float64) * dimg[0]).sum())
        rhs = dot_tables(grads, tan) if table else float(g_dir.astype(np.float64) @ d_v[0])
        scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
        if n == "direction":
            scale_dir = scale
        if n == "radial":
            assert abs(lhs) <= 1e-4 * scale_dir and abs(rhs) <= 1e-4 * scale_dir, (lhs, rhs, scale_dir)
            continue
        # (Lambertian planes under a distant light look the same from every camera, and the primary edges move with their own table: that column is zero)
        assert scale > 0 or (name != "bunny_light" and n == "cam_to_world"), n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
    # the shadow boundary reaches the secondary-edge rows, the receiver's triangle rows and the direction
    o_se = point_opts(spp, 0, sppse, rng_offset=(2, 3, 4), spp_range=(0, 0))
    _, g, g_dir = host_light_rev(tb, o_se, d, adj, want=["sec_edge", "tri_info"])
    assert np.abs(g["sec_edge"]).sum() > 0 and np.abs(g["tri_info"]).sum() > 0 and np.abs(g_dir).sum() > 0


def test_k3_equals_three_k1_launches():
    """forward mode with K = 3 gives the columns of three K = 1 runs, all three terms on: a geometry set, a texel set and the direction alone.  1e-6 (section 17's;
    1e-5 on the texel column, whose K = 1 run takes the on-surface form of the hit, as there)."""
    tb = load_scene("cbox_occluder", res=16, spp=4, sppe=4, sppse=8)[0].tables(0)
    o = point_opts(4, 4, 8, rng_offset=(2, 3, 4))
    sets = [random_tangents(tb, ["tri_info", "prim_edge", "sec_edge"], seed=1), random_tangents(tb, ["texels"], seed=2), {}]
    d_v = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.3, -0.2, 0.4]], np.float32)
    img3, d3 = host_light_render(tb, o, CBOX_DIR, mode=1, tangent_sets=sets, d_v=d_v)
    for k in range(3):
        img1, d1 = host_light_render(tb, o, CBOX_DIR, mode=1, tangent_sets=[sets[k]], d_v=d_v[k:k + 1] if k == 2 else None)
        assert np.abs(d1).max() > 0
        assert rel_l2(img3, img1) < 1e-6 and rel_l2(d3[k], d1[0]) < (1e-5 if k == 1 else 1e-6), (k, rel_l2(img3, img1), rel_l2(d3[k], d1[0]))


def _rotated(d, axis, angle):
    """Rodrigues: d turned about the unit axis by angle (float64)"""
    d, a = np.asarray(d, np.float64), unit(axis)
    return d * np.cos(angle) + np.cross(a, d) * np.sin(angle) + a * (a @ d) * (1.0 - np.cos(angle))


def _fd(render, step=1.0):
    """central difference from two seeds: (mean, distance of the two relative to it)"""
    fds = []
    for seed in (0, 1):
        im = [render(s, point_opts(FD_SPP, rng_offset=(1000 * seed, 0, 0))).astype(np.float64) for s in (+step, -step)]
        fds.append((im[0] - im[1]) / (2.0 * step))
    return (fds[0] + fds[1]) / 2.0, rel_l2(fds[0], fds[1])


def _ad_check(label, fd, floor, ad_of):
    """the section-12 recipe: e_all <= 1.5 (FD floor + AD seed distance); returns the bound"""
    ads = [ad_of(point_opts(AD_SPP, AD_SPPE, AD_SPPSE, rng_offset=(77 * seed, 55 * seed, 33 * seed))).astype(np.float64) for seed in (0, 1)]
    ad_dist = float(np.linalg.norm(ads[0] - ads[1]) / np.linalg.norm(fd))
    e_all, bound = rel_l2(ads[0], fd), 1.5 * (floor + ad_dist)
    print("distant light AD vs FD, %s: floor %.4f, AD seed distance %.4f, e_all %.4f (bound %.4f)" % (label, floor, ad_dist, e_all, bound))
    assert np.linalg.norm(fd) > 0
    assert e_all <= bound, (label, e_all, bound)
    return bound


ALONG = (1.0, 0.5, 0.0)
# The direction turned about y.  The central difference takes +-0.004 rad: the outlines that move lie up to 300 units behind the edges that cast them, so they
# move by up to 1.2 units either way -- what the unit translation step of section 17's recipe moves them by, well inside a pixel's 8 units at res 24.  (A larger
# step smears the thin derivative of an outline over the pixels it crosses, which AD does not: measured at 0.02 rad, e_all 0.58 on cbox_occluder.)
AXIS, ROT_STEP = (0.0, 1.0, 0.0), 0.004


def _cbox_occluder(spp, sppe=0, sppse=0, offset=None):
    """cbox_occluder at res 24, Mesh[1] (the occluder) translated along ALONG: by P (offset None) or by a number"""
    from psdr_cuda.fixtures import scene_path
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_occluder"), False)
    sc.opts.width = sc.opts.height = 24
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    P = None
    if offset is None:
        P = FloatD(0.)
        ek.set_requires_gradient(P)
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(ALONG)) * P))
    else:
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(ALONG)) * FloatD(float(offset))))
    sc.configure()
    return sc, P


def test_ad_vs_fd_occluder_translation():
    """cbox_occluder, res 24, the occluder translated, lit through the open front: AD with all three terms on against the central difference of the harness' own
    renderC, by section 12's recipe and bound formula.
    Measured: floor 0.0245, AD seed distance 0.0226, e_all 0.0292 (bound 0.0707)."""
    fd, floor = _fd(lambda s, o: host_light_render(_cbox_occluder(FD_SPP, offset=s)[0].tables(0), o, CBOX_DIR, nthreads=NT))
    sc, P = _cbox_occluder(AD_SPP, AD_SPPE, AD_SPPSE)
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    _ad_check("occluder", fd, floor, lambda o: host_light_render(tb, o, CBOX_DIR, mode=1, tangent_sets=[tan], nthreads=NT)[1][0])


def test_ad_vs_fd_direction_rotation():
    """the same scene, the DIRECTION turned about y: interior (wo alone) + shadow boundary (every outline in the room moves) against the central difference.
    Measured: floor 0.0427, AD seed distance 0.0322, e_all 0.0426 (bound 0.1124)."""
    tb = _cbox_occluder(FD_SPP, offset=0.0)[0].tables(0)
    fd, floor = _fd(lambda s, o: host_light_render(tb, o, _rotated(CBOX_DIR, AXIS, s), nthreads=NT), ROT_STEP)
    tba = _cbox_occluder(AD_SPP, AD_SPPE, AD_SPPSE, offset=0.0)[0].tables(0)
    t = np.cross(unit(AXIS), CBOX_DIR)[None, :]
    _ad_check("direction", fd, floor, lambda o: host_light_render(tba, o, CBOX_DIR, mode=1, d_v=t, nthreads=NT)[1][0])


def test_ad_vs_fd_direction_rotation_smooth_normals():
    """bunny_light at res 24 (a bunny with interpolated shading normals in front of a backdrop: it shadows itself and the backdrop), the direction turned about y.
    Measured: floor 0.0240, AD seed distance 0.0654, e_all 0.0548 (bound 0.1341)."""
    tb = load_scene("bunny_light", res=24, spp=4, sppe=4, sppse=4)[0].tables(0)
    d = (0.4, 0.6, -1.0)          # (the camera of bunny_light looks along +z)
    fd, floor = _fd(lambda s, o: host_light_render(tb, o, _rotated(d, AXIS, s), nthreads=NT), ROT_STEP)
    t = np.cross(unit(AXIS), d)[None, :]
    _ad_check("direction, smooth normals", fd, floor, lambda o: host_light_render(tb, o, d, mode=1, d_v=t, nthreads=NT)[1][0])


def test_ad_vs_fd_roughness_texel():
    """A MicrofacetBSDF quad with 4 x 4 maps, tilted 30 degrees, under the front direction: d image / d (one roughness texel) in forward mode against the central
    difference (step 0.02) of the harness' own renderC; reverse mode reaches the same texel.
    Measured: floor 0.0030, AD seed distance 0.0139, e_all 0.0108 (bound 0.0254)."""
    import torch
    from colloc_microfacet_helpers import record
    d, eps = DIRS["front"], 0.02
    tb = scene(uv_quad_xml(microfacet_xml(0.3), 30.0), 24, 4, textured=True).tables(0)
    idx = record(tb, "plain")[1]["roughness"] + 5          # an inner texel of the 4 x 4 map
    onehot = torch.zeros(tb["texels"].numel())
    onehot[idx] = 1.0
    ts = [{"texels": onehot.reshape(tb["texels"].shape)}]

    def moved(s):
        t = dict(tb)
        t["texels"] = tb["texels"].detach().clone()
        t["texels"].reshape(-1)[idx] += s
        return t
    fd, floor = _fd(lambda s, o: host_light_render(moved(s), o, d, nthreads=NT), eps)
    _ad_check("roughness texel", fd, floor, lambda o: host_light_render(tb, o, d, mode=1, tangent_sets=ts, nthreads=NT)[1][0])
    adj = np.random.default_rng(8).random((24 * 24, 3)).astype(np.float32)
    o = point_opts(16, rng_offset=(4, 0, 0))
    col = host_light_render(tb, o, d, mode=1, tangent_sets=ts)[1][0].astype(np.float64)
    _, g, _ = host_light_rev(tb, o, d, adj, want=["texels"], light=False)
    lhs, scale = float((adj * col).sum()), float(np.abs(adj * col).sum())
    assert scale > 0 and abs(lhs - float(g["texels"].reshape(-1)[idx])) <= 1e-4 * scale, (lhs, g["texels"].reshape(-1)[idx], scale)


# ---------------------------------------------------------------- 8. stacks
# cbox_occluder: directions through the open front, and section 18's point lights inside the room
STACK_DIRS = np.array([(0.2, 0.5, 1.0), (-0.6, 0.3, 1.0), (0.2, 0.5, 1.0), (0.5, -0.2, 2.0), (0.0, 1.5, 1.0), (-0.3, 0.8, 0.6)], np.float32)
STACK_POINTS = np.array([(30.3, 181.7, 50.9), (-60.7, 170.3, 120.9), (30.3, 181.7, 50.9), (10.3, -50.7, 40.9), (10.3, 97.3, 30.9), (10.3, 120.7, -70.9)], np.float32)


def stack_of(L, mixed):
    """(kinds [L], vectors [L, 3]): all distant, or alternating distant / point starting with a distant light"""
    kinds = np.array([DISTANT if (not mixed or l % 2 == 0) else POINT for l in range(L)], np.int32)
    return kinds, np.where((kinds == DISTANT)[:, None], STACK_DIRS[:L], STACK_POINTS[:L]).astype(np.float32)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3, 6])
def test_stack_planes_are_the_single_light_images(L, mixed):
    """renderC and forward mode (K = 1 and 3, all three terms, table tangents and light tangents) of the stack harness: every plane against the single-light
    harness of that light's kind at section 18's 1e-6; one light's tangent leaves every other light's derivative plane exactly 0."""
    res, spp, sppe, sppse = 12, 2, 2, 4
    tb = load_scene("cbox_occluder", res=res, spp=spp, sppe=sppe, sppse=sppse)[0].tables(0)
    kinds, v = stack_of(L, mixed)
    o, po = stack_opts(spp, sppe, sppse, rng_offset=(2, 3, 4)), point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    img = host_lights_render(tb, o, kinds, v)
    singles = [host_light_render(tb, po, v[l], kind=kinds[l]) for l in range(L)]
    for l in range(L):
        assert np.abs(singles[l]).max() > 0 or (kinds[l] == POINT and l == 3)          # (the point light below the floor lights nothing)
        assert np.abs(singles[l]).max() == 0 and np.abs(img[l]).max() == 0 or rel_l2(img[l], singles[l]) < 1e-6, (l, rel_l2(img[l], singles[l]))
    rng = np.random.default_rng(11)
    for K in (1, 3):
        sets = [random_tangents(tb, ["tri_info", "prim_edge", "sec_edge", "texels"], seed=1 + k) for k in range(K)]
        d_v = (rng.random((K, L, 3)) - 0.5).astype(np.float32)
        img1, dimg = host_lights_render(tb, o, kinds, v, mode=1, tangent_sets=sets, d_v=d_v)
        for l in range(L):
            s_img, s_d = host_light_render(tb, po, v[l], kind=kinds[l], mode=1, tangent_sets=sets, d_v=d_v[:, l])
            for k in range(K):
                if np.abs(s_d[k]).max() == 0:
                    assert np.abs(dimg[k, l]).max() == 0
                else:
                    assert rel_l2(dimg[k, l], s_d[k]) < 1e-6, (K, k, l, rel_l2(dimg[k, l], s_d[k]))
    if L > 1:
        d_v = np.zeros((1, L, 3), np.float32)
        d_v[0, 1] = (0.3, -0.2, 0.4)
        _, dimg = host_lights_render(tb, o, kinds, v, mode=1, tangent_sets=[{}], d_v=d_v)
        assert np.abs(dimg[0, 1]).max() > 0
        for l in range(L):
            assert l == 1 or (dimg[0, l] == 0).all(), l


@pytest.mark.parametrize("mixed", [False, True])
def test_stack_forward_equals_reverse_and_sums_the_single_lights(mixed):
    """L = 6: <A, J t> = <J^T A, t> per table and for the lights' vectors, and the stack's table gradients against the sum of the single-light reverse runs
    (1e-4, section 18's), its g_v rows against theirs."""
    L, res, spp, sppe, sppse = 6, 12, 2, 2, 4
    tb = load_scene("cbox_occluder", res=res, spp=spp, sppe=sppe, sppse=sppse)[0].tables(0)
    kinds, v = stack_of(L, mixed)
    o, po = stack_opts(spp, sppe, sppse, rng_offset=(2, 3, 4)), point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    A = np.random.default_rng(5).random((L, res * res, 3)).astype(np.float32)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge"]
    img_r, grads, g_v = host_lights_rev(tb, o, kinds, v, A, want=names)
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = host_lights_render(tb, o, kinds, v, mode=1, tangent_sets=[tan])
        assert rel_l2(img_r, img) < 1e-6
        lhs, rhs = float((A.astype(np.float64) * dimg[0]).sum()), dot_tables(grads, tan)
        scale = float(np.abs(A.astype(np.float64) * dimg[0]).sum())
        # (all distant: Lambertian planes look the same from every camera -- the camera's column is zero; the mixed stack's point lights fill it)
        assert scale > 0 or (not mixed and n == "cam_to_world"), n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
    d_v = (np.random.default_rng(6).random((1, L, 3)) - 0.5).astype(np.float32)
    _, dimg = host_lights_render(tb, o, kinds, v, mode=1, tangent_sets=[{}], d_v=d_v)
    lhs, rhs = float((A.astype(np.float64) * dimg[0]).sum()), float((g_v.astype(np.float64) * d_v[0]).sum())
    scale = float(np.abs(A.astype(np.float64) * dimg[0]).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
    total = {n: np.zeros_like(grads[n]) for n in grads}
    for l in range(L):
        _, g1, gv1 = host_light_rev(tb, po, v[l], A[l], kind=kinds[l], want=names)
        for n in g1:
            total[n] += g1[n]
        if np.abs(gv1).max() > 0:
            assert rel_l2(g_v[l], gv1) < 1e-4, (l, g_v[l], gv1)
        else:
            assert (g_v[l] == 0).all()
    for n in total:
        if not mixed and n == "cam_to_world":
            assert not np.any(total[n]) and not np.any(grads[n])
            continue
        assert np.abs(total[n]).max() > 0 and rel_l2(grads[n], total[n]) < 1e-4, (n, rel_l2(grads[n], total[n]))


# ---------------------------------------------------------------- 9. the surface (what needs no GPU) and the sanitizers
def test_constructor_checks():
    integ = psdr_cuda.DistantLightIntegrator((1.0, 2.0, 3.0), (0.5, 1.0, 2.0))
    assert isinstance(integ, psdr_cuda.PointLightIntegrator) and integ._kind == _abi.INTEGRATOR_POINT and integ._light_kind == _abi.LIGHT_DISTANT
    assert integ.m_direction.numpy().tolist() == [[1.0, 2.0, 3.0]] and integ.m_intensity.numpy().tolist() == [[0.5, 1.0, 2.0]]
    assert psdr_cuda.DistantLightIntegrator(Vector3fD([4.0, 5.0, 6.0])).m_intensity.numpy().tolist() == [[1.0, 1.0, 1.0]]
    integ.m_direction = Vector3fD([0.0, 0.0, 2.0])
    assert integ.m_position.numpy().tolist() == [[0.0, 0.0, 2.0]]          # the vector the inherited code reads IS m_direction
    for bad in ((1.0, 2.0), (1.0, 2.0, float("nan")), 3.0, (0.0, 0.0, 0.0), Vector3fD([0.0, 0.0, 0.0]), (float("inf"), 0.0, 1.0)):
        with pytest.raises(Exception, match="direction"):
            psdr_cuda.DistantLightIntegrator(bad)
    with pytest.raises(Exception):
        psdr_cuda.DistantLightIntegrator((0.0, 0.0, 1.0), (1.0, 2.0))
    assert psdr_cuda.PointLightIntegrator((0.0, 0.0, 0.0))._light_kind == _abi.LIGHT_POINT          # a position may be the origin
    stage = psdr_cuda.LightStageIntegrator(STACK_DIRS[:3], 2.0, distant=[True, False, True])
    assert stage.distant == [True, False, True] and psdr_cuda.LightStageIntegrator(STACK_DIRS[:3]).distant is None
    with pytest.raises(Exception, match="distant"):
        psdr_cuda.LightStageIntegrator(STACK_DIRS[:3], distant=[True, False])
    with pytest.raises(Exception, match="all zero"):
        psdr_cuda.LightStageIntegrator([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], distant=[True, False])
    psdr_cuda.LightStageIntegrator([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], distant=[False, True])          # a POSITION may be the origin
    with pytest.raises(Exception):
        psdr_cuda.LightStageIntegrator([[0.0, float("nan"), 0.0]], distant=[True])


def test_environment_map_refusal_text():
    """a distant light cannot reach a scene inside an environment map's bounding mesh: the integrators raise, before the native call, the text the native render
    calls return (tests/test_distantlight_gpu.py exercises both); here: the two texts are one"""
    assert ENV_MESSAGE in _abi.DISTANT_IN_ENV
    csrc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(psdr_cuda.__file__))), "csrc", "psdr_hip.hip")).read()
    assert '"' + _abi.DISTANT_IN_ENV + '"' in csrc


@pytest.mark.parametrize("L", [1, 6])
def test_host_functions_run_clean_under_the_sanitizers(tmp_path, L):
    """tests/hostcheck/distantlight_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_distantlight.cpp, built with
    -fsanitize=address,undefined for the host (hostlibs.san_program): render, forward and reverse with all three terms -- the distant model alone (L = 1) and a
    mixed stack of six, plus light 0 through the single-light functions; it must end clean and report what the library reports."""
    exe = san_program("distantlight_san", HC_DEPS)
    res, spp, sppe, sppse = 8, 2, 2, 8
    tb = load_scene("cbox_occluder", res=res, spp=spp, sppe=sppe, sppse=sppse)[0].tables(0)
    o = stack_opts(spp, sppe, sppse, rng_offset=(1, 2, 3))
    names = ("tri_info", "texels", "prim_edge", "sec_edge")
    tan = random_tangents(tb, list(names), seed=3)
    kinds, v = stack_of(L, L > 1)
    adj = np.random.default_rng(4).random((L, res * res, 3)).astype(np.float32)
    d_v = (np.random.default_rng(5).random((1, L, 3)) - 0.5).astype(np.float32)
    tbc, desc, keep = cpu_desc(tb)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in names], adj, v, d_v, kinds)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path, str(L)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_lights_render(tb, o, kinds, v, mode=1, tangent_sets=[tan], d_v=d_v, nthreads=2)
    _, grads, g_v = host_lights_rev(tb, o, kinds, v, adj, want=list(names))
    one, done = host_light_render(tb, o, v[0], kind=kinds[0], mode=1, tangent_sets=[tan], d_v=d_v[:, 0], nthreads=2)
    _, _, g_v1 = host_light_rev(tb, o, v[0], adj[0], kind=kinds[0], want=list(names))
    want = [np.abs(host_lights_render(tb, o, kinds, v, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + \
           [np.abs(grads[n].astype(np.float64)).sum() for n in names] + [np.abs(g_v.astype(np.float64)).sum()] + \
           [np.abs(one.astype(np.float64)).sum(), np.abs(done.astype(np.float64)).sum(), np.abs(g_v1.astype(np.float64)).sum()]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
