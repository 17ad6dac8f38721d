"""MicrofacetBSDF with a height map (csrc/psdr_colloc_microfacet.h, DESIGN.md section 16: record type PSDR_BSDF_MICROFACET_HEIGHT, evaluated by the
CollocatedIntegrator) on the HOST: the product's PSDR_HD functions run slot by slot by tests/hostcheck/hostcheck_collocated.cpp.  The model is build-defined and
the oracle is not extended, so it is pinned on its closed form written out in float64 (height gradient and surface-gradient basis included), on the type-3
record that a ramp equals, on its limits against the record without a map, on its degenerate inputs, on forward = reverse and on AD against central differences
of the harness' own renderC."""
import os
import subprocess

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import HC_DEPS, _HEAD, colloc_opts, host_colloc_render, host_colloc_rev, host_film_samples, xml_scene
from colloc_microfacet_helpers import (KINDS, MESSAGE, NOT_BOTH, ONE_CELL, SIGMA, bunny_xml, closed_form_image, encode, height_xml, map_words, microfacet_xml, mixed_xml,
                                       named_scene, normal_xml, perturbed_normal64, quad, record, scene, uv_quad_xml)
from enoki.cuda_autodiff import Float32 as FloatD
from helpers import dot_tables, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, san_program, write_tables_file
from psdr_cuda import _abi

RES, SPP = 16, 4
TILTS, ROUGHNESS = (0.0, 30.0, 70.0), (0.3, 0.6)
NAMES = ["texels", "tri_info", "cam_to_world", "prim_edge"]
MIXED_IDS = ("d", "c", "m", "n", "h")          # the quads of mixed_xml: record types 0 .. 4


# ---------------------------------------------------------------- 1. closed form
MEASURED_CLOSED_FORM = 6.37e-7          # the largest of the cases below, measured on the host (70 degrees, 4 x 4 map, r = 0.3, UVs turned by 37 degrees)


@pytest.mark.parametrize("case", ["2x2", "4x4"])
@pytest.mark.parametrize("uv", [None, "rot37", "mirror"], ids=["uv", "uv-rot37", "uv-mirror"])
@pytest.mark.parametrize("r", ROUGHNESS)
@pytest.mark.parametrize("tilt", TILTS)
def test_closed_form(tilt, r, uv, case):
    """The tilted quad: the harness' renderC against section 16 written out in float64 numpy at the harness' own film samples -- (h_u, h_v) from the four texels
    of the hit's cell, p_u and p_v from the triangle's edges and UVs, their parts in the shading plane, the dual basis, n', the lobes at the angle between the
    view direction and n'.  Maps: 2 x 2 (one cell: the slopes vary through the cross term alone) and 4 x 4 random in [0, 1], sigma = 6 (slopes below about 0.5).
    UVs: as the mesh has them, turned 37 degrees in the plane, and mirrored (J < 0).
    Bound: image rel-L2 <= max(2e-6, 4 x the largest value measured here) = 2.55e-6.
    Measured (rel-L2): 6.7e-8 .. 4.1e-7 at 0 degrees, 1.1e-7 .. 1.2e-7 at 30, 2.5e-7 .. 6.37e-7 at 70; the 2 x 2 and the 4 x 4 map alike (slopes below 0.5 keep wi'.z
    away from zero, unlike the 50-degree normals of section 15's 4 x 4 map)."""
    if case == "2x2":
        sc = scene(uv_quad_xml(height_xml(r), tilt), RES, SPP, uv=uv, height=ONE_CELL, map_res=(2, 2))
    else:
        sc = scene(uv_quad_xml(height_xml(r), tilt), RES, SPP, uv=uv, height="random")
    tb = sc.tables(0)
    assert tb["material_mask"] == 1 << _abi.BSDF_MICROFACET_HEIGHT
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(tb, o)
    ref = closed_form_image(tb, host_film_samples(tb, o), SPP, "height")
    assert (ref > 0).any() and (ref == 0).any()          # the quad and the background are both seen
    e = rel_l2(img, ref)
    print("height map closed form tilt %g r %g %s %s: rel-L2 %.2e" % (tilt, r, uv, case, e))
    assert e <= max(2e-6, 4 * MEASURED_CLOSED_FORM), e


def test_closed_form_tells_the_map():
    """the closed form itself tells the maps apart: the 4 x 4 image differs from the flat one by more than 1e-2"""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    a = host_colloc_render(scene(uv_quad_xml(height_xml(0.3), 30.0), RES, SPP, height="random").tables(0), o)
    b = host_colloc_render(scene(uv_quad_xml(height_xml(0.3), 30.0), RES, SPP).tables(0), o)
    assert rel_l2(a, b) > 1e-2


# ---------------------------------------------------------------- 2. against existing code: a ramp is a constant normal texel
@pytest.mark.parametrize("axis", ["u", "v"])
@pytest.mark.parametrize("tilt", TILTS)
def test_ramp_equals_a_constant_normal_map(tilt, axis):
    """A 2 x 2 ramp h = k u (or k v) has the slopes (k, 0) (or (0, k)) at every uv, wrap included.  On the rectangular quad p_u and p_v are orthogonal and lie in the
    shading plane, so g_u = p_u / |p_u|^2, g_v = p_v / |p_v|^2 and the type-4 record equals the type-3 record whose constant texel encodes
    v = (-sigma h_u / |p_u|, -/+ sigma h_v / |p_v|, 1) in that record's frame (s' along p_u, t' = n x s': the sign of the second component is that of t' . p_v,
    taken from the tables).  Images to 2e-6 rel-L2.  Measured: 0 .. 1.65e-7."""
    k = 0.8
    tex = np.array([0.0, k, 0.0, k] if axis == "u" else [k, k, 0.0, 0.0], np.float32)          # (row 0 is v -> 1: the lookup flips v)
    tbh = scene(uv_quad_xml(height_xml(0.3), tilt), RES, SPP, height=tex, map_res=(2, 2)).tables(0)
    T = tbh["tri_info"].detach().cpu().numpy().astype(np.float64)[0]
    q = tbh["tri_uv"].detach().cpu().numpy().astype(np.float64).reshape(tbh["num_tris"], -1)[0, :6]
    e1, e2, n = T[3:6], T[6:9], T[18:21] / np.linalg.norm(T[18:21])
    det = (q[2] - q[0]) * (q[5] - q[1]) - (q[4] - q[0]) * (q[3] - q[1])
    pu, pv = (e1 * (q[5] - q[1]) - e2 * (q[3] - q[1])) / det, (e2 * (q[2] - q[0]) - e1 * (q[4] - q[0])) / det
    assert abs(pu @ pv) < 1e-3 and abs(np.linalg.norm(pu) - 80.0) < 1e-2          # the rectangular quad: 160 wide over two units of u
    s1 = pu / np.linalg.norm(pu)
    t1 = np.cross(n, s1)
    hu, hv = (k, 0.0) if axis == "u" else (0.0, k)
    vec = (-SIGMA * hu / np.linalg.norm(pu), -SIGMA * hv * (t1 @ pv) / (pv @ pv), 1.0)
    assert np.allclose(perturbed_normal64(n, e1, e2, q, SIGMA, np.array([hu]), np.array([hv]))[0], (vec[0] * s1 + vec[1] * t1 + n) / np.linalg.norm(vec), atol=1e-12)
    tbn = scene(uv_quad_xml(normal_xml(0.3, tuple(encode(vec))), tilt), RES, SPP).tables(0)
    assert tbn["material_mask"] == 8 and tbh["material_mask"] == 16
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    a, b = host_colloc_render(tbh, o), host_colloc_render(tbn, o)
    print("height ramp in %s at tilt %g against the type-3 record: rel-L2 %.2e" % (axis, tilt, rel_l2(a, b)))
    assert b.max() > 0 and rel_l2(a, b) <= 2e-6, rel_l2(a, b)
    flat = host_colloc_render(scene(uv_quad_xml(microfacet_xml(0.3), tilt), RES, SPP).tables(0), o)
    assert rel_l2(a, flat) > 1e-3          # (and the ramp shows)


# ---------------------------------------------------------------- 3. limits
@pytest.mark.parametrize("case", ["1x1", "4x4-constant", "sigma0"])
@pytest.mark.parametrize("tilt", TILTS)
def test_limit_flat_height_is_no_map(tilt, case):
    """A constant height map (1 x 1, and 4 x 4 of one value) and a random map under sigma = 0 each equal height_map = None to 1e-6 rel-L2 (n' = n; what differs is
    the rounding of Frame(n).to_local(Frame(n).to_world(wi)))."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    kw = {"1x1": {}, "4x4-constant": dict(height=np.full(16, 0.7, np.float32)), "sigma0": dict(height="random", scale=0.0)}[case]
    tb = scene(uv_quad_xml(height_xml(0.3, height=0.7), tilt), RES, SPP, **kw).tables(0)
    assert tb["material_mask"] == 16
    img = host_colloc_render(tb, o)
    ref = host_colloc_render(scene(uv_quad_xml(microfacet_xml(0.3), tilt), RES, SPP).tables(0), o)
    assert ref.max() > 0
    assert rel_l2(img, ref) <= 1e-6, rel_l2(img, ref)


@pytest.mark.parametrize("tilt", TILTS)
def test_no_map_is_the_record_of_section_14(tilt):
    """height_map = None: the tables are those of the scene loaded without the child, word for word -- record type 2, PSDR_SLOT_ALPHA_V = PSDR_SLOT_K = (0, 1, 1),
    mask 4 -- whatever height_scale says, and the image equals it bit for bit."""
    xml = uv_quad_xml(microfacet_xml(0.3), tilt)

    def explicit(sc):
        b = sc.m_bsdfs[0]
        nb = psdr_cuda.MicrofacetBSDF(b.specular_reflectance, b.diffuse_reflectance, b.roughness, normal_map=None, height_map=None, height_scale=3.0)
        nb.id = b.id
        sc.m_bsdfs[0] = sc.param_map["BSDF[0]"] = sc.param_map["BSDF[id=m]"] = nb
        for m in sc.m_meshes:
            m.bsdf = nb
    tb, tb2 = xml_scene(xml, RES, SPP).tables(0), xml_scene(xml, RES, SPP, prepare=explicit).tables(0)
    row, _ = record(tb2, "plain")
    assert row[0] == _abi.BSDF_MICROFACET == 2 and list(row[7:10]) == [0, 1, 1] and list(row[13:16]) == [0, 1, 1] and tb2["material_mask"] == 4
    assert np.array_equal(tb["bsdf_rec"].cpu().numpy(), tb2["bsdf_rec"].cpu().numpy()) and np.array_equal(tb["texels"].cpu().numpy(), tb2["texels"].cpu().numpy())
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    assert np.array_equal(host_colloc_render(tb, o), host_colloc_render(tb2, o))


def test_mixed_scene_dispatches_per_mesh():
    """A diffuse, a rough-conductor, a microfacet, a normal-mapped and a height-mapped microfacet quad (record types 0 .. 4) in one scene: each mesh's pixels equal
    those of the scene that holds that mesh alone, bit for bit."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    kw = dict(textured=True, normal="random", height="random")
    tbm = scene(mixed_xml(MIXED_IDS), RES, SPP, **kw).tables(0)
    rec = tbm["bsdf_rec"].cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    assert list(rec[:, 0]) == [0, 1, 2, 3, 4] and tbm["material_mask"] == 31
    mixed = host_colloc_render(tbm, o)
    covered = np.zeros(len(mixed), bool)
    solos = {}
    for bid in MIXED_IDS:
        solo = host_colloc_render(scene(mixed_xml(MIXED_IDS, only=bid), RES, SPP, **kw).tables(0), o)
        px = (solo != 0).any(axis=1)
        assert px.sum() >= 4 and not (covered & px).any(), bid          # the five quads cover separate pixels
        assert np.array_equal(mixed[px], solo[px]), bid
        covered |= px
        solos[bid] = solo[px].mean(axis=0)
    assert (mixed[~covered] == 0).all()
    assert not np.allclose(solos["m"], solos["h"], rtol=1e-2)          # the relief shows


# ---------------------------------------------------------------- 4. degenerate input
def _all_modes(tb, res, spp, sppe):
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    tan = random_tangents(tb, NAMES, seed=1)
    img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    img_r, grads = host_colloc_rev(tb, o, adj, want=NAMES)
    assert np.isfinite(img).all() and np.isfinite(dimg).all() and np.isfinite(img_r).all()
    for n in NAMES:
        assert np.isfinite(grads[n]).all(), n
    assert rel_l2(img_r, img) < 1e-6 or img.max() == 0
    return o, img, grads


def _height_texel_dimg(tb, o):
    """forward mode with a random tangent on the height map's texels and on the scale"""
    row, off = record(tb, "height")
    tan = torch.zeros_like(tb["texels"])
    n = map_words(row, "height")
    tan[off["height"]:off["height"] + n] = torch.rand(n, generator=torch.Generator().manual_seed(3)) - 0.5
    tan[off["scale"]] = 1.0
    return host_colloc_render(tb, o, mode=1, tangents={"texels": tan})[1]


def _scale_uv(factor):
    def f(sc):
        for m in sc.m_meshes:
            m._vertex_uv = (m._vertex_uv * factor).contiguous()
    return f


@pytest.mark.parametrize("case", ["coincident-uvs", "sliver"])
def test_degenerate_flat_cases(case):
    """Flat cases.  coincident-uvs: a quad whose UVs all coincide (det = 0).  sliver: J = (e1 x e2) . n / det, the triangle's area per unit of uv area, under the
    threshold 1e-20 -- the quad with its UVs scaled by 1e13 (det of order 1e27, J of order 1e-23): a sliver in the texture's units, so that the film still hits
    it.  In both n' = n: the image is that of the record without a map (1e-6 rel-L2, as the flat limit) whatever the map says; forward and reverse mode agree
    that the height texels and the scale receive nothing, and the other maps still receive their gradient."""
    res, spp, sppe = 16, 4, 4
    kw = dict(uv="collapse") if case == "coincident-uvs" else dict(extra=_scale_uv(1e13))
    tb = scene(uv_quad_xml(height_xml(0.3), 30.0), res, spp, sppe, height="random", textured=True, **kw).tables(0)
    uvs = tb["tri_uv"].cpu().numpy().astype(np.float64).reshape(tb["num_tris"], -1)[:, :6]
    det = (uvs[:, 2] - uvs[:, 0]) * (uvs[:, 5] - uvs[:, 1]) - (uvs[:, 4] - uvs[:, 0]) * (uvs[:, 3] - uvs[:, 1])
    if case == "coincident-uvs":
        assert (det == 0).all()
    else:
        T = tb["tri_info"].cpu().numpy().astype(np.float64)
        J = np.abs(np.einsum("ij,ij->i", np.cross(T[:, 3:6], T[:, 6:9]), T[:, 18:21]) / det)
        assert (det != 0).all() and np.isfinite(det).all() and (J < 1e-21).all() and (J > 0).all()
    o, img, grads = _all_modes(tb, res, spp, sppe)
    ref = host_colloc_render(scene(uv_quad_xml(height_xml(0.3), 30.0), res, spp, sppe, height="random", textured=True, drop_height=True, **kw).tables(0), o)
    assert ref.max() > 0 and rel_l2(img, ref) <= 1e-6
    row, off = record(tb, "height")
    assert (grads["texels"][off["height"]:off["height"] + map_words(row, "height")] == 0).all() and grads["texels"][off["scale"]] == 0
    assert np.abs(grads["texels"][off["kd"]:off["kd"] + 48]).max() > 0
    assert (_height_texel_dimg(tb, o) == 0).all()


def test_degenerate_last_cell():
    """Hits whose wrapped u is 1 and whose wrapped, flipped v is 1 in fp32 (u = -1e-9 .., v = +1e-9 ..: the quad's UVs mirrored and scaled by 1e-9): px = w - 1 and
    py = h - 1 are clamped to the last cell with w1x = w1y = 0, the corner the lookup itself reads there.  The scale is raised by 1e9 with it so that the slopes
    are those of the plain case.  Everything is finite in every mode and the image is the closed form evaluated with the texture coordinates wrapped in fp32
    (in float64 the wrap gives 1 - 1e-9 and the other end of the cell) at the closed-form bound; the height texels of the last cell, and only those, receive a
    gradient."""
    res, spp, sppe = 16, 4, 4
    tb = scene(uv_quad_xml(height_xml(0.3), 30.0), res, spp, sppe, uv="mirror", height="random", scale=SIGMA * 1e9, extra=_scale_uv(1e-9)).tables(0)
    o, img, grads = _all_modes(tb, res, spp, sppe)
    ref = closed_form_image(tb, host_film_samples(tb, o), spp, "height", fp32_uv=True)
    flat = host_colloc_render(scene(uv_quad_xml(microfacet_xml(0.3), 30.0), res, spp).tables(0), o)
    assert ref.max() > 0 and rel_l2(ref, flat) > 1e-3          # the slopes of the last cell show
    assert rel_l2(img, ref) <= max(2e-6, 4 * MEASURED_CLOSED_FORM), rel_l2(img, ref)
    row, off = record(tb, "height")
    g = grads["texels"][off["height"]:off["height"] + 16].reshape(4, 4)
    mask = np.ones((4, 4), bool)
    mask[2:, 2:] = False
    assert (g[mask] == 0).all() and np.abs(g[2:, 2:]).max() > 0


# ---------------------------------------------------------------- 5. forward = reverse
@pytest.mark.parametrize("name", ["quad", "room", "bunny"])
def test_forward_equals_reverse(name):
    """<adj, J t> = <J^T adj, t> with random tangents and a random adjoint image for the texels (four 4 x 4 maps and the scale), the triangle rows, the camera pose
    and the primary-edge rows; on the quad with UVs turned by 37 degrees, on cbox_uv with a height-mapped floor (no tree) and on bunny_light with a height-mapped,
    smooth-shaded bunny (one tree, planar UVs).  |lhs - rhs| <= 1e-4 x scale, as test_colloc_normal_host.py::test_forward_equals_reverse.  The height map's texel
    range and the scale receive a gradient, and the triangle-row gradient differs from that of the same scene without the map."""
    res, spp, sppe = 16, 4, 4
    tb = named_scene("height", name, res, spp, sppe).tables(0)
    assert tb["material_mask"] & (1 << _abi.BSDF_MICROFACET_HEIGHT)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    row, off = record(tb, "height")
    for n in NAMES:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan)
        img_r, grads = host_colloc_rev(tb, o, adj, want=[n])
        assert rel_l2(img_r, img) < 1e-6
        lhs, rhs = float((adj.astype(np.float64) * dimg).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg).sum())
        assert scale > 0, n
        print("height map forward = reverse, %s %s: lhs %.6e rhs %.6e scale %.3e" % (name, n, lhs, rhs, scale))
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        if n == "texels":
            for key, width in (("kd", 48), ("f0", 48), ("roughness", 16), ("height", map_words(row, "height")), ("scale", 1)):
                assert np.abs(grads["texels"][off[key]:off[key] + width]).max() > 0, key
            # ... and the height texels and the scale alone
            t2 = torch.zeros_like(tan["texels"])
            t2[off["height"]:off["height"] + 16] = tan["texels"][off["height"]:off["height"] + 16]
            t2[off["scale"]] = tan["texels"][off["scale"]]
            d2 = host_colloc_render(tb, o, mode=1, tangents={"texels": t2})[1]
            lhs, rhs = float((adj.astype(np.float64) * d2).sum()), dot_tables(grads, {"texels": t2})
            scale = float(np.abs(adj.astype(np.float64) * d2).sum())
            assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)
        if n == "tri_info":
            tb0 = named_scene("height", name, res, spp, sppe, drop_height=True).tables(0)
            assert np.array_equal(tb0["tri_info"].detach().cpu().numpy(), tb["tri_info"].detach().cpu().numpy())
            g0 = host_colloc_rev(tb0, o, adj, want=[n])[1][n]
            assert np.abs(grads[n] - g0).max() > 1e-3 * np.abs(g0).max()


# ---------------------------------------------------------------- 6. AD against central differences
def _big_quad(spp, offset=0.0, grad=False, one_cell=False, drop=False):
    """a 400 x 400 height-mapped quad (it fills the film: no silhouette), UVs turned by 37 degrees.  Four 4 x 4 maps, sigma = 15; or (one_cell) constant other maps
    and the 2 x 2 height map, sigma = 300, with the UVs shrunk and shifted into one period of the texture (0.05 .. 0.95: no wrap, so the bilinear patch has no
    crease anywhere on the quad) and raw vertex 2 moved by `offset` along raw x, in the quad's own plane: the hit points stay, the uv interpolation and p_u, p_v
    move."""
    P = FloatD(float(offset))
    if grad:
        ek.set_requires_gradient(P)

    def move(sc):
        m = sc.m_meshes[0]
        e = torch.zeros_like(m._vertex_positions_raw)
        e[2, 0] = 1.0
        m._vertex_positions_raw = m._vertex_positions_raw + e * P.t
        m._vertex_uv = (m._vertex_uv * 0.25 + torch.tensor([0.5, 0.05], device=m._vertex_uv.device)).contiguous()
    xml = _HEAD + height_xml(0.3) + quad("m", 30.0, 400.0) + "</scene>\n"
    if one_cell:
        return scene(xml, RES, spp, 0, uv="rot37", height=ONE_CELL, map_res=(2, 2), scale=300.0, drop_height=drop, extra=move), P
    return scene(xml, RES, spp, 0, uv="rot37", height="random", scale=15.0, textured=True), P


@pytest.mark.parametrize("which", ["height-texel", "scale", "vertex"])
def test_ad_against_central_differences(which):
    """d image / d parameter in forward mode against the central difference of the harness' own renderC at two steps on the same streams, by the method and
    acceptance rule of test_colloc_normal_host.py::test_ad_against_central_differences: floor = distance of the two differences; AD must lie within 3 x floor of
    their mean.  Parameters: an inner texel of the 4 x 4 height map (steps 1e-2 and 2e-2 of its range 1); the scale (steps 0.15 and 0.3 of 15); one coordinate of a
    vertex of a quad that fills the film, moved in the quad's plane (steps 4 and 8 of 400) under the 2 x 2 map with constant other maps -- no silhouette is seen,
    the hit points stay, and the one-cell map has no crease: what moves is uv (the cross term) and p_u, p_v (the same scene without the map has a zero derivative,
    asserted).
    Measured, image L2 norms (|AD - mean|, floor, |mean|): texel 6.474e-12, 1.145e-11, 2.118e-7; scale 5.058e-13, 1.030e-12, 1.065e-8; vertex 3.557e-11, 4.241e-11,
    1.515e-9."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    if which == "vertex":
        fds = [(host_colloc_render(_big_quad(SPP, +h, one_cell=True)[0].tables(0), o).astype(np.float64) - host_colloc_render(_big_quad(SPP, -h, one_cell=True)[0].tables(0), o).astype(np.float64)) / (2.0 * h)
               for h in (4.0, 8.0)]
        sc, P = _big_quad(SPP, 0.0, grad=True, one_cell=True)
        tb = sc.tables(0)
        uv = tb["tri_uv"].cpu().numpy().reshape(tb["num_tris"], -1)[:, :6]
        assert uv.min() > 0.0 and uv.max() < 1.0          # one period
        tan = tangents_wrt(tb, P)
        assert tan["tri_info"] is not None and float(tan["tri_info"].abs().max()) > 0
        ad = host_colloc_render(tb, o, mode=1, tangents=tan)[1].astype(np.float64)
        tb0 = _big_quad(SPP, 0.0, one_cell=True, drop=True)[0].tables(0)
        assert tb0["material_mask"] == 4 and np.abs(host_colloc_render(tb0, o, mode=1, tangents=tan)[1]).max() <= 1e-4 * np.abs(ad).max()
    else:
        tb = _big_quad(SPP)[0].tables(0)
        _, off = record(tb, "height")
        i, steps = (off["height"] + 5, (1e-2, 2e-2)) if which == "height-texel" else (off["scale"], (0.15, 0.3))
        base = tb["texels"].detach().clone()
        v0 = float(base[i])

        def render(delta):
            t = dict(tb)
            t["texels"] = base.clone()
            t["texels"][i] = v0 + delta
            return host_colloc_render(t, o).astype(np.float64)
        fds = [(render(+h) - render(-h)) / (2.0 * h) for h in steps]
        tan = base.clone().zero_()
        tan[i] = 1.0
        ad = host_colloc_render(tb, o, mode=1, tangents={"texels": tan})[1].astype(np.float64)
    floor, mean = float(np.linalg.norm(fds[0] - fds[1])), (fds[0] + fds[1]) / 2.0
    dist = float(np.linalg.norm(ad - mean))
    print("height map AD vs central differences, %s: |AD - mean| %.3e, floor %.3e, |mean| %.3e" % (which, dist, floor, np.linalg.norm(mean)))
    assert np.linalg.norm(mean) > 0 and floor > 0
    assert dist <= 3.0 * floor, (dist, floor)


# ---------------------------------------------------------------- 7. surface, loader, errors
def test_python_class():
    b = psdr_cuda.MicrofacetBSDF(0.05, (0.5, 0.4, 0.3), 0.25)
    assert b.height_map is None and b.normal_map is None
    assert isinstance(b.height_scale, psdr_cuda.Bitmap1fD) and np.allclose(b.height_scale.tensor().cpu().numpy(), 1.0)
    c = psdr_cuda.MicrofacetBSDF(0.05, (0.5, 0.4, 0.3), 0.25, height_map=0.3, height_scale=2.5)
    assert isinstance(c.height_map, psdr_cuda.Bitmap1fD) and np.allclose(c.height_map.tensor().cpu().numpy(), 0.3)
    assert np.allclose(c.height_scale.tensor().cpu().numpy(), 2.5) and tuple(c.height_scale.resolution) == (1, 1)
    bm, sm = psdr_cuda.Bitmap1fD(0.0), psdr_cuda.Bitmap1fD(4.0)
    d = psdr_cuda.MicrofacetBSDF(height_map=bm, height_scale=sm)
    assert d.height_map is bm and d.height_scale is sm
    with pytest.raises(RuntimeError, match=NOT_BOTH):
        psdr_cuda.MicrofacetBSDF(normal_map=(0.5, 0.5, 1.0), height_map=0.0)
    assert c.type_name() == "MicrofacetBSDF" and c.anisotropic() is False


def test_loader_record_and_mask():
    """<bsdf type="microfacet"> with the children heightMap / height_map (a constant float or a bitmap texture) and heightScale / height_scale; without heightMap: no
    map.  The records and masks tables() emits: type 2 / bit 2 without a map, as before; with one, type 4 / bit 4, the three slots of type 2 unchanged, the scale's
    (offset, 1, 1) in PSDR_SLOT_ALPHA_V and the map's (offset, w, h) in PSDR_SLOT_K.  param_map reaches both, and so does the torch graph."""
    sc = scene(uv_quad_xml(height_xml(0.3, 0.25, 2.5)), RES, SPP)
    sc2 = scene(uv_quad_xml(height_xml(0.3, 0.25, 2.5, name="height_map", scale_name="height_scale")), RES, SPP)
    plain = scene(uv_quad_xml(microfacet_xml(0.3)), RES, SPP)
    tb, tb2, tbp = sc.tables(0), sc2.tables(0), plain.tables(0)
    assert tbp["material_mask"] == 4 and tb["material_mask"] == 1 << _abi.BSDF_MICROFACET_HEIGHT == 16
    assert plain.param_map["BSDF[id=m]"].height_map is None
    assert np.array_equal(tb["bsdf_rec"].cpu().numpy(), tb2["bsdf_rec"].cpu().numpy()) and np.array_equal(tb["texels"].cpu().numpy(), tb2["texels"].cpu().numpy())
    row, off = record(tb, "height")
    rowp, offp = record(tbp, "plain")
    assert row[0] == 4 and rowp[0] == 2 and list(row[1:7]) == list(rowp[1:7]) and list(row[10:13]) == list(rowp[10:13]) and list(rowp[7:10]) == [0, 1, 1] == list(rowp[13:16])
    assert list(row[7:10]) == [off["scale"], 1, 1] and list(row[13:16]) == [off["height"], 1, 1]
    texels = tb["texels"].cpu().numpy()
    assert np.allclose(texels[off["scale"]], 2.5) and np.allclose(texels[off["height"]], 0.25)
    n0 = min(off["scale"], off["height"])
    assert np.array_equal(texels[:n0], tbp["texels"].cpu().numpy()[:n0])
    b = sc.param_map["BSDF[id=m]"]
    assert isinstance(b, psdr_cuda.MicrofacetBSDF) and isinstance(b.height_map, psdr_cuda.Bitmap1fD) and sc.param_map["BSDF[0]"].height_map is b.height_map
    # the scale without a map: kept on the object, the record stays of type 2
    only_scale = scene(uv_quad_xml(microfacet_xml(0.3).replace("</bsdf>", '<float name="heightScale" value="3"/></bsdf>')), RES, SPP)
    assert only_scale.tables(0)["material_mask"] == 4 and np.allclose(only_scale.param_map["BSDF[id=m]"].height_scale.tensor().cpu().numpy(), 3.0)
    # a bitmap texture
    bmp = height_xml(0.3).replace('<float name="heightMap" value="0"/>',
                                  '<texture name="heightMap" type="bitmap"><string name="filename" value="./data/textures/test_texture.exr"/></texture>')
    assert "texture" in bmp
    sb = scene(uv_quad_xml(bmp), RES, SPP)
    w, h = sb.param_map["BSDF[id=m]"].height_map.resolution
    assert w > 1 and h > 1
    rowb, _ = record(sb.tables(0), "height")
    assert list(rowb[14:16]) == [w, h]
    # both maps in one element
    with pytest.raises(RuntimeError, match=NOT_BOTH):
        scene(uv_quad_xml(normal_xml(0.3).replace("</bsdf>", '<float name="heightMap" value="0"/></bsdf>')), RES, SPP)
    late = scene(uv_quad_xml(height_xml(0.3)), RES, SPP)
    late.param_map["BSDF[id=m]"].normal_map = psdr_cuda.Bitmap3fD((0.5, 0.5, 1.0))
    with pytest.raises(RuntimeError, match=NOT_BOTH):
        late.configure()
    # requires_grad / the torch graph reaches the map and the scale: the texel pool's gradient lands in the bitmaps' tensors
    ek.set_requires_gradient(b.height_map.data)
    ek.set_requires_gradient(b.height_scale.data)
    sc.configure()
    pool = sc.tables(0)["texels"]
    assert pool.requires_grad
    (pool[off["height"]] + 2.0 * pool[off["scale"]]).backward()
    assert np.allclose(b.height_map.data.t.grad.cpu().numpy(), 1.0) and np.allclose(b.height_scale.data.t.grad.cpu().numpy(), 2.0)


def test_refusals():
    """DirectIntegrator and PathTracer keep raising the MicrofacetBSDF message for a height-mapped record; a mesh without texture coordinates under a height map
    raises the new message before any native call, from every entry of the CollocatedIntegrator -- bunny_light as it is: bunny_low.obj has no texture
    coordinates."""
    sc = scene(uv_quad_xml(height_xml(0.3)), RES, SPP, height="random")
    direct, path = psdr_cuda.DirectIntegrator(1, 1), psdr_cuda.PathTracer(3, True)
    for call in (lambda: direct.renderC(sc), lambda: direct.renderD(sc), lambda: direct.preprocess_secondary_edges(sc, 0, [2, 2, 2, 1]),
                 lambda: path.renderC(sc), lambda: path.renderD(sc), lambda: path.preprocess_path_secondary_edges(sc, 0, [2, 2, 2, 1])):
        with pytest.raises(RuntimeError, match=MESSAGE):
            call()
    psdr_cuda.CollocatedIntegrator(1.0)._check_bsdfs(sc)
    bare = scene(bunny_xml("plain").replace("</bsdf>", '<float name="heightMap" value="0"/></bsdf>', 1), RES, SPP)
    assert bare.tables(0)["tri_uv"] is None and bare.tables(0)["material_mask"] & 16
    colloc = psdr_cuda.CollocatedIntegrator(1.0)
    for call in (lambda: colloc.renderC(bare), lambda: colloc.renderD(bare)):
        with pytest.raises(RuntimeError, match=KINDS["height"].needs_uv):
            call()
    with pytest.raises(RuntimeError, match=MESSAGE):          # the older message first, as the C ABI orders them
        direct.renderC(bare)


# ---------------------------------------------------------------- 8. the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers(tmp_path):
    """tests/hostcheck/colloc_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_collocated.cpp, built with
    -fsanitize=address,undefined for the host (hostlibs.san_program) and asked for a record of type BSDF_MICROFACET_HEIGHT:
    render, forward and reverse on the tiny scene of the five record types; it must end clean and report what the
    library reports.  It refuses tables without a type-4 record."""
    exe = san_program("colloc_san", HC_DEPS)
    res, spp, sppe = 8, 2, 2
    o = colloc_opts(spp, sppe, rng_offset=(1, 2, 0))
    adj = np.random.default_rng(4).random((res * res, 3)).astype(np.float32)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(tb, name):
        tan = random_tangents(tb, ["tri_info", "texels", "prim_edge"], seed=3)
        tbc, desc, keep = cpu_desc(tb)
        path = str(tmp_path / name)
        write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in ("tri_info", "texels", "prim_edge")], adj)
        return tan, subprocess.run([exe, path, str(_abi.BSDF_MICROFACET_HEIGHT)], capture_output=True, text=True, env=env, timeout=600)
    _, r = run(scene(mixed_xml(MIXED_IDS, only="n"), res, spp, sppe, textured=True, normal="random", uv="rot37", drop_height=True).tables(0), "no_height.bin")
    assert r.returncode == 2 and "no height-mapped" in r.stderr, (r.returncode, r.stderr[-1000:])
    tb = scene(mixed_xml(MIXED_IDS), res, spp, sppe, textured=True, normal="random", height="random", uv="rot37").tables(0)
    tan, r = run(tb, "tables.bin")
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan, nthreads=2)
    _, grads = host_colloc_rev(tb, o, adj, want=["tri_info", "texels", "prim_edge"])
    want = [np.abs(host_colloc_render(tb, o, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + [np.abs(grads[n].astype(np.float64)).sum() for n in ("tri_info", "texels", "prim_edge")]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
