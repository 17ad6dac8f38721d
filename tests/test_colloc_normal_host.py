"""MicrofacetBSDF with a tangent-space normal map (csrc/psdr_colloc_microfacet.h, DESIGN.md section 15: record type PSDR_BSDF_MICROFACET_NORMAL, evaluated by the
CollocatedIntegrator) on the HOST: the product's PSDR_HD functions run slot by slot by tests/hostcheck/hostcheck_collocated.cpp.  The model is build-defined and
the oracle is not extended, so it is pinned on its closed form written out in float64 (tangent frame from the triangle's UVs included), on its limits against
the record without a map, on its degenerate inputs, on forward = reverse and on AD against central differences of the harness' own renderC."""
import os
import subprocess

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import HC_DEPS, _HEAD, colloc_opts, host_colloc_render, host_colloc_rev, host_film_samples, xml_scene
from colloc_microfacet_helpers import (FLAT, KINDS, MESSAGE, bunny_xml, closed_form_image, encode, lean_texel, map_words, microfacet_xml, mixed_xml, named_scene, normal_xml,
                                       quad, random_normal_texels, record, scene, uv_quad_xml)
from enoki.cuda_autodiff import Float32 as FloatD
from helpers import dot_tables, random_tangents, rel_l2, tangents_wrt
from hostlibs import cpu_desc, san_program, write_tables_file
from psdr_cuda import _abi

RES, SPP = 16, 4
TILTS, ROUGHNESS = (0.0, 30.0, 70.0), (0.3, 0.6)
NAMES = ["texels", "tri_info", "cam_to_world", "prim_edge"]
MIXED_IDS = ("d", "c", "m", "n")          # the quads of mixed_xml: record types 0 .. 3


# ---------------------------------------------------------------- 1. closed form
MEASURED_CLOSED_FORM = 5.75e-6          # the largest of the cases below, measured on the host (70 degrees, 4 x 4 map, r = 0.3, plain UVs)


@pytest.mark.parametrize("case", ["lean20", "4x4"])
@pytest.mark.parametrize("uv", [None, "rot37", "mirror"], ids=["uv", "uv-rot37", "uv-mirror"])
@pytest.mark.parametrize("r", ROUGHNESS)
@pytest.mark.parametrize("tilt", TILTS)
def test_closed_form(tilt, r, uv, case):
    """The tilted quad: the harness' renderC against section 15 written out in float64 numpy at the harness' own film samples -- dp_du from the triangle's edges
    and UVs, s' = its part orthogonal to n, t' = n x s', n' from the decoded texel, the lobes at the angle between the view direction and n'.  Maps: 1 x 1 leaning
    the normal 20 degrees about the u axis; 4 x 4 random with every v.z >= 0.5.  UVs: as the mesh has them, turned 37 degrees in the plane, and mirrored
    (det < 0) -- in the last two s' is not Frame(n).s, and a kernel with another tangent misses the bound by orders of magnitude (1e-1).
    Bound: image rel-L2 <= max(2e-6, 4 x the largest value measured here) = 2.3e-5.
    Measured (rel-L2): 1 x 1 map 6.7e-8 .. 9.6e-8 at 0 / 30 degrees, 3.5e-7 .. 4.6e-7 at 70; 4 x 4 map 1.6e-7 .. 1.6e-6 at 0 / 30 degrees, 6.9e-7 .. 5.75e-6 at 70:
    with the normal leaning up to 50 degrees on a quad seen at 70, samples reach wi'.z -> 0, where the specular lobe's 1 / (4 wi'.z) amplifies the fp32 rounding
    of wi'.z."""
    if case == "lean20":
        sc = scene(uv_quad_xml(normal_xml(r, lean_texel(20.0)), tilt), RES, SPP, uv=uv)
    else:
        sc = scene(uv_quad_xml(normal_xml(r), tilt), RES, SPP, uv=uv, normal="random")
    tb = sc.tables(0)
    assert tb["material_mask"] == 1 << _abi.BSDF_MICROFACET_NORMAL
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(tb, o)
    ref = closed_form_image(tb, host_film_samples(tb, o), SPP, "normal")
    assert (ref > 0).any() and (ref == 0).any()          # the quad and the background are both seen
    e = rel_l2(img, ref)
    print("normal map closed form tilt %g r %g %s %s: rel-L2 %.2e" % (tilt, r, uv, case, e))
    assert e <= max(2e-6, 4 * MEASURED_CLOSED_FORM), e


def test_closed_form_tells_the_tangent():
    """the closed form itself tells the frames apart: the lean-20 image with plain UVs differs from the one with UVs turned by 37 degrees by more than 1e-2"""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    a, b = (host_colloc_render(scene(uv_quad_xml(normal_xml(0.3, lean_texel(20.0)), 30.0), RES, SPP, uv=uv).tables(0), o) for uv in (None, "rot37"))
    assert rel_l2(a, b) > 1e-2


# ---------------------------------------------------------------- 2. limits
@pytest.mark.parametrize("tilt", TILTS)
def test_limit_flat_map_is_no_map(tilt):
    """A 1 x 1 map (0.5, 0.5, 1) equals normal_map = None to 1e-6 rel-L2 (n' = n; what differs is the rounding of Frame(n).to_local(Frame(n).to_world(wi)))."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(scene(uv_quad_xml(normal_xml(0.3, FLAT), tilt), RES, SPP).tables(0), o)
    ref = host_colloc_render(scene(uv_quad_xml(microfacet_xml(0.3), tilt), RES, SPP).tables(0), o)
    assert ref.max() > 0
    assert rel_l2(img, ref) <= 1e-6, rel_l2(img, ref)


@pytest.mark.parametrize("r", ROUGHNESS)
@pytest.mark.parametrize("tilt", TILTS)
def test_no_map_is_the_record_of_section_14(tilt, r):
    """normal_map = None: the tables are those of the scene loaded without the child, word for word -- record type 2, PSDR_SLOT_K = (0, 1, 1), mask 4 -- the image
    equals it bit for bit, and it meets the type-2 closed form of test_colloc_microfacet_host.py::test_closed_form at that test's bound (2e-6)."""
    xml = uv_quad_xml(microfacet_xml(r), tilt)

    def explicit(sc):
        b = sc.m_bsdfs[0]
        nb = psdr_cuda.MicrofacetBSDF(b.specular_reflectance, b.diffuse_reflectance, b.roughness, normal_map=None)
        nb.id = b.id
        sc.m_bsdfs[0] = sc.param_map["BSDF[0]"] = sc.param_map["BSDF[id=m]"] = nb
        for m in sc.m_meshes:
            m.bsdf = nb
    tb, tb2 = xml_scene(xml, RES, SPP).tables(0), xml_scene(xml, RES, SPP, prepare=explicit).tables(0)
    row, _ = record(tb2, "plain")
    assert row[0] == _abi.BSDF_MICROFACET == 2 and list(row[1 + 3 * _abi.SLOT_K:4 + 3 * _abi.SLOT_K]) == [0, 1, 1] and tb2["material_mask"] == 4
    assert np.array_equal(tb["bsdf_rec"].cpu().numpy(), tb2["bsdf_rec"].cpu().numpy()) and np.array_equal(tb["texels"].cpu().numpy(), tb2["texels"].cpu().numpy())
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img, img2 = host_colloc_render(tb, o), host_colloc_render(tb2, o)
    assert np.array_equal(img, img2)
    assert rel_l2(img2, closed_form_image(tb2, host_film_samples(tb2, o), SPP, "plain")) <= 2e-6


def test_mixed_scene_dispatches_per_mesh():
    """A diffuse, a rough-conductor, a microfacet and a normal-mapped microfacet quad (record types 0, 1, 2, 3) in one scene: each mesh's pixels equal those of the
    scene that holds that mesh alone, bit for bit."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    tbm = scene(mixed_xml(MIXED_IDS), RES, SPP, textured=True).tables(0)
    rec = tbm["bsdf_rec"].cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    assert list(rec[:, 0]) == [0, 1, 2, 3] and tbm["material_mask"] == 15
    mixed = host_colloc_render(tbm, o)
    covered = np.zeros(len(mixed), bool)
    solos = {}
    for bid in MIXED_IDS:
        solo = host_colloc_render(scene(mixed_xml(MIXED_IDS, only=bid), RES, SPP, textured=True).tables(0), o)
        px = (solo != 0).any(axis=1)
        assert px.sum() >= 4 and not (covered & px).any(), bid          # the four quads cover separate pixels
        assert np.array_equal(mixed[px], solo[px]), bid
        covered |= px
        solos[bid] = solo[px].mean(axis=0)
    assert (mixed[~covered] == 0).all()
    assert not np.allclose(solos["m"], solos["n"], rtol=1e-2)          # the leaning normal shows


# ---------------------------------------------------------------- 3. degenerate input
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


def _normal_texel_dimg(tb, o):
    """forward mode with a random tangent on the normal map's texels alone"""
    row, off = record(tb, "normal")
    tan = torch.zeros_like(tb["texels"])
    n = map_words(row, "normal")
    tan[off["normal"]:off["normal"] + n] = torch.rand(n, generator=torch.Generator().manual_seed(3)) - 0.5
    return host_colloc_render(tb, o, mode=1, tangents={"texels": tan})[1]


def test_degenerate_coincident_uvs():
    """A quad whose UVs all coincide (det = 0): n' = n, so the image is that of the record without a map (1e-6 rel-L2, as the flat-map limit) whatever the map says;
    forward and reverse mode agree that the normal texels receive nothing, and the other maps still receive their gradient."""
    res, spp, sppe = 16, 4, 4
    tb = scene(uv_quad_xml(normal_xml(0.3), 30.0), res, spp, sppe, uv="collapse", normal="random", textured=True).tables(0)
    uvs = tb["tri_uv"].cpu().numpy().reshape(tb["num_tris"], -1)[:, :6]
    assert (uvs[:, 0:2] == uvs[:, 2:4]).all() and (uvs[:, 0:2] == uvs[:, 4:6]).all()
    o, img, grads = _all_modes(tb, res, spp, sppe)
    ref = host_colloc_render(scene(uv_quad_xml(normal_xml(0.3), 30.0), res, spp, sppe, uv="collapse", normal="random", textured=True, drop_normal=True).tables(0), o)
    assert ref.max() > 0 and rel_l2(img, ref) <= 1e-6
    row, off = record(tb, "normal")
    assert (grads["texels"][off["normal"]:off["normal"] + map_words(row, "normal")] == 0).all()
    assert np.abs(grads["texels"][off["kd"]:off["kd"] + 48]).max() > 0
    assert (_normal_texel_dimg(tb, o) == 0).all()


def test_degenerate_zero_vector_texel():
    """A texel that decodes to v = 0 (c = 0.5, 0.5, 0.5): as a 1 x 1 map the value is zero everywhere, and so are the derivative image and every gradient; as one
    texel of a 4 x 4 map (|v| -> 0 around its centre, where n' turns arbitrarily fast) everything stays finite."""
    res, spp, sppe = 16, 4, 4
    tb = scene(uv_quad_xml(normal_xml(0.3, (0.5, 0.5, 0.5)), 30.0), res, spp, sppe).tables(0)
    o, img, grads = _all_modes(tb, res, spp, 0)
    assert (img == 0).all() and (_normal_texel_dimg(tb, o) == 0).all()
    for n in ("texels", "tri_info", "cam_to_world"):
        assert (grads[n] == 0).all(), n
    tex = random_normal_texels()
    tex[5] = 0.5
    tb = scene(uv_quad_xml(normal_xml(0.3), 0.0), res, spp, sppe, normal=tex, textured=True).tables(0)
    _, img, _ = _all_modes(tb, res, spp, sppe)
    assert img.max() > 0


def test_degenerate_normal_below_the_surface():
    """Texels with v.z < 0.  v = (0, 0, -1): n' = -n, wi'.z < 0 at every hit -- zero image, zero gradients.  v = (0.8, 0, -0.3) on the quad tilted towards +u and
    away from it: n' is below the surface, yet where it still faces the camera the lobes are evaluated about it -- the closed form, and zero where it does not."""
    res, spp, sppe = 16, 4, 4
    tb = scene(uv_quad_xml(normal_xml(0.3, tuple(encode((0.0, 0.0, -1.0)))), 30.0), res, spp, sppe).tables(0)
    o, img, grads = _all_modes(tb, res, spp, 0)
    assert (img == 0).all() and (_normal_texel_dimg(tb, o) == 0).all()
    for n in ("texels", "tri_info", "cam_to_world"):
        assert (grads[n] == 0).all(), n
    lit = []
    for tilt in (70.0, -70.0):
        tb = scene(uv_quad_xml(normal_xml(0.3, tuple(encode((0.8, 0.0, -0.3)))), tilt), res, spp, sppe).tables(0)
        o, img, grads = _all_modes(tb, res, spp, sppe)
        ref = closed_form_image(tb, host_film_samples(tb, o), spp, "normal")
        lit.append(ref.max() > 0)
        assert (img[ref.sum(1) == 0] == 0).all()
        if lit[-1]:
            assert rel_l2(img, ref) <= max(2e-6, 4 * MEASURED_CLOSED_FORM)
    assert sorted(lit) == [False, True]          # one tilt turns n' towards the camera, the other away from it


# ---------------------------------------------------------------- 4. forward = reverse
@pytest.mark.parametrize("name", ["quad", "room", "bunny"])
def test_forward_equals_reverse(name):
    """<adj, J t> = <J^T adj, t> with random tangents and a random adjoint image for the texels (four 4 x 4 maps), the triangle rows, the camera pose and the
    primary-edge rows; on the quad with UVs turned by 37 degrees, on cbox_uv with a normal-mapped floor (no tree) and on bunny_light with a normal-mapped,
    smooth-shaded bunny (one tree; bunny_low.obj has no texture coordinates, the scene gives it planar ones -- the file as it is serves the refusal test below).
    |lhs - rhs| <= 1e-4 x scale, as test_collocated_host.py::test_forward_equals_reverse.  The normal map's texel range receives a gradient, and the triangle-row
    gradient differs from that of the same scene without the map: the tangent-frame path carries something."""
    res, spp, sppe = 16, 4, 4
    tb = named_scene("normal", name, res, spp, sppe).tables(0)
    assert tb["material_mask"] & (1 << _abi.BSDF_MICROFACET_NORMAL)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    row, off = record(tb, "normal")
    for n in NAMES:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan)
        img_r, grads = host_colloc_rev(tb, o, adj, want=[n])
        assert rel_l2(img_r, img) < 1e-6
        lhs, rhs = float((adj.astype(np.float64) * dimg).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg).sum())
        assert scale > 0, n
        print("normal map forward = reverse, %s %s: lhs %.6e rhs %.6e scale %.3e" % (name, n, lhs, rhs, scale))
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        if n == "texels":
            for key, width in (("kd", 48), ("f0", 48), ("roughness", 16), ("normal", map_words(row, "normal"))):
                assert np.abs(grads["texels"][off[key]:off[key] + width]).max() > 0, key
        if n == "tri_info":
            tb0 = named_scene("normal", name, res, spp, sppe, drop_normal=True).tables(0)
            assert np.array_equal(tb0["tri_info"].detach().cpu().numpy(), tb["tri_info"].detach().cpu().numpy())
            g0 = host_colloc_rev(tb0, o, adj, want=[n])[1][n]
            assert np.abs(grads[n] - g0).max() > 1e-3 * np.abs(g0).max()


# ---------------------------------------------------------------- 5. AD against central differences
def _big_quad(spp, offset=0.0, grad=False, constant=False):
    """a 400 x 400 normal-mapped quad (it fills the film: no silhouette), UVs turned by 37 degrees; raw vertex 2 moved by `offset` along raw x, in the quad's own
    plane: the hit points stay, the uv interpolation and dp_du move.  Four 4 x 4 maps, or (constant) 1 x 1 maps with the normal v = (0.3, 0.35, 0.9): then no
    lookup depends on uv and dp_du is all that moves."""
    P = FloatD(float(offset))
    if grad:
        ek.set_requires_gradient(P)

    def move(sc):
        m = sc.m_meshes[0]
        e = torch.zeros_like(m._vertex_positions_raw)
        e[2, 0] = 1.0
        m._vertex_positions_raw = m._vertex_positions_raw + e * P.t
    if constant:
        xml = _HEAD + normal_xml(0.3, tuple(encode((0.3, 0.35, 0.9)))) + quad("m", 30.0, 400.0) + "</scene>\n"
        return scene(xml, RES, spp, 0, uv="rot37", extra=move), P
    xml = _HEAD + normal_xml(0.3) + quad("m", 30.0, 400.0) + "</scene>\n"
    return scene(xml, RES, spp, 0, uv="rot37", normal="random", textured=True, extra=move), P


@pytest.mark.parametrize("which", ["normal-texel-x", "vertex"])
def test_ad_against_central_differences(which):
    """d image / d parameter in forward mode against the central difference of the harness' own renderC at two steps on the same streams, by the method and
    acceptance rule of test_colloc_microfacet_host.py::test_ad_against_central_differences: floor = distance of the two differences; AD must lie within 3 x floor
    of their mean.  Parameters: the x channel of an inner texel of the 4 x 4 normal map (steps 1e-2 and 2e-2 of the channel's range 1); one coordinate of a
    vertex of a quad that fills the film, with constant maps, moved in the quad's plane (steps 4 and 8 of 400) -- no silhouette is seen, the hit points stay and
    no lookup depends on uv: what moves is dp_du, i.e. the tangent frame, alone (the same scene without the map has a zero derivative, asserted).
    Measured, image L2 norms (|AD - mean|, floor, |mean|): texel 3.122e-10, 3.719e-10, 1.623e-6; vertex 1.355e-10, 1.481e-10, 1.399e-9 -- both floors are the
    differences' third-order term (at steps 1 and 2 the vertex floor is fp32 rounding instead, 2.8e-11, and AD lies 6.3e-11 from the mean)."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    if which == "vertex":
        fds = [(host_colloc_render(_big_quad(SPP, +h, constant=True)[0].tables(0), o).astype(np.float64) - host_colloc_render(_big_quad(SPP, -h, constant=True)[0].tables(0), o).astype(np.float64)) / (2.0 * h)
               for h in (4.0, 8.0)]
        sc, P = _big_quad(SPP, 0.0, grad=True, constant=True)
        tb = sc.tables(0)
        tan = tangents_wrt(tb, P)
        assert tan["tri_info"] is not None and float(tan["tri_info"].abs().max()) > 0
        ad = host_colloc_render(tb, o, mode=1, tangents=tan)[1].astype(np.float64)
        # dp_du is all of it: the same scene without the map has no derivative (analytically zero: the hit point, its normal and its distance stay; what fp32
        # leaves are cancellation residues of the dual Moeller-Trumbore, a few 1e-6 of this derivative -- 1e-4 tells the two apart with room)
        tb0 = scene(_HEAD + normal_xml(0.3, tuple(encode((0.3, 0.35, 0.9)))) + quad("m", 30.0, 400.0) + "</scene>\n", RES, SPP, 0, uv="rot37", drop_normal=True).tables(0)
        assert tb0["material_mask"] == 4 and np.abs(host_colloc_render(tb0, o, mode=1, tangents=tan)[1]).max() <= 1e-4 * np.abs(ad).max()
    else:
        tb = _big_quad(SPP)[0].tables(0)
        _, off = record(tb, "normal")
        i = off["normal"] + 3 * 5          # texel (1, 1), an inner one; the x channel
        base = tb["texels"].detach().clone()
        v0 = float(base[i])

        def render(delta):
            t = dict(tb)
            t["texels"] = base.clone()
            t["texels"][i] = v0 + delta
            return host_colloc_render(t, o).astype(np.float64)
        fds = [(render(+h) - render(-h)) / (2.0 * h) for h in (1e-2, 2e-2)]
        tan = base.clone().zero_()
        tan[i] = 1.0
        ad = host_colloc_render(tb, o, mode=1, tangents={"texels": tan})[1].astype(np.float64)
    floor, mean = float(np.linalg.norm(fds[0] - fds[1])), (fds[0] + fds[1]) / 2.0
    dist = float(np.linalg.norm(ad - mean))
    print("normal map AD vs central differences, %s: |AD - mean| %.3e, floor %.3e, |mean| %.3e" % (which, dist, floor, np.linalg.norm(mean)))
    assert np.linalg.norm(mean) > 0 and floor > 0
    assert dist <= 3.0 * floor, (dist, floor)


# ---------------------------------------------------------------- 6. surface, loader, errors
def test_python_class():
    b = psdr_cuda.MicrofacetBSDF(0.05, (0.5, 0.4, 0.3), 0.25)
    assert b.normal_map is None
    c = psdr_cuda.MicrofacetBSDF(0.05, (0.5, 0.4, 0.3), 0.25, (0.5, 0.6, 0.9))
    assert isinstance(c.normal_map, psdr_cuda.Bitmap3fD) and np.allclose(c.normal_map.tensor().cpu().numpy(), [[0.5, 0.6, 0.9]])
    bm = psdr_cuda.Bitmap3fD(FLAT)
    assert psdr_cuda.MicrofacetBSDF(normal_map=bm).normal_map is bm
    assert c.type_name() == "MicrofacetBSDF" and c.anisotropic() is False


def test_loader_record_and_mask():
    """<bsdf type="microfacet"> with a child normalMap / normal_map, as a constant rgb and as a bitmap texture; without the child: no map.  The records and masks
    tables() emits: type 2 / bit 2 without a map, as before; with one, type 3 / bit 3, the three slots of type 2 unchanged and the map's (offset, w, h) in
    PSDR_SLOT_K.  param_map reaches the map."""
    tex = lean_texel()
    sc = scene(uv_quad_xml(normal_xml(0.3, tex)), RES, SPP)
    sc2 = scene(uv_quad_xml(normal_xml(0.3, tex, name="normal_map")), RES, SPP)
    plain = scene(uv_quad_xml(microfacet_xml(0.3)), RES, SPP)
    tb, tb2, tbp = sc.tables(0), sc2.tables(0), plain.tables(0)
    assert tbp["material_mask"] == 4 and tb["material_mask"] == 1 << _abi.BSDF_MICROFACET_NORMAL == 8
    assert plain.param_map["BSDF[id=m]"].normal_map is None
    assert np.array_equal(tb["bsdf_rec"].cpu().numpy(), tb2["bsdf_rec"].cpu().numpy()) and np.array_equal(tb["texels"].cpu().numpy(), tb2["texels"].cpu().numpy())
    row, off = record(tb, "normal")
    rowp, offp = record(tbp, "plain")
    assert row[0] == 3 and rowp[0] == 2 and list(row[1:13]) == list(rowp[1:13]) and list(rowp[13:16]) == [0, 1, 1]
    assert list(row[13:16]) == [off["normal"], 1, 1]
    texels = tb["texels"].cpu().numpy()
    assert np.allclose(texels[off["normal"]:off["normal"] + 3], tex) and np.array_equal(texels[:off["normal"]], tbp["texels"].cpu().numpy()[:off["normal"]])
    b = sc.param_map["BSDF[id=m]"]
    assert isinstance(b, psdr_cuda.MicrofacetBSDF) and isinstance(b.normal_map, psdr_cuda.Bitmap3fD) and sc.param_map["BSDF[0]"].normal_map is b.normal_map
    # a bitmap texture
    bmp = normal_xml(0.3).replace('<rgb name="normalMap" value="0.5, 0.5, 1"/>',
                                  '<texture name="normalMap" type="bitmap"><string name="filename" value="./data/textures/test_texture.exr"/></texture>')
    assert "texture" in bmp
    sb = scene(uv_quad_xml(bmp), RES, SPP)
    w, h = sb.param_map["BSDF[id=m]"].normal_map.resolution
    assert w > 1 and h > 1
    rowb, _ = record(sb.tables(0), "normal")
    assert list(rowb[14:16]) == [w, h]
    # requires_grad / the torch graph reaches the map: the texel pool's gradient lands in the bitmap's tensor
    ek.set_requires_gradient(b.normal_map.data)
    sc.configure()
    pool = sc.tables(0)["texels"]
    assert pool.requires_grad
    pool[off["normal"]:off["normal"] + 3].sum().backward()
    g = b.normal_map.data.t.grad
    assert g is not None and np.allclose(g.cpu().numpy(), 1.0)


def test_refusals():
    """DirectIntegrator and PathTracer keep raising the MicrofacetBSDF message for a normal-mapped record; a mesh without texture coordinates under a normal map
    raises the new message before any native call, from every integrator's entry -- bunny_light as it is: bunny_low.obj has no texture coordinates."""
    sc = scene(uv_quad_xml(normal_xml(0.3, lean_texel())), RES, SPP)
    direct, path = psdr_cuda.DirectIntegrator(1, 1), psdr_cuda.PathTracer(3, True)
    for call in (lambda: direct.renderC(sc), lambda: direct.renderD(sc), lambda: direct.preprocess_secondary_edges(sc, 0, [2, 2, 2, 1]),
                 lambda: path.renderC(sc), lambda: path.renderD(sc), lambda: path.preprocess_path_secondary_edges(sc, 0, [2, 2, 2, 1])):
        with pytest.raises(RuntimeError, match=MESSAGE):
            call()
    psdr_cuda.CollocatedIntegrator(1.0)._check_bsdfs(sc)
    bare = scene(bunny_xml("plain").replace("</bsdf>", '<rgb name="normalMap" value="0.5, 0.5, 1"/></bsdf>', 1), RES, SPP)
    assert bare.tables(0)["tri_uv"] is None and bare.tables(0)["material_mask"] & 8
    colloc = psdr_cuda.CollocatedIntegrator(1.0)
    for call in (lambda: colloc.renderC(bare), lambda: colloc.renderD(bare)):
        with pytest.raises(RuntimeError, match=KINDS["normal"].needs_uv):
            call()
    with pytest.raises(RuntimeError, match=MESSAGE):          # the older message first, as the C ABI orders them
        direct.renderC(bare)


# ---------------------------------------------------------------- 7. the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers(tmp_path):
    """tests/hostcheck/colloc_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_collocated.cpp, built with
    -fsanitize=address,undefined for the host (hostlibs.san_program) and asked for a record of type BSDF_MICROFACET_NORMAL:
    render, forward and reverse on the tiny scene of the four record types; it must end clean and report what the
    library reports."""
    exe = san_program("colloc_san", HC_DEPS)
    res, spp, sppe = 8, 2, 2
    tb = scene(mixed_xml(MIXED_IDS), res, spp, sppe, textured=True, normal="random", uv="rot37").tables(0)
    o = colloc_opts(spp, sppe, rng_offset=(1, 2, 0))
    tan = random_tangents(tb, ["tri_info", "texels", "prim_edge"], seed=3)
    adj = np.random.default_rng(4).random((res * res, 3)).astype(np.float32)
    tbc, desc, keep = cpu_desc(tb)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in ("tri_info", "texels", "prim_edge")], adj)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path, str(_abi.BSDF_MICROFACET_NORMAL)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan, nthreads=2)
    _, grads = host_colloc_rev(tb, o, adj, want=["tri_info", "texels", "prim_edge"])
    want = [np.abs(host_colloc_render(tb, o, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + [np.abs(grads[n].astype(np.float64)).sum() for n in ("tri_info", "texels", "prim_edge")]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
