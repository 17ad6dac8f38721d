"""MicrofacetBSDF (csrc/psdr_colloc_microfacet.h, DESIGN.md section 14: Lambertian diffuse + GGX specular with a Schlick Fresnel term, evaluated by the
CollocatedIntegrator) on the HOST: the product's PSDR_HD functions run slot by slot by tests/hostcheck/hostcheck_collocated.cpp.  The model is build-defined and
the oracle is not extended, so it is pinned on its closed form written out in float64, on its two limits against the project's DiffuseBSDF and
RoughConductorBSDF, on forward = reverse and on AD against central differences of the harness' own renderC."""
import os
import subprocess

import numpy as np
import pytest

import psdr_cuda
from collocated_helpers import HC_DEPS, ROUGH, colloc_opts, host_colloc_render, host_colloc_rev, host_film_samples, xml_scene
from colloc_microfacet_helpers import (F0, KD, MESSAGE, bunny_xml, closed_form_image, diffuse_xml, microfacet_xml, mixed_xml, record, room_xml,
                                       scene, uv_quad_xml)
from helpers import dot_tables, host_render, random_tangents, rel_l2
from hostlibs import cpu_desc, san_program, write_tables_file
from psdr_cuda import _abi

RES, SPP = 16, 4
TILTS, ROUGHNESS = (0.0, 30.0, 70.0), (0.3, 0.6)
MIXED_IDS = ("d", "c", "m")          # the quads of mixed_xml: record types 0 .. 2


# ---------------------------------------------------------------- 1. closed form
@pytest.mark.parametrize("textured", [False, True], ids=["1x1", "4x4"])
@pytest.mark.parametrize("r", ROUGHNESS)
@pytest.mark.parametrize("tilt", TILTS)
def test_closed_form(tilt, r, textured):
    """The tilted quad: the harness' renderC against kd / pi cos + F0 D(wi) G1(wi)^2 / (4 cos), all over d^2, written out in float64 numpy at the harness' own
    film samples (hit, frame, uv and distance from the float64 tables; 4 x 4 maps: bilinear lookups in float64 too).  Bound 2e-6 image rel-L2, the bound of
    test_collocated_host.py::test_rough_conductor_retro_reflection for the same arithmetic.  Measured: 6.9e-8 .. 1.6e-7 with 1 x 1 maps, 1.8e-7 .. 6.2e-7 with
    4 x 4 maps (largest at 70 degrees)."""
    sc = scene(uv_quad_xml(microfacet_xml(r), tilt), RES, SPP, textured=textured, r=r)
    tb = sc.tables(0)
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(tb, o)
    ref = closed_form_image(tb, host_film_samples(tb, o), SPP, "plain")
    assert (ref > 0).any() and (ref == 0).any()          # the quad and the background are both seen
    e = rel_l2(img, ref)
    print("microfacet closed form tilt %g r %g %s: rel-L2 %.2e" % (tilt, r, "4x4" if textured else "1x1", e))
    assert e <= 2e-6, e


# ---------------------------------------------------------------- 2. limits against existing code
@pytest.mark.parametrize("tilt", TILTS)
def test_limit_no_specular_is_the_diffuse_bsdf(tilt):
    """F0 = 0: the image equals the DiffuseBSDF render of the same kd to 1e-6 rel-L2."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(scene(uv_quad_xml(microfacet_xml(0.3, f0=(0, 0, 0)), tilt), RES, SPP).tables(0), o)
    ref = host_colloc_render(scene(uv_quad_xml(diffuse_xml(), tilt), RES, SPP).tables(0), o)
    assert ref.max() > 0
    assert rel_l2(img, ref) <= 1e-6, rel_l2(img, ref)


def _conductor_fresnel_normal(eta, k):
    """the conductor Fresnel term at cos = 1 in float64 (the reference's fresnel_conductor, utils.h, at normal incidence: ((eta - 1)^2 + k^2) / ((eta + 1)^2 + k^2))"""
    eta, k = np.asarray(eta, np.float64), np.asarray(k, np.float64)
    return ((eta - 1) ** 2 + k ** 2) / ((eta + 1) ** 2 + k ** 2)


MEASURED_KD0 = 7.1e-8          # the largest of the six cases below, measured on the host


@pytest.mark.parametrize("r", ROUGHNESS)
@pytest.mark.parametrize("tilt", TILTS)
def test_limit_no_diffuse_is_the_rough_conductor(tilt, r):
    """kd = 0: the image equals the RoughConductorBSDF render with alpha_u = alpha_v = r^2 and specular_reflectance = 1, times F0 / F_c per channel, F_c the
    conductor's Fresnel term at normal incidence in float64 from its eta and k.  Bound max(2e-6, 4 x measured) = 2e-6.
    Measured on the host (rel-L2), tilt 0 / 30 / 70: r = 0.3: 5.44e-8, 5.48e-8, 7.04e-8; r = 0.6: 5.56e-8, 5.47e-8, 6.58e-8 -- the two BSDFs run the same GGX
    arithmetic, what differs is the rounding of the Fresnel factor."""
    eta, k = (0.2, 0.92, 1.1), (3.9, 2.45, 2.14)
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    img = host_colloc_render(scene(uv_quad_xml(microfacet_xml(r, kd=(0, 0, 0)), tilt), RES, SPP).tables(0), o)

    def prepare(sc):
        a = float(np.float32(r) * np.float32(r))
        sc.m_bsdfs[0].alpha_u.fill(a); sc.m_bsdfs[0].alpha_v.fill(a)
    cond = host_colloc_render(xml_scene(uv_quad_xml(ROUGH % (r * r), tilt), RES, SPP, prepare=prepare).tables(0), o)
    ref = cond.astype(np.float64) * (np.asarray(F0, np.float32).astype(np.float64) / _conductor_fresnel_normal(np.float32(eta), np.float32(k)))[None, :]
    assert ref.max() > 0
    e = rel_l2(img, ref)
    print("microfacet kd = 0 against the rough conductor, tilt %g r %g: rel-L2 %.2e" % (tilt, r, e))
    assert e <= max(2e-6, 4 * MEASURED_KD0), e


# ---------------------------------------------------------------- 3. forward = reverse
def _fwd_rev_scene(name, res, spp, sppe):
    xml = {"quad": uv_quad_xml(microfacet_xml(0.3), 30.0), "room": room_xml("plain"), "bunny": bunny_xml("plain")}[name]
    return scene(xml, res, spp, sppe, textured=True)


@pytest.mark.parametrize("name", ["quad", "room", "bunny"])
def test_forward_equals_reverse(name):
    """<adj, J t> = <J^T adj, t> with random tangents and a random adjoint image for the texels (kd, F0 and roughness maps at 4 x 4), the triangle rows, the
    camera pose and the primary-edge rows; on the quad, on cbox_uv with a microfacet floor (no tree) and on bunny_light with a microfacet bunny (one tree).
    |lhs - rhs| <= 1e-4 x scale, as test_collocated_host.py::test_forward_equals_reverse."""
    res, spp, sppe = 16, 4, 4
    tb = _fwd_rev_scene(name, res, spp, sppe).tables(0)
    assert tb["material_mask"] & (1 << _abi.BSDF_MICROFACET)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    _, off = record(tb, "plain")
    for n in ("texels", "tri_info", "cam_to_world", "prim_edge"):
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan)
        img_r, grads = host_colloc_rev(tb, o, adj, want=[n])
        assert rel_l2(img_r, img) < 1e-6
        lhs, rhs = float((adj.astype(np.float64) * dimg).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg).sum())
        assert scale > 0, n
        print("microfacet forward = reverse, %s %s: lhs %.6e rhs %.6e scale %.3e" % (name, n, lhs, rhs, scale))
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        if n == "texels":          # each of the three maps receives a gradient
            for key, width in (("kd", 48), ("f0", 48), ("roughness", 16)):
                assert np.abs(grads["texels"][off[key]:off[key] + width]).max() > 0, key


# ---------------------------------------------------------------- 4. AD against central differences
@pytest.mark.parametrize("which", ["roughness", "kd", "f0"])
def test_ad_against_central_differences(which):
    """d image / d (one texel of a 4 x 4 map) in forward mode against the central difference of the harness' own renderC at two steps, relative 1e-2 and 2e-2, on
    the same streams (nothing sampled depends on a material parameter).  floor = distance of the two differences; AD must lie within 3 x floor of their mean.
    Measured, image L2 norms (|AD - mean|, floor, |mean|): roughness 1.085e-11, 2.226e-11, 3.950e-8; kd 2.601e-12, 4.820e-12, 6.125e-7; F0 3.212e-11, 5.745e-11,
    2.572e-8.  kd and F0 enter linearly: their floor is fp32 rounding over the step; the roughness floor is the differences' third-order term."""
    tb = scene(uv_quad_xml(microfacet_xml(0.3), 30.0), RES, SPP, textured=True).tables(0)
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    _, off = record(tb, "plain")
    i = off[which] + (5 if which == "roughness" else 3 * 5 + 1)          # texel (1, 1), an inner one; the green channel
    base = tb["texels"].detach().clone()
    v0 = float(base[i])

    def render(delta):
        t = dict(tb)
        t["texels"] = base.clone()
        t["texels"][i] = v0 + delta
        return host_colloc_render(t, o).astype(np.float64)
    fds = [(render(+h) - render(-h)) / (2.0 * h) for h in (1e-2 * v0, 2e-2 * v0)]
    floor, mean = float(np.linalg.norm(fds[0] - fds[1])), (fds[0] + fds[1]) / 2.0
    tan = base.clone().zero_()
    tan[i] = 1.0
    ad = host_colloc_render(tb, o, mode=1, tangents={"texels": tan})[1].astype(np.float64)
    dist = float(np.linalg.norm(ad - mean))
    print("microfacet AD vs central differences, %s texel: |AD - mean| %.3e, floor %.3e, |mean| %.3e" % (which, dist, floor, np.linalg.norm(mean)))
    assert np.linalg.norm(mean) > 0 and floor > 0
    assert dist <= 3.0 * floor, (dist, floor)


# ---------------------------------------------------------------- 5. mixed scene
def test_mixed_scene_dispatches_per_mesh():
    """A diffuse, a rough-conductor and a microfacet quad in one scene: each mesh's pixels equal those of the scene that holds that mesh alone, bit for bit."""
    o = colloc_opts(SPP, rng_offset=(5, 0, 0))
    mixed = host_colloc_render(scene(mixed_xml(MIXED_IDS), RES, SPP, textured=True).tables(0), o)
    covered = np.zeros(len(mixed), bool)
    solos = {}
    for bid in ("d", "c", "m"):
        solo = host_colloc_render(scene(mixed_xml(MIXED_IDS, only=bid), RES, SPP, textured=True).tables(0), o)
        px = (solo != 0).any(axis=1)
        assert px.sum() >= 4 and not (covered & px).any(), bid          # the three quads cover separate pixels
        assert np.array_equal(mixed[px], solo[px]), bid
        covered |= px
        solos[bid] = solo[px].mean(axis=0)
    assert (mixed[~covered] == 0).all()
    assert not np.allclose(solos["d"], solos["m"]) and not np.allclose(solos["c"], solos["m"])          # three different materials


# ---------------------------------------------------------------- 6. degenerate input
def test_zero_roughness_texel_stays_finite():
    """A 4 x 4 roughness map with one texel at 0 (alpha = 0 at that texel's centre: GGX::eval's cut-off answers 0 there and the value is the diffuse lobe; next to
    it the lobe is a narrow, finite spike): image, derivative image and every gradient table stay finite."""
    res, spp, sppe = 16, 4, 4
    tb = scene(uv_quad_xml(microfacet_xml(0.3), 0.0), res, spp, sppe, textured=True, zero_roughness_texel=5).tables(0)
    _, off = record(tb, "plain")
    assert float(tb["texels"][off["roughness"] + 5]) == 0.0
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    names = ["texels", "tri_info", "cam_to_world", "prim_edge"]
    tan = random_tangents(tb, names, seed=1)
    img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    img_r, grads = host_colloc_rev(tb, o, adj, want=names)
    assert np.isfinite(img).all() and np.isfinite(dimg).all() and np.isfinite(img_r).all() and img.max() > 0
    for n in names:
        assert np.isfinite(grads[n]).all(), n
    # the value at alpha = 0 exactly: a 1 x 1 roughness of 0 renders the diffuse lobe alone
    o1 = colloc_opts(SPP, rng_offset=(5, 0, 0))
    zero = host_colloc_render(scene(uv_quad_xml(microfacet_xml(0.0), 30.0), RES, SPP).tables(0), o1)
    diff = host_colloc_render(scene(uv_quad_xml(diffuse_xml(), 30.0), RES, SPP).tables(0), o1)
    assert diff.max() > 0 and rel_l2(zero, diff) <= 1e-6


# ---------------------------------------------------------------- 7. surface, loader, errors
def test_python_class():
    b = psdr_cuda.MicrofacetBSDF(0.05, (0.5, 0.4, 0.3), 0.25)
    assert b.type_name() == "MicrofacetBSDF" and b.anisotropic() is False
    b.id = "x"
    assert b.to_string() == "MicrofacetBSDF[id=x]"
    assert np.allclose(b.specular_reflectance.tensor().cpu().numpy(), 0.05) and np.allclose(b.diffuse_reflectance.tensor().cpu().numpy(), [[0.5, 0.4, 0.3]])
    assert np.allclose(b.roughness.tensor().cpu().numpy(), 0.25)
    d = psdr_cuda.MicrofacetBSDF()
    assert np.allclose(d.specular_reflectance.tensor().cpu().numpy(), 0.04) and np.allclose(d.diffuse_reflectance.tensor().cpu().numpy(), 0.5)
    assert np.allclose(d.roughness.tensor().cpu().numpy(), 0.5)
    bm = psdr_cuda.Bitmap1fD(0.7)
    assert psdr_cuda.MicrofacetBSDF(roughness=bm).roughness is bm


def test_loader_record_and_mask():
    """<bsdf type="microfacet">: camel-case and snake-case children give the same record; a missing child takes the constructor's default; the record's slots and
    the mask's bit 2 are as include/psdr_hip.h documents them; param_map names the BSDF."""
    sc = scene(uv_quad_xml(microfacet_xml(0.3)), RES, SPP)
    snake = microfacet_xml(0.3).replace("diffuseReflectance", "diffuse_reflectance").replace("specularReflectance", "specular_reflectance")
    assert "diffuse_reflectance" in snake and "specular_reflectance" in snake
    sc2 = scene(uv_quad_xml(snake), RES, SPP)
    tb, tb2 = sc.tables(0), sc2.tables(0)
    assert tb["material_mask"] == 1 << _abi.BSDF_MICROFACET == 4
    row, off = record(tb, "plain")
    assert np.array_equal(tb["bsdf_rec"].cpu().numpy(), tb2["bsdf_rec"].cpu().numpy()) and np.array_equal(tb["texels"].cpu().numpy(), tb2["texels"].cpu().numpy())
    tex = tb["texels"].cpu().numpy()
    assert np.allclose(tex[off["kd"]:off["kd"] + 3], KD) and np.allclose(tex[off["f0"]:off["f0"] + 3], F0) and np.isclose(tex[off["roughness"]], 0.3)
    assert row[0] == 2 and list(row[1 + 3 * _abi.SLOT_ALPHA_V:4 + 3 * _abi.SLOT_ALPHA_V]) == [0, 1, 1] and list(row[1 + 3 * _abi.SLOT_K:4 + 3 * _abi.SLOT_K]) == [0, 1, 1]
    b = sc.param_map["BSDF[id=m]"]
    assert isinstance(b, psdr_cuda.MicrofacetBSDF) and sc.param_map["BSDF[0]"] is b
    bare = scene(uv_quad_xml('<bsdf id="m" type="microfacet"><float name="roughness" value="0.2"/></bsdf>\n'), RES, SPP)
    bb = bare.param_map["BSDF[id=m]"]
    assert np.allclose(bb.diffuse_reflectance.tensor().cpu().numpy(), 0.5) and np.allclose(bb.specular_reflectance.tensor().cpu().numpy(), 0.04)
    assert np.allclose(bb.roughness.tensor().cpu().numpy(), 0.2)
    none = scene(uv_quad_xml('<bsdf id="m" type="microfacet"/>\n'), RES, SPP)
    assert np.allclose(none.param_map["BSDF[id=m]"].roughness.tensor().cpu().numpy(), 0.5)
    with pytest.raises(RuntimeError, match="Unsupported BSDF"):
        scene(uv_quad_xml('<bsdf id="m" type="plastic"/>\n'), RES, SPP)


def test_sampling_integrators_refuse_the_scene():
    """DirectIntegrator and PathTracer raise before any native call -- renderC, renderD and the preprocess methods; the FieldExtractionIntegrator evaluates no BSDF:
    its check passes and the general harness renders a field from the microfacet tables."""
    sc = scene(uv_quad_xml(microfacet_xml(0.3)), RES, SPP)
    direct, path = psdr_cuda.DirectIntegrator(1, 1), psdr_cuda.PathTracer(3, True)
    for call in (lambda: direct.renderC(sc), lambda: direct.renderD(sc), lambda: direct.preprocess_secondary_edges(sc, 0, [2, 2, 2, 1]),
                 lambda: path.renderC(sc), lambda: path.renderD(sc), lambda: path.preprocess_path_secondary_edges(sc, 0, [2, 2, 2, 1])):
        with pytest.raises(RuntimeError, match=MESSAGE):
            call()
    psdr_cuda.FieldExtractionIntegrator("depth")._check_bsdfs(sc)
    psdr_cuda.CollocatedIntegrator(1.0)._check_bsdfs(sc)
    tb = sc.tables(0)
    depth = host_render(tb, _abi.make_opts(integrator=_abi.INTEGRATOR_FIELD, field=_abi.FIELDS["depth"], spp=SPP))
    assert np.isfinite(depth).all() and depth.max() > 900          # the quad is 1000 away


# ---------------------------------------------------------------- 8. the same host functions under the sanitizers
def test_host_functions_run_clean_under_the_sanitizers(tmp_path):
    """tests/hostcheck/colloc_san.cpp: a stand-alone program (its own main, no Python) over hostcheck_collocated.cpp, built with
    -fsanitize=address,undefined for the host (hostlibs.san_program) and asked for a record of type BSDF_MICROFACET:
    render, forward and reverse on the tiny mixed scene; it must end clean and report what the library reports."""
    exe = san_program("colloc_san", HC_DEPS)
    res, spp, sppe = 8, 2, 2
    tb = scene(mixed_xml(MIXED_IDS), res, spp, sppe, textured=True).tables(0)
    o = colloc_opts(spp, sppe, rng_offset=(1, 2, 0))
    tan = random_tangents(tb, ["tri_info", "texels", "prim_edge"], seed=3)
    adj = np.random.default_rng(4).random((res * res, 3)).astype(np.float32)
    tbc, desc, keep = cpu_desc(tb)
    path = str(tmp_path / "tables.bin")
    write_tables_file(path, desc, keep, o, *[tan[n].detach().cpu().numpy().astype(np.float32) for n in ("tri_info", "texels", "prim_edge")], adj)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path, str(_abi.BSDF_MICROFACET)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-3000:])
    got = [float(x) for x in r.stdout.split()]
    img, dimg = host_colloc_render(tb, o, mode=1, tangents=tan, nthreads=2)
    _, grads = host_colloc_rev(tb, o, adj, want=["tri_info", "texels", "prim_edge"])
    want = [np.abs(host_colloc_render(tb, o, nthreads=2).astype(np.float64)).sum(), np.abs(dimg.astype(np.float64)).sum()] + [np.abs(grads[n].astype(np.float64)).sum() for n in ("tri_info", "texels", "prim_edge")]
    assert all(w > 0 for w in want), want
    assert np.allclose(got, want, rtol=1e-5), (got, want)          # (-O1 against -O2: the last bits of a float sum may differ)
