"""MicrofacetBSDF on the GPU (csrc/psdr_colloc_microfacet.h inside the rough flag sets of csrc/psdr_collocated.hip), through the C ABI and the Python surface,
against the host harness that runs the same functions (tests/test_colloc_microfacet_host.py pins that one on the closed form, the two limits and AD against
central differences)."""
import ctypes as C

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import colloc_opts, host_colloc_render, host_colloc_rev
from colloc_microfacet_helpers import MESSAGE, bunny_xml, microfacet_xml, mixed_xml, record, room_xml, scene, uv_quad_xml
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import GpuScene, dot_tables, isolated_pixels_unbiased, random_tangents, rel_l2
from psdr_cuda import _abi

pytestmark = pytest.mark.gpu
MIXED_IDS = ("d", "c", "m")          # the quads of mixed_xml: record types 0 .. 2


def _xml(name):
    return {"quad": uv_quad_xml(microfacet_xml(0.3), 30.0), "room": room_xml("plain"), "bunny": bunny_xml("plain"), "mixed": mixed_xml(MIXED_IDS)}[name]


@pytest.mark.parametrize("name,tree", [("quad", False), ("room", False), ("bunny", True), ("mixed", False)])
def test_render_c_matches_the_harness(name, tree):
    """renderC against the host run of the same code, 4 x 4 maps: the quad, cbox_uv with a microfacet floor (kernel-argument primitives), bunny_light with a
    microfacet bunny (a tree) and the scene that mixes the three BSDF types.  Bounds of test_collocated_gpu.py::test_render_c_matches_the_harness: rel-L2 < 1e-4,
    on the tree scene outside isolated silhouette pixels (at most 0.5 % of the pixels, held to helpers.isolated_pixels_unbiased).  19 x 19 x 3: a partly filled
    last workgroup and the atomic splat; 32 x 32 x 16: the plain-store path."""
    for res, spp in ((19, 3), (32, 16)):
        tb = scene(_xml(name), res, spp, textured=True).tables(0)
        o = colloc_opts(spp, rng_offset=(7, 0, 0))
        ref = host_colloc_render(tb, o)
        g = GpuScene(tb)
        img = g.render_c(o)
        assert np.isfinite(img).all() and ref.max() > 0
        assert g.counters()[0] == res * res * spp          # one ray per sample
        bad = np.abs(img - ref).max(axis=1) > 1e-3 * (1 + np.abs(ref).max(axis=1)) if tree else np.zeros(len(ref), bool)
        print("microfacet %s %dx%dx%d: rel-L2 %.2e, isolated pixels %d" % (name, res, res, spp, rel_l2(img[~bad], ref[~bad]), bad.sum()))
        assert bad.mean() <= 5e-3, bad.mean()
        assert rel_l2(img[~bad], ref[~bad]) < 1e-4, rel_l2(img[~bad], ref[~bad])
        isolated_pixels_unbiased(img, ref, bad, name)


def _map_sets(tb):
    """one tangent set per map of the MicrofacetBSDF: random tangents on the 4 x 4 kd, F0 and roughness texels, zero elsewhere"""
    _, off = record(tb, "plain")
    rnd = random_tangents(tb, ["texels"], seed=2)["texels"]
    sets = []
    for key, width in (("kd", 48), ("f0", 48), ("roughness", 16)):
        t = torch.zeros_like(rnd)
        t[off[key]:off[key] + width] = rnd[off[key]:off[key] + width]
        sets.append({"texels": t})
    return sets


def test_forward_mode_matches_the_harness():
    """Forward mode against the host run: material duals on each of the three maps (the quad, K = 1 and all three as one K = 3 launch), geometry duals with the
    primary-edge kernel (the room with a microfacet floor: triangle rows, camera pose and edge rows at once, K = 1 and K = 3).  Bounds of
    test_collocated_gpu.py::test_forward_mode_matches_the_harness: 1e-4, 1e-3 for a geometry derivative image, K = 3 columns to 1e-6 / 1e-5."""
    tb = scene(_xml("quad"), 24, 8, textured=True).tables(0)
    o = colloc_opts(8, rng_offset=(3, 0, 0))
    g = GpuScene(tb)
    sets, cols = _map_sets(tb), []
    for ts in sets:
        ref_img, ref_d = host_colloc_render(tb, o, mode=1, tangents=ts)
        img, d = g.render_d_fwd(o, [ts])
        assert np.abs(ref_d).max() > 0
        assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-4, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))
        cols.append(d[0])
    _, d3 = g.render_d_fwd(o, sets)
    assert all(rel_l2(d3[k], cols[k]) < 1e-6 for k in range(3)), [rel_l2(d3[k], cols[k]) for k in range(3)]
    tb2 = scene(_xml("room"), 24, 8, 8, textured=True).tables(0)
    o2 = colloc_opts(8, 8, rng_offset=(3, 4, 0))
    tan = random_tangents(tb2, ["tri_info", "cam_to_world", "prim_edge"], seed=4)
    ref_img, ref_d = host_colloc_render(tb2, o2, mode=1, tangents=tan)
    g2 = GpuScene(tb2)
    img, d = g2.render_d_fwd(o2, [tan])
    assert np.abs(ref_d).max() > 0
    assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-3, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))
    still = {k: torch.zeros_like(v) for k, v in tan.items()}
    _, d3 = g2.render_d_fwd(o2, [tan, still, tan])
    assert rel_l2(d3[0], d[0]) < 1e-5 and rel_l2(d3[2], d[0]) < 1e-5 and np.abs(d3[1]).max() == 0, (rel_l2(d3[0], d[0]), np.abs(d3[1]).max())


@pytest.mark.parametrize("name", ["quad", "room", "bunny"])
def test_reverse_equals_forward(name):
    """<adj, J t> = <J^T adj, t> on the GPU for the texels (three 4 x 4 maps), the triangle rows, the camera pose and the primary-edge rows, and the reverse
    launch's gradient tables against the host's, table by table (bounds of test_collocated_gpu.py::test_reverse_equals_forward)."""
    res, spp, sppe = 16, 4, 4
    tb = scene(_xml(name), res, spp, sppe, textured=True).tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    g = GpuScene(tb)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge"]
    img_r, grads = g.render_d_rev(o, adj, want=names)
    _, host_grads = host_colloc_rev(tb, o, adj, want=names)
    _, off = record(tb, "plain")
    for key, width in (("kd", 48), ("f0", 48), ("roughness", 16)):
        assert np.abs(grads["texels"][off[key]:off[key] + width]).max() > 0, key
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = g.render_d_fwd(o, [tan])
        assert rel_l2(img_r, img) < 1e-5
        lhs, rhs = float((adj.astype(np.float64) * dimg[0]).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        assert rel_l2(grads[n], host_grads[n]) < (1e-3 if name == "bunny" else 1e-4), (n, rel_l2(grads[n], host_grads[n]))
    _, gm = g.render_d_rev(o, adj, want=["texels"])          # material-only launch: the same texel gradient
    assert rel_l2(gm["texels"], grads["texels"]) < 1e-5


def test_python_surface():
    """CollocatedIntegrator.renderD + enoki.backward on a microfacet scene: a gradient on each of the three maps and on m_intensity, equal to the C ABI's reverse
    call with the scaled adjoint image."""
    inten = [2.0, 1.0, 0.5]
    sc = scene(_xml("quad"), 16, 4, 4, textured=True)
    b = sc.param_map["BSDF[id=m]"]
    maps = (b.diffuse_reflectance.data, b.specular_reflectance.data, b.roughness.data)
    for m in maps:
        ek.set_requires_gradient(m)
    I = Vector3fD(inten)
    ek.set_requires_gradient(I)
    sc.configure()
    img = psdr_cuda.CollocatedIntegrator(I).renderD(sc)
    target = torch.full_like(img.t, 1e-7)
    ek.backward(FloatD._wrap(((img.t - target) ** 2).sum().reshape(1)))
    adj = (2.0 * (img.t - target)).detach().cpu().numpy()
    tb = sc.tables(0)
    o = colloc_opts(4, 4)
    g = GpuScene(tb)
    unit = g.render_c(colloc_opts(4))
    gI = ek.gradient(I).numpy().reshape(3)
    want_I = (adj.astype(np.float64) * unit).sum(axis=0)
    assert np.abs(want_I).min() > 0 and np.allclose(gI, want_I, rtol=1e-4), (gI, want_I)
    _, cg = g.render_d_rev(o, adj * np.array(inten, np.float32), want=["texels"])
    _, off = record(tb, "plain")
    for m, key in zip(maps, ("kd", "f0", "roughness")):
        got = ek.gradient(m).numpy().reshape(-1)
        want = cg["texels"][off[key]:off[key] + got.size]
        assert np.isfinite(got).all() and np.abs(want).max() > 0, key
        assert rel_l2(got, want) < 1e-4, (key, rel_l2(got, want))


def test_two_spp_shards_sum_to_the_whole():
    tb = scene(_xml("mixed"), 24, 8, 8, textured=True).tables(0)
    g = GpuScene(tb)
    full = g.render_c(colloc_opts(8, rng_offset=(1, 0, 0)))
    parts = sum(g.render_c(colloc_opts(8, rng_offset=(1, 0, 0), spp_range=r)).astype(np.float64) for r in ((0, 3), (3, 8)))
    assert full.max() > 0 and rel_l2(parts, full) < 1e-6, rel_l2(parts, full)
    tan = random_tangents(tb, ["texels", "tri_info", "prim_edge"], seed=2)
    _, dfull = g.render_d_fwd(colloc_opts(8, 8, rng_offset=(1, 2, 0)), [tan])
    dparts = sum(g.render_d_fwd(colloc_opts(8, 8, rng_offset=(1, 2, 0), spp_range=r, sppe_range=r), [tan])[1][0].astype(np.float64) for r in ((0, 3), (3, 8)))
    assert rel_l2(dparts, dfull[0]) < 1e-6, rel_l2(dparts, dfull[0])


def test_error_returns():
    """DirectIntegrator / PathTracer entry points of the C ABI on a microfacet scene: an error return before any launch, psdr_last_error names the reason.  The
    FieldExtractionIntegrator renders; so does the CollocatedIntegrator afterwards (the handle is intact)."""
    light = '<ref id="m"/><emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter>'          # (an emitter, so that "No Emitter!" is not the answer)
    sc = scene(uv_quad_xml(microfacet_xml(0.3), 30.0).replace('<ref id="m"/>', light), 16, 4, 4)
    tb = sc.tables(0)
    assert tb["num_emitters"] == 1 and tb["material_mask"] == 4
    g = GpuScene(tb)
    adj = np.ones((16 * 16, 3), np.float32)
    tan = random_tangents(tb, ["texels"], seed=1)
    for kind, depth in ((_abi.INTEGRATOR_DIRECT, 1), (_abi.INTEGRATOR_PATH, 3)):
        o = _abi.make_opts(integrator=kind, max_depth=depth, spp=4, sppe=4, sppse=4)
        for call in (lambda: g.render_c(o), lambda: g.render_d_fwd(o, [tan]), lambda: g.render_d_rev(o, adj, want=["texels"]), lambda: g.guide_build(o, [2, 2, 2, 1], 1)):
            with pytest.raises(RuntimeError, match=MESSAGE):
                call()
    o = _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=3, spp=4, sppse=4)
    mass = torch.zeros(8, dtype=torch.float32, device="cuda")
    rc = g.lib.psdr_path_guide_build(g.h, C.byref(o), 1, (C.c_int32 * 4)(2, 2, 2, 1), 1, mass.data_ptr(), None)
    assert rc != 0 and MESSAGE in g.lib.psdr_last_error().decode()
    depth = g.render_c(_abi.make_opts(integrator=_abi.INTEGRATOR_FIELD, field=_abi.FIELDS["depth"], spp=4))
    assert np.isfinite(depth).all() and depth.max() > 900
    ref = host_colloc_render(tb, colloc_opts(4))
    assert rel_l2(g.render_c(colloc_opts(4)), ref) < 1e-4
    with pytest.raises(RuntimeError, match=MESSAGE):
        psdr_cuda.DirectIntegrator(1, 1).renderC(sc)


# ---------------------------------------------------------------- a small recovery
RECOVERY_TILTS = (0.0, 35.0, 65.0)


def _recovery_scene(tilt, spp, kd, rough):
    sc = scene(uv_quad_xml(microfacet_xml(0.4, f0=(0.08, 0.08, 0.08)), tilt), 32, spp)
    b = sc.param_map["BSDF[id=m]"]
    b.diffuse_reflectance.resolution = b.roughness.resolution = (4, 4)
    b.diffuse_reflectance.data, b.roughness.data = kd, rough
    return sc


def test_recover_albedo_and_roughness_maps():
    """The quad at 32 x 32 x 4 spp seen under three tilts (0 / 35 / 65 degrees), 4 x 4 kd and roughness maps started flat, F0 known; the target rendered at 64
    spp; 40 Adam steps on both maps.  Condition: the mean texel error of both maps ends below half of its start (the lobes separate by angle, the only noise is
    film jitter).  Measured at lr 0.05: kd 0.1507 -> 0.0259, roughness 0.0890 -> 0.0099 -- by the same loop over the host harness, whose figures at lr 0.03
    (0.0381, 0.0115) were the MI355X's to four digits; on the MI355X the test at lr 0.05 passed, its figures were not printed.  (At lr 0.03 the kd error ended at 0.0381, 1.98 x inside
    the bound: the step was too short for 40 iterations, so the step was lengthened; the problem and the bound are as stated.)"""
    rng = np.random.default_rng(11)
    kd_true = rng.uniform(0.2, 0.8, (16, 3)).astype(np.float32)
    r_true = rng.uniform(0.3, 0.6, 16).astype(np.float32)
    integ = psdr_cuda.CollocatedIntegrator(1e6)          # the quad is 1000 away: pixel values of order 0.1
    targets = []
    for tilt in RECOVERY_TILTS:
        ref = _recovery_scene(tilt, 64, Vector3fD(torch.from_numpy(kd_true)), FloatD(torch.from_numpy(r_true)))
        ref.configure()
        targets.append(integ.renderC(ref).torch().clone())
    kd = Vector3fD(torch.full((16, 3), 0.5))
    rough = FloatD(torch.full((16,), 0.45))
    ek.set_requires_gradient(kd)
    ek.set_requires_gradient(rough)
    scenes = [_recovery_scene(tilt, 4, kd, rough) for tilt in RECOVERY_TILTS]

    def errors():
        return float(np.abs(kd.numpy() - kd_true).mean()), float(np.abs(rough.numpy().reshape(-1) - r_true).mean())
    start = errors()
    opt = torch.optim.Adam([kd.t, rough.t], lr=0.05)
    for it in range(40):
        opt.zero_grad()
        for sc, target in zip(scenes, targets):
            sc.configure()
            img = integ.renderD(sc)
            ek.backward(ek.hmean(ek.hsum(ek.sqr(img - Vector3fD._wrap(target)))))
        opt.step()
        kd.t.data.clamp_(0.01, 0.99)
        rough.t.data.clamp_(0.05, 1.0)
    end = errors()
    print("microfacet recovery: mean texel error kd %.4f -> %.4f, roughness %.4f -> %.4f" % (start[0], end[0], start[1], end[1]))
    assert end[0] < 0.5 * start[0] and end[1] < 0.5 * start[1], (start, end)
