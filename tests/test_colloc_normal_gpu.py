"""MicrofacetBSDF with a tangent-space normal map on the GPU (record type PSDR_BSDF_MICROFACET_NORMAL, csrc/psdr_colloc_microfacet.h inside the rough flag sets of
csrc/psdr_collocated.hip), through the C ABI and the Python surface, against the host harness that runs the same functions
(tests/test_colloc_normal_host.py pins that one on the closed form, the limits, the degenerate inputs and AD against central differences)."""
import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import colloc_opts, host_colloc_render, host_colloc_rev
from colloc_microfacet_helpers import KINDS, MESSAGE, RECOVERY, lean_texel, map_words, mixed_xml, named_scene, normal_xml, record, scene, uv_quad_xml
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import GpuScene, dot_tables, isolated_pixels_unbiased, random_tangents, rel_l2
from psdr_cuda import _abi

pytestmark = pytest.mark.gpu
MIXED_IDS = ("d", "c", "m", "n")          # the quads of mixed_xml: record types 0 .. 3
R = RECOVERY["normal"]


def _scene(name, res, spp, sppe=0):
    """the scene forms of the host file's forward = reverse test (rotated-UV quad, room without a tree, bunny with one), the mirrored-UV quad and the scene of the
    four record types; 4 x 4 maps on every slot"""
    if name == "mirror":
        return scene(uv_quad_xml(normal_xml(0.3), 30.0), res, spp, sppe, uv="mirror", normal="random", textured=True)
    if name == "mixed":
        return scene(mixed_xml(MIXED_IDS), res, spp, sppe, uv="rot37", normal="random", textured=True)
    return named_scene("normal", name, res, spp, sppe)


@pytest.mark.parametrize("name,tree", [("quad", False), ("room", False), ("bunny", True), ("mirror", False)])
def test_render_c_matches_the_harness(name, tree):
    """renderC against the host run of the same code.  Bounds of test_colloc_microfacet_gpu.py::test_render_c_matches_the_harness: rel-L2 < 1e-4, on the tree scene
    outside isolated silhouette pixels (at most 0.5 % of the pixels, held to helpers.isolated_pixels_unbiased).  19 x 19 x 3: a partly filled last workgroup and
    the atomic splat; 32 x 32 x 16: the plain-store path."""
    for res, spp in ((19, 3), (32, 16)):
        tb = _scene(name, res, spp).tables(0)
        assert tb["material_mask"] & (1 << _abi.BSDF_MICROFACET_NORMAL)
        o = colloc_opts(spp, rng_offset=(7, 0, 0))
        ref = host_colloc_render(tb, o)
        g = GpuScene(tb)
        img = g.render_c(o)
        assert np.isfinite(img).all() and ref.max() > 0
        assert g.counters()[0] == res * res * spp          # one ray per sample
        bad = np.abs(img - ref).max(axis=1) > 1e-3 * (1 + np.abs(ref).max(axis=1)) if tree else np.zeros(len(ref), bool)
        print("normal map %s %dx%dx%d: rel-L2 %.2e, isolated pixels %d" % (name, res, res, spp, rel_l2(img[~bad], ref[~bad]), bad.sum()))
        assert bad.mean() <= 5e-3, bad.mean()
        assert rel_l2(img[~bad], ref[~bad]) < 1e-4, rel_l2(img[~bad], ref[~bad])
        isolated_pixels_unbiased(img, ref, bad, name)


def _normal_sets(tb):
    """three tangent sets on the normal map's texels: random on the x, the y and the z channel of every texel"""
    row, off = record(tb, "normal")
    rnd = random_tangents(tb, ["texels"], seed=2)["texels"]
    sets = []
    for ch in range(3):
        t = torch.zeros_like(rnd)
        idx = torch.arange(off["normal"] + ch, off["normal"] + map_words(row, "normal"), 3)
        t[idx] = rnd[idx]
        sets.append({"texels": t})
    return sets


def test_forward_mode_matches_the_harness():
    """Forward mode against the host run: material duals on the normal map (the rotated-UV quad, K = 1 per channel and the three as one K = 3 launch), geometry
    duals with the primary-edge kernel (the room with a normal-mapped floor: triangle rows, camera pose and edge rows at once, K = 1 and K = 3).  Bounds of
    test_colloc_microfacet_gpu.py::test_forward_mode_matches_the_harness: 1e-4, 1e-3 for a geometry derivative image, K = 3 columns to 1e-6 / 1e-5."""
    tb = _scene("quad", 24, 8).tables(0)
    o = colloc_opts(8, rng_offset=(3, 0, 0))
    g = GpuScene(tb)
    sets, cols = _normal_sets(tb), []
    for ts in sets:
        ref_img, ref_d = host_colloc_render(tb, o, mode=1, tangents=ts)
        img, d = g.render_d_fwd(o, [ts])
        assert np.abs(ref_d).max() > 0
        assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-4, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))
        cols.append(d[0])
    _, d3 = g.render_d_fwd(o, sets)
    assert all(rel_l2(d3[k], cols[k]) < 1e-6 for k in range(3)), [rel_l2(d3[k], cols[k]) for k in range(3)]
    tb2 = _scene("room", 24, 8, 8).tables(0)
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
    """<adj, J t> = <J^T adj, t> on the GPU for the texels (four 4 x 4 maps), the triangle rows, the camera pose and the primary-edge rows, and the reverse launch's
    gradient tables against the host's, table by table (bounds of test_colloc_microfacet_gpu.py::test_reverse_equals_forward)."""
    res, spp, sppe = 16, 4, 4
    tb = _scene(name, res, spp, sppe).tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    g = GpuScene(tb)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge"]
    img_r, grads = g.render_d_rev(o, adj, want=names)
    _, host_grads = host_colloc_rev(tb, o, adj, want=names)
    row, off = record(tb, "normal")
    for key, width in (("kd", 48), ("f0", 48), ("roughness", 16), ("normal", map_words(row, "normal"))):
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
    """CollocatedIntegrator.renderD + enoki.backward on a normal-mapped scene: a gradient on each of the four maps, equal to the C ABI's reverse call with the
    scaled adjoint image."""
    inten = [2.0, 1.0, 0.5]
    sc = _scene("quad", 16, 4, 4)
    b = sc.param_map["BSDF[id=m]"]
    maps = (b.diffuse_reflectance.data, b.specular_reflectance.data, b.roughness.data, b.normal_map.data)
    for m in maps:
        ek.set_requires_gradient(m)
    sc.configure()
    img = psdr_cuda.CollocatedIntegrator(Vector3fD(inten)).renderD(sc)
    target = torch.full_like(img.t, 1e-7)
    ek.backward(FloatD._wrap(((img.t - target) ** 2).sum().reshape(1)))
    adj = (2.0 * (img.t - target)).detach().cpu().numpy()
    tb = sc.tables(0)
    g = GpuScene(tb)
    _, cg = g.render_d_rev(colloc_opts(4, 4), adj * np.array(inten, np.float32), want=["texels"])
    _, off = record(tb, "normal")
    for m, key in zip(maps, ("kd", "f0", "roughness", "normal")):
        got = ek.gradient(m).numpy().reshape(-1)
        want = cg["texels"][off[key]:off[key] + got.size]
        assert np.isfinite(got).all() and np.abs(want).max() > 0, key
        assert rel_l2(got, want) < 1e-4, (key, rel_l2(got, want))


def test_two_spp_shards_sum_to_the_whole():
    tb = _scene("mixed", 24, 8, 8).tables(0)
    g = GpuScene(tb)
    full = g.render_c(colloc_opts(8, rng_offset=(1, 0, 0)))
    parts = sum(g.render_c(colloc_opts(8, rng_offset=(1, 0, 0), spp_range=r)).astype(np.float64) for r in ((0, 3), (3, 8)))
    assert full.max() > 0 and rel_l2(parts, full) < 1e-6, rel_l2(parts, full)
    tan = random_tangents(tb, ["texels", "tri_info", "prim_edge"], seed=2)
    _, dfull = g.render_d_fwd(colloc_opts(8, 8, rng_offset=(1, 2, 0)), [tan])
    dparts = sum(g.render_d_fwd(colloc_opts(8, 8, rng_offset=(1, 2, 0), spp_range=r, sppe_range=r), [tan])[1][0].astype(np.float64) for r in ((0, 3), (3, 8)))
    assert rel_l2(dparts, dfull[0]) < 1e-6, rel_l2(dparts, dfull[0])


def test_error_returns():
    """A type-3 record under PSDR_INTEGRATOR_DIRECT / _PATH: the MicrofacetBSDF error return before any launch, from every render entry point and the guide
    build.  A type-3 record in tables whose tri_uv is NULL: "a normal map needs texture coordinates" from the three render entry points, no silent fallback.  The
    handle stays intact: with the table back, the CollocatedIntegrator renders what the harness renders."""
    light = '<ref id="m"/><emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter>'          # (an emitter, so that "No Emitter!" is not the answer)
    sc = scene(uv_quad_xml(normal_xml(0.3, lean_texel()), 30.0).replace('<ref id="m"/>', light), 16, 4, 4)
    tb = sc.tables(0)
    assert tb["num_emitters"] == 1 and tb["material_mask"] == 8
    g = GpuScene(tb)
    adj = np.ones((16 * 16, 3), np.float32)
    tan = random_tangents(tb, ["texels"], seed=1)
    for kind, depth in ((_abi.INTEGRATOR_DIRECT, 1), (_abi.INTEGRATOR_PATH, 3)):
        o = _abi.make_opts(integrator=kind, max_depth=depth, spp=4, sppe=4, sppse=4)
        for call in (lambda: g.render_c(o), lambda: g.render_d_fwd(o, [tan]), lambda: g.render_d_rev(o, adj, want=["texels"]), lambda: g.guide_build(o, [2, 2, 2, 1], 1)):
            with pytest.raises(RuntimeError, match=MESSAGE):
                call()
    ref = host_colloc_render(tb, colloc_opts(4))
    assert rel_l2(g.render_c(colloc_opts(4)), ref) < 1e-4
    bare = dict(tb)
    bare["tri_uv"] = None
    gb = GpuScene(bare)
    o = colloc_opts(4, 4)
    for call in (lambda: gb.render_c(o), lambda: gb.render_d_fwd(o, [tan]), lambda: gb.render_d_rev(o, adj, want=["texels"])):
        with pytest.raises(RuntimeError, match=KINDS["normal"].needs_uv):
            call()
    with pytest.raises(RuntimeError, match=MESSAGE):          # the older message first
        gb.render_c(_abi.make_opts(integrator=_abi.INTEGRATOR_DIRECT, max_depth=1, spp=4))


# ---------------------------------------------------------------- a small recovery
def _recovery_scene(tilt, spp, kd, nm):
    def maps(sc):
        b = sc.m_bsdfs[0]
        b.diffuse_reflectance.resolution = b.normal_map.resolution = (4, 4)
        b.diffuse_reflectance.data, b.normal_map.data = kd, nm
    return scene(R.xml(tilt), 32, spp, 0, extra=maps)


def test_recover_albedo_and_normal_maps():
    """The normal-mapped quad at 32 x 32 x 4 spp seen under three tilts (35 and -35 degrees about y, 35 about x: tilts about one axis alone leave the sign of the
    normal's component along it open), a 4 x 4 kd map started at 0.5 and a 4 x 4 normal map started flat, roughness and F0 known; the target rendered at 64 spp;
    40 Adam steps on both maps.  Condition: the mean kd texel error and the mean angular error of the normals both end below half of their start.
    The step length (0.05) comes from the same loop over the host harness: kd 0.1507 -> 0.0217, normals 17.04 -> 3.40 degrees (at 0.02: 0.0214, 3.70)."""
    kd_true, n_true = R.truth()
    integ = psdr_cuda.CollocatedIntegrator(R.intensity)          # the quad is 1000 away: pixel values of order 0.1
    targets = []
    for tilt in R.tilts:
        ref = _recovery_scene(tilt, 64, Vector3fD(torch.from_numpy(kd_true)), Vector3fD(torch.from_numpy(n_true)))
        targets.append(integ.renderC(ref).torch().clone())
    kd0, nm0 = R.start()
    kd, nm = Vector3fD(torch.from_numpy(kd0)), Vector3fD(torch.from_numpy(nm0))
    ek.set_requires_gradient(kd)
    ek.set_requires_gradient(nm)
    scenes = [_recovery_scene(tilt, 4, kd, nm) for tilt in R.tilts]
    start = R.errors(kd.numpy(), nm.numpy())
    opt = torch.optim.Adam([kd.t, nm.t], lr=R.lr)
    for it in range(R.steps):
        opt.zero_grad()
        for sc, target in zip(scenes, targets):
            sc.configure()
            img = integ.renderD(sc)
            ek.backward(ek.hmean(ek.hsum(ek.sqr(img - Vector3fD._wrap(target)))))
        opt.step()
        kd.t.data.clamp_(0.01, 0.99)
        nm.t.data.clamp_(0.0, 1.0)
    end = R.errors(kd.numpy(), nm.numpy())
    print("normal map recovery: mean kd texel error %.4f -> %.4f, mean angular error of the normals %.2f -> %.2f degrees" % (start[0], end[0], start[1], end[1]))
    assert end[0] < 0.5 * start[0] and end[1] < 0.5 * start[1], (start, end)
