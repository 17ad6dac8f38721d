"""The CollocatedIntegrator on the GPU (csrc/psdr_collocated.hip), through the C ABI and the Python surface, against the host harness that runs the same estimator
(tests/hostcheck/hostcheck_collocated.cpp; tests/test_collocated_host.py pins that one on closed forms, the second oracle's BSDF values and AD against FD)."""
import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import DIFFUSE, colloc_opts, host_colloc_render, host_colloc_rev, quad_xml, xml_scene
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import GpuScene, dot_tables, isolated_pixels_unbiased, load_scene, random_tangents, rel_l2, tangents_wrt
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scene,tree", [("cbox", False), ("cbox_rough", False), ("cbox_uv", False), ("cbox_bunny", True), ("bunny_light", True)])
def test_render_c_matches_the_harness(scene, tree):
    """renderC against the host run of the same code: kernel-argument primitives (cbox, cbox_rough, cbox_uv), a two-level tree (cbox_bunny), a single tree
    (bunny_light).  rel-L2 <= 1e-4, the bound of test_gpu_parity.py; on the tree scenes outside isolated silhouette pixels (one sample resolves an epsilon-sized
    tie the other way between two fp32 evaluations), which are held to helpers.isolated_pixels_unbiased and capped at 0.5 % of the pixels.  19 x 19 x 3: the last
    workgroup is partly filled and a pixel's samples straddle waves (atomic splat); 16 spp at 32 x 32: the plain-store path of a wave that owns its pixels."""
    for res, spp in ((19, 3), (32, 16)):
        sc, _ = load_scene(scene, res=res, spp=spp)
        tb = sc.tables(0)
        o = colloc_opts(spp, rng_offset=(7, 0, 0))
        ref = host_colloc_render(tb, o)
        g = GpuScene(tb)
        img = g.render_c(o)
        assert np.isfinite(img).all() and ref.max() > 0
        assert g.counters()[0] == res * res * spp          # one ray per sample
        bad = np.abs(img - ref).max(axis=1) > 1e-3 * (1 + np.abs(ref).max(axis=1)) if tree else np.zeros(len(ref), bool)
        print("%s %dx%dx%d: rel-L2 %.2e, isolated pixels %d" % (scene, res, res, spp, rel_l2(img[~bad], ref[~bad]), bad.sum()))
        assert bad.mean() <= 5e-3, bad.mean()
        assert rel_l2(img[~bad], ref[~bad]) < 1e-4, rel_l2(img[~bad], ref[~bad])
        isolated_pixels_unbiased(img, ref, bad, scene)


def _texel_sets(tb):
    """tangent sets on the albedo texels and on the alpha texels of cbox_rough's rough conductor (constant textures: bsdf_rec names the texel offsets)"""
    rec = tb["bsdf_rec"].detach().cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    r = rec[rec[:, 0] == _abi.BSDF_ROUGHCONDUCTOR][0]
    n = tb["texels"].numel()
    albedo, alpha = torch.zeros(n), torch.zeros(n)
    for row in rec:          # every reflectance texel
        albedo[int(row[1 + 3 * _abi.SLOT_REFLECTANCE]):int(row[1 + 3 * _abi.SLOT_REFLECTANCE]) + 3] = torch.tensor([1.0, 0.5, 0.25])
    alpha[int(r[1 + 3 * _abi.SLOT_ALPHA_U])] = 1.0
    alpha[int(r[1 + 3 * _abi.SLOT_ALPHA_V])] = 1.0
    return {"texels": albedo}, {"texels": alpha}


def test_forward_mode_matches_the_harness():
    """Forward mode against the host run: an albedo texel set and an alpha texel set (cbox_rough, material duals), a mesh translation with sppe > 0
    (cbox_occluder: geometry duals + the primary-edge kernel); K = 1 and K = 3 give the same columns."""
    sc, _ = load_scene("cbox_rough", res=24, spp=8)
    tb = sc.tables(0)
    o = colloc_opts(8, rng_offset=(3, 0, 0))
    sets = list(_texel_sets(tb))
    g = GpuScene(tb)
    cols = []
    for ts in sets:
        ref_img, ref_d = host_colloc_render(tb, o, mode=1, tangents=ts)
        img, d = g.render_d_fwd(o, [ts])
        assert np.abs(ref_d).max() > 0
        assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-4, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))
        cols.append(d[0])
    sc2, P = load_scene("cbox_occluder", res=24, spp=8, sppe=8, translate=(1, (1.0, 0.5, 0.0)))
    tb2 = sc2.tables(0)
    tan = tangents_wrt(tb2, P)
    o2 = colloc_opts(8, 8, rng_offset=(3, 4, 0))
    ref_img, ref_d = host_colloc_render(tb2, o2, mode=1, tangents=tan)
    _, ref_interior = host_colloc_render(tb2, colloc_opts(8, 0, rng_offset=(3, 4, 0)), mode=1, tangents=tan)
    g2 = GpuScene(tb2)
    img, d = g2.render_d_fwd(o2, [tan])
    assert np.abs(ref_interior).max() > 0 and np.abs(ref_d - ref_interior).max() > 0          # both terms contribute
    assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-3, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))          # (1e-3: smoke()'s bound for a geometry derivative image)
    # K = 3: the same columns as three K = 1 launches
    img3, d3 = g.render_d_fwd(o, [sets[0], sets[1], sets[0]])
    assert rel_l2(d3[0], cols[0]) < 1e-6 and rel_l2(d3[1], cols[1]) < 1e-6 and rel_l2(d3[2], cols[0]) < 1e-6
    wall = {k: (torch.zeros_like(v) if v is not None else None) for k, v in tan.items()}
    img3, d3 = g2.render_d_fwd(o2, [tan, wall, tan])
    assert rel_l2(d3[0], d[0]) < 1e-5 and rel_l2(d3[2], d[0]) < 1e-5 and np.abs(d3[1]).max() == 0, (rel_l2(d3[0], d[0]), np.abs(d3[1]).max())


@pytest.mark.parametrize("scene", ["cbox_uv", "cbox_rough", "bunny_light"])
def test_reverse_equals_forward(scene):
    """<adj, J t> = <J^T adj, t> on the GPU for the tables of the host test (triangle rows, texels, the camera pose, primary-edge rows), and the reverse launch's
    gradient tables against the host's."""
    res, spp, sppe = 16, 4, 4
    sc, _ = load_scene(scene, res=res, spp=spp, sppe=sppe)
    tb = sc.tables(0)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = colloc_opts(spp, sppe, rng_offset=(2, 3, 0))
    g = GpuScene(tb)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge"]
    img_r, grads = g.render_d_rev(o, adj, want=names)
    _, host_grads = host_colloc_rev(tb, o, adj, want=names)
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = g.render_d_fwd(o, [tan])
        assert rel_l2(img_r, img) < 1e-5
        lhs, rhs = float((adj.astype(np.float64) * dimg[0]).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        assert rel_l2(grads[n], host_grads[n]) < (1e-3 if scene == "bunny_light" else 1e-4), (n, rel_l2(grads[n], host_grads[n]))
    # material-only launch (no geometry table wanted): the same texel gradient
    _, gm = g.render_d_rev(o, adj, want=["texels"])
    assert rel_l2(gm["texels"], grads["texels"]) < 1e-5


def _surface_scene(res=16, spp=4, sppe=4):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_uv"), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, 4, 0
    return sc


def test_python_surface():
    """CollocatedIntegrator(...).renderC / renderD; enoki.forward with respect to an albedo; enoki.backward of an L2 loss with respect to vertex positions, texels
    and m_intensity.  The intensity gradient equals the per-channel sum of adjoint x unit image."""
    assert psdr_cuda.CollocatedIntegrator(2.0).m_intensity.numpy().tolist() == [[2.0, 2.0, 2.0]]
    inten = [2.0, 1.0, 0.5]
    # renderC = intensity x the unit render
    sc = _surface_scene()
    sc.configure()
    unit = psdr_cuda.CollocatedIntegrator(1.0).renderC(sc).numpy()
    sc._rng_offset = [0, 0, 0]
    img = psdr_cuda.CollocatedIntegrator(inten).renderC(sc).numpy()
    assert unit.shape == (256, 3) and unit.max() > 0 and np.allclose(img, unit * np.array(inten, np.float32), rtol=1e-6)
    with pytest.raises(RuntimeError, match="only DirectIntegrator"):
        psdr_cuda.CollocatedIntegrator(1.0).preprocess_secondary_edges(sc, 0, [2, 2, 2, 1])
    # forward mode with respect to an albedo: d image / d P with the floor's reflectance = base + P
    sc = _surface_scene()
    floor = next(b for b in sc.m_bsdfs if b.id == "floor_tex")
    P = FloatD(0.0)
    ek.set_requires_gradient(P)
    floor.reflectance.data = Vector3fD(floor.reflectance.data.t.detach()) + Vector3fD([1.0, 0.5, 0.25]) * P
    sc.configure()
    integ = psdr_cuda.CollocatedIntegrator(inten)
    img = integ.renderD(sc)
    ek.forward(P)
    d = ek.gradient(img).numpy()
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    o = colloc_opts(4, 4)
    ref_img, ref_d = host_colloc_render(tb, o, mode=1, tangents=tan)
    assert np.abs(ref_d).max() > 0
    assert rel_l2(img.numpy(), ref_img * np.array(inten, np.float32)) < 1e-4 and rel_l2(d, ref_d * np.array(inten, np.float32)) < 1e-4
    # reverse mode: L2 loss, gradients to vertex positions, texels and the intensity
    sc = _surface_scene()
    mesh = sc.param_map["Mesh[1]"]
    floor = next(b for b in sc.m_bsdfs if b.id == "floor_tex")
    ek.set_requires_gradient(mesh.vertex_positions)
    ek.set_requires_gradient(floor.reflectance.data)
    I = Vector3fD(inten)
    ek.set_requires_gradient(I)
    sc.configure()
    integ = psdr_cuda.CollocatedIntegrator(I)
    assert integ.m_intensity is I
    img = integ.renderD(sc)
    target = torch.full_like(img.t, 1e-6)
    loss = FloatD._wrap(((img.t - target) ** 2).sum().reshape(1))
    ek.backward(loss)
    adj = (2.0 * (img.t - target)).detach().cpu().numpy()
    tb = sc.tables(0)
    o = colloc_opts(4, 4)
    unit_ref = host_colloc_render(tb, o)
    gI = ek.gradient(I).numpy().reshape(3)
    want_I = (adj.astype(np.float64) * unit_ref).sum(axis=0)
    assert np.allclose(gI, want_I, rtol=1e-4), (gI, want_I)
    gv, gt = ek.gradient(mesh.vertex_positions).numpy(), ek.gradient(floor.reflectance.data).numpy()
    assert np.isfinite(gv).all() and np.abs(gv).max() > 0 and np.isfinite(gt).all() and np.abs(gt).max() > 0
    # the texel gradient against the host's reverse run with the scaled adjoint image
    _, hg = host_colloc_rev(tb, o, adj * np.array(inten, np.float32), want=["texels"])
    rec = tb["bsdf_rec"].detach().cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    off = int(rec[[b.id for b in sc.m_bsdfs].index("floor_tex")][1 + 3 * _abi.SLOT_REFLECTANCE])
    assert np.allclose(gt.reshape(-1), hg["texels"][off:off + 3], rtol=1e-3), (gt, hg["texels"][off:off + 3])


def test_two_spp_shards_sum_to_the_whole():
    sc, _ = load_scene("cbox_rough", res=24, spp=8, sppe=8)
    tb = sc.tables(0)
    g = GpuScene(tb)
    full = g.render_c(colloc_opts(8, rng_offset=(1, 0, 0)))
    parts = sum(g.render_c(colloc_opts(8, rng_offset=(1, 0, 0), spp_range=r)).astype(np.float64) for r in ((0, 3), (3, 8)))
    assert rel_l2(parts, full) < 1e-6, rel_l2(parts, full)
    tan = random_tangents(tb, ["tri_info", "prim_edge"], seed=2)
    _, dfull = g.render_d_fwd(colloc_opts(8, 8, rng_offset=(1, 2, 0)), [tan])
    dparts = sum(g.render_d_fwd(colloc_opts(8, 8, rng_offset=(1, 2, 0), spp_range=r, sppe_range=r), [tan])[1][0].astype(np.float64) for r in ((0, 3), (3, 8)))
    assert rel_l2(dparts, dfull[0]) < 1e-6, rel_l2(dparts, dfull[0])


def test_scene_without_an_emitter():
    """A scene without any emitter renders with this integrator, through the C ABI and the surface; DirectIntegrator on it still fails with "No Emitter!"."""
    sc = xml_scene(quad_xml(DIFFUSE, 30.0), 16, 4)
    tb = sc.tables(0)
    assert tb["num_emitters"] == 0
    ref = host_colloc_render(tb, colloc_opts(4))
    g = GpuScene(tb)
    assert ref.max() > 0 and rel_l2(g.render_c(colloc_opts(4)), ref) < 1e-4
    with pytest.raises(RuntimeError, match="No Emitter!"):
        g.render_c(_abi.make_opts(spp=4))
    assert rel_l2(psdr_cuda.CollocatedIntegrator(1.0).renderC(sc).numpy(), ref) < 1e-4
    with pytest.raises(RuntimeError, match="No Emitter!"):
        psdr_cuda.DirectIntegrator(1, 1).renderC(sc)
