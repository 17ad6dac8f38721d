"""The PointLightIntegrator on the GPU (csrc/psdr_pointlight.hip), through the C ABI and the Python surface, against the host harness that runs the same estimator
(tests/hostcheck/hostcheck_pointlight.cpp; tests/test_pointlight_host.py pins that one on closed forms, the collocated limit, an analytic shadow and AD against FD)."""
import ctypes as C

import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import xml_scene
from colloc_microfacet_helpers import scene as mf_scene
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import GpuScene, dot_tables, isolated_pixels_unbiased, load_scene, random_tangents, rel_l2, tangents_wrt
from pointlight_helpers import floor_occluder_xml, host_point_render, host_point_rev, point_opts
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu

# per scene: the light (inside the room / between camera and bunny), chosen so that the shadow outlines fall between pixel centres of no particular grid
LIGHT = {"cbox": (30.3, 181.7, 50.9), "cbox_rough": (30.3, 181.7, 50.9), "cbox_occluder": (30.3, 181.7, 50.9), "cbox_bunny": (-41.3, 171.9, 120.7), "cbox_env": (10.3, 100.7, 300.9)}          # (cbox_env: inside the environment map's bounding mesh, which ends at y = 168)


def _light(name, tb):
    if name in LIGHT:
        return np.array(LIGHT[name], np.float32)
    T = tb["tri_info"].detach().cpu().numpy()          # bunny_light: halfway between the camera and the scene's centre, off the axis
    cam = tb["cam"].detach().cpu().numpy()[_abi.CAM_POS:_abi.CAM_POS + 3]
    return (0.5 * (cam + T[:, 0:3].mean(axis=0)) + np.array([40.3, 60.7, 0.0])).astype(np.float32)


class PointScene(GpuScene):
    """GpuScene + psdr_scene_set_point_light"""

    def set_light(self, pos, d_pos=None, want_grad=False):
        pos = np.ascontiguousarray(pos, np.float32).reshape(3)
        K = 0 if d_pos is None else len(d_pos)
        d = np.ascontiguousarray(d_pos, np.float32).reshape(-1) if K else None
        self.g_pos = torch.zeros(3, dtype=torch.float32, device="cuda") if want_grad else None
        _abi.check(self.lib, self.lib.psdr_scene_set_point_light(self.h, pos.ctypes.data_as(C.POINTER(C.c_float)), K,
                                                                 d.ctypes.data_as(C.POINTER(C.c_float)) if K else None, self.g_pos.data_ptr() if want_grad else None))
        return self

    def light_grad(self):
        torch.cuda.synchronize()
        return self.g_pos.cpu().numpy()


def _split(img, ref, tree):
    bad = np.abs(img - ref).max(axis=1) > 1e-3 * (1 + np.abs(ref).max(axis=1)) if tree else np.zeros(len(ref), bool)
    return bad


@pytest.mark.parametrize("name,tree", [("cbox_occluder", False), ("cbox_rough", False), ("bunny_light", True), ("cbox_bunny", True), ("cbox_env", False)])
def test_render_c_matches_the_harness(name, tree):
    """renderC against the host run of the same code on the five scene forms: kernel-argument primitives (cbox_occluder: tiny), the GGX flag set (cbox_rough:
    general), one tree (bunny_light), a two-level tree (cbox_bunny), the environment-map flag set (cbox_env).  rel-L2 < 1e-4 outside the pixels
    helpers.isolated_pixels_unbiased isolates (tree scenes; capped at 0.5 % of the pixels).  19 x 19 x 3: a partly filled last workgroup and pixels that straddle
    waves (atomic splat); 32 x 32 x 16: the plain-store path of a wave that owns its pixels."""
    for res, spp in ((19, 3), (32, 16)):
        sc, _ = load_scene(name, res=res, spp=spp)
        tb = sc.tables(0)
        pos = _light(name, tb)
        o = point_opts(spp, rng_offset=(7, 0, 0))
        ref = host_point_render(tb, o, pos)
        g = PointScene(tb).set_light(pos)
        img = g.render_c(o)
        assert np.isfinite(img).all() and ref.max() > 0 and (ref == 0).any()
        bad = _split(img, ref, tree)
        print("%s %dx%dx%d: rel-L2 %.2e, isolated pixels %d" % (name, res, res, spp, rel_l2(img[~bad], ref[~bad]), bad.sum()))
        assert bad.mean() <= 5e-3, bad.mean()
        assert rel_l2(img[~bad], ref[~bad]) < 1e-4, rel_l2(img[~bad], ref[~bad])
        isolated_pixels_unbiased(img, ref, bad, name)


def test_forward_mode_matches_the_harness():
    """Forward mode against the host run: a texel set on cbox_rough (material duals, 1e-4), the occluder's translation with all three terms on and the light's
    translation on cbox_occluder (geometry duals, the primary-edge and the shadow-boundary kernel: 1e-3, test_collocated_gpu's bounds); K = 3 gives the columns of
    three K = 1 launches."""
    sc, _ = load_scene("cbox_rough", res=24, spp=8)
    tb = sc.tables(0)
    pos = _light("cbox_rough", tb)
    o = point_opts(8, rng_offset=(3, 0, 0))
    ts = random_tangents(tb, ["texels"], seed=2)
    g = PointScene(tb).set_light(pos)
    ref_img, ref_d = host_point_render(tb, o, pos, mode=1, tangents=ts)
    img, d = g.render_d_fwd(o, [ts])
    assert np.abs(ref_d).max() > 0
    assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-4, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))
    img3, d3 = g.render_d_fwd(o, [ts, ts, ts])
    assert rel_l2(d3[0], d[0]) < 1e-6 and rel_l2(d3[2], d[0]) < 1e-6

    sc2, P = load_scene("cbox_occluder", res=24, spp=8, sppe=8, sppse=16, translate=(1, (1.0, 0.5, 0.0)))
    tb2 = sc2.tables(0)
    pos2 = _light("cbox_occluder", tb2)
    tan = tangents_wrt(tb2, P)
    o2 = point_opts(8, 8, 16, rng_offset=(3, 4, 5))
    ref_img, ref_d = host_point_render(tb2, o2, pos2, mode=1, tangents=tan)
    _, ref_no_se = host_point_render(tb2, point_opts(8, 8, 0, rng_offset=(3, 4, 5)), pos2, mode=1, tangents=tan)
    g2 = PointScene(tb2).set_light(pos2)
    img, d = g2.render_d_fwd(o2, [tan])
    assert np.abs(ref_d - ref_no_se).max() > 0          # the shadow boundary contributes
    print("forward, occluder translation: image %.2e, derivative %.2e" % (rel_l2(img, ref_img), rel_l2(d[0], ref_d)))
    assert rel_l2(img, ref_img) < 1e-4 and rel_l2(d[0], ref_d) < 1e-3, (rel_l2(img, ref_img), rel_l2(d[0], ref_d))
    # the light's translation: the tangent travels through psdr_scene_set_point_light
    dl = np.array([[1.0, 0.5, 0.0]], np.float32)
    none = {k: None for k in tan}
    _, ref_dl = host_point_render(tb2, o2, pos2, mode=1, d_pos=dl[0])
    g2.set_light(pos2, d_pos=dl)
    _, d_l = g2.render_d_fwd(o2, [none])
    print("forward, light translation: derivative %.2e" % rel_l2(d_l[0], ref_dl))
    assert np.abs(ref_dl).max() > 0 and rel_l2(d_l[0], ref_dl) < 1e-3, rel_l2(d_l[0], ref_dl)
    # K = 3: columns (occluder, light x, light y) against K = 1 launches
    g2.set_light(pos2, d_pos=np.array([[0, 0, 0], [1.0, 0.5, 0.0], [0, 0, 0]], np.float32))
    _, d3 = g2.render_d_fwd(o2, [tan, none, none])
    assert rel_l2(d3[0], d[0]) < 1e-5 and rel_l2(d3[1], d_l[0]) < 1e-5 and np.abs(d3[2]).max() == 0, (rel_l2(d3[0], d[0]), rel_l2(d3[1], d_l[0]))


@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_rough", "bunny_light"])
def test_reverse_equals_forward(name):
    """<adj, J t> = <J^T adj, t> on the GPU per table (triangle rows, texels, the camera pose, primary-edge rows, secondary-edge rows, the light position) with
    all three terms on, and the reverse launch's tables -- g_pos included -- against the host's: 1e-4, 1e-3 on bunny_light."""
    res, spp, sppe, sppse = 16, 4, 4, 8
    sc, _ = load_scene(name, res=res, spp=spp, sppe=sppe, sppse=sppse)
    tb = sc.tables(0)
    pos = _light(name, tb)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    tol = 1e-3 if name == "bunny_light" else 1e-4
    g = PointScene(tb).set_light(pos, want_grad=True)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge"]
    img_r, grads = g.render_d_rev(o, adj, want=names)
    g_pos = g.light_grad()
    _, host_grads, host_gpos = host_point_rev(tb, o, pos, adj, want=names)
    print("%s: g_pos %s host %s" % (name, g_pos, host_gpos))
    assert np.abs(host_gpos).max() > 0 and rel_l2(g_pos, host_gpos) < tol, (g_pos, host_gpos)
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        g.set_light(pos)
        img, dimg = g.render_d_fwd(o, [tan])
        assert rel_l2(img_r, img) < 1e-5
        lhs, rhs = float((adj.astype(np.float64) * dimg[0]).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
        assert scale > 0, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        assert rel_l2(grads[n], host_grads[n]) < tol, (n, rel_l2(grads[n], host_grads[n]))
    dl = np.array([[0.3, -0.2, 0.4]], np.float32)
    g.set_light(pos, d_pos=dl)
    _, dimg = g.render_d_fwd(o, [{}])
    lhs, rhs = float((adj.astype(np.float64) * dimg[0]).sum()), float(g_pos.astype(np.float64) @ dl[0])
    scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


def test_shadow_boundary_kernels_alone():
    """spp = sppe = 0 in the shard: only k_point_sedge / k_point_sedge_rev run; forward and reverse against the harness (1e-3 / 1e-4), on the tiny scene and on a
    scene of two quads where the occluder's outline crosses the receiver"""
    for name in ("cbox_occluder", "quad"):
        if name == "quad":
            def prep(sc):
                sc.opts.sppse = 32
            sc = xml_scene(floor_occluder_xml(), 16, 4, 0, prepare=prep)
            pos = np.array([60.3, 180.7, 600.0], np.float32)
        else:
            sc, _ = load_scene(name, res=16, spp=4, sppse=32)
            pos = _light(name, sc.tables(0))
        tb = sc.tables(0)
        o = point_opts(4, 0, 32, rng_offset=(0, 0, 9), spp_range=(0, 0))
        tan = random_tangents(tb, ["sec_edge", "tri_info"], seed=4)
        adj = np.random.default_rng(6).random((16 * 16, 3)).astype(np.float32)
        _, ref_d = host_point_render(tb, o, pos, mode=1, tangents=tan)
        g = PointScene(tb).set_light(pos, want_grad=True)
        img, d = g.render_d_fwd(o, [tan])
        assert np.abs(img).max() == 0 and np.abs(ref_d).max() > 0
        assert rel_l2(d[0], ref_d) < 1e-3, rel_l2(d[0], ref_d)
        _, grads = g.render_d_rev(o, adj, want=["sec_edge", "tri_info"], with_image=False)
        _, hg, hpos = host_point_rev(tb, o, pos, adj, want=["sec_edge", "tri_info"])
        for n in ("sec_edge", "tri_info"):
            assert np.abs(hg[n]).max() > 0 and rel_l2(grads[n], hg[n]) < 1e-4, (name, n, rel_l2(grads[n], hg[n]))
        assert np.abs(hpos).max() > 0 and rel_l2(g.light_grad(), hpos) < 1e-4, (g.light_grad(), hpos)


def test_shards_sum_to_the_full_launch():
    """spp / sppe / sppse shards of psdr_render_d_fwd sum to the unsharded launch: 1e-6"""
    sc, P = load_scene("cbox_occluder", res=16, spp=6, sppe=4, sppse=8, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    pos = _light("cbox_occluder", tb)
    tan = tangents_wrt(tb, P)
    g = PointScene(tb).set_light(pos)
    full_img, full_d = g.render_d_fwd(point_opts(6, 4, 8, rng_offset=(1, 2, 3)), [tan])
    img, d = np.zeros_like(full_img, np.float64), np.zeros_like(full_d[0], np.float64)
    for a, b, c in (((0, 2), (0, 1), (0, 3)), ((2, 6), (1, 4), (3, 8))):
        i, dd = g.render_d_fwd(point_opts(6, 4, 8, rng_offset=(1, 2, 3), spp_range=a, sppe_range=b, sppse_range=c), [tan])
        img += i
        d += dd[0]
    assert rel_l2(img, full_img) < 1e-6 and rel_l2(d, full_d[0]) < 1e-6, (rel_l2(img, full_img), rel_l2(d, full_d[0]))


def test_error_returns():
    """kind 4 without a light: an error before any launch, in all three render calls; a light that is not finite or K out of range is refused; Direct and Path keep
    refusing a MicrofacetBSDF and keep asking for an emitter"""
    sc, _ = load_scene("cbox", res=8, spp=1)
    tb = sc.tables(0)
    g = PointScene(tb)
    o = point_opts(1)
    adj = np.ones((64, 3), np.float32)
    for call in (lambda: g.render_c(o), lambda: g.render_d_fwd(o, [{}]), lambda: g.render_d_rev(o, adj, want=["texels"])):
        with pytest.raises(RuntimeError, match="no light set"):
            call()
    with pytest.raises(RuntimeError, match="not finite"):
        g.set_light((0.0, float("inf"), 0.0))
    with pytest.raises(RuntimeError, match="K must be"):
        g.set_light((0.0, 0.0, 0.0), d_pos=np.zeros((4, 3), np.float32))
    g.set_light((10.0, 100.0, 50.0))
    assert np.isfinite(g.render_c(o)).all()
    _abi.check(g.lib, g.lib.psdr_scene_set_point_light(g.h, None, 0, None, None))          # the light removed again
    with pytest.raises(RuntimeError, match="no light set"):
        g.render_c(o)
    from colloc_microfacet_helpers import MESSAGE, microfacet_xml, uv_quad_xml
    tbm = mf_scene(uv_quad_xml(microfacet_xml(0.3), 0.0), 8, 1).tables(0)
    gm = PointScene(tbm).set_light((10.0, 150.0, 500.0))
    assert gm.render_c(o).max() > 0          # no emitter, a MicrofacetBSDF: valid for this kind
    for kind in (_abi.INTEGRATOR_DIRECT, _abi.INTEGRATOR_PATH):
        with pytest.raises(RuntimeError, match=MESSAGE):
            gm.render_c(_abi.make_opts(integrator=kind, spp=1))


def _surface_scene(res=16, spp=4, sppe=4, sppse=8):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_occluder"), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    return sc


def test_python_surface_matches_the_c_abi():
    """PointLightIntegrator.renderC / renderD against the C ABI on the same tables and RNG offsets; enoki.forward through a mesh translation, the intensity and the
    position; enoki.backward to the intensity and the position, against the forward-mode derivative images."""
    pos, inten = (30.3, 181.7, 50.9), (2.0, 1.0, 0.5)
    sc = _surface_scene()
    sc.configure()
    integ = psdr_cuda.PointLightIntegrator(pos, inten)
    tb = sc.tables(0)
    g = PointScene(tb).set_light(pos)
    ref = g.render_c(point_opts(4, rng_offset=tuple(sc._rng_offset))) * np.asarray(inten, np.float32)[None, :]
    img = integ.renderC(sc).numpy()
    assert rel_l2(img, ref) < 1e-6, rel_l2(img, ref)
    # forward mode through the position
    P = FloatD(0.)
    ek.set_requires_gradient(P)
    integ.m_position = Vector3fD(list(pos)) + Vector3fD([1.0, 0.5, 0.0]) * P
    off = tuple(sc._rng_offset)
    imgd = integ.renderD(sc)
    ek.forward(P)
    d = ek.gradient(imgd).numpy()
    g.set_light(pos, d_pos=np.array([[1.0, 0.5, 0.0]], np.float32))
    ref_img, ref_d = g.render_d_fwd(point_opts(4, 4, 8, rng_offset=off), [{}])
    scale = np.asarray(inten, np.float32)[None, :]
    assert rel_l2(imgd.numpy(), ref_img * scale) < 1e-6 and np.abs(ref_d).max() > 0
    assert rel_l2(d, ref_d[0] * scale) < 1e-5, rel_l2(d, ref_d[0] * scale)
    # reverse mode: d loss / d position and d loss / d intensity
    integ2 = psdr_cuda.PointLightIntegrator(pos, inten)
    ek.set_requires_gradient(integ2.m_position)
    ek.set_requires_gradient(integ2.m_intensity)
    off = tuple(sc._rng_offset)
    imgd = integ2.renderD(sc)
    w = torch.as_tensor(np.random.default_rng(3).random((16 * 16, 3)).astype(np.float32), device=imgd.t.device)
    ek.backward(FloatD._wrap((imgd.t * w).sum().reshape(1)))
    gp, gi = ek.gradient(integ2.m_position).numpy().reshape(3), ek.gradient(integ2.m_intensity).numpy().reshape(3)
    g.set_light(pos, want_grad=True)
    adj = (w.cpu().numpy() * scale).astype(np.float32)
    unit, _ = g.render_d_rev(point_opts(4, 4, 8, rng_offset=off), adj, want=[])
    ref_gp = g.light_grad()
    ref_gi = (unit.astype(np.float64) * w.cpu().numpy()).sum(axis=0)
    print("python surface: g_pos %s ref %s, g_intensity %s ref %s" % (gp, ref_gp, gi, ref_gi))
    assert np.abs(ref_gp).max() > 0 and rel_l2(gp, ref_gp) < 1e-5 and rel_l2(gi, ref_gi) < 1e-5


def test_refusals_unchanged_on_the_python_surface():
    from colloc_microfacet_helpers import MESSAGE, microfacet_xml, uv_quad_xml
    sc = mf_scene(uv_quad_xml(microfacet_xml(0.3), 0.0), 8, 1)
    assert psdr_cuda.PointLightIntegrator((10.0, 150.0, 500.0)).renderC(sc).numpy().max() > 0
    for integ in (psdr_cuda.DirectIntegrator(1, 1), psdr_cuda.PathTracer(2)):
        with pytest.raises(RuntimeError, match=MESSAGE):
            integ.renderC(sc)


# ---------------------------------------------------------------- a small recovery under three lamps
RECOVERY_LAMPS = [(600.0 * np.cos(a), 125.0 + 600.0 * np.sin(a), 800.0) for a in np.radians([0.0, 120.0, 240.0])]          # 120 degrees apart, about 37 degrees off the axis


def test_recover_albedo_and_normal_maps_under_three_lights():
    """The normal-mapped quad of tests/test_colloc_normal_gpu.py's recovery, head-on at 32 x 32 x 4 spp from ONE camera, under three lamps (one PointLightIntegrator
    each; their images are separate photographs): a 4 x 4 kd map started at 0.5 and a 4 x 4 normal map started flat, roughness and F0 known; targets at 64 spp;
    the same 40 Adam steps of the same length.  Condition (that test's): the mean kd texel error and the mean angular error of the normals both end below half of
    their start.  Measured: kd 0.1507 -> 0.0192, normals 17.04 -> 2.80 degrees (the three-tilt collocated test: 0.0217, 3.40)."""
    from colloc_microfacet_helpers import RECOVERY
    R = RECOVERY["normal"]

    def view(spp, kd, nm):
        def maps(sc):
            b = sc.m_bsdfs[0]
            b.diffuse_reflectance.resolution = b.normal_map.resolution = (4, 4)
            b.diffuse_reflectance.data, b.normal_map.data = kd, nm
        return mf_scene(R.xml((0.0, 0.0)), 32, spp, 0, extra=maps)
    kd_true, n_true = R.truth()
    integs = [psdr_cuda.PointLightIntegrator(p, R.intensity) for p in RECOVERY_LAMPS]
    ref = view(64, Vector3fD(torch.from_numpy(kd_true)), Vector3fD(torch.from_numpy(n_true)))
    targets = [integ.renderC(ref).torch().clone() for integ in integs]
    kd0, nm0 = R.start()
    kd, nm = Vector3fD(torch.from_numpy(kd0)), Vector3fD(torch.from_numpy(nm0))
    ek.set_requires_gradient(kd)
    ek.set_requires_gradient(nm)
    sc = view(4, kd, nm)
    start = R.errors(kd.numpy(), nm.numpy())
    opt = torch.optim.Adam([kd.t, nm.t], lr=R.lr)
    for it in range(R.steps):
        opt.zero_grad()
        sc.configure()
        for integ, target in zip(integs, targets):
            img = integ.renderD(sc)
            ek.backward(ek.hmean(ek.hsum(ek.sqr(img - Vector3fD._wrap(target)))))
        opt.step()
        kd.t.data.clamp_(0.01, 0.99)
        nm.t.data.clamp_(0.0, 1.0)
    end = R.errors(kd.numpy(), nm.numpy())
    print("three-light recovery: mean kd texel error %.4f -> %.4f, mean angular error of the normals %.2f -> %.2f degrees" % (start[0], end[0], start[1], end[1]))
    assert end[0] < 0.5 * start[0] and end[1] < 0.5 * start[1], (start, end)
