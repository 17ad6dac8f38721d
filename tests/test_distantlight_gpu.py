"""The distant light on the GPU: the PSDR_LIGHT_DISTANT kernels of csrc/psdr_pointlight.hip (kind 4) and the mixed loop of csrc/psdr_lightstage.hip (kind 5),
through psdr_scene_set_light / psdr_scene_set_lights and the Python surface, against the host harness that runs the same estimator
(tests/hostcheck/hostcheck_distantlight.cpp; tests/test_distantlight_host.py pins that one on closed forms, line integrals of the moving outline and AD against
FD) and, for the stack, against the kind-4 launch of every light."""
import numpy as np
import pytest
import torch

import enoki as ek
import psdr_cuda
from collocated_helpers import xml_scene
from colloc_microfacet_helpers import microfacet_xml, quad
from distantlight_helpers import DISTANT, ENV_MESSAGE, POINT, KindScene, host_light_render, host_light_rev, unit
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import dot_tables, isolated_pixels_unbiased, load_scene, random_tangents, rel_l2, tangents_wrt
from lightstage_helpers import OCCLUDER_LIGHTS, stack_opts
from pointlight_helpers import floor_occluder_xml, point_opts
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)

# per scene: the direction TOWARDS the light.  The Cornell boxes are lit through their open front (+z), from above; no component is a round number, so that the
# shadow outlines fall between pixel centres of no particular grid
DIRECTION = {"cbox": (0.23, 0.51, 1.0), "cbox_rough": (0.23, 0.51, 1.0), "cbox_occluder": (0.23, 0.51, 1.0), "cbox_bunny": (-0.31, 0.47, 1.0), "bunny_light": (0.41, 0.63, -1.0),
             "cbox_env": (0.23, 0.51, 1.0)}
# six directions for the stacks on cbox_occluder (two coincide), and section 18's point lights for the mixed ones
STACK_DIRS = np.array([(0.23, 0.51, 1.0), (-0.61, 0.33, 1.0), (0.23, 0.51, 1.0), (0.52, -0.21, 2.0), (0.03, 1.52, 1.0), (-0.31, 0.83, 0.6)], np.float32)


def _dir(name):
    return np.array(DIRECTION[name], np.float32)


def _mixed(L=6):
    kinds = np.array([DISTANT if l % 2 == 0 else POINT for l in range(L)], np.int32)
    return kinds, np.where((kinds == DISTANT)[:, None], STACK_DIRS[:L], OCCLUDER_LIGHTS[:L]).astype(np.float32)


def _planes_match(plane, ref, label):
    """two instantiations of one expression: per pixel within 4 eps32 of the plane's maximum (section 18's bound); returns the worst ratio"""
    top = float(np.abs(ref).max())
    if top == 0:
        assert not np.any(plane), label
        return 0.0
    ratio = float(np.abs(plane.astype(np.float64) - ref).max() / (EPS32 * top))
    assert ratio <= 4.0, (label, ratio)
    return ratio


# ---------------------------------------------------------------- 1. renderC
@pytest.mark.parametrize("name,tree", [("cbox_occluder", False), ("cbox_rough", False), ("bunny_light", True), ("cbox_bunny", True), ("cbox_env", False)])
def test_render_c_matches_the_harness(name, tree):
    """renderC against the host run of the same code on the scene forms of test_pointlight_gpu.py, at that file's bounds form by form: rel-L2 < 1e-4 outside the
    pixels helpers.isolated_pixels_unbiased isolates (tree scenes; at most 0.5 % of the pixels).  19 x 19 x 3: a partly filled last workgroup and pixels that
    straddle waves (atomic splat); 32 x 32 x 16: the plain-store path.  The fifth form, the environment-map flag set, is the one a distant light cannot light:
    there every render call is refused before any launch (the buffer of NaN stays as it is), and the point light on the same handle still renders."""
    for res, spp in ((19, 3), (32, 16)):
        sc, _ = load_scene(name, res=res, spp=spp)
        tb = sc.tables(0)
        d = _dir(name)
        o = point_opts(spp, rng_offset=(7, 0, 0))
        g = KindScene(tb).set_kind_light(DISTANT, d)
        if name == "cbox_env":
            adj = np.ones((res * res, 3), np.float32)
            for call in (lambda: g.render_c(o), lambda: g.render_d_fwd(o, [{}]), lambda: g.render_d_rev(o, adj, want=["texels"])):
                with pytest.raises(RuntimeError, match=ENV_MESSAGE):
                    call()
            assert g.set_kind_light(POINT, (10.3, 100.7, 300.9)).render_c(o).max() > 0
            continue
        ref = host_light_render(tb, o, d)
        img = g.render_c(o)
        assert np.isfinite(img).all() and ref.max() > 0 and (ref == 0).any()
        bad = np.abs(img - ref).max(axis=1) > 1e-3 * (1 + np.abs(ref).max(axis=1)) if tree else np.zeros(len(ref), bool)
        print("distant %s %dx%dx%d: rel-L2 %.2e, isolated pixels %d" % (name, res, res, spp, rel_l2(img[~bad], ref[~bad]), bad.sum()))
        assert bad.mean() <= 5e-3, bad.mean()
        assert rel_l2(img[~bad], ref[~bad]) < 1e-4, rel_l2(img[~bad], ref[~bad])
        isolated_pixels_unbiased(img, ref, bad, name)


# ---------------------------------------------------------------- 2. forward mode
def test_forward_mode_matches_the_harness():
    """Forward mode against the host run: a texel set on cbox_rough (material duals, 1e-4), the occluder's translation with all three terms on and the
    direction's tangent on cbox_occluder (geometry duals, the primary-edge and the shadow-boundary kernel: 1e-3, test_pointlight_gpu's bounds); K = 3 gives the
    columns of K = 1 launches."""
    tb = load_scene("cbox_rough", res=24, spp=8)[0].tables(0)
    d = _dir("cbox_rough")
    o = point_opts(8, rng_offset=(3, 0, 0))
    ts = random_tangents(tb, ["texels"], seed=2)
    g = KindScene(tb).set_kind_light(DISTANT, d)
    ref_img, ref_d = host_light_render(tb, o, d, mode=1, tangent_sets=[ts])
    img, dd = g.render_d_fwd(o, [ts])
    assert np.abs(ref_d).max() > 0
    assert rel_l2(img, ref_img) < 1e-4 and rel_l2(dd[0], ref_d[0]) < 1e-4, (rel_l2(img, ref_img), rel_l2(dd[0], ref_d[0]))
    _, d3 = g.render_d_fwd(o, [ts, ts, ts])
    assert rel_l2(d3[0], dd[0]) < 1e-6 and rel_l2(d3[2], dd[0]) < 1e-6

    sc2, P = load_scene("cbox_occluder", res=24, spp=8, sppe=8, sppse=16, translate=(1, (1.0, 0.5, 0.0)))
    tb2 = sc2.tables(0)
    d2 = _dir("cbox_occluder")
    tan = tangents_wrt(tb2, P)
    o2 = point_opts(8, 8, 16, rng_offset=(3, 4, 5))
    ref_img, ref_d = host_light_render(tb2, o2, d2, mode=1, tangent_sets=[tan])
    _, ref_no_se = host_light_render(tb2, point_opts(8, 8, 0, rng_offset=(3, 4, 5)), d2, mode=1, tangent_sets=[tan])
    g2 = KindScene(tb2).set_kind_light(DISTANT, d2)
    img, dd = g2.render_d_fwd(o2, [tan])
    assert np.abs(ref_d - ref_no_se).max() > 0          # the shadow boundary contributes
    print("distant forward, occluder translation: image %.2e, derivative %.2e" % (rel_l2(img, ref_img), rel_l2(dd[0], ref_d[0])))
    assert rel_l2(img, ref_img) < 1e-4 and rel_l2(dd[0], ref_d[0]) < 1e-3, (rel_l2(img, ref_img), rel_l2(dd[0], ref_d[0]))
    # the direction's tangent travels through psdr_scene_set_light
    dl = np.array([[1.0, 0.5, -0.2]], np.float32)
    none = {k: None for k in tan}
    _, ref_dl = host_light_render(tb2, o2, d2, mode=1, d_v=dl)
    g2.set_kind_light(DISTANT, d2, d_v=dl)
    _, d_l = g2.render_d_fwd(o2, [none])
    print("distant forward, direction tangent: derivative %.2e" % rel_l2(d_l[0], ref_dl[0]))
    assert np.abs(ref_dl).max() > 0 and rel_l2(d_l[0], ref_dl[0]) < 1e-3, rel_l2(d_l[0], ref_dl[0])
    g2.set_kind_light(DISTANT, d2, d_v=np.array([[0, 0, 0], [1.0, 0.5, -0.2], [0, 0, 0]], np.float32))
    _, d3 = g2.render_d_fwd(o2, [tan, none, none])
    assert rel_l2(d3[0], dd[0]) < 1e-5 and rel_l2(d3[1], d_l[0]) < 1e-5 and np.abs(d3[2]).max() == 0, (rel_l2(d3[0], dd[0]), rel_l2(d3[1], d_l[0]))


# ---------------------------------------------------------------- 3. reverse mode
@pytest.mark.parametrize("name", ["cbox_occluder", "cbox_rough", "bunny_light"])
def test_reverse_equals_forward(name):
    """<adj, J t> = <J^T adj, t> on the GPU per table and for the direction with all three terms on, and the reverse launch's tables -- g_dir included -- against
    the host's: 1e-4, 1e-3 on bunny_light (test_pointlight_gpu's bounds)."""
    res, spp, sppe, sppse = 16, 4, 4, 8
    tb = load_scene(name, res=res, spp=spp, sppe=sppe, sppse=sppse)[0].tables(0)
    d = _dir(name)
    adj = np.random.default_rng(5).random((res * res, 3)).astype(np.float32)
    o = point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    tol = 1e-3 if name == "bunny_light" else 1e-4
    g = KindScene(tb).set_kind_light(DISTANT, d, want_grad=True)
    names = ["tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge"]
    img_r, grads = g.render_d_rev(o, adj, want=names)
    g_dir = g.light_grad()
    _, host_grads, host_gdir = host_light_rev(tb, o, d, adj, want=names)
    print("distant %s: g_dir %s host %s" % (name, g_dir, host_gdir))
    assert np.abs(host_gdir).max() > 0 and rel_l2(g_dir, host_gdir) < tol, (g_dir, host_gdir)
    assert abs(float(g_dir.astype(np.float64) @ unit(d))) <= 1e-4 * float(np.abs(g_dir).max())          # tangential
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        g.set_kind_light(DISTANT, d)
        img, dimg = g.render_d_fwd(o, [tan])
        assert rel_l2(img_r, img) < 1e-5
        lhs, rhs = float((adj.astype(np.float64) * dimg[0]).sum()), dot_tables(grads, tan)
        scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
        # (cbox_occluder: Lambertian planes under a distant light look the same from every camera, and the primary edges move with their own table)
        flat = name == "cbox_occluder" and n == "cam_to_world"
        assert scale > 0 or flat, n
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (n, lhs, rhs, scale)
        assert (flat and not np.any(host_grads[n]) and np.abs(grads[n]).max() <= 1e-6) or rel_l2(grads[n], host_grads[n]) < tol, (n, rel_l2(grads[n], host_grads[n]))
    dl = np.array([[0.3, -0.2, 0.4]], np.float32)
    g.set_kind_light(DISTANT, d, d_v=dl)
    _, dimg = g.render_d_fwd(o, [{}])
    lhs, rhs = float((adj.astype(np.float64) * dimg[0]).sum()), float(g_dir.astype(np.float64) @ dl[0])
    scale = float(np.abs(adj.astype(np.float64) * dimg[0]).sum())
    assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (lhs, rhs, scale)


# ---------------------------------------------------------------- 4. the shadow-boundary kernels alone
def test_shadow_boundary_kernels_alone():
    """spp = sppe = 0 in the shard: only k_point_sedge / k_point_sedge_rev of the distant family run; forward and reverse against the harness (1e-3 / 1e-4), on
    the tiny scene and on a scene of two quads where the occluder's outline crosses the receiver"""
    for name in ("cbox_occluder", "quad"):
        if name == "quad":
            def prep(sc):
                sc.opts.sppse = 32
            sc = xml_scene(floor_occluder_xml(), 16, 4, 0, prepare=prep)
            d = np.array([0.13, 0.11, 1.0], np.float32)
        else:
            sc, _ = load_scene(name, res=16, spp=4, sppse=32)
            d = _dir(name)
        tb = sc.tables(0)
        o = point_opts(4, 0, 32, rng_offset=(0, 0, 9), spp_range=(0, 0))
        tan = random_tangents(tb, ["sec_edge", "tri_info"], seed=4)
        adj = np.random.default_rng(6).random((16 * 16, 3)).astype(np.float32)
        _, ref_d = host_light_render(tb, o, d, mode=1, tangent_sets=[tan])
        g = KindScene(tb).set_kind_light(DISTANT, d, want_grad=True)
        img, dd = g.render_d_fwd(o, [tan])
        assert np.abs(img).max() == 0 and np.abs(ref_d).max() > 0
        assert rel_l2(dd[0], ref_d[0]) < 1e-3, rel_l2(dd[0], ref_d[0])
        _, grads = g.render_d_rev(o, adj, want=["sec_edge", "tri_info"], with_image=False)
        _, hg, hdir = host_light_rev(tb, o, d, adj, want=["sec_edge", "tri_info"])
        for n in ("sec_edge", "tri_info"):
            assert np.abs(hg[n]).max() > 0 and rel_l2(grads[n], hg[n]) < 1e-4, (name, n, rel_l2(grads[n], hg[n]))
        assert np.abs(hdir).max() > 0 and rel_l2(g.light_grad(), hdir) < 1e-4, (g.light_grad(), hdir)


# ---------------------------------------------------------------- 5. shards
def test_shards_sum_to_the_full_launch():
    """spp / sppe / sppse shards of psdr_render_d_fwd sum to the unsharded launch: 1e-6"""
    sc, P = load_scene("cbox_occluder", res=16, spp=6, sppe=4, sppse=8, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    g = KindScene(tb).set_kind_light(DISTANT, _dir("cbox_occluder"))
    full_img, full_d = g.render_d_fwd(point_opts(6, 4, 8, rng_offset=(1, 2, 3)), [tan])
    img, d = np.zeros_like(full_img, np.float64), np.zeros_like(full_d[0], np.float64)
    for a, b, c in (((0, 2), (0, 1), (0, 3)), ((2, 6), (1, 4), (3, 8))):
        i, dd = g.render_d_fwd(point_opts(6, 4, 8, rng_offset=(1, 2, 3), spp_range=a, sppe_range=b, sppse_range=c), [tan])
        img += i
        d += dd[0]
    assert np.abs(full_d).max() > 0
    assert rel_l2(img, full_img) < 1e-6 and rel_l2(d, full_d[0]) < 1e-6, (rel_l2(img, full_img), rel_l2(d, full_d[0]))


# ---------------------------------------------------------------- 6. kind 5: planes against kind 4
def test_stack_planes_are_the_kind_4_launches():
    """L = 1 and L = 256 all distant at 8 x 8 x 1 with a guard plane of NaN, and stacks of six -- all distant and mixed -- at 19 x 19 x 3 and 32 x 32 x 16: every
    plane within 4 eps32 of its maximum, per pixel, of the kind-4 launch of its light (section 18's bound); forward mode's planes at 1e-5 rel-L2 (that file's
    bound between launches); the point planes of the mixed stack against the same lights in an all-point stack through the OLD entry point, bit for bit."""
    tb = load_scene("cbox_occluder", res=8, spp=1)[0].tables(0)
    g = KindScene(tb)
    o, po = stack_opts(1, rng_offset=(5, 0, 0)), point_opts(1, rng_offset=(5, 0, 0))
    rng = np.random.default_rng(11)
    dirs = np.stack([rng.uniform(-0.6, 0.6, 256), rng.uniform(-0.2, 1.2, 256), rng.uniform(0.6, 2.0, 256)], axis=1).astype(np.float32)
    dirs[255] = STACK_DIRS[1]
    for L in (1, 256):
        img = g.set_kind_lights(np.full(L, DISTANT), dirs[256 - L:]).stack_render_c(o, guard_planes=1)
        assert np.isfinite(img[:L]).all() and np.isnan(img[L]).all()
        _planes_match(img[L - 1], g.set_kind_light(DISTANT, dirs[255]).render_c(po), L)
        assert img[L - 1].max() > 0
        if L == 256:
            for l in (0, 100):
                _planes_match(img[l], g.set_kind_light(DISTANT, dirs[l]).render_c(po), l)
    worst = 0.0
    for res, spp in ((19, 3), (32, 16)):
        tb = load_scene("cbox_occluder", res=res, spp=spp)[0].tables(0)
        g = KindScene(tb)
        off = (7, 0, 0)
        for kinds, v in ((np.full(6, DISTANT), STACK_DIRS), _mixed()):
            img = g.set_kind_lights(kinds, v).stack_render_c(stack_opts(spp, rng_offset=off))
            assert np.isfinite(img).all()
            for l in range(6):
                worst = max(worst, _planes_match(img[l], g.set_kind_light(kinds[l], v[l]).render_c(point_opts(spp, rng_offset=off)), (res, l)))
        kinds, v = _mixed()
        allpoint = g.set_lights(OCCLUDER_LIGHTS).stack_render_c(stack_opts(spp, rng_offset=off))
        for l in np.nonzero(kinds == POINT)[0]:
            assert np.array_equal(img[l], allpoint[l]), (res, l)
        assert np.array_equal(img[0], img[2]) and img[0].max() > 0          # coincident directions
    print("distant stacks: worst |stack plane - kind-4 launch| / (eps32 * plane max) = %.2f" % worst)
    # forward mode, geometry duals and the lights' tangents, all three terms
    sc2, P = load_scene("cbox_occluder", res=24, spp=8, sppe=8, sppse=16, translate=(1, (1.0, 0.5, 0.0)))
    tb2 = sc2.tables(0)
    tan = tangents_wrt(tb2, P)
    kinds, v = _mixed()
    dl = (np.random.default_rng(6).random((1, 6, 3)) - 0.5).astype(np.float32)
    o2, po2 = stack_opts(8, 8, 16, rng_offset=(3, 4, 5)), point_opts(8, 8, 16, rng_offset=(3, 4, 5))
    g2 = KindScene(tb2).set_kind_lights(kinds, v, d_v=dl)
    img, d = g2.stack_render_d_fwd(o2, [tan])
    for l in range(6):
        rimg, rd = g2.set_kind_light(kinds[l], v[l], d_v=dl[:, l]).render_d_fwd(po2, [tan])
        if not np.any(rd):
            assert not np.any(d[0, l])
            continue
        assert rel_l2(img[l], rimg) < 1e-5 and rel_l2(d[0, l], rd[0]) < 1e-5, (l, rel_l2(d[0, l], rd[0]))


def test_stack_reverse_mode():
    """the mixed stack of six: <A, J t> = <J^T A, t> per table and per light's vector (1e-4 of the scale), the tables and g_v against the sum of kind-4 reverse
    launches over the lights (1e-4, section 18's)"""
    res, spp, sppe, sppse = 16, 4, 4, 8
    tb = load_scene("cbox_occluder", res=res, spp=spp, sppe=sppe, sppse=sppse)[0].tables(0)
    kinds, v = _mixed()
    L = 6
    A = np.random.default_rng(5).random((L, res * res, 3)).astype(np.float32)
    A64 = A.astype(np.float64)
    o, po = stack_opts(spp, sppe, sppse, rng_offset=(2, 3, 4)), point_opts(spp, sppe, sppse, rng_offset=(2, 3, 4))
    names = ["tri_info", "texels", "cam_to_world", "prim_edge", "sec_edge"]
    g = KindScene(tb).set_kind_lights(kinds, v, want_grad=True)
    img_r, grads = g.stack_render_d_rev(o, A, want=names)
    g_v = g.lights_grad()
    for n in names:
        tan = random_tangents(tb, [n], seed=1)
        img, dimg = g.set_kind_lights(kinds, v).stack_render_d_fwd(o, [tan])
        assert rel_l2(img_r, img) < 1e-5
        lhs, rhs, scale = float((A64 * dimg[0]).sum()), dot_tables(grads, tan), float(np.abs(A64 * dimg[0]).sum())
        assert scale > 0 and abs(lhs - rhs) <= 1e-4 * scale, (n, lhs, rhs, scale)
    dl = (np.random.default_rng(6).random((1, L, 3)) - 0.5).astype(np.float32)
    _, dimg = g.set_kind_lights(kinds, v, d_v=dl).stack_render_d_fwd(o, [{}])
    for l in range(L):
        lhs, rhs, scale = float((A64[l] * dimg[0, l]).sum()), float(g_v[l].astype(np.float64) @ dl[0, l]), float(np.abs(A64[l] * dimg[0, l]).sum())
        assert abs(lhs - rhs) <= 1e-4 * max(scale, 1e-6), (l, lhs, rhs, scale)
    total = {n: np.zeros_like(grads[n], np.float64) for n in grads}
    for l in range(L):
        g.set_kind_light(kinds[l], v[l], want_grad=True)
        _, g1 = g.render_d_rev(po, A[l], want=names)
        gv1 = g.light_grad()
        for n in g1:
            total[n] += g1[n]
        if np.any(gv1):
            assert rel_l2(g_v[l], gv1) < 1e-4, (l, g_v[l], gv1)
        else:
            assert not np.any(g_v[l])
    for n in total:
        assert np.abs(total[n]).max() > 0 and rel_l2(grads[n], total[n]) < 1e-4, (n, rel_l2(grads[n], total[n]))


# ---------------------------------------------------------------- 7. kind 5: the edge terms
def test_stack_edge_terms_alone():
    """an empty spp range: only the edge kernels run, once per light with the light's kind.  One-wave launches (8 x 8, one sppe / sppse slot per pixel in the
    shard): bit for bit the kind-4 launch's, after checking that kind 4 reproduces itself there.  Launches of several waves (16 x 16, sppe 4, sppse 16), where
    the order of the float atomics differs from launch to launch: within 4 eps32 of the plane's maximum."""
    S = 4
    sc, P = load_scene("cbox_occluder", res=8, spp=1, sppe=S, sppse=S, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    kinds, v = _mixed()
    g = KindScene(tb).set_kind_lights(kinds, v)
    nonzero = 0
    for i in range(S):
        kw = dict(rng_offset=(0, 8, 9), spp_range=(0, 0), sppe_range=(i, i + 1), sppse_range=(i, i + 1))
        img, d = g.stack_render_d_fwd(stack_opts(1, S, S, **kw), [tan])
        assert not np.any(img)
        for l in range(6):
            ref = g.set_kind_light(kinds[l], v[l]).render_d_fwd(point_opts(1, S, S, **kw), [tan])[1][0]
            again = g.render_d_fwd(point_opts(1, S, S, **kw), [tan])[1][0]
            assert np.array_equal(again, ref), ("kind 4 does not reproduce itself", i, l)
            assert np.array_equal(d[0, l], ref), (i, l)
            nonzero += int(np.count_nonzero(ref)) if kinds[l] == DISTANT else 0
    assert nonzero > 20, nonzero
    sc, P = load_scene("cbox_occluder", res=16, spp=4, sppe=4, sppse=16, translate=(1, (1.0, 0.5, 0.0)))
    tb = sc.tables(0)
    tan = tangents_wrt(tb, P)
    kw = dict(rng_offset=(0, 8, 9), spp_range=(0, 0))
    g = KindScene(tb).set_kind_lights(kinds, v)
    img, d = g.stack_render_d_fwd(stack_opts(4, 4, 16, **kw), [tan])
    assert not np.any(img)
    for l in range(6):
        ref = g.set_kind_light(kinds[l], v[l]).render_d_fwd(point_opts(4, 4, 16, **kw), [tan])[1][0]
        print("distant edge terms alone, light %d: |stack plane - kind 4| / (eps32 * max) = %.2f" % (l, _planes_match(d[0, l], ref, l)))


# ---------------------------------------------------------------- 8. error returns
def test_error_returns():
    """every message of the new entry points, before any launch; the old entry points unchanged (they mean PSDR_LIGHT_POINT and take the origin as a position)"""
    tb = load_scene("cbox", res=8, spp=1)[0].tables(0)
    g = KindScene(tb)
    o, so = point_opts(1), stack_opts(1)
    with pytest.raises(RuntimeError, match="no light set"):
        g.render_c(o)
    with pytest.raises(RuntimeError, match="unknown light kind 2"):
        g.set_kind_light(2, (0.0, 0.0, 1.0))
    with pytest.raises(RuntimeError, match="direction is not finite"):
        g.set_kind_light(DISTANT, (0.0, float("inf"), 1.0))
    with pytest.raises(RuntimeError, match="direction is all zero"):
        g.set_kind_light(DISTANT, (0.0, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="position is not finite"):
        g.set_kind_light(POINT, (0.0, float("nan"), 1.0))
    with pytest.raises(RuntimeError, match="K must be"):
        g.set_kind_light(DISTANT, (0.0, 0.0, 1.0), d_v=np.zeros((4, 3), np.float32))
    with pytest.raises(RuntimeError, match="no light set"):          # a refused call sets nothing
        g.render_c(o)
    assert g.set_kind_light(POINT, (0.0, 0.0, 0.0)).render_c(o) is not None          # the origin is a position
    assert g.set_light((0.0, 0.0, 0.0)).render_c(o) is not None
    with pytest.raises(RuntimeError, match="not finite"):
        g.set_light((0.0, float("inf"), 0.0))
    img_d = g.set_kind_light(DISTANT, (0.23, 0.51, 1.0)).render_c(o)
    with pytest.raises(RuntimeError, match="K must be"):          # a refused call of either entry point leaves the light, its kind included, as it is
        g.set_light((0.23, 0.51, 1.0), d_pos=np.zeros((4, 3), np.float32))
    with pytest.raises(RuntimeError, match="K must be"):
        g.set_kind_light(POINT, (0.23, 0.51, 1.0), d_v=np.zeros((4, 3), np.float32))
    assert np.array_equal(g.render_c(o), img_d)
    img_p = g.set_light((0.23, 0.51, 1.0)).render_c(o)          # the OLD entry point means a point light, also after a distant one
    assert img_d.max() > 0 and not np.array_equal(img_d, img_p)
    g.set_kind_light(DISTANT, None)
    with pytest.raises(RuntimeError, match="no light set"):
        g.render_c(o)
    # the stack
    g.L = 1
    with pytest.raises(RuntimeError, match="no lights set"):
        g.stack_render_c(so)
    two = np.array([(0.0, 0.0, 1.0), (1.0, 0.0, 1.0)], np.float32)
    with pytest.raises(RuntimeError, match="unknown light kind 7 of light 1"):
        g.set_kind_lights([DISTANT, 7], two)
    with pytest.raises(RuntimeError, match="direction of light 1 is not finite"):
        g.set_kind_lights([POINT, DISTANT], [(0.0, 0.0, 0.0), (0.0, float("inf"), 1.0)])
    with pytest.raises(RuntimeError, match="direction of light 0 is all zero"):
        g.set_kind_lights([DISTANT, POINT], [(0.0, 0.0, 0.0), (1.0, 0.0, 1.0)])
    with pytest.raises(RuntimeError, match="position of light 1 is not finite"):
        g.set_kind_lights([DISTANT, POINT], [(0.0, 0.0, 1.0), (0.0, float("nan"), 1.0)])
    with pytest.raises(RuntimeError, match="L must be"):
        g.set_kind_lights(np.zeros(257, np.int32), np.ones((257, 3), np.float32))
    g.L = 1
    with pytest.raises(RuntimeError, match="no lights set"):
        g.stack_render_c(so)
    assert np.isfinite(g.set_kind_lights([POINT, DISTANT], [(0.0, 0.0, 0.0), (0.0, 0.5, 1.0)]).stack_render_c(so)).all()
    g.set_kind_lights(None, None)
    g.L = 1
    with pytest.raises(RuntimeError, match="no lights set"):
        g.stack_render_c(so)
    # an environment map: the stack with one distant light is refused, the all-point stack renders
    tbe = load_scene("cbox_env", res=8, spp=1)[0].tables(0)
    ge = KindScene(tbe).set_kind_lights([POINT, DISTANT], [(10.3, 100.7, 300.9), (0.0, 0.5, 1.0)])
    with pytest.raises(RuntimeError, match=ENV_MESSAGE):
        ge.stack_render_c(so)
    assert ge.set_kind_lights([POINT, POINT], [(10.3, 100.7, 300.9), (0.0, 100.5, 300.0)]).stack_render_c(so).max() > 0


# ---------------------------------------------------------------- 9. the Python surface
def _surface_scene(res=16, spp=4, sppe=4, sppse=8, name="cbox_occluder"):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(name), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    return sc


def test_python_surface_matches_the_c_abi():
    """DistantLightIntegrator.renderC / renderD against the C ABI on the same tables and RNG offsets; enoki.forward through the direction; enoki.backward to the
    irradiance and the direction; LightStageIntegrator(distant=...) stacked and combined, its gradients of m_positions and m_intensities against the C ABI's."""
    d, irr = (0.23, 0.51, 1.0), (2.0, 1.0, 0.5)
    scale = np.asarray(irr, np.float32)[None, :]
    sc = _surface_scene()
    sc.configure()
    integ = psdr_cuda.DistantLightIntegrator(d, irr)
    tb = sc.tables(0)
    g = KindScene(tb).set_kind_light(DISTANT, d)
    ref = g.render_c(point_opts(4, rng_offset=tuple(sc._rng_offset))) * scale
    img = integ.renderC(sc).numpy()
    assert ref.max() > 0 and rel_l2(img, ref) < 1e-6, rel_l2(img, ref)
    P = FloatD(0.)
    ek.set_requires_gradient(P)
    integ.m_direction = Vector3fD(list(d)) + Vector3fD([1.0, 0.5, -0.2]) * P
    off = tuple(sc._rng_offset)
    imgd = integ.renderD(sc)
    ek.forward(P)
    dd = ek.gradient(imgd).numpy()
    g.set_kind_light(DISTANT, d, d_v=np.array([[1.0, 0.5, -0.2]], np.float32))
    ref_img, ref_d = g.render_d_fwd(point_opts(4, 4, 8, rng_offset=off), [{}])
    assert rel_l2(imgd.numpy(), ref_img * scale) < 1e-6 and np.abs(ref_d).max() > 0
    assert rel_l2(dd, ref_d[0] * scale) < 1e-5, rel_l2(dd, ref_d[0] * scale)
    integ2 = psdr_cuda.DistantLightIntegrator(d, irr)
    ek.set_requires_gradient(integ2.m_direction)
    ek.set_requires_gradient(integ2.m_intensity)
    off = tuple(sc._rng_offset)
    imgd = integ2.renderD(sc)
    w = torch.as_tensor(np.random.default_rng(3).random((16 * 16, 3)).astype(np.float32), device=imgd.t.device)
    ek.backward(FloatD._wrap((imgd.t * w).sum().reshape(1)))
    gd, gi = ek.gradient(integ2.m_direction).numpy().reshape(3), ek.gradient(integ2.m_intensity).numpy().reshape(3)
    g.set_kind_light(DISTANT, d, want_grad=True)
    unit_img, _ = g.render_d_rev(point_opts(4, 4, 8, rng_offset=off), (w.cpu().numpy() * scale).astype(np.float32), want=[])
    ref_gd, ref_gi = g.light_grad(), (unit_img.astype(np.float64) * w.cpu().numpy()).sum(axis=0)
    print("distant python surface: g_dir %s ref %s, g_irradiance %s ref %s" % (gd, ref_gd, gi, ref_gi))
    assert np.abs(ref_gd).max() > 0 and rel_l2(gd, ref_gd) < 1e-5 and rel_l2(gi, ref_gi) < 1e-5
    # the stack: mixed kinds, stacked and combined
    kinds, v = _mixed()
    L = 6
    inten = np.random.default_rng(2).uniform(0.5, 2.0, (L, 3)).astype(np.float32)
    flags = [bool(k == DISTANT) for k in kinds]
    stage = psdr_cuda.LightStageIntegrator(v, inten, distant=flags)
    off = tuple(sc._rng_offset)
    planes = stage.renderC(sc).numpy().reshape(L, -1, 3)
    refp = g.set_kind_lights(kinds, v).stack_render_c(stack_opts(4, rng_offset=off)) * inten[:, None, :]
    assert rel_l2(planes, refp) < 1e-6, rel_l2(planes, refp)
    comb = psdr_cuda.LightStageIntegrator(v, inten, combine=True, distant=flags)
    ek.set_requires_gradient(comb.m_positions)
    ek.set_requires_gradient(comb.m_intensities)
    off = tuple(sc._rng_offset)
    imgd = comb.renderD(sc)
    ek.backward(FloatD._wrap((imgd.t * w).sum().reshape(1)))
    gp, gi = ek.gradient(comb.m_positions).numpy().reshape(L, 3), ek.gradient(comb.m_intensities).numpy().reshape(L, 3)
    A = (w.cpu().numpy()[None, :, :] * inten[:, None, :]).astype(np.float32)
    g.set_kind_lights(kinds, v, want_grad=True)
    unit_planes, _ = g.stack_render_d_rev(stack_opts(4, 4, 8, rng_offset=off), A, want=[])
    ref_gp = g.lights_grad()
    ref_gi = (unit_planes.astype(np.float64) * w.cpu().numpy()[None, :, :]).sum(axis=1)
    assert rel_l2(imgd.numpy(), (unit_planes * inten[:, None, :]).sum(axis=0)) < 1e-5
    assert np.abs(ref_gp).max() > 0 and rel_l2(gp, ref_gp) < 1e-5 and rel_l2(gi, ref_gi) < 1e-5, (gp, ref_gp)
    # an environment map: raised in Python, with the native text, before the native call
    sce = _surface_scene(8, 1, 0, 0, "cbox_env")
    sce.configure()
    with pytest.raises(Exception, match=ENV_MESSAGE):
        psdr_cuda.DistantLightIntegrator(d).renderC(sce)
    with pytest.raises(Exception, match=ENV_MESSAGE):
        psdr_cuda.LightStageIntegrator(v[:2], distant=[True, False]).renderC(sce)
    assert psdr_cuda.LightStageIntegrator([(10.3, 100.7, 300.9), (0.0, 100.5, 300.0)], distant=[False, False]).renderC(sce).numpy().max() > 0          # (inside the bounding mesh)


# ---------------------------------------------------------------- 10. recovery: light calibration
CALIB_XML_QUAD = microfacet_xml(0.3, bid="mq") + quad("mq", 20.0, size=80.0, x=-40.0, y=60.0).replace('z="0"/></transform>', 'z="40"/></transform>')
CALIB_TRUE = np.array([(0.23, 0.51, 1.0), (-0.45, 0.35, 1.0), (0.1, 0.9, 1.0)], np.float64)
CALIB_LR = 0.06          # measured on the MI355X, 40 steps: 0.03 ends at a mean of 11.55 degrees (the momentum carries two lights past and back), 0.06 at 2.47, 0.1 at 5.16


def _calib_scene(spp, sppe, sppse):
    """cbox_occluder plus a MicrofacetBSDF quad (80 x 80, tilted 20 degrees, in front of the left half of the back wall), everything known"""
    xml = open(scene_path("cbox_occluder")).read().replace("</scene>", CALIB_XML_QUAD + "</scene>")

    def prep(sc):
        sc.opts.sppse = sppse
    return xml_scene(xml, 32, spp, sppe, prepare=prep)


def _angles(dirs, truth):
    return np.degrees(np.arccos(np.clip([unit(a) @ unit(b) for a, b in zip(dirs, truth)], -1.0, 1.0)))


def _calibrate(lr=CALIB_LR, steps=40, log=None):
    """the fit of test_recover_three_light_directions: (angular errors at the start, at the end)"""
    rng = np.random.default_rng(4)
    start = []
    for i, t in enumerate(CALIB_TRUE):          # turn each true direction by 15, 17.5 and 20 degrees about a random axis perpendicular to it
        axis = np.cross(unit(t), rng.normal(size=3))
        a, ang = unit(axis), np.radians(15.0 + 2.5 * i)
        start.append(unit(t) * np.cos(ang) + np.cross(a, unit(t)) * np.sin(ang))
    start = np.array(start)
    ref_scene = _calib_scene(64, 0, 0)
    targets = psdr_cuda.LightStageIntegrator(CALIB_TRUE, 1.0, distant=[True] * 3).renderC(ref_scene).torch().clone()
    sc = _calib_scene(8, 8, 16)
    dirs = Vector3fD(torch.from_numpy(start.astype(np.float32)))
    ek.set_requires_gradient(dirs)
    stage = psdr_cuda.LightStageIntegrator(dirs, 1.0, distant=[True] * 3)
    e0 = _angles(start, CALIB_TRUE)
    opt = torch.optim.Adam([dirs.t], lr=lr)
    for it in range(steps):
        opt.zero_grad()
        img = stage.renderD(sc)
        ek.backward(ek.hmean(ek.hsum(ek.sqr(img - Vector3fD._wrap(targets)))))
        if log is not None:
            log(it, _angles(dirs.numpy().astype(np.float64), CALIB_TRUE), dirs.t.grad.detach().cpu().numpy().copy())
        opt.step()
    return e0, _angles(dirs.numpy().astype(np.float64), CALIB_TRUE)


def test_recover_three_light_directions():
    """Light calibration: the scene known, three distant lights in ONE stack, their directions started 15 to 20 degrees off; Adam on the directions alone
    (m_positions of LightStageIntegrator(distant=[True] * 3)), 40 steps of CALIB_LR, 32 x 32, 8 spp, sppe 8, sppse 16, targets at 64 spp.  Condition, as in the
    sibling recoveries: the mean angular error ends below half of its start."""
    e0, e1 = _calibrate()
    print("light calibration: angular errors %s -> %s degrees (mean %.2f -> %.2f)" % (np.round(e0, 2), np.round(e1, 2), e0.mean(), e1.mean()))
    assert e1.mean() < 0.5 * e0.mean(), (e0, e1)
