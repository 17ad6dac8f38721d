"""Texture lookups on the MI355X, PIXEL BY PIXEL against the fp64 oracle (run with `-m gpu`; inputs, references and checks: tests/texture_cases.py, their host
half: tests/test_texture_cases.py).  bitmap_eval reads texels from the LDS-staged pool (num_texels <= 256, the tiny and the two-level kernel instances) or
from global memory (larger pools; the general and the one-tree instances always); forward mode stages K tangent pools behind the value pool; reverse mode
scatters four weights per lookup into the LDS texel cache (<= 2048 words) or global atomics.  Every case asserts the scene class (psdr_scene_info) and the
route it meant to take, and prints its worst ratio (kernel error / max(r, FLOOR)) before it asserts."""
import numpy as np
import pytest

import texture_cases as tc
from helpers import GpuScene, host_render_rev_f64
from psdr_cuda import _abi
from test_gradient_sink_gpu import _ref as entries_against_f64

pytestmark = pytest.mark.gpu

POOLS = {"lds": 256, "global": 257}          # num_texels after padding: at the threshold and one word above it


def _gpu(name, tb, extra=None):
    g = GpuScene(tb, options=dict(tc.SCENE_OPTIONS[name], **(extra or {})))
    tc.check_scene_class(name, _abi.scene_stats(g.h), tb)
    return g


def _route(name, tb):
    """the texel route a launch of scene class `name` on these tables takes"""
    return "lds" if name in ("tiny", "forest") and tc.staged(tb) else "global"


def _tables(name, pool, **kw):
    base = tc.scene_tables(tc.SCENE_TABLES[name], **kw)
    tb = tc.padded(base, POOLS[pool])
    want = pool if name in ("tiny", "forest") else "global"
    assert tb["texels"].numel() == POOLS[pool] and _route(name, tb) == want, (name, pool, tb["texels"].numel())
    return base, tb


def _agree(chk, label, imgs, r):
    """all launch forms of one scene agree with each other within the bound they each keep against the reference"""
    names = list(imgs)
    for a in names[1:]:
        chk.pixels("%s: %s against %s" % (label, a, names[0]), imgs[a], np.asarray(imgs[names[0]], np.float64), r)


# ------------------------------------------------------------------------------------------------------------------------------------------------ renderC
@pytest.mark.parametrize("kind", ["direct11", "path3"])
@pytest.mark.parametrize("pool", list(POOLS))
@pytest.mark.parametrize("name", list(tc.SCENE_OPTIONS))
def test_render_c_per_pixel(name, pool, kind):
    base, tb = _tables(name, pool)
    ref, r = tc.reference(base, kind)
    g = _gpu(name, tb)
    label = "%s %s %s" % (name, pool, kind)
    imgs = {"default": g.render_c(tc.opts(kind))}
    if name == "forest" and kind == "path3":
        imgs["fused"] = g.render_c(tc.opts(kind, flags=_abi.FLAG_FUSED))
        imgs["wavefront"] = g.render_c(tc.opts(kind, flags=_abi.FLAG_WAVEFRONT))
    chk = tc.Checks()
    for form, img in imgs.items():
        chk.pixels("%s %s" % (label, form), img, ref, r)
    _agree(chk, label, imgs, r)
    g.close()
    chk.done()


@pytest.mark.parametrize("name", ["tiny-2x2", "tiny-2x5", "tiny-5x2", "tiny-16x16", "forest-2x5+6x5", "forest-16x16+2x2"])
def test_render_c_every_map(name):
    """the maps the cases above do not carry, at their natural pool size: 2 x 2 ... 5 x 2 staged, 16 x 16 x 3 (768 words) from global memory"""
    tb = tc.diffuse_set(name)
    cls = tc.DIFFUSE_SETS[name][0]
    g = _gpu(cls, tb)
    assert _route(cls, tb) == ("global" if "16x16" in name else "lds")
    chk = tc.Checks()
    for kind in ("direct11", "path3"):
        ref, r = tc.reference(tb, kind)
        chk.pixels("%s %s" % (name, kind), g.render_c(tc.opts(kind)), ref, r)
    g.close()
    chk.done()


@pytest.mark.parametrize("pool", list(POOLS))
def test_forest_large_launch_forms(pool):
    """from 2^16 slots a two-level scene runs PathTracer as the traced wavefront and DirectIntegrator(1, 1) as probe + dense trace + final pass
    (csrc/psdr_plan.h use_wavefront / probe_direct): 256 x 256 at spp 1, against the reference and against the forms the handle options switch back to"""
    base, tb = _tables("forest", pool, res=256)
    assert tb["width"] * tb["height"] == 1 << 16
    g, g_off = _gpu("forest", tb), _gpu("forest", tb, dict(wf_traced=0, probe=0))
    chk = tc.Checks()
    for kind in ("direct11", "path3"):
        ref, r = tc.reference(base, kind)
        imgs = {"default": g.render_c(tc.opts(kind)), "wf_traced=0 probe=0": g_off.render_c(tc.opts(kind)), "fused": g.render_c(tc.opts(kind, flags=_abi.FLAG_FUSED))}
        if kind == "path3":
            imgs["wavefront flag"] = g.render_c(tc.opts(kind, flags=_abi.FLAG_WAVEFRONT))
            imgs["binned wavefront"] = g_off.render_c(tc.opts(kind, flags=_abi.FLAG_WAVEFRONT))
        for form, img in imgs.items():
            chk.pixels("forest 256^2 %s %s %s" % (pool, kind, form), img, ref, r)
        _agree(chk, "forest 256^2 %s %s" % (pool, kind), imgs, r)
    g.close(); g_off.close()
    chk.done()


@pytest.mark.parametrize("kind", ["direct11", "path2"])
@pytest.mark.parametrize("pool", list(POOLS))
@pytest.mark.parametrize("name", ["tiny", "forest"])
def test_render_c_rough_floor_per_pixel(name, pool, kind):
    """all five parameters of the rough-conductor floor textured (133 words of maps of five resolutions, one- and three-channel)"""
    base, tb = _tables(name, pool, rough="4x3")
    ref, r = tc.rough_reference(base, kind)
    g = _gpu(name, tb)
    tc.check_pixels("rough %s %s %s" % (name, pool, kind), g.render_c(tc.opts(kind)), ref, r, rough=True)
    g.close()


def test_render_c_rough_floor_alpha_map_of_256_words():
    """alpha_u as a one-channel 16 x 16 map: 256 words on their own, behind the other maps a pool above the threshold"""
    tb = tc.scene_tables("tiny", rough="16x16x1")
    assert (16, 16) in [(w, h) for _, _, _, w, h, c in tc.bitmap_slots(tb) if c == 1] and not tc.staged(tb)
    g = _gpu("tiny", tb)
    for kind in ("direct11", "path2"):
        ref, r = tc.rough_reference(tb, kind)
        tc.check_pixels("rough tiny alpha_u 16x16 %s" % kind, g.render_c(tc.opts(kind)), ref, r, rough=True)
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------ forward mode
def _sets(base):
    return [("random", tc.tangent_random(base)), ("emitter", tc.tangent_emitter(base)), ("last", tc.tangent_last_row_col(base))]


FWD_CASES = [("tiny", "lds"), ("tiny", "global"), ("forest", "lds"), ("forest", "global"), ("one_tree", "global")]


@pytest.mark.parametrize("kind", ["direct11", "path3"])
@pytest.mark.parametrize("name,pool", FWD_CASES, ids=["%s-%s" % c for c in FWD_CASES])
def test_forward_k1_and_k3_per_pixel(name, pool, kind):
    base, tb = _tables(name, pool)
    total = tb["texels"].numel()
    g = _gpu(name, tb)
    sets = _sets(base)
    o = tc.opts(kind)
    label = "%s %s %s" % (name, pool, kind)
    chk = tc.Checks()
    img3, d3 = g.render_d_fwd(o, [tc.padded_tangents(t, total) for _, t in sets])          # K = 3; set 1 has no d_texels: its staged pool must be zeros
    for k, (tag, tan) in enumerate(sets):
        ref, r, dref, rd = tc.reference(base, kind, tan, tag)
        assert np.abs(dref).max() > 0
        img1, d1 = g.render_d_fwd(o, [tc.padded_tangents(tan, total)])                     # K = 1, that set alone
        if k == 0:
            chk.pixels("%s K=3 image" % label, img3, ref, r)
            chk.pixels("%s K=1 image" % label, img1, ref, r)
        chk.pixels("%s K=1 %s" % (label, tag), d1[0], dref, rd)
        chk.pixels("%s K=3 plane %d %s" % (label, k, tag), d3[k], dref, rd)
        chk.pixels("%s K=3 plane %d against K=1" % (label, k), d3[k], d1[0].astype(np.float64), rd)
        if tag == "emitter":
            # a path that never reaches the emitter carries no emitter tangent, and nothing else may leak into the plane
            dark = (dref == 0).all(1)
            assert dark.sum() > 100 and (d3[k][dark] == 0).all() and (d1[0][dark] == 0).all(), (label, int(dark.sum()))
    g.close()
    chk.done()


@pytest.mark.parametrize("logd", [0, 1])
@pytest.mark.parametrize("pool", list(POOLS))
def test_forward_path_tracer_log_derivative_and_dual_kernels(pool, logd):
    """PathTracer forward mode with tangents on albedo texels only, on the plain diffuse scene without a tree: the log-derivative kernel (logd = 1) or the
    dual-number kernel (logd = 0)"""
    base, tb = _tables("tiny", pool)
    g = _gpu("tiny", tb, dict(logd=logd))
    for tag, tan in (("random", tc.tangent_random(base)), ("last", tc.tangent_last_row_col(base))):
        ref, r, dref, rd = tc.reference(base, "path3", tan, tag)
        img, d = g.render_d_fwd(tc.opts("path3"), [tc.padded_tangents(tan, tb["texels"].numel())])
        tc.check_pixels("tiny %s logd=%d image" % (pool, logd), img, ref, r)
        tc.check_pixels("tiny %s logd=%d %s" % (pool, logd, tag), d[0], dref, rd)
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------ 256 / 257
@pytest.mark.parametrize("name", ["tiny", "forest"])
def test_threshold_256_257_same_bits(name):
    """A pool of 256 words (LDS) and of 257 (global memory) under the same kernel instance: only the texel source differs.
    renderC: the same bits.  Forward mode (image and derivative planes, K = 1 and 3): NOT the same bits in the product build -- 3 to 8 % of the values
    differ, by at most 0.95 fp32 epsilons of the plane's maximum (measured: 4.8e-7 absolute, 1.1e-7 of the maximum).  The cause, found by building the
    kernels once with -ffp-contract=off: every image and every plane of the two routes is then bit-identical.  bitmap_eval_from<LDS = true> and <LDS =
    false> are two instantiations of one expression, (v00 w0x + v10 w1x) w0y + (v01 w0x + v11 w1x) w1y on dual numbers, and the compiler is free to
    fuse their multiply-adds differently; the arithmetic is the same up to that.  A bilinear lookup is seven roundings deep, fusing removes up to four
    of them: the two routes may differ by a few epsilons of the lookup, and the estimator is linear in it -- bound: FLOOR = 4 epsilons of the maximum.
    (That trial build is not part of the tree: nothing here re-checks the cause.  What the bound still excludes: the padding words and the tangents behind
    them are random in [0.1, 0.9] and [-0.5, 0.5], so a fetch from a wrong word or stride moves a lookup by about 0.1 -- 10^5 times the bound.)"""
    (base, tb_in), (_, tb_out) = _tables(name, "lds"), _tables(name, "global")
    g_in, g_out = _gpu(name, tb_in), _gpu(name, tb_out)
    sets = _sets(base)
    worst = 0.0
    for kind in ("direct11", "path3"):
        o = tc.opts(kind)
        assert np.array_equal(g_in.render_c(o), g_out.render_c(o)), (name, kind, "image")
        for K in (1, 3):
            a = g_in.render_d_fwd(o, [tc.padded_tangents(t, 256) for _, t in sets[:K]])
            b = g_out.render_d_fwd(o, [tc.padded_tangents(t, 257) for _, t in sets[:K]])
            for what, x, y in [("image", a[0], b[0])] + [("plane %d" % k, a[1][k], b[1][k]) for k in range(K)]:
                e = float(np.abs(x.astype(np.float64) - y).max() / np.abs(x).max())
                worst = max(worst, e)
                print("  %s %s K=%d %s: %d of %d values differ, max |a - b| = %.2f eps32 of the maximum" % (name, kind, K, what, int((x != y).sum()), x.size, e / tc.EPS32))
                assert e <= tc.FLOOR, (name, kind, K, what, e)
    g_in.close(); g_out.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------ reverse mode
# k_max: the outlier entries allowed, 2x the number measured on the MI355X as in test_gradient_sink_gpu.py: 16 x 16 none (tiny) and 1 of 807 (forest); 32 x 32
# 18 of 3069 (tiny) and 29 of 3087 (forest), every one off by at most 2e-3 of its own magnitude sum S -- an entry of this map is reached by a handful of
# samples, and a bilinear weight is u (w - 1) minus its floor with |u| up to 9.5 and w - 1 = 31: an ulp of u is 3e-5 of a weight, above the 512 eps32 S
# of the bound for an entry made of one small-weight piece.
REV_K_MAX = {("tiny", "16x16"): 0, ("forest", "16x16"): 2, ("tiny", "32x32"): 36, ("forest", "32x32"): 58}


@pytest.mark.parametrize("fmap,cached", [("16x16", True), ("32x32", False)], ids=["lds_cache", "global_atomics"])
@pytest.mark.parametrize("name", ["tiny", "forest"])
def test_reverse_texel_gradients_per_entry(name, fmap, cached):
    """bilinear maps: four texels written per lookup; 16 x 16 x 3 words in the LDS cache, 32 x 32 x 3 = 3072 above its 2048 words"""
    tb = tc.scene_tables(name, fmap, "5x2")
    o = tc.opts("path3")
    adj = np.random.default_rng(11).random((tb["width"] * tb["height"], 3)).astype(np.float32)
    _, ref = host_render_rev_f64(tb, o, adj, want=["texels"])
    g = _gpu(name, tb)
    _, grads = g.render_d_rev(o, adj, want=["texels"], with_image=False)
    lay = _abi.rev_layout(g.h)
    print("\n%s %s: layout %s" % (name, fmap, lay))
    assert lay["tex_n"] == (tb["texels"].numel() if cached else 0), lay
    assert (tb["texels"].numel() <= 2048) == cached
    off, w, h = tc.albedo_slot(tb, tb["_uv_meshes"][0])
    assert (ref["texels"][1][off:off + w * h * 3] > 0).mean() > 0.9          # (the 64 x 64 image reaches nearly every texel)
    entries_against_f64("%s %s" % (name, fmap), grads, ref, ["texels"], REV_K_MAX[(name, fmap)])
    g.close()


# ------------------------------------------------------------------------------------------------------------------------------------------------ environment map
ENV_CASES = [(s, m, p) for s in tc.ENV_SCENES for m in tc.ENV_MAPS for p in (1, -1)]
ENV_IDS = ["%s-%s-%s" % (s, m, "north" if p > 0 else "south") for s, m, p in ENV_CASES]


def _env_gpu(scene, tb):
    """bunny_env: the bunny in one tree; cbox_env: floor + bunny + light in one tree.  A scene with an environment map stages no tables (csrc/psdr_plan.h
    small_tables_fit): its lookups read global memory whatever the size of the pool"""
    g = GpuScene(tb)
    info = _abi.scene_stats(g.h)
    assert info["n_blas"] == 0 and info["leaf_tris"] > 0 and tb["env_emitter"] >= 0, info
    return g


@pytest.mark.parametrize("scene,emap,pole", ENV_CASES, ids=ENV_IDS)
def test_env_render_c_and_forward_per_pixel(scene, emap, pole):
    """the pole and the u = 0 / 1 seam of the lat-long lookup in the background: renderC, and forward mode (K = 3) with the map's scale, a rotation of its
    toWorld and its texels.  Pixels within POLE_RAD of the pole are left out of the derivative comparisons only (1 / sin(theta) in env_eval_vjp; the
    lookup itself jumps at v = 1) -- they must still be finite."""
    tb = tc.env_tables(scene, emap, pole)
    rough = scene == "bunny_env"
    keep = tc.check_env_coverage("%s %s %+d" % (scene, emap, pole), tb, pole)
    g = _env_gpu(scene, tb)
    tans = tc.env_tangents(tb)
    for kind in tc.ENV_SCENES[scene]:
        label = "%s %s %+d %s" % (scene, emap, pole, kind)
        ref, r = tc.rough_reference(tb, kind) if rough else tc.reference(tb, kind)
        tc.check_pixels(label + " renderC", g.render_c(tc.opts(kind)), ref, r, rough=rough)
        img, d = g.render_d_fwd(tc.opts(kind), list(tans.values()))
        assert np.isfinite(img).all() and np.isfinite(d).all(), label
        tc.check_pixels(label + " forward image", img, ref, r, rough=rough)
        for k, (tag, tan) in enumerate(tans.items()):
            _, _, dref, rd = tc.env_reference(tb, kind, tan, tag, rough)
            assert np.abs(dref).max() > 0
            tc.check_pixels("%s d/d %s" % (label, tag), d[k], dref, rd, rough=rough, keep=keep)
    g.close()


# k_max: 2x the outlier entries measured on the MI355X (as test_gradient_sink_gpu.py does); every one of them is off by at most 2.5e-3 of its own magnitude sum.
# Measured, env_f + texels: bunny_env 2 x 2 north 3 + 0, south 3 + 0; 3 x 2 north 0, south 2 + 0; 64 x 32 north 1 + 0, south 0; cbox_env 2 x 2 and 3 x 2 none,
# 64 x 32 north 0 + 10 (of 3411), south 0 + 9 (of 3456).
# The 2 x 2 map on bunny_env: the 3 outliers are env_f[3..5], the row of the from-world matrix that yields v.y, off by 1800 - 2300 eps32 S (2.6e-4 S); the
# other seven entries are within 2.6 eps32 S, and the host harness in fp32 keeps all ten within 16.  The error vector (+0.025, -0.034, +0.21 for either
# pole) is parallel to the pole's direction: it comes from the few background samples next to the pole (the nearest at 0.0036 rad), through
# a_v.y = -a_tv / (pi sqrt(1 - v.y^2)) in env_eval_vjp (csrc/psdr_reverse.h).  There 1 - v.y^2 = 1.3e-5 cancels: one ulp of v.y^2 (6e-8) is 0.5 % of it,
# those samples carry 1 / sin(theta) = 100 - 280 times an ordinary piece, and the GPU build (contracted multiply-adds) rounds the difference otherwise
# than the host.  With h = 2 all of v is one cell, so d value / d v is the full top-to-bottom contrast at the pole too; 3 x 2 shows the same at 7e-5 S.
# Not a flip and not a wrong fetch: a conditioning weakness of that line (v.x^2 + v.z^2 is at hand and does not cancel) -- COVERAGE.md row N8, left open.
ENV_K_MAX = {("bunny_env", "2x2", 1): 6, ("bunny_env", "2x2", -1): 6, ("bunny_env", "3x2", -1): 4, ("bunny_env", "64x32", 1): 2,
             ("cbox_env", "64x32", 1): 20, ("cbox_env", "64x32", -1): 18}


@pytest.mark.parametrize("scene,emap,pole", ENV_CASES, ids=ENV_IDS)
def test_env_reverse_gradients_per_entry(scene, emap, pole):
    tb = tc.env_tables(scene, emap, pole)
    o = tc.opts("direct11")
    adj = np.random.default_rng(11).random((tb["width"] * tb["height"], 3)).astype(np.float32)
    names = ["env_f", "texels"]
    _, ref = host_render_rev_f64(tb, o, adj, want=names)
    g = _env_gpu(scene, tb)
    _, grads = g.render_d_rev(o, adj, want=names, with_image=False)
    lay = _abi.rev_layout(g.h)
    print("\n%s %s %+d: layout %s" % (scene, emap, pole, lay))
    assert lay["env_n"] == _abi.ENV_WORDS and lay["tex_n"] == (tb["texels"].numel() if tb["texels"].numel() <= 2048 else 0), lay
    assert all(np.isfinite(grads[n]).all() and np.abs(grads[n]).max() > 0 for n in names)
    entries_against_f64("%s %s %+d" % (scene, emap, pole), grads, ref, names, ENV_K_MAX.get((scene, emap, pole), 0))
    g.close()
