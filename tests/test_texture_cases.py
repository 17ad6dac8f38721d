"""Texture lookups per pixel, the host half (no GPU): the inputs of tests/test_texture_cases_gpu.py cover what they claim (every cell of every map, negative and
wrapped coordinates), the fp64 oracle's own Bitmap::eval is pinned against a float64 numpy lookup that shares no code with it, the product code on the host
(hostcheck) passes the per-pixel check the GPU has to pass, and the check catches seeded defects an image-level norm does not."""
import numpy as np
import pytest
import torch

import texture_cases as tc
from helpers import entry_errors, host_render, host_render_rev, host_render_rev_f64, rel_l2
from test_gradient_sink_gpu import C_REF, FLOOR as ENTRY_FLOOR


def _uv_maps(name):
    kind, fm, gm = tc.DIFFUSE_SETS[name]
    tb = tc.diffuse_set(name)
    return tb, list(zip(tb["_uv_meshes"], [fm] + ([gm] if gm else [])))


@pytest.mark.parametrize("name", list(tc.DIFFUSE_SETS))
def test_every_cell_and_every_wrap_is_in_view(name):
    tb, maps = _uv_maps(name)
    assert len(maps) == len(tb["_uv_meshes"])
    for mesh, m in maps:
        w, h, _ = tc.MAPS[m]
        assert tc.albedo_slot(tb, mesh)[1:] == (w, h)
        tc.check_coverage("%s mesh %d %s" % (name, mesh, m), tb, mesh, w, h)


@pytest.mark.parametrize("name", list(tc.DIFFUSE_SETS))
def test_oracle_lookup_equals_numpy_bilinear(name):
    tb, maps = _uv_maps(name)
    for mesh, m in maps:
        tc.check_anchor("%s mesh %d %s" % (name, mesh, m), tb, mesh)


def test_numpy_bilinear_by_hand():
    """the anchor itself on values worked out by hand: a 3 x 2 one-channel map 0 1 2 / 10 11 12"""
    t = [0, 1, 2, 10, 11, 12]
    f = lambda u, v: float(tc.bilinear_f64(t, 3, 2, 1, [u], [v], flip_v=False)[0][0, 0])
    assert f(0.0, 0.0) == 0 and f(0.25, 0.0) == 0.5 and f(0.75, 0.5) == 1.5 + 5.0
    assert f(1.25, 0.0) == 0.5 and f(-0.25, 0.0) == 1.5                              # wraps
    assert abs(f(1.0 - 1e-12, 1.0 - 1e-12) - 12.0) < 1e-10                           # last column and row of cells
    assert float(tc.bilinear_f64(t, 3, 2, 1, [0.0], [0.75])[0][0, 0]) == 2.5          # flipped: v = -0.75 wraps to 0.25


HOST_SETS = ["tiny-6x5", "tiny-16x16", "forest-6x5+5x2"]


@pytest.mark.parametrize("kind", ["direct11", "path2", "path3"])
@pytest.mark.parametrize("name", HOST_SETS)
def test_host_harness_per_pixel(name, kind):
    tb = tc.diffuse_set(name)
    ref, r = tc.reference(tb, kind)
    tc.check_pixels("host %s %s renderC" % (name, kind), host_render(tb, tc.opts(kind)), ref, r)
    for tag, tan in (("random", tc.tangent_random(tb)), ("last", tc.tangent_last_row_col(tb))):
        ref, r, dref, rd = tc.reference(tb, kind, tan, tag)
        img, dimg = host_render(tb, tc.opts(kind), mode=1, tangents=tan)
        assert np.abs(dref).max() > 0
        tc.check_pixels("host %s %s forward image" % (name, kind), img, ref, r)
        tc.check_pixels("host %s %s forward d/d texels (%s)" % (name, kind, tag), dimg, dref, rd)


@pytest.mark.parametrize("name", ["tiny-6x5", "forest-6x5+5x2"])
def test_host_harness_texel_gradients_per_entry(name):
    tb = tc.diffuse_set(name)
    o = tc.opts("path3")
    adj = np.random.default_rng(11).random((tb["width"] * tb["height"], 3)).astype(np.float32)
    _, ref = host_render_rev_f64(tb, o, adj, want=["texels"])
    _, g = host_render_rev(tb, o, adj, want=["texels"])
    ratio, bad = entry_errors(g["texels"], ref["texels"], C_REF, ENTRY_FLOOR)
    print("  host %s: texel gradient, worst entry at %.3f of its bound, %d live entries" % (name, ratio, int((ref["texels"][1] > 0).sum())))
    assert not bad.any() and (ref["texels"][1] > 0).sum() >= 90, (ratio, int(bad.sum()))
    # every texel of the last row and column of the floor's map is reached
    off, w, h = tc.albedo_slot(tb, tb["_uv_meshes"][0])
    live = (ref["texels"][1][off:off + w * h * 3] > 0).reshape(h, w, 3)
    assert live.all()


@pytest.mark.parametrize("name", ["tiny", "forest"])
@pytest.mark.parametrize("kind", ["direct11", "path2"])
def test_host_harness_rough_floor_stays_under_the_cap(name, kind):
    """the five-texture rough-conductor floor: the host harness against the fp64 oracle leaves out at most ROUGH_SHARE of the pixels (the cap the GPU test uses)"""
    tb = tc.scene_tables(name, rough="4x3")
    o = tc.opts(kind)
    ref, r = tc.rough_reference(tb, kind)
    tc.check_pixels("host rough %s %s" % (name, kind), host_render(tb, o), ref, r, rough=True)


# ------------------------------------------------------------------------------------------------------------------------------------------------
# the checks catch seeded defects: the fp32 host harness stands in for a perfect GPU and is fed damaged tables
def _damaged(tb, what):
    off, w, h = tc.albedo_slot(tb, tb["_uv_meshes"][0])
    out = dict(tb)
    t = tb["texels"].clone()
    m = t[off:off + w * h * 3].reshape(h, w, 3)
    if what == "last_column_texel":
        m[h // 2, w - 1, :] *= 1.02
    elif what == "rolled":
        m[:] = torch.roll(m, 1, dims=1)
    out["texels"] = t
    return out


def test_the_per_pixel_check_catches_what_an_image_norm_does_not():
    tb = tc.diffuse_set("tiny-16x16")
    kind = "path3"
    ref, r = tc.reference(tb, kind)
    good = host_render(tb, tc.opts(kind))
    tc.check_pixels("host undamaged", good, ref, r)
    sharper = 0
    for what in ("last_column_texel", "rolled"):
        img = host_render(_damaged(tb, what), tc.opts(kind))
        l2 = rel_l2(img, ref)
        print("  %s: rel_l2 %.2e" % (what, l2))
        with pytest.raises(AssertionError, match="pixels above"):
            tc.check_pixels("host, " + what, img, ref, r)
        sharper += l2 < 1e-4
    # a tangent pool read one word off
    tan = tc.tangent_random(tb)
    ref, r, dref, rd = tc.reference(tb, kind, tan, "random")
    _, dgood = host_render(tb, tc.opts(kind), mode=1, tangents=tan)
    tc.check_pixels("host undamaged tangent", dgood, dref, rd)
    _, dimg = host_render(tb, tc.opts(kind), mode=1, tangents={"texels": torch.roll(tan["texels"], 1)})
    with pytest.raises(AssertionError, match="pixels above"):
        tc.check_pixels("host, tangent pool shifted by one word", dimg, dref, rd)
    assert sharper >= 1, "no seeded defect passed rel_l2 < 1e-4: the per-pixel check was not shown to be the sharper one"


# ------------------------------------------------------------------------------------------------------------------------------------------------
# environment map: the pole and the seam of the lat-long lookup in view
ENV_CASES = [(s, m, p) for s in tc.ENV_SCENES for m in tc.ENV_MAPS for p in (1, -1)]


@pytest.mark.parametrize("scene,emap,pole", ENV_CASES, ids=["%s-%s-%s" % (s, m, "north" if p > 0 else "south") for s, m, p in ENV_CASES])
def test_env_pole_and_seam_are_in_view_and_host_per_pixel(scene, emap, pole):
    """Every map: the coverage of the view, and the host harness's renderC per pixel.  The host harness's forward derivatives (scale, rotation, texels) are
    checked for the 3 x 2 map only -- the one with the bright texel in its last column and row; the 2 x 2 and 64 x 32 maps get their derivative checks on
    the GPU alone (test_texture_cases_gpu.test_env_render_c_and_forward_per_pixel runs all maps)."""
    tb = tc.env_tables(scene, emap, pole)
    keep = tc.check_env_coverage("%s %s %+d" % (scene, emap, pole), tb, pole)
    rough = scene == "bunny_env"          # (its bunny is a rough conductor)
    kind = tc.ENV_SCENES[scene][1]
    ref, r = tc.rough_reference(tb, kind) if rough else tc.reference(tb, kind)
    tc.check_pixels("host %s %s %+d %s" % (scene, emap, pole, kind), host_render(tb, tc.opts(kind)), ref, r, rough=rough)
    if emap == "3x2":
        for tag, tan in tc.env_tangents(tb).items():
            _, _, dref, rd = tc.env_reference(tb, kind, tan, tag, rough)
            _, dimg = host_render(tb, tc.opts(kind), mode=1, tangents=tan)
            assert np.abs(dref).max() > 0 and np.isfinite(dimg).all()
            tc.check_pixels("host %s %s %+d %s d/d %s" % (scene, emap, pole, kind, tag), dimg, dref, rd, rough=rough, keep=keep)
