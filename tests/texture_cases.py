"""Texture lookups, PIXEL BY PIXEL (COVERAGE.md rows a11 and N2): the inputs, the references and the checks that tests/test_texture_cases.py (host) and
tests/test_texture_cases_gpu.py (MI355X) share.

Scenes (64 x 64, spp 1: every pixel is ONE sample, one add per pixel, so a render is deterministic and a single wrong texel fetch is a wrong pixel):
  tiny          cbox_uv with the floor's texture coordinates under an affine map (scaled 3.5x, rotated 0.3 rad, shifted by (-1.25, -1.6)): the image sweeps negative
                coordinates and several wraps of a map that is NOT periodic, in both axes
  forest        the same room plus the stock bunny and a uv-mapped grid mesh of 128 faces with a texture of its own (lookups at tree hits, texture
                coordinates from the global tri_uv table)
  one_tree      the forest tables on a handle with two_level = 0;   tiny_general: the tiny tables with tiny_variants = 0
The texel pool is padded with words no BSDF reads (random, not zero: a fetch that leaves its map shows), which moves num_texels across the 256 words up
to which the kernels read the pool from LDS (csrc/psdr_plan.h kLdsTexels) without changing the image.

The per-pixel check: the reference is the fp64 oracle with its image kept in double; the yardstick is the fp32 oracle's own distance from it,
    r = max over pixels |oracle fp32 - oracle fp64| / max |oracle fp64|            per scene, mode and quantity,
and a result passes when EVERY pixel is within C * max(r, FLOOR) of the reference on the same scale (max |oracle fp64|)."""
import functools
import os

import numpy as np
import torch

import oracle
import psdr_cuda
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from helpers import isolated_pixels_unbiased
from psdr_cuda import _abi
from psdr_cuda.fixtures import DATA_DIR, scene_path

EPS32 = float(np.finfo(np.float32).eps)
PATH, DIRECT, FIELD = _abi.INTEGRATOR_PATH, _abi.INTEGRATOR_DIRECT, _abi.INTEGRATOR_FIELD
RES = 64
KINDS = {"direct11": dict(integrator=DIRECT, bsdf_samples=1, light_samples=1), "path2": dict(integrator=PATH, max_depth=2), "path3": dict(integrator=PATH, max_depth=3)}
RNG_OFFSET = (3, 0, 0)

# FLOOR: a few fp32 epsilons of the image maximum (a pixel of that size cannot be known better in fp32).  C: the smallest of {2, 4, 8} that leaves a factor
# of 2 over the worst ratio (kernel error / max(r, FLOOR)) recorded on the MI355X ON THE SCENES THAT LEAVE OUT NO PIXEL -- 2.97 (cbox_env, d/d texels
# under PathTracer(2); the diffuse bitmap cases stay at or under 1.23; COVERAGE.md "Texture lookups per pixel" lists the ratios).  The product is built with
# -fapprox-func -freciprocal-math, its rounding is wider than the oracle's: that is what the margin is for.
# The rough-conductor scenes do NOT have that factor of 2.  Their yardstick r is trimmed (all but ROUGH_SHARE of the pixels) and their error has a long
# tail: the rough floor reaches 4.74 (DirectIntegrator) and 7.01 - 10.74 (PathTracer(2)) before its at most 4 pixels above 8 are left out, so the worst
# pixel still HELD to the bound sits near 7 of 8; bunny_env reaches 20 - 28 in that unit.  Its worst pixels (13 - 22 r) are no rough-conductor samples:
# they are the six BACKGROUND pixels within 0.013 rad of the pole (524 - 527, 589, 591 at 64 x 64), where u = atan2(x, -z) / 2 pi of the direct lookup
# has a condition of 1 / sin(theta) = 80 - 280 and the kernel's atan2 and normalisation under -fapprox-func are a few ulps wider than libm's.  They are
# rounding-sized (1e-5 to 4e-4 of the pixel), not flips; the trimmed r leaves just these pixels out of the yardstick, and against the untrimmed one they
# are 1.9 - 4.6.  The fp32 oracle ITSELF has pixels at up to 9.2 trimmed r there, and one flipped GGX sample at 3049 r (64 x 32 south, PathTracer(3))
# that the kernel reproduces to 5 digits.  8 is the top of the set the bound is chosen from; these cases pass by the exclusion the rough scenes are
# allowed (at most ROUGH_SHARE of the pixels, unbiased), not by a margin.
FLOOR = 4.0 * EPS32
C = 8.0
# rough-conductor scenes: an isolated GGX sample may resolve an epsilon-sized tie the other way; at most this share of the pixels may be left out, and
# only if helpers.isolated_pixels_unbiased finds them unbiased
ROUGH_SHARE = 0.005
KLDS_TEXELS = 256          # csrc/psdr_plan.h kLdsTexels

# (w, h, channels); the diffuse floor takes the 3-channel ones, the 1-channel 16 x 16 (256 words) is the alpha_u of the rough floor
MAPS = {"2x2": (2, 2, 3), "2x5": (2, 5, 3), "5x2": (5, 2, 3), "6x5": (6, 5, 3), "16x16": (16, 16, 3), "16x16x1": (16, 16, 1),
        "32x32": (32, 32, 3)}          # (32 x 32: reverse mode only, 3072 words -- above the 2048 of the LDS texel cache)
DIFFUSE_MAPS = ["2x2", "2x5", "5x2", "6x5", "16x16"]
# the 225 cells of a 16 x 16 map get their 3 pixels each from 160 x 160 on (the floor is a seventh of the image); 25 600 slots: still the small-launch forms
MAP_RES = {"16x16": 160}
# the diffuse table sets of the tests: name -> (scene tables, the floor's map, the grid mesh's map)
DIFFUSE_SETS = {"tiny-2x2": ("tiny", "2x2", None), "tiny-2x5": ("tiny", "2x5", None), "tiny-5x2": ("tiny", "5x2", None), "tiny-6x5": ("tiny", "6x5", None),
                "tiny-16x16": ("tiny", "16x16", None), "forest-6x5+5x2": ("forest", "6x5", "5x2"), "forest-2x5+6x5": ("forest", "2x5", "6x5"),
                "forest-16x16+2x2": ("forest", "16x16", "2x2")}


def diffuse_set(name):
    kind, fm, gm = DIFFUSE_SETS[name]
    return scene_tables(kind, fm, gm or "5x2", res=MAP_RES.get(fm, RES))


def map_values(name, seed=7):
    w, h, c = MAPS[name]
    g = torch.Generator().manual_seed(seed + 13 * w + h)
    return w, h, torch.rand(w * h, c, generator=g) * 0.8 + 0.1          # in [0.1, 0.9], not periodic


def affine_uv(uv, scale, angle, shift):
    c, s = np.cos(angle), np.sin(angle)
    m = torch.tensor([[c, -s], [s, c]], dtype=torch.float32) * scale
    return (torch.as_tensor(uv, dtype=torch.float32).cpu() @ m.T + shift).contiguous()


def _base(res):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_uv"), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 0, 0, 0
    floor = [m for m in sc.m_meshes if m.m_has_uv][0]
    floor.vertex_uv = affine_uv(floor._vertex_uv, 3.5, 0.3, torch.tensor([-1.25, -1.6])).to(floor._vertex_uv.device)
    return sc, floor


def _rough_floor(sc, floor, alpha_u="4x3"):
    """the floor as a rough conductor whose alpha_u / alpha_v / eta / k / specular reflectance are ALL bitmaps of different resolutions
    (roughconductor.cpp:40-92 does five texture lookups per call)"""
    g = torch.Generator().manual_seed(11)
    metal = psdr_cuda.RoughConductor(0.2, (0.2, 0.9, 1.1), (3.9, 2.4, 2.2))
    if alpha_u == "4x3":
        metal.alpha_u = psdr_cuda.Bitmap1fD(4, 3, FloatD(torch.rand(12, generator=g) * 0.3 + 0.08))
    else:
        w, h, v = map_values(alpha_u)
        torch.rand(12, generator=g)
        metal.alpha_u = psdr_cuda.Bitmap1fD(w, h, FloatD(v.reshape(-1) * 0.375 + 0.0425))          # in [0.08, 0.38], as the 4 x 3 one
    metal.alpha_v = psdr_cuda.Bitmap1fD(2, 5, FloatD(torch.rand(10, generator=g) * 0.3 + 0.08))
    metal.eta = psdr_cuda.Bitmap3fD(3, 3, Vector3fD(torch.rand(9, 3, generator=g) * 1.0 + 0.2))
    metal.k = psdr_cuda.Bitmap3fD(2, 2, Vector3fD(torch.rand(4, 3, generator=g) * 3.0 + 1.0))
    metal.specular_reflectance = psdr_cuda.Bitmap3fD(5, 4, Vector3fD(torch.rand(20, 3, generator=g) * 0.5 + 0.5))
    metal.m_anisotropic = True
    metal.id = "rough_tex"
    sc.add_bsdf(metal)
    floor.bsdf = metal
    floor.use_face_normals = False


def textured_scene(res=24, spp=8):
    """cbox_uv with a 6 x 5 albedo map on its floor (the stock texture coordinates)"""
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_uv"), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, 0, 0, 0
    g = torch.Generator().manual_seed(7)
    w, h = 6, 5
    data = torch.rand(w * h, 3, generator=g) * 0.8 + 0.1
    sc.param_map["BSDF[id=floor_tex]"].reflectance = psdr_cuda.Bitmap3fD(w, h, Vector3fD(data))
    sc.configure()
    return sc


def rough_textured_scene(res=24, spp=8):
    """the uv-mapped floor as a rough conductor whose alpha_u / alpha_v / eta / k / specular reflectance are ALL
    bitmaps of different resolutions (roughconductor.cpp:40-92 does five texture lookups per call)"""
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path("cbox_uv"), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, 0, 0, 0
    floor = [m for m in sc.m_meshes if m.m_has_uv][0]
    _rough_floor(sc, floor)
    sc.configure()
    return sc


GRID_N = 8          # 8 x 8 quads = 128 faces: above the 16 faces up to which a mesh stays inline in a two-level scene


def _grid_mesh():
    """a tilted panel left of the bunny, facing camera and light, with texture coordinates under an affine map of their own"""
    n = GRID_N
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    s, t = i.reshape(-1) / n, j.reshape(-1) / n
    verts = np.stack([-92.0 + 58.0 * s, 28.0 + 60.0 * t, 125.0 - 50.0 * t], axis=1)
    uv = affine_uv(np.stack([s, t], axis=1), 2.7, -0.4, 0.35 - 1.0).numpy()
    vid = lambda a, b: a * (n + 1) + b
    faces = []
    for a in range(n):
        for b in range(n):
            faces += [[vid(a, b), vid(a + 1, b), vid(a + 1, b + 1)], [vid(a, b), vid(a + 1, b + 1), vid(a, b + 1)]]
    m = psdr_cuda.Mesh()
    m.set_geometry(verts, faces, uv, faces, fname="<grid>")
    m.use_face_normals = True
    m.id = "grid"
    return m


@functools.lru_cache(maxsize=None)
def scene_tables(kind, floor_map="6x5", grid_map="5x2", res=RES, rough=None):
    """The tables of scene `kind` ("tiny" / "forest") as CPU tensors, unpadded.  floor_map / grid_map: names of MAPS (albedo of the floor / the grid mesh);
    rough: None, or the name of the rough floor's alpha_u map ("4x3" = rough_textured_scene's)."""
    sc, floor = _base(res)
    if rough is not None:
        _rough_floor(sc, floor, rough)
    else:
        w, h, v = map_values(floor_map)
        sc.param_map["BSDF[id=floor_tex]"].reflectance = psdr_cuda.Bitmap3fD(w, h, Vector3fD(v))
    if kind == "forest":
        bunny = psdr_cuda.Mesh()
        bunny.load(os.path.join(DATA_DIR, "objects", "bunny", "bunny_low.obj"))
        bunny.id = "bunny"
        # Face normals.  With interpolated normals a BSDF sample may leave its triangle at any angle to the triangle's PLANE, also within rounding of it,
        # and such a ray re-hits its own face beyond RayEpsilon or not depending on the last bits of the fp32 hit point: at 64 x 64 one sample in 4096 was
        # of that kind (PathTracer(3), pixel 3700: the two-level kernels and the one-tree kernels resolved it differently, 1809 max(r, FLOOR) apart; the fp64
        # oracle does either from origins 3 ulps apart).  No fp32 evaluation is bound to either outcome, so a per-pixel check cannot hold there.  With
        # face normals a cosine-distributed sample lies within c of the plane with probability c^2 -- 4e-6 for the c = 2e-3 at which an ulp of the
        # origin matters.  The texture lookups at tree hits are the same.
        bunny.use_face_normals = True
        a = np.deg2rad(-30.0)
        xf = np.eye(4)
        xf[:3, :3] = 0.9 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        xf[:3, 3] = [15, 45, 20]
        bunny._to_world_raw = torch.as_tensor(xf, dtype=torch.float32, device=bunny._to_world_raw.device)
        sc.add_mesh(bunny, sc.param_map["BSDF[id=white]"])
        w, h, v = map_values(grid_map, seed=23)
        tex = psdr_cuda.Diffuse()
        tex.reflectance = psdr_cuda.Bitmap3fD(w, h, Vector3fD(v))
        tex.id = "grid_tex"
        sc.add_bsdf(tex)
        sc.add_mesh(_grid_mesh(), tex)
        sc.finalize()
    else:
        assert kind == "tiny", kind
    sc.configure()
    tb = {k: (v.detach().cpu().clone() if isinstance(v, torch.Tensor) else v) for k, v in sc.tables(0).items()}
    tb["_uv_meshes"] = [i for i, m in enumerate(sc.m_meshes) if m.m_has_uv]
    return tb


# handle options of the four scene classes, and what psdr_scene_info must say of each
SCENE_OPTIONS = {"tiny": {}, "tiny_general": {"tiny_variants": 0}, "forest": {}, "one_tree": {"two_level": 0}}
SCENE_TABLES = {"tiny": "tiny", "tiny_general": "tiny", "forest": "forest", "one_tree": "forest"}


def check_scene_class(name, info, tb):
    if SCENE_TABLES[name] == "tiny":
        assert info["n_blas"] == 0 and info["n_tiny"] > 0, (name, info)
    elif name == "forest":
        assert info["n_blas"] >= 1 and info["n_tiny"] > 0, (name, info)
    else:
        assert info["n_blas"] == 0 and info["n_tiny"] == 0 and info["leaf_tris"] > 0, (name, info)          # one tree, no kernel-argument primitives


def staged(tb):
    """does a launch on these tables read the texel pool from LDS (where the scene class stages tables at all)"""
    return 0 < tb["texels"].numel() <= KLDS_TEXELS


def padded(tb, total, seed=5):
    """the tables with the texel pool grown to `total` words by words no BSDF reads (random in [0.1, 0.9])"""
    n = tb["texels"].numel()
    if total is None or total == n:
        return tb
    assert n < total, (n, total)
    out = dict(tb)
    g = torch.Generator().manual_seed(seed)
    out["texels"] = torch.cat([tb["texels"], torch.rand(total - n, generator=g) * 0.8 + 0.1]).contiguous()
    return out


def pad_tangent(t, total, seed=6):
    """a texel tangent of the unpadded pool for the pool padded to `total` words (the words no lookup reads get random values: a pool read at
    the wrong stride shows)"""
    n = t.numel()
    if total is None or total == n:
        return t
    g = torch.Generator().manual_seed(seed)
    return torch.cat([t, torch.rand(total - n, generator=g) - 0.5]).contiguous()


def bitmap_slots(tb):
    """(bsdf, slot, offset, w, h, channels) of every texture slot of the BSDF records"""
    ch = {_abi.BSDF_DIFFUSE: (3,), _abi.BSDF_ROUGHCONDUCTOR: (3, 1, 1, 3, 3)}
    out = []
    for b, r in enumerate(tb["bsdf_rec"].tolist()):
        for s, c in enumerate(ch[r[0]]):
            out.append((b, s, r[1 + 3 * s], r[2 + 3 * s], r[3 + 3 * s], c))
    return out


# ---------------------------------------------------------------------------------------------------------------- tangent sets of the forward tests
def tangent_random(tb, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"texels": (torch.rand(tb["texels"].shape, generator=g) - 0.5).float()}


def tangent_emitter(tb, seed=4):
    g = torch.Generator().manual_seed(seed)
    return {"emitter_rad": (torch.rand(tb["emitter_rad"].shape, generator=g) + 0.5).float()}          # d_texels stays NULL


def tangent_last_row_col(tb, seed=8):
    """non-zero only in the last row and the last column of every bilinear map"""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(tb["texels"].numel())
    for _, _, off, w, h, c in bitmap_slots(tb):
        if w > 1 and h > 1:
            m = torch.zeros(h, w, c)
            m[-1, :, :] = torch.rand(w, c, generator=g) + 0.5
            m[:, -1, :] = torch.rand(h, c, generator=g) + 0.5
            t[off:off + w * h * c] = m.reshape(-1)
    return {"texels": t}


def padded_tangents(tan, total):
    return {k: (pad_tangent(v, total) if k == "texels" else v) for k, v in tan.items()}


# ---------------------------------------------------------------------------------------------------------------- references
def opts(kind, **kw):
    return _abi.make_opts(spp=1, rng_offset=RNG_OFFSET, **dict(KINDS[kind], **kw))


_REF = {}


def reference(tb, kind, tangents=None, tag=None):
    """(ref64, r) of renderC, or (ref64, r, dref64, rd) of forward mode: the fp64 oracle's images in double and the fp32 oracle's distance from them.
    Cached per (tables object, kind, tag): `tb` must be a table set that lives as long as the process (scene_tables / a module-level dict)."""
    key = (id(tb), kind, tag)
    if key in _REF:
        return _REF[key]
    o = opts(kind)
    if tangents is None:
        r64 = oracle.render(tb, o, precision=1, out64=True)
        r32 = oracle.render(tb, o)
        out = (r64, yardstick(r32, r64))
    else:
        r64, d64 = oracle.render(tb, o, mode=1, tangents=tangents, precision=1, out64=True)
        r32, d32 = oracle.render(tb, o, mode=1, tangents=tangents)
        out = (r64, yardstick(r32, r64), d64, yardstick(d32, d64))
    _REF[key] = out
    _KEEP.append(tb)          # (tb stays alive: its id stays unique)
    return out


_KEEP = []


def rough_reference(tb, kind):
    """(ref64, r) of renderC on a rough-conductor scene: r over all but ROUGH_SHARE of the pixels (yardstick)"""
    key = (id(tb), kind, "rough")
    if key not in _REF:
        r64 = oracle.render(tb, opts(kind), precision=1, out64=True)
        _REF[key] = (r64, yardstick(oracle.render(tb, opts(kind)), r64, share=ROUGH_SHARE))
        _KEEP.append(tb)
    return _REF[key]


def yardstick(a32, ref64, share=0.0):
    """max over pixels |a32 - ref64| / max |ref64|; share > 0 (rough scenes): over all but that share of the pixels, the largest left out -- the
    yardstick gets the allowance the result gets"""
    e = np.abs(np.asarray(a32, np.float64) - ref64).reshape(ref64.shape[0], -1).max(1) / max(float(np.abs(ref64).max()), 1e-300)
    if share > 0:
        k = int(np.floor(share * e.size))
        e = np.sort(e)[:e.size - k]
    return float(e.max())


def pixel_ratios(a, ref64, r):
    """per pixel: |a - ref64| / max |ref64|, over max(r, FLOOR)"""
    e = np.abs(np.asarray(a, np.float64) - ref64).reshape(ref64.shape[0], -1).max(1) / max(float(np.abs(ref64).max()), 1e-300)
    return e / max(r, FLOOR)


def check_pixels(label, a, ref64, r, c=None, rough=False, keep=None):
    """EVERY pixel of `a` within c max(r, FLOOR) of the fp64 reference (keep: boolean mask of the pixels compared, default all).  rough: pixels above the
    bound are left out if they are at most ROUGH_SHARE of the image and unbiased.  Returns the worst ratio among the pixels held to the bound."""
    c = C if c is None else c
    a = np.asarray(a, np.float64)
    assert a.shape == ref64.shape and np.isfinite(a).all(), (label, a.shape, ref64.shape)
    ratio = pixel_ratios(a, ref64, r)
    if keep is not None:
        ratio = np.where(keep, ratio, 0.0)
    bad = ratio > c
    worst = float(ratio[~bad].max(initial=0.0)) if rough else float(ratio.max(initial=0.0))
    at = int(ratio.argmax())
    print("  %-58s r = %.2e  worst ratio %7.3f at pixel %d (%s against %s)%s" % (label, r, worst, at, np.array2string(a[at], precision=7), np.array2string(ref64[at], precision=7),
                                                                           ", left out: %d" % int(bad.sum()) if rough else ""))
    if rough:
        print("  %-58s pixels above 2 / 4 / 8: %d / %d / %d, the largest ratio up to 8: %.3f" % (
            "", int((ratio > 2).sum()), int((ratio > 4).sum()), int((ratio > 8).sum()), float(ratio[ratio <= 8].max(initial=0.0))))
        assert bad.mean() <= ROUGH_SHARE, "%s: %d pixels (%.2f %%) above %g max(r, floor)" % (label, int(bad.sum()), 100 * bad.mean(), c)
        isolated_pixels_unbiased(a, ref64, bad, label)
    else:
        assert not bad.any(), "%s: %d pixels above %g max(r, floor) = %.2e of the image maximum, worst ratio %.2f at pixel %d" % (
            label, int(bad.sum()), c, c * max(r, FLOOR), float(ratio.max()), int(ratio.argmax()))
    return worst


class Checks:
    """check_pixels for a test that makes several of them: every check runs and prints, done() fails with all that failed"""

    def __init__(self):
        self.failed = []

    def pixels(self, *args, **kw):
        try:
            return check_pixels(*args, **kw)
        except AssertionError as e:
            self.failed.append(str(e))
            return None

    def done(self):
        assert not self.failed, "%d checks failed:\n%s" % (len(self.failed), "\n".join(self.failed))


# ---------------------------------------------------------------------------------------------------------------- coverage and the independent anchor
def bilinear_f64(tex, w, h, c, u, v, flip_v=True):
    """Bitmap::eval (bitmap.cpp:41-89) in float64 numpy: flip, wrap, scale by (w - 1, h - 1), floor, weights BEFORE the clamp.  tex: [h * w * c]."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    t = np.asarray(tex, np.float64).reshape(h, w, c)
    if flip_v:
        v = -v
    u, v = u - np.floor(u), v - np.floor(v)
    u, v = u * (w - 1), v * (h - 1)
    px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    w1x, w1y = (u - px)[:, None], (v - py)[:, None]
    w0x, w0y = 1.0 - w1x, 1.0 - w1y
    px, py = np.minimum(px, w - 2), np.minimum(py, h - 2)
    return (t[py, px] * w0x + t[py, px + 1] * w1x) * w0y + (t[py + 1, px] * w0x + t[py + 1, px + 1] * w1x) * w1y, px, py


def mesh_uv(tb, mesh):
    """(mask, u, v): the pixels whose ONE sample hits `mesh` first, and the fp64 oracle's texture coordinates there (PSDR_FIELD_UV of the same slots;
    the other meshes' rows of tri_uv are zeroed, so their pixels read exactly (0, 0))"""
    t = dict(tb)
    uv = tb["tri_uv"].clone()
    uv[(tb["tri_mesh"] & ~_abi.TRI_FACE_NORMALS) != mesh] = 0
    t["tri_uv"] = uv
    f = oracle.render(t, _abi.make_opts(integrator=FIELD, field=_abi.FIELDS["uv"], spp=1, rng_offset=RNG_OFFSET), precision=1, out64=True)
    return (f[:, 0] != 0) | (f[:, 1] != 0), f[:, 0], f[:, 1]


def albedo_slot(tb, mesh):
    r = tb["bsdf_rec"][int(tb["mesh_bsdf"][mesh])].tolist()
    assert r[0] == _abi.BSDF_DIFFUSE
    return r[1], r[2], r[3]


def check_coverage(label, tb, mesh, w, h, min_cell=3, min_out=20):
    """every cell (px, py) of the map receives >= min_cell pixels -- the last column and row of cells included -- and >= min_out pixels have u < 0,
    u > 1, v < 0, v > 1 each"""
    m, u, v = mesh_uv(tb, mesh)
    _, px, py = bilinear_f64(np.zeros(w * h), w, h, 1, u[m], v[m])
    cells = np.zeros((h - 1, w - 1), np.int64)
    np.add.at(cells, (py, px), 1)
    out = [int((u[m] < 0).sum()), int((u[m] > 1).sum()), int((v[m] < 0).sum()), int((v[m] > 1).sum())]
    print("  %-30s %d pixels, cells %d x %d: min %d per cell; u<0 %d, u>1 %d, v<0 %d, v>1 %d" % (label, int(m.sum()), w - 1, h - 1, cells.min(), *out))
    assert cells.min() >= min_cell, (label, cells)
    assert min(out) >= min_out, (label, out)
    return cells


def white_tables(tb, mesh):
    """the tables with the albedo map of `mesh` replaced by a 1 x 1 white one (its first texel set to 1; the record says 1 x 1)"""
    off, w, h = albedo_slot(tb, mesh)
    out = dict(tb)
    out["texels"] = tb["texels"].clone()
    out["texels"][off:off + 3] = 1.0
    out["bsdf_rec"] = tb["bsdf_rec"].clone()
    b = int(tb["mesh_bsdf"][mesh])
    out["bsdf_rec"][b, 2] = 1
    out["bsdf_rec"][b, 3] = 1
    return out


def check_anchor(label, tb, mesh, tol=1e-9):
    """DirectIntegrator(1, 1) at spp 1 with the map over the same render with a white map = the albedo at the primary hit (diffuse sampling does not depend
    on the albedo: the two renders share their paths).  From the fp64 oracle this ratio must equal the float64 numpy lookup at the oracle's FIELD_UV."""
    off, w, h = albedo_slot(tb, mesh)
    m, u, v = mesh_uv(tb, mesh)
    o = opts("direct11")
    a = oracle.render(tb, o, precision=1, out64=True)
    b = oracle.render(white_tables(tb, mesh), o, precision=1, out64=True)
    lit = m & (b > 0).all(1)
    assert lit.sum() > 0.5 * m.sum() > 0, (label, int(lit.sum()), int(m.sum()))
    want, _, _ = bilinear_f64(tb["texels"][off:off + w * h * 3].numpy(), w, h, 3, u[lit], v[lit])
    err = float(np.abs(a[lit] / b[lit] - want).max())
    print("  %-30s anchor: %d lit pixels, max |ratio - numpy lookup| = %.2e" % (label, int(lit.sum()), err))
    assert err <= tol, (label, err)
    return err


# ---------------------------------------------------------------------------------------------------------------- environment map (COVERAGE.md row N2)
# lat-long maps; "3x2" carries ONE bright texel, in its last column and last row
ENV_MAPS = {"2x2": (2, 2), "3x2": (3, 2), "64x32": (64, 32)}
ENV_SCENES = {"bunny_env": ("direct11", "path3"), "cbox_env": ("direct11", "path2")}
POLE_RAD = 1e-3          # derivative comparisons leave out the pixels whose direction lies within this angle of a pole of the map


def env_map_values(name):
    w, h = ENV_MAPS[name]
    g = torch.Generator().manual_seed(31 + w)
    v = torch.rand(w * h, 3, generator=g) * 0.8 + 0.1
    if name == "3x2":
        v[-1] = torch.tensor([6.0, 5.0, 4.0])
    return w, h, v


def _rotation_onto(a, b):
    """the rotation that turns unit vector a into unit vector b (Rodrigues)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    v, c = np.cross(a, b), float(a @ b)
    k = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + k + k @ k / (1.0 + c)


def _view_direction(cam, sx, sy):
    """world direction of the camera ray through the film point (sx, sy) in [0, 1]^2 (helpers.camera_rays)"""
    cam = np.asarray(cam, np.float64)
    s2c, tw = cam[0:16].reshape(4, 4), cam[16:32].reshape(4, 4)
    v = s2c @ np.array([sx, sy, 0.0, 1.0])
    d = tw[:3, :3] @ (v[:3] / v[3])
    return d / np.linalg.norm(d)


@functools.lru_cache(maxsize=None)
def env_tables(scene, emap, pole, res=RES):
    """`scene` (bunny_env / cbox_env) under map `emap`, its toWorld rotated so that the pole `pole` (+1: v = 0, -1: v = 1) of the map lies in the upper
    left of the view -- and with it the u = 0 / 1 seam, which ends there.  (Both poles in one view is not possible: they are 180 degrees apart, the views
    25 and 30 degrees wide; the two values of `pole` cover them in turn.)"""
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(scene), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = 1, 0, 0, 0
    env = sc.param_map["Emitter[0]"]
    w, h, v = env_map_values(emap)
    env.radiance = psdr_cuda.Bitmap3fD(w, h, Vector3fD(v))
    sc.configure()
    d = _view_direction(sc.tables(0)["cam"].detach().cpu().numpy(), 0.22, 0.14)
    # the seam meridian (map frame: x = 0, z < 0) is turned about the pole so that it runs into the view, not out of it
    r = _rotation_onto([0.0, float(pole), 0.0], d)
    m = np.eye(4)
    m[:3, :3] = r
    env._to_world_raw = torch.eye(4, device=env._to_world_raw.device)
    env.set_transform(torch.as_tensor(m, dtype=torch.float32))
    sc.configure()
    tb = {k: (x.detach().cpu().clone() if isinstance(x, torch.Tensor) else x) for k, x in sc.tables(0).items()}
    assert tb["env_emitter"] >= 0 and list(tb["env_tex"][1:]) == [w, h]
    return tb


def env_background(tb):
    """(mask, u, v, pole_angle) per pixel from the fp64 oracle's PSDR_FIELD_POSITION of the same slots: the pixels whose one sample leaves the scene (its
    hit lies on the bounding box of the map), their lat-long coordinates in the map's frame (envmap.cpp:41-59) and their angle to the nearer pole"""
    p = oracle.render(tb, _abi.make_opts(integrator=FIELD, field=_abi.FIELDS["position"], spp=1, rng_offset=RNG_OFFSET), precision=1, out64=True)
    f = tb["env_f"].numpy().astype(np.float64)
    lo, hi = f[19:22], f[22:25]
    tol = 1e-5 * (hi - lo).max()
    on_box = ((np.abs(p - lo) < tol) | (np.abs(p - hi) < tol)).any(1)
    o = np.asarray(tb["cam"], np.float64)[16:32].reshape(4, 4)[:3, 3]
    d = p - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    vm = d @ f[0:9].reshape(3, 3).T
    u = np.arctan2(vm[:, 0], -vm[:, 2]) / (2 * np.pi)
    u -= np.floor(u)
    vy = np.clip(vm[:, 1], -1, 1)
    v = np.arccos(vy) / np.pi
    ang = np.minimum(np.arccos(vy), np.pi - np.arccos(vy))
    return on_box, u, v, ang


def check_env_coverage(label, tb, pole):
    """background pixels fall into the first and the last column of cells (either side of the seam) and into the pole's row of cells; at most 1 % of the
    image lies within POLE_RAD of the pole.  Returns the mask of the pixels the derivative comparisons keep."""
    w, h = tb["env_tex"][1:]
    m, u, v, ang = env_background(tb)
    px = np.minimum(np.floor(u[m] * (w - 1)).astype(int), w - 2)
    py = np.minimum(np.floor(v[m] * (h - 1)).astype(int), h - 2)
    first, last, row = int((px == 0).sum()), int((px == w - 2).sum()), int((py == (0 if pole > 0 else h - 2)).sum())
    near = m & (ang < POLE_RAD)
    print("  %-34s %d background pixels: first column %d, last column %d, pole row %d; nearest %.2e rad, within %g rad of the pole: %d" % (
        label, int(m.sum()), first, last, row, float(ang[m].min()), POLE_RAD, int(near.sum())))
    assert m.sum() >= 200 and first >= 3 and last >= 3 and row >= 3, (label, int(m.sum()), first, last, row)
    assert ang[m].min() < 0.02, (label, "the pole is not in view", float(ang[m].min()))
    assert near.mean() <= 0.01
    return ~near


def env_tangents(tb, seed=9):
    """{name: tangent set}: the map's scale, a rotation of its toWorld about the world's y axis, its texels"""
    z = torch.zeros_like(tb["env_f"])
    scale = z.clone()
    scale[18] = 1.0
    rot = z.clone()
    fw = tb["env_f"][0:9].reshape(3, 3).double()
    rot[0:9] = (fw @ torch.tensor([[0.0, 0, -1], [0, 0, 0], [1, 0, 0]], dtype=torch.float64)).float().reshape(-1)          # d/dt (Ry(t) R)^-1 at t = 0
    g = torch.Generator().manual_seed(seed)
    return {"scale": {"env_f": scale}, "rotation": {"env_f": rot}, "texels": {"texels": (torch.rand(tb["texels"].shape, generator=g) - 0.5).float()}}


def env_reference(tb, kind, tangents, tag, rough):
    """reference() for an environment-lit scene; rough (bunny_env): both yardsticks over all but ROUGH_SHARE of the pixels"""
    if not rough:
        return reference(tb, kind, tangents, tag)
    key = (id(tb), kind, tag, "rough")
    if key not in _REF:
        o = opts(kind)
        r64, d64 = oracle.render(tb, o, mode=1, tangents=tangents, precision=1, out64=True)
        r32, d32 = oracle.render(tb, o, mode=1, tangents=tangents)
        _REF[key] = (r64, yardstick(r32, r64, ROUGH_SHARE), d64, yardstick(d32, d64, ROUGH_SHARE))
        _KEEP.append(tb)
    return _REF[key]

