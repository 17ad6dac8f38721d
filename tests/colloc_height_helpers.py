"""Scenes and the float64 closed form that the height-map tests share (tests/test_colloc_height_host.py, tests/test_colloc_height_gpu.py): MicrofacetBSDF with a
height map, DESIGN.md section 16."""
import numpy as np
import torch

import psdr_cuda
from collocated_helpers import _HEAD, xml_scene
from colloc_microfacet_helpers import F0, KD, ROUGH_MAT, _swap_bsdf, bitmap64, diffuse_xml, microfacet64, microfacet_xml
from colloc_normal_helpers import lean_texel, normal_xml, prepare_scene as _prepare_base, quad
from enoki.cuda_autodiff import Float32 as FloatD
from psdr_cuda import _abi

NEEDS_UV = "a height map needs texture coordinates"
NOT_BOTH = "a MicrofacetBSDF takes a normal map or a height map, not both"
SIGMA = 6.0          # world length per unit of height: with texels in [0, 1] on cells of 13 .. 27 world units the slopes stay below about 0.5


def height_xml(r=0.3, height=0.0, scale=SIGMA, bid="m", name="heightMap", scale_name="heightScale", kd=KD, f0=F0):
    """microfacet_xml with a constant height map and a scale as float children"""
    return microfacet_xml(r, kd, f0, bid).replace("</bsdf>", '<float name="%s" value="%.9g"/><float name="%s" value="%.9g"/></bsdf>' % (name, height, scale_name, scale))


def random_height_texels(seed=0, n=16):
    return np.random.default_rng(seed + 200).uniform(0.0, 1.0, n).astype(np.float32)


ONE_CELL = np.array([0.1, 0.9, 0.6, 0.0], np.float32)          # a 2 x 2 map: one cell, h11 - h10 - h01 + h00 = -1.4 (the cross term is all of its curvature)


def set_height_map(b, texels, res, scale=None):
    if b.height_map is None:
        b.height_map = psdr_cuda.Bitmap1fD(0.0)
    b.height_map.resolution = res
    b.height_map.data = FloatD(torch.from_numpy(np.ascontiguousarray(texels, np.float32).reshape(-1)))
    if scale is not None:
        b.height_scale.data = FloatD(torch.tensor([float(scale)]))


def prepare_scene(height=None, map_res=(4, 4), scale=None, drop_height=False, extra=None, **kw):
    """colloc_normal_helpers.prepare_scene (uv = None / "rot37" / "mirror" / "collapse", textured, planar_uv, seed) and, on every MicrofacetBSDF that has a height
    map: height = None (as loaded), "random" (4 x 4 random texels in [0, 1]) or a texel array of resolution `map_res`; scale: the scale texel; drop_height: the map
    removed again (the same scene with records of type 2)."""
    seed = kw.get("seed", 0)

    def maps(sc):
        for b in sc.m_bsdfs:
            if isinstance(b, psdr_cuda.MicrofacetBSDF) and b.height_map is not None:
                if drop_height:
                    b.height_map = None
                elif height is not None:
                    set_height_map(b, random_height_texels(seed) if isinstance(height, str) else height, (4, 4) if isinstance(height, str) else map_res, scale)
        if extra is not None:
            extra(sc)
    return _prepare_base(extra=maps, **kw)


def scene(xml, res=16, spp=4, sppe=0, **kw):
    return xml_scene(xml, res, spp, sppe, prepare=prepare_scene(**kw))


def quad_xml(bsdf, tilt=0.0, size=160.0):
    return _HEAD + bsdf + quad("m", tilt, size) + "</scene>\n"


MIXED_IDS = ("d", "c", "m", "n", "h")


def mixed_xml(only=None, tilt=30.0):
    """five 44 x 44 quads in two rows, 20 and more apart (more than a pixel of the 16 x 16 film) -- diffuse, rough conductor, microfacet, normal-mapped and
    height-mapped microfacet (record types 0 .. 4) -- or one of them alone (the five BSDFs stay declared, so every such scene runs the same kernel instance)"""
    xml = _HEAD + diffuse_xml(bid="d") + ROUGH_MAT % ("c", 0.3) + microfacet_xml(0.3, bid="m") + normal_xml(0.3, lean_texel(), bid="n") + height_xml(0.3, bid="h")
    for i, bid in enumerate(MIXED_IDS):
        if only is None or only == bid:
            xml += quad(bid, tilt, 44.0, 64.0 * (i % 3 - 1), 125.0 + 36.0 * (2 * (i // 3) - 1))
    return xml + "</scene>\n"


def room_xml(r=0.3):
    """cbox_uv (no tree) with the textured floor's BSDF replaced by a height-mapped MicrofacetBSDF"""
    return _swap_bsdf("cbox_uv", "floor_tex", height_xml(r, bid="floor_tex"))


def bunny_xml(r=0.3):
    """bunny_light (one tree) with the smooth-shaded bunny's BSDF replaced; prepare_scene(planar_uv=BUNNY) gives the mesh texture coordinates"""
    return _swap_bsdf("bunny_light", "clr2", height_xml(r, bid="clr2"))


BUNNY = ("bunny2",)
SCENES = {"quad": lambda: (quad_xml(height_xml(0.3), 30.0), dict(uv="rot37")), "room": lambda: (room_xml(), {}), "bunny": lambda: (bunny_xml(), dict(planar_uv=BUNNY))}


def named_scene(name, res, spp, sppe, height="random", **kw):
    """the three scene forms of the forward = reverse tests: the rotated-UV quad, cbox_uv with a height-mapped floor, bunny_light with a height-mapped bunny; 4 x 4
    maps on the four bilinear slots"""
    xml, extra = SCENES[name]()
    extra.update(kw)
    return scene(xml, res, spp, sppe, height=height, textured=True, **extra)


def height_record(tb):
    """(record row, texel offsets {kd, roughness, f0, scale, height}) of the first height-mapped MicrofacetBSDF of the tables"""
    rec = tb["bsdf_rec"].detach().cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    row = rec[rec[:, 0] == _abi.BSDF_MICROFACET_HEIGHT][0]
    return row, {"kd": int(row[1 + 3 * _abi.SLOT_REFLECTANCE]), "roughness": int(row[1 + 3 * _abi.SLOT_ALPHA_U]), "f0": int(row[1 + 3 * _abi.SLOT_ETA]),
                 "scale": int(row[1 + 3 * _abi.SLOT_ALPHA_V]), "height": int(row[1 + 3 * _abi.SLOT_K])}


def height_width(row):
    """the number of texel words of the record's height map"""
    return int(row[2 + 3 * _abi.SLOT_K]) * int(row[3 + 3 * _abi.SLOT_K])


# ---------------------------------------------------------------- the model in float64 numpy
def bitmap_grad64(texels, slot, u, v):
    """(h_u, h_v) of DESIGN.md section 16 in float64: the derivative of bitmap64(., 1 channel) with respect to (u, v), written out"""
    off, w, h = (int(x) for x in slot)
    if (w, h) == (1, 1):
        return np.zeros(len(u)), np.zeros(len(u))
    v = -v
    u, v = u - np.floor(u), v - np.floor(v)
    u, v = u * (w - 1), v * (h - 1)
    px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    w1x, w1y = u - px, v - py
    px, py = np.minimum(px, w - 2), np.minimum(py, h - 2)
    idx = py * w + px
    t = texels[off:off + w * h]
    h00, h10, h01, h11 = t[idx], t[idx + 1], t[idx + w], t[idx + w + 1]
    return (w - 1) * ((1 - w1y) * (h10 - h00) + w1y * (h11 - h01)), -(h - 1) * ((1 - w1x) * (h01 - h00) + w1x * (h11 - h10))


def perturbed_normal64(n, e1, e2, q, sigma, hu, hv):
    """n' of DESIGN.md section 16 for one triangle (n, e1, e2: [3]; q: its six UV words) and per-sample slopes hu, hv: [k]; n where the case is flat"""
    du1, dv1, du2, dv2 = q[2] - q[0], q[3] - q[1], q[4] - q[0], q[5] - q[1]
    det = du1 * dv2 - du2 * dv1
    n1 = np.broadcast_to(n, (len(hu), 3)).copy()
    if det == 0:
        return n1
    pu, pv = (e1 * dv2 - e2 * dv1) / det, (e2 * du1 - e1 * du2) / det
    a, b = pu - n * (n @ pu), pv - n * (n @ pv)
    J = n @ np.cross(a, b)
    if not abs(J) > 1e-20:
        return n1
    gu, gv = np.cross(b, n) / J, np.cross(n, a) / J
    m = n[None, :] - sigma * (hu[:, None] * gu[None, :] + hv[:, None] * gv[None, :])
    return m / np.linalg.norm(m, axis=1, keepdims=True)


def closed_form_image(tb, sxy, spp, fp32_uv=False):
    """The collocated image of a scene of face-normal quads with one height-mapped MicrofacetBSDF, in float64 at the film samples sxy, DESIGN.md section 16 written
    out: hit, uv and distance from the float64 tables as colloc_microfacet_helpers.closed_form_image; then the height gradient at uv, the dual basis from the
    triangle's edges and UVs, n', and the lobes (microfacet64) at the polar angle about n'.  No project code.  fp32_uv: the texture coordinates rounded to fp32 before
    the lookups wrap them (for coordinates so close to a texel border that the wrap itself is a rounding question)."""
    W, H = tb["width"], tb["height"]
    cam = tb["cam"].detach().cpu().numpy().astype(np.float64)
    s2c, tw = cam[0:16].reshape(4, 4), cam[16:32].reshape(4, 4)
    sxy = sxy.astype(np.float64)
    v = np.concatenate([sxy, np.zeros((len(sxy), 1)), np.ones((len(sxy), 1))], axis=1) @ s2c.T
    d = v[:, :3] / v[:, 3:4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ tw[:3, :3].T
    org = tw[:3, 3] / tw[3, 3]
    T = tb["tri_info"].detach().cpu().numpy().astype(np.float64)
    UV = tb["tri_uv"].detach().cpu().numpy().astype(np.float64).reshape(len(T), -1)[:, :6]
    tex = tb["texels"].detach().cpu().numpy().astype(np.float64).reshape(-1)
    row, off = height_record(tb)
    slot = lambda s: row[1 + 3 * s:4 + 3 * s]          # noqa: E731
    sigma = tex[off["scale"]]
    val = np.zeros((len(sxy), 3))
    for tri, q in zip(T, UV):
        p0, e1, e2, fn = tri[0:3], tri[3:6], tri[6:9], tri[18:21]
        hh = np.cross(d, e2)
        f = 1.0 / (hh @ e1)
        s = org - p0
        bu = f * (hh @ s)
        qq = np.cross(s, e1)
        bv = f * (d @ qq)
        t = f * (qq @ e2)
        hit = (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)
        n = fn / np.linalg.norm(fn)
        u = (q[2] - q[0]) * bu + (q[4] - q[0]) * bv + q[0]
        w = (q[3] - q[1]) * bu + (q[5] - q[1]) * bv + q[1]
        if fp32_uv:
            u, w = u.astype(np.float32), w.astype(np.float32)
        kd, f0, r = bitmap64(tex, slot(_abi.SLOT_REFLECTANCE), u, w, 3), bitmap64(tex, slot(_abi.SLOT_ETA), u, w, 3), bitmap64(tex, slot(_abi.SLOT_ALPHA_U), u, w, 1)[:, 0]
        hu, hv = bitmap_grad64(tex, slot(_abi.SLOT_K), u, w)
        n1 = perturbed_normal64(n, e1, e2, q, sigma, hu, hv)
        ok = -(d @ n) > 0
        cos = -(d * n1).sum(1)
        sin = np.linalg.norm(-d - cos[:, None] * n1, axis=1)
        wi = np.stack([sin, np.zeros_like(sin), cos], axis=1)
        fv = microfacet64(wi, wi, kd, f0, r) / (t * t)[:, None]
        fv = np.where(ok[:, None], fv, 0.0)
        val[hit] = fv[hit]
    return val.reshape(W * H, spp, 3).mean(axis=1)


# ---------------------------------------------------------------- the small recovery problem (tests/test_colloc_height_gpu.py; the step length was chosen on the host)
RECOVERY_TILTS = ((35.0, 0.0), (-35.0, 0.0), (0.0, 35.0))          # (about y, about x): the three views of colloc_normal_helpers.RECOVERY_TILTS
RECOVERY_LR, RECOVERY_STEPS, RECOVERY_INTENSITY, RECOVERY_SIGMA = 0.05, 40, 1e6, 6.0


def recovery_truth():
    """4 x 4 kd texels in [0.2, 0.8] and 4 x 4 height texels in [0, 1]"""
    rng = np.random.default_rng(11)
    return rng.uniform(0.2, 0.8, (16, 3)).astype(np.float32), rng.uniform(0.0, 1.0, 16).astype(np.float32)


def recovery_xml(tilt):
    return _HEAD + height_xml(0.4, scale=RECOVERY_SIGMA, f0=(0.08, 0.08, 0.08)) + quad("m", tilt[0], tilt_x=tilt[1]) + "</scene>\n"


def recovery_start():
    return np.full((16, 3), 0.5, np.float32), np.full(16, 0.5, np.float32)


def recovery_errors(kd, hm):
    """(mean kd texel error, mean height texel error with each map's mean removed: a constant offset of the height cannot be observed)"""
    kd_true, h_true = recovery_truth()
    hm = np.asarray(hm, np.float64).reshape(-1)
    return float(np.abs(kd - kd_true).mean()), float(np.abs((hm - hm.mean()) - (h_true.astype(np.float64) - h_true.mean())).mean())
