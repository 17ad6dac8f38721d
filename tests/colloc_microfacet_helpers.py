"""Scenes, record lookups and the float64 closed form that the MicrofacetBSDF tests share (tests/test_colloc_microfacet_host.py, test_colloc_normal_host.py,
test_colloc_height_host.py and the three _gpu.py files beside them), for the three record kinds of the CollocatedIntegrator: plain, with a tangent-space normal map
(section 15) and with a height map (section 16).  KINDS holds what differs between them; everything else is written once."""
from types import SimpleNamespace

import numpy as np
import torch

import psdr_cuda
from collocated_helpers import _HEAD, xml_scene
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

MESSAGE = "MicrofacetBSDF is evaluated by the CollocatedIntegrator only"
NOT_BOTH = "a MicrofacetBSDF takes a normal map or a height map, not both"
KD, F0 = (0.6, 0.4, 0.2), (0.04, 0.06, 0.1)
ROUGH_MAT = '<bsdf id="%s" type="roughconductor"><float name="alpha" value="%g"/><rgb name="eta" value="0.2, 0.92, 1.1"/><rgb name="k" value="3.9, 2.45, 2.14"/></bsdf>\n'
FLAT = (0.5, 0.5, 1.0)
SIGMA = 6.0          # world length per unit of height: with texels in [0, 1] on cells of 13 .. 27 world units the slopes stay below about 0.5
ONE_CELL = np.array([0.1, 0.9, 0.6, 0.0], np.float32)          # a 2 x 2 height map: one cell, h11 - h10 - h01 + h00 = -1.4 (the cross term is all of its curvature)
BUNNY = ("bunny2",)


# ---------------------------------------------------------------- the <bsdf> elements
def microfacet_xml(r=0.3, kd=KD, f0=F0, bid="m"):
    return ('<bsdf id="%s" type="microfacet"><rgb name="diffuseReflectance" value="%g, %g, %g"/><rgb name="specularReflectance" value="%g, %g, %g"/>'
            '<float name="roughness" value="%g"/></bsdf>\n' % ((bid,) + tuple(kd) + tuple(f0) + (r,)))


def normal_xml(r=0.3, texel=FLAT, bid="m", name="normalMap", kd=KD, f0=F0):
    """microfacet_xml with a constant normal map as an rgb child"""
    return microfacet_xml(r, kd, f0, bid).replace("</bsdf>", '<rgb name="%s" value="%.9g, %.9g, %.9g"/></bsdf>' % ((name,) + tuple(texel)))


def height_xml(r=0.3, height=0.0, scale=SIGMA, bid="m", name="heightMap", scale_name="heightScale", kd=KD, f0=F0):
    """microfacet_xml with a constant height map and a scale as float children"""
    return microfacet_xml(r, kd, f0, bid).replace("</bsdf>", '<float name="%s" value="%.9g"/><float name="%s" value="%.9g"/></bsdf>' % (name, height, scale_name, scale))


def diffuse_xml(kd=KD, bid="m"):
    return '<bsdf id="%s" type="diffuse"><rgb name="reflectance" value="%g, %g, %g"/></bsdf>\n' % ((bid,) + tuple(kd))


def encode(v):
    """the image encoding of a normal map: v = 2c - 1"""
    return (np.asarray(v, np.float64) + 1.0) / 2.0


def lean_texel(deg=20.0):
    """a 1 x 1 normal map that leans the normal by `deg` about the u axis: v = (0, sin, cos) in (s', t', n)"""
    a = np.radians(deg)
    return tuple(float(x) for x in encode((0.0, np.sin(a), np.cos(a))))


# ---------------------------------------------------------------- maps on a loaded scene
def random_normal_texels(seed=0, n=16):
    """n texels with every decoded v.z >= 0.5 and the tangential part within +-0.6 (not unit vectors: the model normalises)"""
    rng = np.random.default_rng(seed + 100)
    v = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(0.5, 1.0, (n, 1))], axis=1)
    return encode(v).astype(np.float32)


def random_height_texels(seed=0, n=16):
    return np.random.default_rng(seed + 200).uniform(0.0, 1.0, n).astype(np.float32)


def set_normal_map(b, texels, res):
    if b.normal_map is None:
        b.normal_map = psdr_cuda.Bitmap3fD(FLAT)
    b.normal_map.resolution = res
    b.normal_map.data = Vector3fD(torch.from_numpy(np.ascontiguousarray(texels, np.float32).reshape(-1, 3)))


def set_height_map(b, texels, res, scale=None):
    if b.height_map is None:
        b.height_map = psdr_cuda.Bitmap1fD(0.0)
    b.height_map.resolution = res
    b.height_map.data = FloatD(torch.from_numpy(np.ascontiguousarray(texels, np.float32).reshape(-1)))
    if scale is not None:
        b.height_scale.data = FloatD(torch.tensor([float(scale)]))


def maps_4x4(r=0.3, seed=0, zero_roughness_texel=None):
    """prepare(sc) for xml_scene: every MicrofacetBSDF of the scene gets random 4 x 4 kd, F0 and roughness maps (roughness within r +- 0.1)"""
    def prepare(sc):
        rng = np.random.default_rng(seed)
        for b in sc.m_bsdfs:
            if not isinstance(b, psdr_cuda.MicrofacetBSDF):
                continue
            kd = rng.uniform(0.2, 0.8, (16, 3)).astype(np.float32)
            f0 = rng.uniform(0.02, 0.12, (16, 3)).astype(np.float32)
            rr = rng.uniform(r - 0.1, r + 0.1, 16).astype(np.float32)
            if zero_roughness_texel is not None:
                rr[zero_roughness_texel] = 0.0
            b.diffuse_reflectance.resolution = b.specular_reflectance.resolution = b.roughness.resolution = (4, 4)
            b.diffuse_reflectance.data = Vector3fD(torch.from_numpy(kd))
            b.specular_reflectance.data = Vector3fD(torch.from_numpy(f0))
            b.roughness.data = FloatD(torch.from_numpy(rr))
    return prepare


def prepare_scene(textured=False, r=0.3, seed=0, zero_roughness_texel=None, normal=None, drop_normal=False, height=None, map_res=(4, 4), scale=None, drop_height=False,
                  uv=None, planar_uv=None, extra=None):
    """prepare(sc) for xml_scene.
    textured: the kd, F0 and roughness maps at 4 x 4 (maps_4x4, with r, seed and zero_roughness_texel);
    normal: None (leave the BSDFs as loaded), "random" (a 4 x 4 random map on every MicrofacetBSDF that has a normal map) or a [16, 3] texel array;
    drop_normal: every normal map removed again (the same scene with records of type 2);
    height: None (as loaded), "random" (4 x 4 random texels in [0, 1] on every MicrofacetBSDF that has a height map) or a texel array of resolution `map_res`;
    scale: the scale texel; drop_height: every height map removed again;
    uv: None, "rot37" (the texture coordinates of every mesh turned by 37 degrees in the plane), "mirror" (u -> -u: det < 0) or "collapse" (all UVs equal);
    planar_uv: mesh ids that get texture coordinates uv = (x, y) / 40 of their raw vertices (meshes that come without any);
    extra: a last callable on the scene."""
    def prepare(sc):
        if textured:
            maps_4x4(r, seed, zero_roughness_texel)(sc)
        micro = [b for b in sc.m_bsdfs if isinstance(b, psdr_cuda.MicrofacetBSDF)]
        for b in micro:
            if drop_normal:
                b.normal_map = None
            elif b.normal_map is not None and normal is not None:
                set_normal_map(b, random_normal_texels(seed) if isinstance(normal, str) else normal, (4, 4))
        for m in sc.m_meshes:
            if planar_uv and m.id in planar_uv:
                m.m_has_uv = True
                m._vertex_uv = (m._vertex_positions_raw[:, :2] / 40.0).contiguous()
                m._face_uv_indices = m._face_indices.clone()
            if uv is not None and m.m_has_uv:
                t = m._vertex_uv.detach().cpu().numpy().astype(np.float64)
                if uv == "rot37":
                    c, s = np.cos(np.radians(37.0)), np.sin(np.radians(37.0))
                    t = t @ np.array([[c, s], [-s, c]])
                elif uv == "mirror":
                    t = t * np.array([-1.0, 1.0])
                elif uv == "collapse":
                    t = np.broadcast_to(t[:1], t.shape)
                else:
                    raise ValueError(uv)
                m._vertex_uv = torch.as_tensor(np.ascontiguousarray(t, np.float32), device=m._vertex_uv.device)
        for b in micro:
            if b.height_map is not None:
                if drop_height:
                    b.height_map = None
                elif height is not None:
                    set_height_map(b, random_height_texels(seed) if isinstance(height, str) else height, (4, 4) if isinstance(height, str) else map_res, scale)
        if extra is not None:
            extra(sc)
    return prepare


def scene(xml, res=16, spp=4, sppe=0, **kw):
    return xml_scene(xml, res, spp, sppe, prepare=prepare_scene(**kw))


# ---------------------------------------------------------------- scenes
def quad(ref, tilt, size=160.0, x=0.0, y=125.0, tilt_x=0.0):
    """the cbox floor quad with texture coordinates (200 x 300, uv repeat 2 x 3), centred, scaled to size x size, turned to face the camera, tilted about y and then
    about x, and moved to (x, y)"""
    return ('<shape type="obj"><string name="filename" value="./data/objects/cbox/floor_uv.obj"/><transform name="toWorld"><translate z="-50"/>'
            '<scale x="%g" z="%g"/><rotate angle="90" x="1"/><rotate angle="%g" y="1"/><rotate angle="%g" x="1"/><translate x="%g" y="%g" z="0"/></transform>'
            '<boolean name="faceNormals" value="true"/><ref id="%s"/></shape>\n' % (size / 200.0, size / 300.0, tilt, tilt_x, x, y, ref))


def uv_quad_xml(bsdf, tilt=0.0, size=160.0):
    """collocated_helpers.quad_xml with a quad that carries texture coordinates, so that a 4 x 4 map is looked up across texel borders"""
    return _HEAD + bsdf + quad("m", tilt, size) + "</scene>\n"


_MIXED_BSDF = {"d": lambda: diffuse_xml(bid="d"), "c": lambda: ROUGH_MAT % ("c", 0.3), "m": lambda: microfacet_xml(0.3, bid="m"),
               "n": lambda: normal_xml(0.3, lean_texel(), bid="n"), "h": lambda: height_xml(0.3, bid="h")}
# per number of quads: (size, centre of quad i).  Each layout keeps its quads more than a pixel of the 16 x 16 film apart.
_MIXED_LAYOUT = {3: (44.0, lambda i: (52.0 * (i - 1), 125.0)),                                             # side by side
                 4: (60.0, lambda i: (40.0 * (2 * (i % 2) - 1), 125.0 + 40.0 * (2 * (i // 2) - 1))),        # a 2 x 2 block, 20 apart
                 5: (44.0, lambda i: (64.0 * (i % 3 - 1), 125.0 + 36.0 * (2 * (i // 3) - 1)))}              # two rows, 20 and more apart


def mixed_xml(ids, only=None, tilt=30.0):
    """one quad per id of `ids` -- "d" diffuse, "c" rough conductor, "m" microfacet, "n" normal-mapped and "h" height-mapped microfacet (record types 0 .. 4) --
    or the quad `only` alone (every BSDF stays declared, so every such scene runs the same kernel instance)"""
    size, centre = _MIXED_LAYOUT[len(ids)]
    xml = _HEAD + "".join(_MIXED_BSDF[bid]() for bid in ids)
    for i, bid in enumerate(ids):
        if only is None or only == bid:
            xml += quad(bid, tilt, size, *centre(i))
    return xml + "</scene>\n"


def _swap_bsdf(name, bid, new):
    xml = open(scene_path(name)).read()
    a = xml.index('<bsdf id="%s"' % bid)
    b = xml.index("</bsdf>", a) + len("</bsdf>")
    return xml[:a] + new.strip() + xml[b:]


def room_xml(kind, r=0.3):
    """cbox_uv (no tree) with the textured floor's BSDF replaced by the kind's"""
    return _swap_bsdf("cbox_uv", "floor_tex", KINDS[kind].xml(r, bid="floor_tex"))


def bunny_xml(kind, r=0.3):
    """bunny_light (one tree) with one bunny's BSDF replaced by the kind's: the first bunny's for the plain kind, the smooth-shaded one's for the mapped kinds (its
    mesh has no texture coordinates of its own: prepare_scene(planar_uv=BUNNY) gives it some)"""
    bid = KINDS[kind].bunny_bsdf
    return _swap_bsdf("bunny_light", bid, KINDS[kind].xml(r, bid=bid))


def named_scene(kind, name, res, spp, sppe, **kw):
    """the three scene forms of the forward = reverse tests: the quad tilted by 30 degrees (the mapped kinds: its UVs turned by 37 degrees), cbox_uv with the kind's
    floor, bunny_light with the kind's bunny; random 4 x 4 maps on every bilinear slot"""
    k = KINDS[kind]
    xml, extra = {"quad": lambda: (uv_quad_xml(k.xml(0.3), 30.0), dict(k.quad_kw)), "room": lambda: (room_xml(kind), {}),
                  "bunny": lambda: (bunny_xml(kind), dict(k.bunny_kw))}[name]()
    return scene(xml, res, spp, sppe, **{**dict(textured=True, normal="random", height="random"), **extra, **kw})


# ---------------------------------------------------------------- records
SLOTS = {"kd": (_abi.SLOT_REFLECTANCE, 3), "roughness": (_abi.SLOT_ALPHA_U, 1), "f0": (_abi.SLOT_ETA, 3),          # name: (record slot, channels)
         "normal": (_abi.SLOT_K, 3), "height": (_abi.SLOT_K, 1), "scale": (_abi.SLOT_ALPHA_V, 1)}


def record(tb, kind):
    """(record row, texel offsets {kd, roughness, f0 and the kind's own slots}) of the first record of the kind in the tables"""
    rec = tb["bsdf_rec"].detach().cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    row = rec[rec[:, 0] == KINDS[kind].type][0]
    return row, {key: int(row[1 + 3 * SLOTS[key][0]]) for key in ("kd", "roughness", "f0") + KINDS[kind].slots}


def map_words(row, key):
    """the number of texel words of the record's map `key`"""
    slot, channels = SLOTS[key]
    return int(row[2 + 3 * slot]) * int(row[3 + 3 * slot]) * channels


# ---------------------------------------------------------------- the model in float64 numpy
def bitmap64(texels, slot, u, v, channels):
    """Bitmap::eval (bilinear, v flipped, wrap) of bsdf_rec slot (offset, w, h) in float64"""
    off, w, h = (int(x) for x in slot)
    if (w, h) == (1, 1):
        return np.broadcast_to(texels[off:off + channels], (len(u), channels)).copy()
    v = -v
    u, v = u - np.floor(u), v - np.floor(v)
    u, v = u * (w - 1), v * (h - 1)
    px, py = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    w1x, w1y = (u - px)[:, None], (v - py)[:, None]
    px, py = np.minimum(px, w - 2), np.minimum(py, h - 2)
    idx = py * w + px
    t = texels[off:off + w * h * channels].reshape(w * h, channels)
    return ((1 - w1x) * t[idx] + w1x * t[idx + 1]) * (1 - w1y) + ((1 - w1x) * t[idx + w] + w1x * t[idx + w + 1]) * w1y


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


def microfacet64(wi, wo, kd, f0, r):
    """f cos(theta_o) of DESIGN.md section 14 for local directions [n, 3] and per-sample parameters, written out: no project code"""
    a = r * r
    h = wi + wo
    h = h / np.linalg.norm(h, axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = 1.0 / (np.pi * a * a * ((h[:, 0] / a) ** 2 + (h[:, 1] / a) ** 2 + h[:, 2] ** 2) ** 2)
        D = np.where(D * h[:, 2] > 1e-5, D, 0.0)          # GGX::eval's cut-off

        def g1(v):
            xy = (a * v[:, 0]) ** 2 + (a * v[:, 1]) ** 2
            g = np.where(xy == 0, 1.0, 2.0 / (1.0 + np.sqrt(1.0 + xy / v[:, 2] ** 2)))
            return np.where((v * h).sum(1) * v[:, 2] <= 0, 0.0, g)
        c = (wi * h).sum(1)
        F = f0 + (1.0 - f0) * ((1.0 - c) ** 5)[:, None]
        spec = F * (D * g1(wi) * g1(wo) / (4.0 * wi[:, 2]))[:, None]
    val = kd / np.pi * wo[:, 2:3] + np.where(D[:, None] > 0, spec, 0.0)
    return np.where(((wi[:, 2] > 0) & (wo[:, 2] > 0))[:, None], val, 0.0)


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


# n' of one triangle (unit normal n, edges e1 and e2, six UV words q) at the samples' texture coordinates (u, w), from the texel pool and the record row: the
# perturbed normals [k, 3] and the samples at which the record has a value at all
def _plain_normal64(tex, row, n, e1, e2, q, u, w):
    return np.broadcast_to(n, (len(u), 3)).copy(), np.ones(len(u), bool)


def _mapped_normal64(tex, row, n, e1, e2, q, u, w):
    """the tangent frame from the triangle's edges and UVs (s' = the part of dp_du orthogonal to n, t' = n x s'), n' from the decoded texel;
    a texel that decodes to the zero vector (|v|^2 <= 1e-12) has no value"""
    vv = 2.0 * bitmap64(tex, row[1 + 3 * _abi.SLOT_K:4 + 3 * _abi.SLOT_K], u, w, 3) - 1.0
    du1, dv1, du2, dv2 = q[2] - q[0], q[3] - q[1], q[4] - q[0], q[5] - q[1]
    det = du1 * dv2 - du2 * dv1
    n1 = np.broadcast_to(n, vv.shape).copy()
    if det != 0:
        dp = (e1 * dv2 - e2 * dv1) / det
        p = dp - n * (n @ dp)
        if p @ p > 1e-20:
            s1 = p / np.linalg.norm(p)
            t1 = np.cross(n, s1)
            m = vv[:, 0:1] * s1 + vv[:, 1:2] * t1 + vv[:, 2:3] * n
            with np.errstate(divide="ignore", invalid="ignore"):
                n1 = m / np.linalg.norm(m, axis=1, keepdims=True)
    return n1, (vv * vv).sum(1) > 1e-12


def _height_normal64(tex, row, n, e1, e2, q, u, w):
    """the height gradient at uv, the dual basis from the triangle's edges and UVs, n'"""
    hu, hv = bitmap_grad64(tex, row[1 + 3 * _abi.SLOT_K:4 + 3 * _abi.SLOT_K], u, w)
    return perturbed_normal64(n, e1, e2, q, tex[int(row[1 + 3 * _abi.SLOT_ALPHA_V])], hu, hv), np.ones(len(u), bool)


def closed_form_image(tb, sxy, spp, kind, fp32_uv=False):
    """The collocated image of a scene of face-normal quads with one MicrofacetBSDF of the kind, in float64 at the film samples sxy: hit, uv and distance from the
    float64 tables (Moeller-Trumbore against every triangle, as tests/test_collocated_host.py::test_diffuse_quad_closed_form), bilinear lookups of kd, F0 and
    roughness, n' from the kind (DESIGN.md sections 14 - 16) and the lobes (microfacet64) at the polar angle about n', over d^2.  No project code.
    fp32_uv: the texture coordinates rounded to fp32 before the lookups wrap them (for coordinates so close to a texel border that the wrap itself is a rounding
    question)."""
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
    UV = tb["tri_uv"].detach().cpu().numpy().astype(np.float64).reshape(len(T), -1)[:, :6]          # (rows are padded to 8)
    tex = tb["texels"].detach().cpu().numpy().astype(np.float64).reshape(-1)
    row, _ = record(tb, kind)
    slot = lambda name: row[1 + 3 * SLOTS[name][0]:4 + 3 * SLOTS[name][0]]          # noqa: E731
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
        n = fn / np.linalg.norm(fn)          # (the table's normal is a unit vector to fp32 only: the sine is taken from the tangential part, not from 1 - cos^2)
        u = (q[2] - q[0]) * bu + (q[4] - q[0]) * bv + q[0]
        w = (q[3] - q[1]) * bu + (q[5] - q[1]) * bv + q[1]
        if fp32_uv:
            u, w = u.astype(np.float32), w.astype(np.float32)
        kd, f0, r = bitmap64(tex, slot("kd"), u, w, 3), bitmap64(tex, slot("f0"), u, w, 3), bitmap64(tex, slot("roughness"), u, w, 1)[:, 0]
        n1, ok = KINDS[kind].normal64(tex, row, n, e1, e2, q, u, w)
        ok = ok & (-(d @ n) > 0)          # the geometric side decides whether the surface is seen
        n1 = np.where(ok[:, None], n1, n)
        cos = -(d * n1).sum(1)
        sin = np.linalg.norm(-d - cos[:, None] * n1, axis=1)
        wi = np.stack([sin, np.zeros_like(sin), cos], axis=1)          # isotropic model: only the polar angle about n' matters
        fv = microfacet64(wi, wi, kd, f0, r) / (t * t)[:, None]
        fv = np.where(ok[:, None], fv, 0.0)
        val[hit] = fv[hit]
    return val.reshape(W * H, spp, 3).mean(axis=1)


def angular_error_deg(texels, target):
    """mean angle between the decoded, normalised normals of two [n, 3] texel arrays, in degrees"""
    a, b = 2.0 * np.asarray(texels, np.float64) - 1.0, 2.0 * np.asarray(target, np.float64) - 1.0
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return float(np.degrees(np.arccos(np.clip((a * b).sum(1), -1.0, 1.0))).mean())


# ---------------------------------------------------------------- the record kinds
# type: the _abi.BSDF_* record type; label: how the tests' printed lines name the kind; xml: the <bsdf> builder (r, ..., bid=); slots: the named texel slots beyond
# kd / roughness / f0 (SLOTS has their record slot and channel count); set_map: sets the kind's map on a MicrofacetBSDF; normal64: n' in float64 (above);
# bunny_bsdf: the BSDF id that bunny_xml replaces; quad_kw / bunny_kw: what named_scene adds to prepare_scene for the quad and the bunny; needs_uv: the refusal message
# for a mesh without texture coordinates
KINDS = {
    "plain": SimpleNamespace(type=_abi.BSDF_MICROFACET, label="microfacet", xml=microfacet_xml, slots=(), set_map=None, normal64=_plain_normal64,
                             bunny_bsdf="clr1", quad_kw={}, bunny_kw={}, needs_uv=None),
    "normal": SimpleNamespace(type=_abi.BSDF_MICROFACET_NORMAL, label="normal map", xml=normal_xml, slots=("normal",), set_map=set_normal_map, normal64=_mapped_normal64,
                              bunny_bsdf="clr2", quad_kw=dict(uv="rot37"), bunny_kw=dict(planar_uv=BUNNY), needs_uv="a normal map needs texture coordinates"),
    "height": SimpleNamespace(type=_abi.BSDF_MICROFACET_HEIGHT, label="height map", xml=height_xml, slots=("scale", "height"), set_map=set_height_map, normal64=_height_normal64,
                              bunny_bsdf="clr2", quad_kw=dict(uv="rot37"), bunny_kw=dict(planar_uv=BUNNY), needs_uv="a height map needs texture coordinates"),
}


# ---------------------------------------------------------------- the small recovery problems (tests/test_colloc_normal_gpu.py, tests/test_colloc_height_gpu.py; the step lengths were chosen on the host)
def _normal_truth():
    """4 x 4 kd texels in [0.2, 0.8] and 4 x 4 normal texels leaning up to about 26 degrees (tangential part within +-0.35, v.z = 1)"""
    rng = np.random.default_rng(11)
    kd = rng.uniform(0.2, 0.8, (16, 3)).astype(np.float32)
    v = np.concatenate([rng.uniform(-0.35, 0.35, (16, 2)), np.ones((16, 1))], axis=1)
    return kd, encode(v).astype(np.float32)


def _height_truth():
    """4 x 4 kd texels in [0.2, 0.8] and 4 x 4 height texels in [0, 1]"""
    rng = np.random.default_rng(11)
    return rng.uniform(0.2, 0.8, (16, 3)).astype(np.float32), rng.uniform(0.0, 1.0, 16).astype(np.float32)


def _normal_errors(kd, nm):
    kd_true, n_true = _normal_truth()
    return float(np.abs(kd - kd_true).mean()), angular_error_deg(nm, n_true)


def _height_errors(kd, hm):
    """(mean kd texel error, mean height texel error with each map's mean removed: a constant offset of the height cannot be observed)"""
    kd_true, h_true = _height_truth()
    hm = np.asarray(hm, np.float64).reshape(-1)
    return float(np.abs(kd - kd_true).mean()), float(np.abs((hm - hm.mean()) - (h_true.astype(np.float64) - h_true.mean())).mean())


# tilts: (about y, about x): with tilts about one axis alone the normal's component along it only shows in |n'|.  xml(tilt): the quad under that tilt; truth() and
# start(): (kd texels, map texels); errors(kd, map): the two figures the test halves
RECOVERY = {
    "normal": SimpleNamespace(tilts=((35.0, 0.0), (-35.0, 0.0), (0.0, 35.0)), lr=0.05, steps=40, intensity=1e6, truth=_normal_truth, errors=_normal_errors,
                              xml=lambda tilt: _HEAD + normal_xml(0.4, f0=(0.08, 0.08, 0.08)) + quad("m", tilt[0], tilt_x=tilt[1]) + "</scene>\n",
                              start=lambda: (np.full((16, 3), 0.5, np.float32), np.tile(np.asarray(FLAT, np.float32), (16, 1)))),
    "height": SimpleNamespace(tilts=((35.0, 0.0), (-35.0, 0.0), (0.0, 35.0)), lr=0.05, steps=40, intensity=1e6, truth=_height_truth, errors=_height_errors,
                              xml=lambda tilt: _HEAD + height_xml(0.4, scale=6.0, f0=(0.08, 0.08, 0.08)) + quad("m", tilt[0], tilt_x=tilt[1]) + "</scene>\n",
                              start=lambda: (np.full((16, 3), 0.5, np.float32), np.full(16, 0.5, np.float32))),
}
