"""Scenes and the float64 closed form that the MicrofacetBSDF tests share (tests/test_colloc_microfacet_host.py, tests/test_colloc_microfacet_gpu.py)."""
import numpy as np
import torch

import psdr_cuda
from collocated_helpers import _HEAD, xml_scene
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

MESSAGE = "MicrofacetBSDF is evaluated by the CollocatedIntegrator only"
KD, F0 = (0.6, 0.4, 0.2), (0.04, 0.06, 0.1)
ROUGH_MAT = '<bsdf id="%s" type="roughconductor"><float name="alpha" value="%g"/><rgb name="eta" value="0.2, 0.92, 1.1"/><rgb name="k" value="3.9, 2.45, 2.14"/></bsdf>\n'


def microfacet_xml(r=0.3, kd=KD, f0=F0, bid="m"):
    return ('<bsdf id="%s" type="microfacet"><rgb name="diffuseReflectance" value="%g, %g, %g"/><rgb name="specularReflectance" value="%g, %g, %g"/>'
            '<float name="roughness" value="%g"/></bsdf>\n' % ((bid,) + tuple(kd) + tuple(f0) + (r,)))


def diffuse_xml(kd=KD, bid="m"):
    return '<bsdf id="%s" type="diffuse"><rgb name="reflectance" value="%g, %g, %g"/></bsdf>\n' % ((bid,) + tuple(kd))


def _uv_quad(ref, tilt, size=160.0, x=0.0):
    """the cbox floor quad with texture coordinates (200 x 300, uv repeat 2 x 3), centred, scaled to size x size, turned to face the camera, then tilted about y"""
    return ('<shape type="obj"><string name="filename" value="./data/objects/cbox/floor_uv.obj"/><transform name="toWorld"><translate z="-50"/>'
            '<scale x="%g" z="%g"/><rotate angle="90" x="1"/><rotate angle="%g" y="1"/><translate x="%g" y="125" z="0"/></transform>'
            '<boolean name="faceNormals" value="true"/><ref id="%s"/></shape>\n' % (size / 200.0, size / 300.0, tilt, x, ref))


def uv_quad_xml(bsdf, tilt=0.0):
    """collocated_helpers.quad_xml with a quad that carries texture coordinates, so that a 4 x 4 map is looked up across texel borders"""
    return _HEAD + bsdf + _uv_quad("m", tilt) + "</scene>\n"


MIXED_IDS = ("d", "c", "m")


def mixed_xml(only=None, tilt=30.0):
    """three 44 x 44 quads side by side -- diffuse, rough conductor, microfacet -- or one of them alone (the three BSDFs stay declared, so every such scene
    runs the same kernel instance)"""
    xml = _HEAD + diffuse_xml(bid="d") + ROUGH_MAT % ("c", 0.3) + microfacet_xml(0.3, bid="m")
    for i, bid in enumerate(MIXED_IDS):
        if only is None or only == bid:
            xml += _uv_quad(bid, tilt, 44.0, 52.0 * (i - 1))
    return xml + "</scene>\n"


def _swap_bsdf(name, bid, new):
    xml = open(scene_path(name)).read()
    a = xml.index('<bsdf id="%s"' % bid)
    b = xml.index("</bsdf>", a) + len("</bsdf>")
    return xml[:a] + new.strip() + xml[b:]


def room_xml(r=0.3):
    """cbox_uv (no tree) with the textured floor's BSDF replaced"""
    return _swap_bsdf("cbox_uv", "floor_tex", microfacet_xml(r, bid="floor_tex"))


def bunny_xml(r=0.3):
    """bunny_light (one tree) with the first bunny's BSDF replaced"""
    return _swap_bsdf("bunny_light", "clr1", microfacet_xml(r, bid="clr1"))


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


def scene(xml, res=16, spp=4, sppe=0, textured=False, r=0.3, seed=0, zero_roughness_texel=None):
    return xml_scene(xml, res, spp, sppe, prepare=maps_4x4(r, seed, zero_roughness_texel) if textured else None)


def microfacet_record(tb):
    """(record row, texel offsets {kd, roughness, f0}) of the first MicrofacetBSDF of the tables"""
    rec = tb["bsdf_rec"].detach().cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    row = rec[rec[:, 0] == _abi.BSDF_MICROFACET][0]
    return row, {"kd": int(row[1 + 3 * _abi.SLOT_REFLECTANCE]), "roughness": int(row[1 + 3 * _abi.SLOT_ALPHA_U]), "f0": int(row[1 + 3 * _abi.SLOT_ETA])}


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


def closed_form_image(tb, sxy, spp):
    """The collocated image of a scene of face-normal quads with one MicrofacetBSDF, in float64 at the film samples sxy: hit, frame, uv and distance from the
    float64 tables (Moeller-Trumbore against every triangle, as tests/test_collocated_host.py::test_diffuse_quad_closed_form), the model from microfacet64."""
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
    row, _ = microfacet_record(tb)
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
        nn = fn / np.linalg.norm(fn)          # (the table's normal is a unit vector to fp32 only: the sine is taken from the tangential part, not from 1 - cos^2)
        cos = -(d @ nn)
        sin = np.linalg.norm(-d - cos[:, None] * nn[None, :], axis=1)
        wi = np.stack([sin, np.zeros_like(sin), cos], axis=1)          # isotropic model: only the polar angle matters
        u = (q[2] - q[0]) * bu + (q[4] - q[0]) * bv + q[0]
        w = (q[3] - q[1]) * bu + (q[5] - q[1]) * bv + q[1]
        kd = bitmap64(tex, row[1 + 3 * _abi.SLOT_REFLECTANCE:4 + 3 * _abi.SLOT_REFLECTANCE], u, w, 3)
        f0 = bitmap64(tex, row[1 + 3 * _abi.SLOT_ETA:4 + 3 * _abi.SLOT_ETA], u, w, 3)
        r = bitmap64(tex, row[1 + 3 * _abi.SLOT_ALPHA_U:4 + 3 * _abi.SLOT_ALPHA_U], u, w, 1)[:, 0]
        fv = microfacet64(wi, wi, kd, f0, r) / (t * t)[:, None]
        val[hit] = fv[hit]
    return val.reshape(W * H, spp, 3).mean(axis=1)
