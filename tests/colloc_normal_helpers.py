"""Scenes and the float64 closed form that the normal-map tests share (tests/test_colloc_normal_host.py, tests/test_colloc_normal_gpu.py): MicrofacetBSDF with a
tangent-space normal map, DESIGN.md section 15."""
import numpy as np
import torch

import psdr_cuda
from collocated_helpers import _HEAD, xml_scene
from colloc_microfacet_helpers import F0, KD, ROUGH_MAT, _swap_bsdf, bitmap64, diffuse_xml, maps_4x4, microfacet64, microfacet_xml
from enoki.cuda_autodiff import Vector3f as Vector3fD
from psdr_cuda import _abi
from psdr_cuda.fixtures import scene_path

NEEDS_UV = "a normal map needs texture coordinates"
FLAT = (0.5, 0.5, 1.0)


def encode(v):
    """the image encoding: v = 2c - 1"""
    return (np.asarray(v, np.float64) + 1.0) / 2.0


def lean_texel(deg=20.0):
    """a 1 x 1 map that leans the normal by `deg` about the u axis: v = (0, sin, cos) in (s', t', n)"""
    a = np.radians(deg)
    return tuple(float(x) for x in encode((0.0, np.sin(a), np.cos(a))))


def normal_xml(r=0.3, texel=FLAT, bid="m", name="normalMap", kd=KD, f0=F0):
    """microfacet_xml with a constant normal map as an rgb child"""
    return microfacet_xml(r, kd, f0, bid).replace("</bsdf>", '<rgb name="%s" value="%.9g, %.9g, %.9g"/></bsdf>' % ((name,) + tuple(texel)))


def random_normal_texels(seed=0, n=16):
    """n texels with every decoded v.z >= 0.5 and the tangential part within +-0.6 (not unit vectors: the model normalises)"""
    rng = np.random.default_rng(seed + 100)
    v = np.concatenate([rng.uniform(-0.6, 0.6, (n, 2)), rng.uniform(0.5, 1.0, (n, 1))], axis=1)
    return encode(v).astype(np.float32)


def set_normal_map(b, texels, res):
    if b.normal_map is None:
        b.normal_map = psdr_cuda.Bitmap3fD(FLAT)
    b.normal_map.resolution = res
    b.normal_map.data = Vector3fD(torch.from_numpy(np.ascontiguousarray(texels, np.float32).reshape(-1, 3)))


def prepare_scene(normal=None, uv=None, textured=False, r=0.3, seed=0, planar_uv=None, drop_normal=False, extra=None):
    """prepare(sc) for xml_scene.
    normal: None (leave the BSDFs as loaded), "random" (a 4 x 4 random map on every MicrofacetBSDF that has a normal map) or a [16, 3] texel array;
    uv: None, "rot37" (the texture coordinates of every mesh turned by 37 degrees in the plane) or "mirror" (u -> -u: det < 0) or "collapse" (all UVs equal);
    textured: the other three maps at 4 x 4 (colloc_microfacet_helpers.maps_4x4);
    planar_uv: mesh ids that get texture coordinates uv = (x, y) / 40 of their raw vertices (meshes that come without any);
    drop_normal: every normal map removed again (the same scene with records of type 2); extra: a last callable on the scene."""
    def prepare(sc):
        if textured:
            maps_4x4(r, seed)(sc)
        for b in sc.m_bsdfs:
            if isinstance(b, psdr_cuda.MicrofacetBSDF) and drop_normal:
                b.normal_map = None
            elif isinstance(b, psdr_cuda.MicrofacetBSDF) and b.normal_map is not None and normal is not None:
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
        if extra is not None:
            extra(sc)
    return prepare


def scene(xml, res=16, spp=4, sppe=0, **kw):
    return xml_scene(xml, res, spp, sppe, prepare=prepare_scene(**kw))


def quad(ref, tilt, size=160.0, x=0.0, y=125.0, tilt_x=0.0):
    """colloc_microfacet_helpers._uv_quad with a free centre: the cbox floor quad with texture coordinates, size x size, facing the camera, tilted about y and
    then about x"""
    return ('<shape type="obj"><string name="filename" value="./data/objects/cbox/floor_uv.obj"/><transform name="toWorld"><translate z="-50"/>'
            '<scale x="%g" z="%g"/><rotate angle="90" x="1"/><rotate angle="%g" y="1"/><rotate angle="%g" x="1"/><translate x="%g" y="%g" z="0"/></transform>'
            '<boolean name="faceNormals" value="true"/><ref id="%s"/></shape>\n' % (size / 200.0, size / 300.0, tilt, tilt_x, x, y, ref))


def quad_xml(bsdf, tilt=0.0):
    return _HEAD + bsdf + quad("m", tilt) + "</scene>\n"


MIXED_IDS = ("d", "c", "m", "n")


def mixed_xml(only=None, tilt=30.0):
    """four 60 x 60 quads in a 2 x 2 block, 20 apart (more than a pixel of the 16 x 16 film) -- diffuse, rough conductor, microfacet, normal-mapped microfacet
    (record types 0, 1, 2, 3) -- or one of them alone (the four BSDFs stay declared, so every such scene runs the same kernel instance)"""
    xml = _HEAD + diffuse_xml(bid="d") + ROUGH_MAT % ("c", 0.3) + microfacet_xml(0.3, bid="m") + normal_xml(0.3, lean_texel(), bid="n")
    for i, bid in enumerate(MIXED_IDS):
        if only is None or only == bid:
            xml += quad(bid, tilt, 60.0, 40.0 * (2 * (i % 2) - 1), 125.0 + 40.0 * (2 * (i // 2) - 1))
    return xml + "</scene>\n"


def room_xml(r=0.3, texel=FLAT):
    """cbox_uv (no tree) with the textured floor's BSDF replaced by a normal-mapped MicrofacetBSDF"""
    return _swap_bsdf("cbox_uv", "floor_tex", normal_xml(r, texel, bid="floor_tex"))


def bunny_xml(r=0.3, texel=FLAT):
    """bunny_light (one tree) with the smooth-shaded bunny's BSDF replaced; the mesh has no texture coordinates of its own (prepare_scene(planar_uv=BUNNY)
    gives it some)"""
    return _swap_bsdf("bunny_light", "clr2", normal_xml(r, texel, bid="clr2"))


BUNNY = ("bunny2",)
SCENES = {"quad": lambda: (quad_xml(normal_xml(0.3), 30.0), dict(uv="rot37")), "room": lambda: (room_xml(), {}), "bunny": lambda: (bunny_xml(), dict(planar_uv=BUNNY))}


def named_scene(name, res, spp, sppe, normal="random", **kw):
    """the three scene forms of the forward = reverse tests: the rotated-UV quad, cbox_uv with a normal-mapped floor, bunny_light with a normal-mapped bunny;
    4 x 4 maps on all four slots"""
    xml, extra = SCENES[name]()
    extra.update(kw)
    return scene(xml, res, spp, sppe, normal=normal, textured=True, **extra)


def normal_record(tb):
    """(record row, texel offsets {kd, roughness, f0, normal}) of the first normal-mapped MicrofacetBSDF of the tables"""
    rec = tb["bsdf_rec"].detach().cpu().numpy().reshape(-1, _abi.BSDF_STRIDE)
    row = rec[rec[:, 0] == _abi.BSDF_MICROFACET_NORMAL][0]
    return row, {"kd": int(row[1 + 3 * _abi.SLOT_REFLECTANCE]), "roughness": int(row[1 + 3 * _abi.SLOT_ALPHA_U]), "f0": int(row[1 + 3 * _abi.SLOT_ETA]),
                 "normal": int(row[1 + 3 * _abi.SLOT_K])}


def normal_width(row):
    """the number of texel words of the record's normal map"""
    return int(row[2 + 3 * _abi.SLOT_K]) * int(row[3 + 3 * _abi.SLOT_K]) * 3


# ---------------------------------------------------------------- the model in float64 numpy
def closed_form_image(tb, sxy, spp):
    """The collocated image of a scene of face-normal quads with one normal-mapped MicrofacetBSDF, in float64 at the film samples sxy, DESIGN.md section 15 written
    out: hit, uv and distance from the float64 tables as colloc_microfacet_helpers.closed_form_image; then the tangent frame from the triangle's edges and UVs,
    n' from the decoded texel, and the lobes (microfacet64) at the polar angle about n'.  No project code."""
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
    row, _ = normal_record(tb)
    slot = lambda s: row[1 + 3 * s:4 + 3 * s]          # noqa: E731
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
        kd, f0, r = bitmap64(tex, slot(_abi.SLOT_REFLECTANCE), u, w, 3), bitmap64(tex, slot(_abi.SLOT_ETA), u, w, 3), bitmap64(tex, slot(_abi.SLOT_ALPHA_U), u, w, 1)[:, 0]
        vv = 2.0 * bitmap64(tex, slot(_abi.SLOT_K), u, w, 3) - 1.0
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
        ok = ((vv * vv).sum(1) > 1e-12) & (-(d @ n) > 0)
        n1 = np.where(ok[:, None], n1, n)
        cos = -(d * n1).sum(1)
        sin = np.linalg.norm(-d - cos[:, None] * n1, axis=1)
        wi = np.stack([sin, np.zeros_like(sin), cos], axis=1)
        fv = microfacet64(wi, wi, kd, f0, r) / (t * t)[:, None]
        fv = np.where(ok[:, None], fv, 0.0)
        val[hit] = fv[hit]
    return val.reshape(W * H, spp, 3).mean(axis=1)


def angular_error_deg(texels, target):
    """mean angle between the decoded, normalised normals of two [n, 3] texel arrays, in degrees"""
    a, b = 2.0 * np.asarray(texels, np.float64) - 1.0, 2.0 * np.asarray(target, np.float64) - 1.0
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return float(np.degrees(np.arccos(np.clip((a * b).sum(1), -1.0, 1.0))).mean())


# ---------------------------------------------------------------- the small recovery problem (tests/test_colloc_normal_gpu.py; the step length was chosen on the host)
RECOVERY_TILTS = ((35.0, 0.0), (-35.0, 0.0), (0.0, 35.0))          # (about y, about x): with tilts about one axis alone the normal's component along it only shows in |n'|
RECOVERY_LR, RECOVERY_STEPS, RECOVERY_INTENSITY = 0.05, 40, 1e6


def recovery_truth():
    """4 x 4 kd texels in [0.2, 0.8] and 4 x 4 normal texels leaning up to about 26 degrees (tangential part within +-0.35, v.z = 1)"""
    rng = np.random.default_rng(11)
    kd = rng.uniform(0.2, 0.8, (16, 3)).astype(np.float32)
    v = np.concatenate([rng.uniform(-0.35, 0.35, (16, 2)), np.ones((16, 1))], axis=1)
    return kd, encode(v).astype(np.float32)


def recovery_xml(tilt):
    return _HEAD + normal_xml(0.4, f0=(0.08, 0.08, 0.08)) + quad("m", tilt[0], tilt_x=tilt[1]) + "</scene>\n"


def recovery_start():
    return np.full((16, 3), 0.5, np.float32), np.tile(np.asarray(FLAT, np.float32), (16, 1))


def recovery_errors(kd, nm):
    kd_true, n_true = recovery_truth()
    return float(np.abs(kd - kd_true).mean()), angular_error_deg(nm, n_true)
