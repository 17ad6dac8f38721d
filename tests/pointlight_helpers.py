"""Front-end of tests/hostcheck/hostcheck_pointlight.cpp (the PointLightIntegrator's estimator, csrc/psdr_pointlight.h, run on the host) and the small scenes the
PointLightIntegrator's tests share."""
import ctypes as C

import numpy as np

import hostlibs
from collocated_helpers import _HEAD, DIFFUSE, xml_scene  # noqa: F401
from helpers import _grad_buffers, AD_KEYS
from hostlibs import cpu_desc, host_threads, tangents_struct
from psdr_cuda import _abi

HC_DEPS = hostlibs.deps("pointlight")          # (what the stand-alone sanitizer program is stale against, besides its own source)
CAM_POS = (0.0, 125.0, 1000.0)                 # the camera of collocated_helpers._HEAD and of the cbox fixtures


def pointlight_lib():
    return hostlibs.load("pointlight")


def point_opts(spp, sppe=0, sppse=0, rng_offset=(0, 0, 0), spp_range=None, sppe_range=None, sppse_range=None):
    return _abi.make_opts(integrator=_abi.INTEGRATOR_POINT, spp=spp, sppe=sppe, sppse=sppse, spp_range=spp_range, sppe_range=sppe_range, sppse_range=sppse_range,
                          rng_offset=rng_offset)


def _vec3(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.float32).reshape(3)


def host_point_render(tb, opts, pos, mode=0, tangents=None, d_pos=None, nthreads=None):
    """renderC (mode 0: image) or forward mode, K = 1 (mode 1: image, derivative image: interior + primary edges + shadow boundary) of the product code on the
    host, unit intensity, the light at `pos` (d_pos: its tangent)."""
    tbc, desc, keep = cpu_desc(tb)
    n = tb["width"] * tb["height"] * 3
    img, dimg = np.zeros(n, np.float32), np.zeros(n, np.float32)
    tan = tangents_struct(tangents, keep)
    pos, d_pos = _vec3(pos), _vec3(d_pos)
    rc = pointlight_lib().hostcheck_pointlight_render(C.byref(desc), C.byref(opts), int(mode), C.byref(tan), C.c_void_p(pos.ctypes.data),
                                                      C.c_void_p(d_pos.ctypes.data if d_pos is not None else None), C.c_void_p(img.ctypes.data),
                                                      C.c_void_p(dimg.ctypes.data), nthreads or host_threads())
    assert rc == 0, rc
    return (img.reshape(-1, 3), dimg.reshape(-1, 3)) if mode else img.reshape(-1, 3)


def host_point_rev(tb, opts, pos, adj, want=AD_KEYS, light=True):
    """Reverse mode on the host: (image, {table: gradient}, gradient of the light position or None)."""
    tbc, desc, keep = cpu_desc(tb)
    bufs, g = _grad_buffers(tbc, want)
    adj = np.ascontiguousarray(adj, dtype=np.float32).reshape(-1)
    img = np.zeros(adj.shape[0], np.float32)
    pos = _vec3(pos)
    g_pos = np.zeros(3, np.float32) if light else None
    rc = pointlight_lib().hostcheck_pointlight_rev(C.byref(desc), C.byref(opts), C.c_void_p(pos.ctypes.data), C.c_void_p(adj.ctypes.data), C.c_void_p(img.ctypes.data), C.byref(g),
                                                   C.c_void_p(g_pos.ctypes.data if light else None))
    assert rc == 0, rc
    return img.reshape(-1, 3), bufs, g_pos


# ---------------------------------------------------------------- scenes
def _quad(size, tilt, pos, bsdf_ref="m"):
    """emitter.obj (a 80 x 80 quad in the xz plane, facing -y) scaled by `size`, turned to face +z, tilted about y and moved to `pos`"""
    return ('<shape type="obj"><string name="filename" value="./data/objects/cbox/emitter.obj"/><transform name="toWorld"><scale x="%g" z="%g"/>'
            '<rotate angle="-90" x="1"/><rotate angle="%g" y="1"/><translate x="%g" y="%g" z="%g"/></transform><boolean name="faceNormals" value="true"/><ref id="%s"/></shape>\n'
            % (size, size, tilt, pos[0], pos[1], pos[2], bsdf_ref))


def floor_occluder_xml(occ_size=0.5, occ_pos=(3.7, 128.3, 150.0), floor_size=2.0, bsdf=DIFFUSE):
    """A receiver quad (160 x 160 at floor_size 2) facing the camera at the camera's target and a small square occluder hanging 150 in front of it.  The occluder is
    seen by the camera too (test scenes that want it out of view move it)."""
    return _HEAD + bsdf + _quad(floor_size, 0.0, (0.0, 125.0, 0.0)) + _quad(occ_size, 0.0, occ_pos) + "</scene>\n"


def hidden_occluder_xml(bsdf=DIFFUSE):
    """The receiver quad (z = 0, x in [-80, 80], y in [45, 205]) and a 40 x 40 occluder at (150, 125, 150), outside the camera's view; with the light at
    HIDDEN_LIGHT its shadow is the square of side 160 / 3 about (0, 125) on the receiver: only the shadow is seen, the primary-edge term of the occluder is zero."""
    return floor_occluder_xml(occ_pos=(150.0, 125.0, 150.0), bsdf=bsdf)


HIDDEN_LIGHT = (600.0, 125.0, 600.0)


def cam_pos(tb):
    return tb["cam"].detach().cpu().numpy()[_abi.CAM_POS:_abi.CAM_POS + 3].astype(np.float32)


# ---------------------------------------------------------------- closed forms in float64 (no project code)
def camera_rays64(tb, sxy):
    cam = tb["cam"].detach().cpu().numpy().astype(np.float64)
    s2c, tw = cam[0:16].reshape(4, 4), cam[16:32].reshape(4, 4)
    sxy = np.asarray(sxy, np.float64)
    v = np.concatenate([sxy, np.zeros((len(sxy), 1)), np.ones((len(sxy), 1))], axis=1) @ s2c.T
    d = v[:, :3] / v[:, 3:4]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return tw[:3, 3] / tw[3, 3], d @ tw[:3, :3].T


def point_closed_form(tb, sxy, light, kind=None, rho=(0.7, 0.5, 0.3), rows=None):
    """Per film sample, the UNOCCLUDED value of a scene of face-normal quads under a point light at `light`: hit, uv, r and the directions from the float64 tables
    (Moeller-Trumbore against the triangle rows `rows`, default all).  kind None: a Lambertian rho / pi cos(theta_L) / r_L^2; otherwise the MicrofacetBSDF of
    colloc_microfacet_helpers.KINDS[kind] -- n' from the kind (DESIGN.md sections 14 - 16), wi and wo in a frame about n', the lobes of microfacet64, over r_L^2.
    Returns (values [n, 3], hit mask, hit points [n, 3])."""
    from colloc_microfacet_helpers import KINDS, SLOTS, bitmap64, microfacet64, record
    org, d = camera_rays64(tb, sxy)
    light = np.asarray(light, np.float64)
    T = tb["tri_info"].detach().cpu().numpy().astype(np.float64)
    val, hit_any, pts, tbest = np.zeros((len(d), 3)), np.zeros(len(d), bool), np.zeros((len(d), 3)), np.full(len(d), np.inf)
    if kind is not None:
        UV = tb["tri_uv"].detach().cpu().numpy().astype(np.float64).reshape(len(T), -1)[:, :6]
        tex = tb["texels"].detach().cpu().numpy().astype(np.float64).reshape(-1)
        row, _ = record(tb, kind)
        slot = lambda name: row[1 + 3 * SLOTS[name][0]:4 + 3 * SLOTS[name][0]]          # noqa: E731
    for i in (range(len(T)) if rows is None else rows):
        tri = T[i]
        p0, e1, e2, fn = tri[0:3], tri[3:6], tri[6:9], tri[18:21]
        hh = np.cross(d, e2)
        f = 1.0 / (hh @ e1)
        s = org - p0
        bu = f * (hh @ s)
        qq = np.cross(s, e1)
        bv = f * (d @ qq)
        t = f * (qq @ e2)
        hit = (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0) & (t < tbest)
        n = fn / np.linalg.norm(fn)
        p = p0 + bu[:, None] * e1 + bv[:, None] * e2
        dv = light - p
        r2 = (dv * dv).sum(1)
        l = dv / np.sqrt(r2)[:, None]
        seen = -(d @ n) > 0
        if kind is None:
            fv = np.asarray(rho, np.float32).astype(np.float64)[None, :] / np.pi * np.maximum(l @ n, 0.0)[:, None]
            fv = np.where(seen[:, None], fv, 0.0)
        else:
            q = UV[i]
            u = (q[2] - q[0]) * bu + (q[4] - q[0]) * bv + q[0]
            w = (q[3] - q[1]) * bu + (q[5] - q[1]) * bv + q[1]
            kd, f0, rr = bitmap64(tex, slot("kd"), u, w, 3), bitmap64(tex, slot("f0"), u, w, 3), bitmap64(tex, slot("roughness"), u, w, 1)[:, 0]
            n1, ok = KINDS[kind].normal64(tex, row, n, e1, e2, q, u, w)
            ok = ok & seen & (l @ n > 0)          # the shading frame of the hit (the face normal) decides first, then n'
            n1 = np.where(ok[:, None], n1, n)
            # a frame about n': s1 along the tangential part of -d (the model is isotropic: any frame serves)
            a = -d - (-d * n1).sum(1)[:, None] * n1
            an = np.linalg.norm(a, axis=1, keepdims=True)
            s1 = np.where(an > 1e-12, a / np.maximum(an, 1e-300), np.cross(n1, np.array([0.0, 1.0, 0.0])))
            t1 = np.cross(n1, s1)
            loc = lambda x: np.stack([(x * s1).sum(1), (x * t1).sum(1), (x * n1).sum(1)], axis=1)          # noqa: E731
            fv = np.where(ok[:, None], microfacet64(loc(-d), loc(l), kd, f0, rr), 0.0)
        fv = fv / r2[:, None]
        val[hit], pts[hit], tbest[hit] = fv[hit], p[hit], t[hit]
        hit_any |= hit
    return val, hit_any, pts


# ---------------------------------------------------------------- the moving shadow outline as a line integral, in float64 (no project code)
def film_of64(tb, x):
    """film coordinates [n, 2] of world points [n, 3] through the camera's world-to-sample matrix, float64"""
    m = tb["cam"].detach().cpu().numpy().astype(np.float64)[_abi.CAM_WORLD_TO_SAMPLE:_abi.CAM_WORLD_TO_SAMPLE + 16].reshape(4, 4)
    v = np.concatenate([x, np.ones((len(x), 1))], axis=1) @ m.T
    return v[:, :2] / v[:, 3:4]


def lambert64(x, light, rho, n=(0.0, 0.0, 1.0)):
    """rho / pi cos(theta_L) / r_L^2 at the points x [n, 3] of a receiver with normal n, unoccluded: [n, 3]"""
    dv = np.asarray(light, np.float64) - x
    r2 = (dv * dv).sum(1)
    cos = np.maximum(dv @ np.asarray(n, np.float64), 0.0) / np.sqrt(r2)
    return np.asarray(rho, np.float32).astype(np.float64)[None, :] / np.pi * (cos / r2)[:, None]


def shadow_square(light, occ_lo, occ_hi, zo):
    """the shadow on the plane z = 0 of the axis-parallel square [occ_lo, occ_hi] at height zo under the light: (lo, hi, k) with k = L.z / (L.z - zo)"""
    L = np.asarray(light, np.float64)
    k = L[2] / (L[2] - zo)
    a, b = L[:2] + (np.asarray(occ_lo, np.float64) - L[:2]) * k, L[:2] + (np.asarray(occ_hi, np.float64) - L[:2]) * k
    return np.minimum(a, b), np.maximum(a, b), k


def outline_line_integral(tb, light, lo, hi, vel, rho=(0.7, 0.5, 0.3), n_per_edge=20000):
    """d image / d parameter of the LIT integral when the shadow square [lo, hi] on the receiver z = 0 moves rigidly with velocity vel (2-vector):
        dI_p = - W H  integral over the outline inside pixel p of  Li(x) J(x) (vel . n_out) dl,
    Li the unoccluded closed form, J = |d film / d receiver area| (the film has area 1, a pixel 1 / (W H); central differences of the float64 projection),
    midpoint rule with n_per_edge points per edge, binned by the pixel the point projects into.  [W H, 3]"""
    W, H = tb["width"], tb["height"]
    out = np.zeros((W * H, 3))
    t = (np.arange(n_per_edge) + 0.5) / n_per_edge
    vel = np.asarray(vel, np.float64)
    edges = [((hi[0], lo[1]), (hi[0], hi[1]), (1.0, 0.0)), ((lo[0], lo[1]), (lo[0], hi[1]), (-1.0, 0.0)),
             ((lo[0], hi[1]), (hi[0], hi[1]), (0.0, 1.0)), ((lo[0], lo[1]), (hi[0], lo[1]), (0.0, -1.0))]
    h = 1e-3
    for a, b, nout in edges:
        a, b = np.asarray(a), np.asarray(b)
        xy = a[None, :] + t[:, None] * (b - a)[None, :]
        x = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1)
        q = film_of64(tb, x)
        qx = (film_of64(tb, x + [h, 0, 0]) - film_of64(tb, x - [h, 0, 0])) / (2 * h)
        qy = (film_of64(tb, x + [0, h, 0]) - film_of64(tb, x - [0, h, 0])) / (2 * h)
        J = np.abs(qx[:, 0] * qy[:, 1] - qx[:, 1] * qy[:, 0])
        w = -(vel @ np.asarray(nout)) * np.linalg.norm(b - a) / n_per_edge * W * H
        ix, iy = np.floor(q[:, 0] * W).astype(int), np.floor(q[:, 1] * H).astype(int)
        ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        np.add.at(out, (iy * W + ix)[ok], (lambert64(x, light, rho) * (J * w)[:, None])[ok])
    return out


def interior_light_derivative(tb, light, d_light, lo, hi, rec_lo, rec_hi, rho=(0.7, 0.5, 0.3), m=32):
    """d image / d (light along d_light) with the shadow held still: per pixel, the mean over m x m film points of the central difference (float64, step 1e-3) of
    the closed form at the receiver point the film point sees, zero inside the shadow square [lo, hi] and off the receiver [rec_lo, rec_hi].  [W H, 3]"""
    W, H = tb["width"], tb["height"]
    s = (np.arange(m) + 0.5) / m
    gx, gy = np.meshgrid((np.arange(W)[:, None] + s[None, :]).ravel() / W, (np.arange(H)[:, None] + s[None, :]).ravel() / H)
    org, d = camera_rays64(tb, np.stack([gx.ravel(), gy.ravel()], axis=1))
    x = org + d * (-org[2] / d[:, 2])[:, None]
    lit = (x[:, 0] > rec_lo[0]) & (x[:, 0] < rec_hi[0]) & (x[:, 1] > rec_lo[1]) & (x[:, 1] < rec_hi[1]) & \
        ~((x[:, 0] > lo[0]) & (x[:, 0] < hi[0]) & (x[:, 1] > lo[1]) & (x[:, 1] < hi[1]))
    L, dL, h = np.asarray(light, np.float64), np.asarray(d_light, np.float64), 1e-3
    dv = (lambert64(x, L + h * dL, rho) - lambert64(x, L - h * dL, rho)) / (2 * h) * lit[:, None]
    return dv.reshape(H, m, W, m, 3).mean(axis=(1, 3)).reshape(W * H, 3)


def host_point_render_k3(tb, opts, pos, tangent_sets, d_pos=None, nthreads=None):
    """forward mode with K = 3 on the host: (image, [3] derivative images); tangent_sets: three {table: tensor} dicts, d_pos: [3][3] or None"""
    tbc, desc, keep = cpu_desc(tb)
    n = tb["width"] * tb["height"] * 3
    img, dimg = np.zeros(n, np.float32), np.zeros(3 * n, np.float32)
    tarr = (_abi.Tangents * 3)(*[tangents_struct(ts, keep) for ts in tangent_sets])
    pos = _vec3(pos)
    d = None if d_pos is None else np.ascontiguousarray(d_pos, dtype=np.float32).reshape(9)
    rc = pointlight_lib().hostcheck_pointlight_render_k3(C.byref(desc), C.byref(opts), tarr, C.c_void_p(pos.ctypes.data), C.c_void_p(d.ctypes.data if d is not None else None),
                                                         C.c_void_p(img.ctypes.data), C.c_void_p(dimg.ctypes.data), nthreads or host_threads())
    assert rc == 0, rc
    return img.reshape(-1, 3), dimg.reshape(3, -1, 3)
