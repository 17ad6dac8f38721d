"""Front-end of tests/hostcheck/hostcheck_distantlight.cpp (the estimators of csrc/psdr_pointlight.h and csrc/psdr_lightstage.h run on the host with a light model
per light), the float64 references of the distant light (numpy, no project code) and the ctypes drivers of psdr_scene_set_light / psdr_scene_set_lights."""
import ctypes as C

import numpy as np

import hostlibs
from helpers import _grad_buffers, AD_KEYS
from hostlibs import cpu_desc, host_threads, tangents_struct
from lightstage_helpers import StackScene
from pointlight_helpers import camera_rays64, film_of64
from psdr_cuda import _abi

HC_DEPS = hostlibs.deps("distantlight")          # (what the stand-alone sanitizer program is stale against, besides its own source)
POINT, DISTANT = _abi.LIGHT_POINT, _abi.LIGHT_DISTANT
ENV_MESSAGE = "a distant light cannot reach a scene inside an environment map's bounding mesh"


def distantlight_lib():
    return hostlibs.load("distantlight")


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else None)


def unit(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d)


# ---------------------------------------------------------------- the harness: one light
def host_light_render(tb, opts, v, kind=DISTANT, mode=0, tangent_sets=None, d_v=None, nthreads=None):
    """renderC (mode 0: [WH, 3]) or forward mode with K = len(tangent_sets) in (1, 3) (mode 1: image, derivative images [K, WH, 3]) of the product code on the
    host, unit intensity / irradiance.  v [3]: position or direction by kind; d_v [K, 3] or None."""
    tbc, desc, keep = cpu_desc(tb)
    n = tb["width"] * tb["height"] * 3
    sets = tangent_sets if tangent_sets is not None else [{}]
    K = len(sets)
    tarr = (_abi.Tangents * K)(*[tangents_struct(ts, keep) for ts in sets])
    v = _f32(v).reshape(3)
    d = None if d_v is None else _f32(d_v).reshape(K, 3)
    img, dimg = np.zeros(n, np.float32), np.zeros(K * n, np.float32)
    rc = distantlight_lib().hostcheck_distantlight_render(C.byref(desc), C.byref(opts), int(mode), K, tarr, int(kind), _ptr(v), _ptr(d), _ptr(img), _ptr(dimg), nthreads or host_threads())
    assert rc == 0, rc
    return (img.reshape(-1, 3), dimg.reshape(K, -1, 3)) if mode else img.reshape(-1, 3)


def host_light_rev(tb, opts, v, adj, kind=DISTANT, want=AD_KEYS, light=True):
    """Reverse mode on the host: (image, {table: gradient}, gradient of the light's vector or None)."""
    tbc, desc, keep = cpu_desc(tb)
    bufs, g = _grad_buffers(tbc, want)
    adj = _f32(adj).reshape(-1)
    img = np.zeros(adj.shape[0], np.float32)
    v = _f32(v).reshape(3)
    g_v = np.zeros(3, np.float32) if light else None
    rc = distantlight_lib().hostcheck_distantlight_rev(C.byref(desc), C.byref(opts), int(kind), _ptr(v), _ptr(adj), _ptr(img), C.byref(g), _ptr(g_v))
    assert rc == 0, rc
    return img.reshape(-1, 3), bufs, g_v


# ---------------------------------------------------------------- the harness: a stack
def host_lights_render(tb, opts, kinds, v, mode=0, tangent_sets=None, d_v=None, nthreads=None):
    """renderC (mode 0: [L, WH, 3]) or forward mode (mode 1: images [L, WH, 3], derivative images [K, L, WH, 3]); kinds [L], v [L, 3], d_v [K, L, 3] or None"""
    tbc, desc, keep = cpu_desc(tb)
    v = _f32(v).reshape(-1, 3)
    L, n = len(v), tb["width"] * tb["height"] * 3
    kinds = np.ascontiguousarray(kinds, np.int32).reshape(L)
    sets = tangent_sets if tangent_sets is not None else [{}]
    K = len(sets)
    tarr = (_abi.Tangents * K)(*[tangents_struct(ts, keep) for ts in sets])
    d = None if d_v is None else _f32(d_v).reshape(K, L, 3)
    img, dimg = np.zeros(L * n, np.float32), np.zeros(K * L * n, np.float32)
    rc = distantlight_lib().hostcheck_distantstack_render(C.byref(desc), C.byref(opts), int(mode), K, tarr, L, _ptr(kinds), _ptr(v), _ptr(d), _ptr(img), _ptr(dimg),
                                                          nthreads or host_threads())
    assert rc == 0, rc
    return (img.reshape(L, -1, 3), dimg.reshape(K, L, -1, 3)) if mode else img.reshape(L, -1, 3)


def host_lights_rev(tb, opts, kinds, v, adj, want=AD_KEYS, light=True):
    """Reverse mode on the host: (images [L, WH, 3], {table: gradient}, gradients of the lights' vectors [L, 3] or None); adj [L, WH, 3]"""
    tbc, desc, keep = cpu_desc(tb)
    bufs, g = _grad_buffers(tbc, want)
    v = _f32(v).reshape(-1, 3)
    L = len(v)
    kinds = np.ascontiguousarray(kinds, np.int32).reshape(L)
    adj = _f32(adj).reshape(-1)
    img = np.zeros(adj.shape[0], np.float32)
    g_v = np.zeros((L, 3), np.float32) if light else None
    rc = distantlight_lib().hostcheck_distantstack_rev(C.byref(desc), C.byref(opts), L, _ptr(kinds), _ptr(v), _ptr(adj), _ptr(img), C.byref(g), _ptr(g_v))
    assert rc == 0, rc
    return img.reshape(L, -1, 3), bufs, g_v


# ---------------------------------------------------------------- the C ABI with kinds
class KindScene(StackScene):
    """StackScene + psdr_scene_set_light / psdr_scene_set_lights (the old entry points stay reachable as set_light / set_lights)"""

    def set_kind_light(self, kind, v, d_v=None, want_grad=False):
        import torch
        fp = C.POINTER(C.c_float)
        v = None if v is None else _f32(v).reshape(3)
        K = 0 if d_v is None else len(d_v)
        d = _f32(d_v).reshape(-1) if K else None
        self.g_pos = torch.zeros(3, dtype=torch.float32, device="cuda") if want_grad else None
        _abi.check(self.lib, self.lib.psdr_scene_set_light(self.h, int(kind), None if v is None else v.ctypes.data_as(fp), K, d.ctypes.data_as(fp) if K else None,
                                                           self.g_pos.data_ptr() if want_grad else None))
        return self

    def set_kind_lights(self, kinds, v, d_v=None, want_grad=False):
        import torch
        fp = C.POINTER(C.c_float)
        v = None if v is None else _f32(v).reshape(-1, 3)
        L = 0 if v is None else len(v)
        kinds = None if kinds is None else np.ascontiguousarray(kinds, np.int32).reshape(-1)
        d = None if d_v is None else _f32(d_v).reshape(-1, max(L, 1), 3)
        K = 0 if d is None else len(d)
        self.g_stack = torch.zeros((max(L, 1), 3), dtype=torch.float32, device="cuda") if want_grad else None
        _abi.check(self.lib, self.lib.psdr_scene_set_lights(self.h, L, None if kinds is None else kinds.ctypes.data_as(C.POINTER(C.c_int32)), None if v is None else v.ctypes.data_as(fp), K,
                                                            d.ctypes.data_as(fp) if K else None, self.g_stack.data_ptr() if want_grad else None))
        self.L = L
        return self


# ---------------------------------------------------------------- closed forms in float64 (no project code)
def distant_closed_form(tb, sxy, direction, kind=None, rho=(0.7, 0.5, 0.3), rows=None):
    """Per film sample, the UNOCCLUDED value of a scene of face-normal quads under a distant light of unit irradiance whose direction (towards the light) is
    `direction`: the hit and uv from the float64 tables (Moeller-Trumbore against the triangle rows `rows`, default all), l = direction / |direction| at every
    hit, NO falloff.  kind None: a Lambertian rho / pi max(0, n . l); otherwise the MicrofacetBSDF of colloc_microfacet_helpers.KINDS[kind] -- n' from the kind
    (DESIGN.md sections 14 - 16), wi and wo in a frame about n', the lobes of microfacet64.  Returns (values [n, 3], hit mask, hit points [n, 3])."""
    from colloc_microfacet_helpers import KINDS, SLOTS, bitmap64, microfacet64, record
    org, d = camera_rays64(tb, sxy)
    lu = unit(direction)
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
        l = np.broadcast_to(lu, p.shape)
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
            a = -d - (-d * n1).sum(1)[:, None] * n1
            an = np.linalg.norm(a, axis=1, keepdims=True)
            s1 = np.where(an > 1e-12, a / np.maximum(an, 1e-300), np.cross(n1, np.array([0.0, 1.0, 0.0])))
            t1 = np.cross(n1, s1)
            loc = lambda x: np.stack([(x * s1).sum(1), (x * t1).sum(1), (x * n1).sum(1)], axis=1)          # noqa: E731
            fv = np.where(ok[:, None], microfacet64(loc(-d), loc(l), kd, f0, rr), 0.0)
        val[hit], pts[hit], tbest[hit] = fv[hit], p[hit], t[hit]
        hit_any |= hit
    return val, hit_any, pts


def lambert_distant64(n_points, direction, rho, n=(0.0, 0.0, 1.0)):
    """rho / pi max(0, n . u) at n_points points of a receiver with normal n, unoccluded: [n_points, 3] (the same at every point)"""
    cos = max(float(unit(direction) @ np.asarray(n, np.float64)), 0.0)
    return np.broadcast_to(np.asarray(rho, np.float32).astype(np.float64)[None, :] / np.pi * cos, (n_points, 3))


def shadow_square_distant(direction, occ_lo, occ_hi, zo):
    """the shadow on the plane z = 0 of the axis-parallel square [occ_lo, occ_hi] at height zo under the distant light: every point moves by -zo d_xy / d_z"""
    d = np.asarray(direction, np.float64)
    shift = -zo * d[:2] / d[2]
    return np.asarray(occ_lo, np.float64) + shift, np.asarray(occ_hi, np.float64) + shift


def outline_line_integral_distant(tb, direction, lo, hi, vel, rho=(0.7, 0.5, 0.3), n_per_edge=20000):
    """d image / d parameter of the LIT integral when the shadow square [lo, hi] on the receiver z = 0 moves rigidly with velocity vel (2-vector):
        dI_p = - W H  integral over the outline inside pixel p of  Li J (vel . n_out) dl,
    Li = rho / pi max(0, n . u), the unoccluded value under the distant light (no falloff: the same along the outline), J = |d film / d receiver area| (central
    differences of the float64 projection), midpoint rule with n_per_edge points per edge, binned by the pixel the point projects into.  [W H, 3]"""
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
        np.add.at(out, (iy * W + ix)[ok], (lambert_distant64(len(x), direction, rho) * (J * w)[:, None])[ok])
    return out


def interior_direction_derivative(tb, direction, d_direction, lo, hi, rec_lo, rec_hi, rho=(0.7, 0.5, 0.3), m=32):
    """d image / d (direction along d_direction) with the shadow held still: rho / pi n . du, du = (t - u (u . t)) / |d| the derivative of u = d / |d|, on the lit
    part of the receiver z = 0 -- per pixel, the share of m x m film points that see the receiver [rec_lo, rec_hi] outside the shadow square [lo, hi].  [W H, 3]"""
    W, H = tb["width"], tb["height"]
    s = (np.arange(m) + 0.5) / m
    gx, gy = np.meshgrid((np.arange(W)[:, None] + s[None, :]).ravel() / W, (np.arange(H)[:, None] + s[None, :]).ravel() / H)
    org, d = camera_rays64(tb, np.stack([gx.ravel(), gy.ravel()], axis=1))
    x = org + d * (-org[2] / d[:, 2])[:, None]
    lit = (x[:, 0] > rec_lo[0]) & (x[:, 0] < rec_hi[0]) & (x[:, 1] > rec_lo[1]) & (x[:, 1] < rec_hi[1]) & \
        ~((x[:, 0] > lo[0]) & (x[:, 0] < hi[0]) & (x[:, 1] > lo[1]) & (x[:, 1] < hi[1]))
    dd, tt = np.asarray(direction, np.float64), np.asarray(d_direction, np.float64)
    u = unit(dd)
    du = (tt - u * (u @ tt)) / np.linalg.norm(dd)
    val = np.asarray(rho, np.float32).astype(np.float64) / np.pi * du[2] * (1.0 if u[2] > 0 else 0.0)
    return (lit[:, None] * val[None, :]).reshape(H, m, W, m, 3).mean(axis=(1, 3)).reshape(W * H, 3)
