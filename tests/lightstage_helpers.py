"""Front-end of tests/hostcheck/hostcheck_lightstage.cpp (the LightStageIntegrator's estimator, csrc/psdr_lightstage.h, run on the host), the light sets the
LightStageIntegrator's host and GPU tests share, and the ctypes driver of the stack's C ABI."""
import ctypes as C

import numpy as np

import hostlibs
from helpers import _grad_buffers, AD_KEYS, GpuScene
from hostlibs import cpu_desc, host_threads, tangents_struct
from psdr_cuda import _abi

HC_DEPS = hostlibs.deps("lightstage")          # (what the stand-alone sanitizer program is stale against, besides its own source)
KIND = 5                                       # PSDR_INTEGRATOR_POINT_STACK
LIGHTS_MAX = 256                               # PSDR_POINT_LIGHTS_MAX

# cbox_occluder (room x in [-100, 100], y in [0, 200], z in [-100, 200]; the occluder: y = 100, x in [-20, 40], z in [0, 60]):
OCCLUDER_LIGHTS = np.array([
    (30.3, 181.7, 50.9),          # test_pointlight_gpu.LIGHT: above the occluder
    (-60.7, 170.3, 120.9),        # elsewhere under the ceiling
    (30.3, 181.7, 50.9),          # coincident with the first
    (10.3, -50.7, 40.9),          # below the floor: the floor faces away from it and hides every other surface from it -- its plane is exactly 0
    (10.3, 97.3, 30.9),           # just under the occluder: all of the room above y = 100 is in its umbra
    (10.3, 120.7, -70.9),         # behind the occluder, seen from the camera
], np.float32)
BELOW_FLOOR = 3
# the light of tests/test_pointlight_gpu.py and one offset from it
_S17 = {"cbox": (30.3, 181.7, 50.9), "cbox_rough": (30.3, 181.7, 50.9), "cbox_occluder": (30.3, 181.7, 50.9), "cbox_bunny": (-41.3, 171.9, 120.7), "cbox_env": (10.3, 100.7, 300.9)}
_OFFSET = np.array([-25.4, -30.2, 20.6], np.float32)


def section17_light(name, tb):
    if name in _S17:
        return np.array(_S17[name], np.float32)
    T = tb["tri_info"].detach().cpu().numpy()          # bunny_light: halfway between the camera and the scene's centre, off the axis
    cam = tb["cam"].detach().cpu().numpy()[_abi.CAM_POS:_abi.CAM_POS + 3]
    return (0.5 * (cam + T[:, 0:3].mean(axis=0)) + np.array([40.3, 60.7, 0.0])).astype(np.float32)


def lights_of(name, tb):
    """[L][3]: the six lights of cbox_occluder, the section-17 light plus one offset light everywhere else"""
    if name == "cbox_occluder":
        return OCCLUDER_LIGHTS.copy()
    p = section17_light(name, tb)
    return np.stack([p, p + _OFFSET]).astype(np.float32)


def stack_opts(spp, sppe=0, sppse=0, rng_offset=(0, 0, 0), spp_range=None, sppe_range=None, sppse_range=None):
    return _abi.make_opts(integrator=KIND, spp=spp, sppe=sppe, sppse=sppse, spp_range=spp_range, sppe_range=sppe_range, sppse_range=sppse_range, rng_offset=rng_offset)


def lightstage_lib():
    return hostlibs.load("lightstage")


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else None)


def host_stack_render(tb, opts, pos, mode=0, tangent_sets=None, d_pos=None, nthreads=None):
    """renderC (mode 0: [L, WH, 3]) or forward mode with K = len(tangent_sets) in (1, 3) (mode 1: images [L, WH, 3], derivative images [K, L, WH, 3]) of the
    product code on the host, unit intensities.  pos [L, 3]; d_pos [K, L, 3] or None."""
    tbc, desc, keep = cpu_desc(tb)
    pos = _f32(pos).reshape(-1, 3)
    L, n = len(pos), tb["width"] * tb["height"] * 3
    sets = tangent_sets if tangent_sets is not None else [{}]
    K = len(sets)
    tarr = (_abi.Tangents * K)(*[tangents_struct(ts, keep) for ts in sets])
    d = None if d_pos is None else _f32(d_pos).reshape(K, L, 3)
    img, dimg = np.zeros(L * n, np.float32), np.zeros(K * L * n, np.float32)
    rc = lightstage_lib().hostcheck_lightstage_render(C.byref(desc), C.byref(opts), int(mode), K, tarr, L, _ptr(pos), _ptr(d), _ptr(img), _ptr(dimg), nthreads or host_threads())
    assert rc == 0, rc
    return (img.reshape(L, -1, 3), dimg.reshape(K, L, -1, 3)) if mode else img.reshape(L, -1, 3)


def host_stack_rev(tb, opts, pos, adj, want=AD_KEYS, light=True):
    """Reverse mode on the host: (images [L, WH, 3], {table: gradient}, gradients of the light positions [L, 3] or None); adj [L, WH, 3]"""
    tbc, desc, keep = cpu_desc(tb)
    bufs, g = _grad_buffers(tbc, want)
    pos = _f32(pos).reshape(-1, 3)
    L = len(pos)
    adj = _f32(adj).reshape(-1)
    img = np.zeros(adj.shape[0], np.float32)
    g_pos = np.zeros((L, 3), np.float32) if light else None
    rc = lightstage_lib().hostcheck_lightstage_rev(C.byref(desc), C.byref(opts), L, _ptr(pos), _ptr(adj), _ptr(img), C.byref(g), _ptr(g_pos))
    assert rc == 0, rc
    return img.reshape(L, -1, 3), bufs, g_pos


class StackScene(GpuScene):
    """GpuScene + psdr_scene_set_point_lights (and psdr_scene_set_point_light: both kinds on one handle); images of kind 5 come back as [L, WH, 3]"""

    L = 0

    def set_lights(self, pos, d_pos=None, want_grad=False, L=None):
        import torch
        fp = C.POINTER(C.c_float)
        pos = None if pos is None else _f32(pos).reshape(-1, 3)
        L = (0 if pos is None else len(pos)) if L is None else L
        d = None if d_pos is None else _f32(d_pos).reshape(-1, max(L, 1), 3)
        K = 0 if d is None else len(d)
        self.g_stack = torch.zeros((max(L, 1), 3), dtype=torch.float32, device="cuda") if want_grad else None
        _abi.check(self.lib, self.lib.psdr_scene_set_point_lights(self.h, L, None if pos is None else pos.ctypes.data_as(fp), K, d.ctypes.data_as(fp) if K else None,
                                                                  self.g_stack.data_ptr() if want_grad else None))
        self.L = L if pos is not None else 0
        return self

    def set_light(self, pos, d_pos=None, want_grad=False):
        """the light of kind 4 (tests/test_pointlight_gpu.py PointScene.set_light)"""
        import torch
        fp = C.POINTER(C.c_float)
        pos = _f32(pos).reshape(3)
        K = 0 if d_pos is None else len(d_pos)
        d = _f32(d_pos).reshape(-1) if K else None
        self.g_pos = torch.zeros(3, dtype=torch.float32, device="cuda") if want_grad else None
        _abi.check(self.lib, self.lib.psdr_scene_set_point_light(self.h, pos.ctypes.data_as(fp), K, d.ctypes.data_as(fp) if K else None, self.g_pos.data_ptr() if want_grad else None))
        return self

    def light_grad(self):
        import torch
        torch.cuda.synchronize()
        return self.g_pos.cpu().numpy()

    def lights_grad(self):
        import torch
        torch.cuda.synchronize()
        return self.g_stack.cpu().numpy()

    def stack_render_c(self, opts, guard_planes=0, fill=float("nan")):
        """[L + guard_planes, WH, 3]: the buffer is filled with `fill` before the call"""
        import torch
        img = torch.full(((self.L + guard_planes) * self.n,), fill, dtype=torch.float32, device="cuda")
        _abi.check(self.lib, self.lib.psdr_render_c(self.h, C.byref(opts), img.data_ptr(), None))
        torch.cuda.synchronize()
        return img.cpu().numpy().reshape(self.L + guard_planes, -1, 3)

    def stack_render_d_fwd(self, opts, tangent_sets):
        import torch
        K, L = len(tangent_sets), self.L
        img = torch.full((L * self.n,), float("nan"), dtype=torch.float32, device="cuda")
        dimg = torch.full((K * L * self.n,), float("nan"), dtype=torch.float32, device="cuda")
        tarr = (_abi.Tangents * K)()
        keep = []
        for k, ts in enumerate(tangent_sets):
            for name, t in ts.items():
                if t is not None:
                    t = t.detach().cuda().float().contiguous()
                    keep.append(t)
                    setattr(tarr[k], "d_" + name, t.data_ptr())
        _abi.check(self.lib, self.lib.psdr_render_d_fwd(self.h, C.byref(opts), K, tarr, img.data_ptr(), dimg.data_ptr(), None))
        torch.cuda.synchronize()
        return img.cpu().numpy().reshape(L, -1, 3), dimg.cpu().numpy().reshape(K, L, -1, 3)

    def stack_render_d_rev(self, opts, adj, want=AD_KEYS, with_image=True):
        import torch
        L = self.L
        adj_t = torch.as_tensor(_f32(adj).reshape(-1)).cuda()
        assert adj_t.numel() == L * self.n
        img = torch.full((L * self.n,), float("nan"), dtype=torch.float32, device="cuda") if with_image else None
        g = _abi.Grads()
        bufs = {}
        for name in want:
            t = self.tb.get(name)
            if t is None:
                continue
            bufs[name] = torch.zeros(tuple(t.shape), dtype=torch.float32, device="cuda")
            setattr(g, "g_" + name, bufs[name].data_ptr())
        _abi.check(self.lib, self.lib.psdr_render_d_rev(self.h, C.byref(opts), adj_t.data_ptr(), img.data_ptr() if with_image else None, C.byref(g), None))
        torch.cuda.synchronize()
        return (img.cpu().numpy().reshape(L, -1, 3) if with_image else None), {k: v.cpu().numpy() for k, v in bufs.items()}
