#!/usr/bin/env python
"""LightStageIntegrator: one fused launch over L lights beside L PointLightIntegrator launches of the SAME build, in one process, alternating windows of
device-event time (the method of tools/pointlight_ab.py).

    python tools/lightstage_ab.py [windows] [renders per window]

Per scene (cbox and cbox_bunny, 512 x 512 x 64) and L = 1, 4, 16, window by window (A B A B ...):
  renderC        kind 4: L times (psdr_scene_set_point_light + psdr_render_c)           kind 5: one psdr_render_c of the stack
  reverse step   kind 4: L psdr_render_d_rev with gradients to the triangle rows, the texels and the light; kind 5: one psdr_render_d_rev of the stack
                 (camera samples only: the edge terms are the same kernels in both)
The margin is the spread of the kind-4 windows.  Then ms per light against L with the least-squares fit  t(L) = S + L P, and the share of the edge terms in a
stack's reverse step at L = 4 (cbox_occluder, sppe = sppse = 16; `lightstage_ab.py W P edges` measures that alone)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "psdr-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from psdr_cuda import _abi  # noqa: E402

RES, SPP = 512, 64
FP = C.POINTER(C.c_float)


def lights(first, L):
    """L lights on a 4-wide grid under the ceiling, the first at `first`"""
    out = np.zeros((L, 3), np.float32)
    for l in range(L):
        out[l] = (first[0] - 17.3 * (l % 4), first[1] - 9.1 * (l // 4), first[2] + 11.7 * (l % 3))
    return out


class Runner:
    def __init__(self, g, pos, sppe=0, sppse=0):
        self.g, self.pos, self.L = g, pos, len(pos)
        n = RES * RES * 3
        self.img = torch.empty(self.L * n, dtype=torch.float32, device="cuda")
        self.adj = torch.rand(self.L * n, dtype=torch.float32, device="cuda")
        self.n = n
        self.o4 = _abi.make_opts(integrator=_abi.INTEGRATOR_POINT, spp=SPP, sppe=sppe, sppse=sppse)
        self.o5 = _abi.make_opts(integrator=_abi.INTEGRATOR_POINT_STACK, spp=SPP, sppe=sppe, sppse=sppse)
        self.grads, self.bufs = _abi.Grads(), []
        for name in ("tri_info", "texels") + (("prim_edge", "sec_edge") if sppe or sppse else ()):
            t = g.tb.get(name)
            if t is not None:
                b = torch.zeros(tuple(t.shape), dtype=torch.float32, device="cuda")
                self.bufs.append(b)
                setattr(self.grads, "g_" + name, b.data_ptr())
        self.g_pos = torch.zeros((self.L, 3), dtype=torch.float32, device="cuda")

    def single(self, reverse):
        g, lib = self.g, self.g.lib
        for l in range(self.L):
            _abi.check(lib, lib.psdr_scene_set_point_light(g.h, self.pos[l].ctypes.data_as(FP), 0, None, self.g_pos.data_ptr() + 12 * l if reverse else None))
            if reverse:
                _abi.check(lib, lib.psdr_render_d_rev(g.h, C.byref(self.o4), self.adj.data_ptr() + 4 * self.n * l, None, C.byref(self.grads), None))
            else:
                _abi.check(lib, lib.psdr_render_c(g.h, C.byref(self.o4), self.img.data_ptr() + 4 * self.n * l, None))

    def stack(self, reverse):
        g, lib = self.g, self.g.lib
        _abi.check(lib, lib.psdr_scene_set_point_lights(g.h, self.L, self.pos.ctypes.data_as(FP), 0, None, self.g_pos.data_ptr() if reverse else None))
        if reverse:
            _abi.check(lib, lib.psdr_render_d_rev(g.h, C.byref(self.o5), self.adj.data_ptr(), None, C.byref(self.grads), None))
        else:
            _abi.check(lib, lib.psdr_render_c(g.h, C.byref(self.o5), self.img.data_ptr(), None))

    def window(self, fn, reverse, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn(reverse)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n


def edge_share(windows):
    """the share of the edge terms in a stack's reverse step: cbox_occluder with its primary- and secondary-edge tables, L = 4, sppe = sppse = 16"""
    from helpers import GpuScene, load_scene
    g = GpuScene(load_scene("cbox_occluder", res=RES, spp=SPP, sppe=16, sppse=16)[0].tables(0))
    pos = lights((30.3, 181.7, 50.9), 4)
    r0, r1 = Runner(g, pos), Runner(g, pos, sppe=16, sppse=16)
    for r in (r0, r1):
        r.window(r.stack, True, 2)
    t0 = float(np.median([r0.window(r0.stack, True, 3) for _ in range(windows)]))
    t1 = float(np.median([r1.window(r1.stack, True, 3) for _ in range(windows)]))
    k0 = float(np.median([r0.window(r0.single, True, 3) for _ in range(windows)]))
    k1 = float(np.median([r1.window(r1.single, True, 3) for _ in range(windows)]))
    print("cbox_occluder reverse step, L = 4, %d x %d x %d: stack, camera samples only %.4f ms, with sppe = sppse = 16 %.4f ms: the edge terms (L launches of each kernel) take "
          "%.1f %% of the stack's step; 4 kind-4 launches: %.4f ms and %.4f ms" % (RES, RES, SPP, t0, t1, 100.0 * (t1 - t0) / t1, k0, k1))


def main():
    windows = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    if "edges" in sys.argv[3:]:          # only the edge terms' share
        return edge_share(windows)
    from helpers import GpuScene, load_scene
    first = {"cbox": (30.3, 181.7, 50.9), "cbox_bunny": (-41.3, 171.9, 120.7)}
    for name in ("cbox", "cbox_bunny"):
        tb = load_scene(name, res=RES, spp=SPP)[0].tables(0)
        g = GpuScene(tb)
        for reverse in (False, True):
            per_w = max(per // 4, 2) if reverse else per
            med_stack, Ls = [], (1, 4, 16)
            for L in Ls:
                r = Runner(g, lights(first[name], L))
                r.window(r.single, reverse, 2), r.window(r.stack, reverse, 2)          # warm-up
                t = {"kind4": [], "stack": []}
                for w in range(windows):
                    t["kind4"].append(r.window(r.single, reverse, per_w))
                    t["stack"].append(r.window(r.stack, reverse, per_w))
                m4, m5 = float(np.median(t["kind4"])), float(np.median(t["stack"]))
                med_stack.append(m5)
                print("%s %s %d x %d x %d, L = %d, %d windows of %d, ms per stack" % (name, "reverse step" if reverse else "renderC", RES, RES, SPP, L, windows, per_w))
                for key in ("kind4", "stack"):
                    print("  %-6s %s" % (key, " ".join("%.4f" % x for x in t[key])))
                print("  median L kind-4 launches %.4f ms, one stack launch %.4f ms: stack / kind 4 = %.4f; spread of the kind-4 windows (max - min) / median = %.4f; "
                      "ms per light: kind 4 %.4f, stack %.4f" % (m4, m5, m5 / m4, (max(t["kind4"]) - min(t["kind4"])) / m4, m4 / L, m5 / L))
            P, S = np.polyfit(np.asarray(Ls, np.float64), np.asarray(med_stack), 1)
            print("%s %s: least-squares fit of the stack's medians  t(L) = S + L P:  S = %.4f ms, P = %.4f ms" % (name, "reverse step" if reverse else "renderC", S, P))
    edge_share(windows)


if __name__ == "__main__":
    main()
