#!/usr/bin/env python
"""Distant lights: this build beside the parent's build of the library in ONE process, alternating windows of device-event time (the
method of tools/pointlight_ab.py and tools/lightstage_ab.py, whose loaders and runners this tool uses), and the orientation timings of the new model.

    python tools/distantlight_ab.py variants/lib_parent.so [windows] [renders per window]

1. What both builds have, window by window (other, this, other, this ...), through the OLD entry points:
     kind 4  renderC of cbox 512 x 512 x 64
     kind 5  renderC and a reverse step (camera samples; gradients to the triangle rows, the texels and the lights) of cbox and cbox_bunny at L = 4 and 16
     PathTracer(3) renderC of cbox 512 x 512 x 16 and CollocatedIntegrator renderC of cbox_rough 512 x 512 x 64 (units whose text is the parent's)
   The yardstick is the spread of the parent's own windows, (max - min) / median.
2. Orientation, this build only, no bar: distant against point, renderC and reverse step, kind 4 and a stack of 4 (all point / all distant / alternating)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "psdr-cuda_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from psdr_cuda import _abi  # noqa: E402
from colloc_microfacet_ab import window  # noqa: E402
from lightstage_ab import RES, SPP, FP, Runner, lights  # noqa: E402
from pointlight_ab import load_both  # noqa: E402

FIRST = {"cbox": (30.3, 181.7, 50.9), "cbox_bunny": (-41.3, 171.9, 120.7)}


def report(label, t):
    med = {k: float(np.median(v)) for k, v in t.items()}
    for key in ("other", "this"):
        print("  %-5s %s" % (key, " ".join("%.4f" % x for x in t[key])))
    print("  %s: median other %.4f ms, this %.4f ms: this / other = %.4f; spread of the other build's windows (max - min) / median = %.4f" %
          (label, med["other"], med["this"], med["this"] / med["other"], (max(t["other"]) - min(t["other"])) / med["other"]))


def ab(label, fns, windows, per):
    """fns: {"other": callable(n) -> ms, "this": ...}"""
    for f in fns.values():
        f(2)
    t = {"other": [], "this": []}
    for w in range(windows):
        for key in ("other", "this"):
            t[key].append(fns[key](per))
    print("%s, %d windows of %d" % (label, windows, per))
    report(label, t)


def main():
    other = sys.argv[1]
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    from helpers import GpuScene, load_scene
    mine, theirs = load_both(other)

    def both(tb):
        out = {}
        for key, lib in (("this", mine), ("other", theirs)):
            _abi._hip = lib
            out[key] = GpuScene(tb)
        _abi._hip = mine
        return out
    img = torch.empty(RES * RES * 3, dtype=torch.float32, device="cuda")
    # units with the parent's text
    for label, name, opts, spp in (("cbox PathTracer(3) renderC x 16 spp", "cbox", _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=3, spp=16), 16),
                                   ("cbox_rough collocated renderC x 64 spp", "cbox_rough", _abi.make_opts(integrator=_abi.INTEGRATOR_COLLOCATED, spp=64), 64)):
        sc = both(load_scene(name, res=RES, spp=spp)[0].tables(0))
        o = C.byref(opts)
        ab(label, {k: (lambda n, g=g: window(g, o, img, n)) for k, g in sc.items()}, windows, per)
    for name in ("cbox", "cbox_bunny"):
        sc = both(load_scene(name, res=RES, spp=SPP)[0].tables(0))
        if name == "cbox":          # kind 4
            o4 = C.byref(_abi.make_opts(integrator=_abi.INTEGRATOR_POINT, spp=SPP))
            pos = (C.c_float * 3)(*FIRST[name])
            for g in sc.values():
                _abi.check(g.lib, g.lib.psdr_scene_set_point_light(g.h, pos, 0, None, None))
            ab("cbox kind-4 renderC %d x %d x %d" % (RES, RES, SPP), {k: (lambda n, g=g: window(g, o4, img, n)) for k, g in sc.items()}, windows, per)
        for L in (4, 16):
            rs = {k: Runner(g, lights(FIRST[name], L)) for k, g in sc.items()}
            for reverse in (False, True):
                ab("%s stack L = %d %s" % (name, L, "reverse step" if reverse else "renderC"),
                   {k: (lambda n, r=r: r.window(r.stack, reverse, n)) for k, r in rs.items()}, windows, max(per // 4, 2) if reverse else per)
    # orientation: this build, distant against point
    for name in ("cbox", "cbox_bunny"):
        g = GpuScene(load_scene(name, res=RES, spp=SPP)[0].tables(0))
        L = 4
        r = Runner(g, lights(FIRST[name], L))
        dirs = np.array([(0.23 - 0.11 * l, 0.51 + 0.07 * l, 1.0) for l in range(L)], np.float32)
        o4, o5 = r.o4, r.o5
        kinds_of = {"all point": [0] * L, "all distant": [1] * L, "alternating": [l % 2 for l in range(L)]}

        def one(kind, v, reverse):
            _abi.check(g.lib, g.lib.psdr_scene_set_light(g.h, kind, v.ctypes.data_as(FP), 0, None, r.g_pos.data_ptr() if reverse else None))
            if reverse:
                _abi.check(g.lib, g.lib.psdr_render_d_rev(g.h, C.byref(o4), r.adj.data_ptr(), None, C.byref(r.grads), None))
            else:
                _abi.check(g.lib, g.lib.psdr_render_c(g.h, C.byref(o4), r.img.data_ptr(), None))

        def stack(kinds, reverse):
            v = np.where(np.asarray(kinds)[:, None] == 1, dirs, r.pos).astype(np.float32)
            k = (C.c_int32 * L)(*kinds)
            _abi.check(g.lib, g.lib.psdr_scene_set_lights(g.h, L, k, v.ctypes.data_as(FP), 0, None, r.g_pos.data_ptr() if reverse else None))
            if reverse:
                _abi.check(g.lib, g.lib.psdr_render_d_rev(g.h, C.byref(o5), r.adj.data_ptr(), None, C.byref(r.grads), None))
            else:
                _abi.check(g.lib, g.lib.psdr_render_c(g.h, C.byref(o5), r.img.data_ptr(), None))
        for reverse in (False, True):
            n = max(per // 4, 2) if reverse else per
            what = "reverse step" if reverse else "renderC"
            for label, fn in [("kind 4 point", lambda rev: one(0, r.pos[0], rev)), ("kind 4 distant", lambda rev: one(1, dirs[0], rev))] + \
                             [("stack of 4, " + k, (lambda rev, kk=kk: stack(kk, rev))) for k, kk in kinds_of.items()]:
                r.window(fn, reverse, 2)
                ts = [r.window(fn, reverse, n) for _ in range(max(windows // 2, 2))]
                print("orientation %s %s %-24s median %.4f ms (%s)" % (name, what, label, float(np.median(ts)), " ".join("%.4f" % x for x in ts)))


if __name__ == "__main__":
    main()
