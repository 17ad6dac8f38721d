#!/usr/bin/env python
"""PointLightIntegrator: this build beside another build of the library in ONE process, alternating windows of device-event time (the method of
tools/colloc_microfacet_ab.py), and one orientation timing.

    python tools/pointlight_ab.py variants/lib_parent.so [windows] [renders per window]

1. What the other build has too, window by window (A B A B ...): PathTracer(3) renderC of cbox 512 x 512 x 16 (the headline's kernel family) and
   CollocatedIntegrator renderC of cbox_rough 512 x 512 x 64 (the unit whose header this integrator shares).  The margin is the spread of the other build's windows.
2. Orientation, this build only: PointLightIntegrator renderC of cbox 512 x 512 x 64 (light under the ceiling) beside CollocatedIntegrator renderC of the same scene.
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "psdr-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from psdr_cuda import _abi  # noqa: E402
from colloc_microfacet_ab import window  # noqa: E402


class _OlderLibrary(C.CDLL):
    """a build from before this integrator has no psdr_scene_set_point_light: _abi.load_hip may set the prototype of a symbol it does not have"""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if not name.startswith("psdr_"):
                raise
            return type("MissingSymbol", (), {})()


def load_both(other):
    mine = _abi.load_hip()
    path = _abi.HIP_LIB_PATH
    _abi._hip, _abi.HIP_LIB_PATH, cdll = None, os.path.abspath(other), _abi.C.CDLL
    _abi.C.CDLL = _OlderLibrary
    try:
        theirs = _abi.load_hip()
    finally:
        _abi.C.CDLL = cdll
        _abi._hip, _abi.HIP_LIB_PATH = mine, path
    return mine, theirs


def main():
    other = sys.argv[1]
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    from helpers import GpuScene, load_scene
    mine, theirs = load_both(other)
    res = 512
    img = torch.empty(res * res * 3, dtype=torch.float32, device="cuda")
    cases = (("cbox PathTracer(3) renderC", "cbox", _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=3, spp=16), 16),
             ("cbox_rough collocated renderC", "cbox_rough", _abi.make_opts(integrator=_abi.INTEGRATOR_COLLOCATED, spp=64), 64))
    for label, name, opts, spp in cases:
        tb = load_scene(name, res=res, spp=spp)[0].tables(0)
        o = C.byref(opts)
        scenes = {}
        for key, lib in (("this", mine), ("other", theirs)):
            _abi._hip = lib
            scenes[key] = GpuScene(tb)
        _abi._hip = mine
        for g in scenes.values():          # warm-up
            window(g, o, img, per)
        t = {"this": [], "other": []}
        for w in range(windows):
            for key in ("other", "this"):
                t[key].append(window(scenes[key], o, img, per))
        print("%s %d x %d x %d, %d windows of %d renders, ms per render" % (label, res, res, spp, windows, per))
        for key in ("other", "this"):
            print("  %-5s %s" % (key, " ".join("%.4f" % x for x in t[key])))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print("  median other %.4f ms, this %.4f ms: this / other = %.4f; spread of the other build's windows (max - min) / median = %.4f" %
              (med["other"], med["this"], med["this"] / med["other"], (max(t["other"]) - min(t["other"])) / med["other"]))
    # orientation: the point light beside the flash at the camera, this build
    tb = load_scene("cbox", res=res, spp=64)[0].tables(0)
    g = GpuScene(tb)
    pos = (C.c_float * 3)(30.3, 181.7, 50.9)
    _abi.check(g.lib, g.lib.psdr_scene_set_point_light(g.h, pos, 0, None, None))
    for label, kind in (("PointLightIntegrator", _abi.INTEGRATOR_POINT), ("CollocatedIntegrator", _abi.INTEGRATOR_COLLOCATED)):
        o = C.byref(_abi.make_opts(integrator=kind, spp=64))
        window(g, o, img, per)
        ts = [window(g, o, img, per) for _ in range(max(windows // 2, 2))]
        print("cbox %-22s renderC %d x %d x 64: median %.4f ms (%s)" % (label, res, res, float(np.median(ts)), " ".join("%.4f" % x for x in ts)))


if __name__ == "__main__":
    main()
