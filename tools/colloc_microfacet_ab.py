#!/usr/bin/env python
"""CollocatedIntegrator renderC, two builds of the library in ONE process, alternating windows of device-event time.

    python tools/colloc_microfacet_ab.py variants/lib_parent.so [windows] [renders per window]

1. cbox_rough, 512 x 512 x 64 spp (the rough flag set without a tree, which gained the MicrofacetBSDF branch): this build against the other one, window by
   window (A B A B ...).  The margin is the spread of the other build's own windows.
2. Orientation, this build only: the microfacet quad against the same quad with a rough conductor, 512 x 512 x 64.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "psdr-cuda_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from psdr_cuda import _abi  # noqa: E402


def load_both(other):
    mine = _abi.load_hip()
    path = _abi.HIP_LIB_PATH
    _abi._hip, _abi.HIP_LIB_PATH = None, os.path.abspath(other)
    theirs = _abi.load_hip()
    _abi._hip, _abi.HIP_LIB_PATH = mine, path
    return mine, theirs


def window(g, o, img, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        _abi.check(g.lib, g.lib.psdr_render_c(g.h, o, img.data_ptr(), None))
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    other = sys.argv[1]
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    per = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    import ctypes as C
    from collocated_helpers import ROUGH, colloc_opts, xml_scene
    from colloc_microfacet_helpers import microfacet_xml, uv_quad_xml
    from helpers import GpuScene, load_scene
    mine, theirs = load_both(other)
    res, spp = 512, 64
    sc, _ = load_scene("cbox_rough", res=res, spp=spp)
    tb = sc.tables(0)
    o = C.byref(colloc_opts(spp))
    scenes = {}
    for name, lib in (("this", mine), ("other", theirs)):
        _abi._hip = lib
        scenes[name] = GpuScene(tb)
    _abi._hip = mine
    img = torch.empty(res * res * 3, dtype=torch.float32, device="cuda")
    for g in scenes.values():          # warm-up
        window(g, o, img, per)
    t = {"this": [], "other": []}
    for w in range(windows):
        for name in ("other", "this"):
            t[name].append(window(scenes[name], o, img, per))
    print("cbox_rough collocated renderC %d x %d x %d, %d windows of %d renders, ms per render" % (res, res, spp, windows, per))
    for name in ("other", "this"):
        print("  %-5s %s" % (name, " ".join("%.4f" % x for x in t[name])))
    med = {k: float(np.median(v)) for k, v in t.items()}
    spread = (max(t["other"]) - min(t["other"])) / med["other"]
    print("  median other %.4f ms, this %.4f ms: this / other = %.4f; spread of the other build's windows (max - min) / median = %.4f" %
          (med["other"], med["this"], med["this"] / med["other"], spread))
    # orientation: the new BSDF against the rough conductor on the quad
    for label, bsdf in (("microfacet r = 0.3", microfacet_xml(0.3)), ("rough conductor alpha = 0.09", ROUGH % 0.09)):
        g = GpuScene(xml_scene(uv_quad_xml(bsdf, 30.0), res, spp).tables(0))
        window(g, o, img, per)
        ts = [window(g, o, img, per) for _ in range(max(windows // 2, 2))]
        print("quad %-30s renderC %d x %d x %d: median %.4f ms (%s)" % (label, res, res, spp, float(np.median(ts)), " ".join("%.4f" % x for x in ts)))


if __name__ == "__main__":
    main()
