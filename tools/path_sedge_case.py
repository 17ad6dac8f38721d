#!/usr/bin/env python
"""Runs the secondary-edge term alone a few times (for rocprofv3 --kernel-trace --stats): python tools/path_sedge_case.py <path|direct> [scene res sppse depth] [--guide]
path: the PathTracer's term (PSDR_FLAG_PATH_SEDGES: k_secondary_edge_filter, k_path_sedge_filter, k_path_sedge, k_path_sedge_rev); direct: DirectIntegrator(1, 1)'s
(k_secondary_edge_filter, k_secondary_edge, k_secondary_edge_rev) on the same scene and slots.  Forward K = 1 and reverse, three launches each after one warm-up,
wall time per call printed.  --guide (path only): first builds both guiding grids (psdr_path_guide_build, [40000, 5, 5, 2] x 4 rounds, or --guide=r0,r1,r2,per,rounds; the
time of each build is printed), then runs the GUIDED term (k_path_sedge_filter_g and the G = true instances of k_path_sedge / k_path_sedge_rev); with `survivors` the
shares are those under grids built on the host at [64, 4, 4, 2] x 16 rounds.  `survivors` prints the share of the slots that get past each filter (host harness, a small slot count: the share does not depend on it)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("psdr-cuda_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import numpy as np, torch
guide = [a for a in sys.argv[1:] if a.startswith("--guide")]
sys.argv = [a for a in sys.argv if not a.startswith("--guide")]
guide_spec = [int(x) for x in guide[0].split("=")[1].split(",")] if guide and "=" in guide[0] else [40000, 5, 5, 2, 4]
from helpers import GpuScene, load_scene, tangents_wrt
from psdr_cuda import _abi
kind = sys.argv[1]
scene = sys.argv[2] if len(sys.argv) > 2 else "cbox_bunny"
res = int(sys.argv[3]) if len(sys.argv) > 3 else 512
sppse = int(sys.argv[4]) if len(sys.argv) > 4 else 16
depth = int(sys.argv[5]) if len(sys.argv) > 5 else 3
if kind == "survivors":
    from path_sedge_helpers import host_path_sedge_survivors, path_opts
    sc, P = load_scene(scene, res=64, spp=0, sppe=0, sppse=16)
    a, b, n = host_path_sedge_survivors(sc.tables(0), path_opts(depth, 16))
    if guide:
        from path_guide_helpers import host_path_guide_mass, host_path_guide_survivors, make_grid
        grids = [make_grid([64, 4, 4], host_path_guide_mass(sc.tables(0), path_opts(depth, 16), seg, [64, 4, 4, 2], 16)) if seg == 1 or depth >= 2 else None for seg in (1, 2)]
        a, b, n = host_path_guide_survivors(sc.tables(0), path_opts(depth, 16), *grids)
    print("%s depth %d%s: %d slots, segment A filter keeps %.4f, segment B filter keeps %.4f" % (scene, depth, " (guided)" if guide else "", n, a / n, b / n))
    sys.exit(0)
sc, P = load_scene(scene, res=res, spp=0, sppe=0, sppse=sppse, translate=(1, (1.0, 0.3, 0.0)))
tb = sc.tables(0); g = GpuScene(tb); tan = tangents_wrt(tb, P)
adj = np.random.default_rng(0).random((res * res, 3)).astype(np.float32)
if kind == "path":
    o = _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=depth, spp=0, sppe=0, sppse=sppse, flags=_abi.FLAG_PATH_SEDGES)
else:
    o = _abi.make_opts(bsdf_samples=1, light_samples=1, spp=0, sppe=0, sppse=sppse)
want = ["tri_info", "sec_edge", "cam_to_world"]
if guide and kind == "path":
    from path_guide_helpers import gpu_path_guide_build, gpu_set_guides, make_grid
    grids = []
    for seg in ((1, 2) if depth >= 2 else (1,)):
        gpu_path_guide_build(g, o, seg, guide_spec[:4], 1)
        t0 = time.perf_counter()
        mass = gpu_path_guide_build(g, o, seg, guide_spec[:4], guide_spec[4])
        print("build segment %d %s x %d rounds: %.3f ms (host wall time, read-back included), mass %.4g, %.4f of the cells empty" % (seg, guide_spec[:4], guide_spec[4], (time.perf_counter() - t0) * 1e3, mass.sum(), (mass == 0).mean()))
        grids.append(make_grid(guide_spec[:3], mass))
    gpu_set_guides(g, grids[0], grids[1] if len(grids) > 1 else None)
    kind = "path guided"
for name, call in (("fwd K=1", lambda: g.render_d_fwd(o, [tan])), ("rev", lambda: g.render_d_rev(o, adj, want=want, with_image=False))):
    call()
    t0 = time.perf_counter()
    for _ in range(3):
        call()
    print("%s %s %s %dx%d sppse %d depth %d: %.3f ms per call (host wall time, copies included), rays %d" % (kind, scene, name, res, res, sppse, depth, (time.perf_counter() - t0) / 3 * 1e3, g.counters()[0]))
