#!/usr/bin/env python
"""Inverse rendering through renderD + backward, after the reference's docs/inverse_diff_render.rst:

    python examples/inverse_rendering.py albedo       # recover a wall colour (material parameter)
    python examples/inverse_rendering.py translation  # move an occluder back (geometry: all three terms)
    python examples/inverse_rendering.py envmap       # recover the environment map's pixels under a metal bunny
    python examples/inverse_rendering.py svbrdf       # recover albedo and roughness maps of a quad from three flash photographs (CollocatedIntegrator)
    python examples/inverse_rendering.py svbrdf --normals     # ... of a quad with a bumpy normal map: albedo, roughness and normals
    python examples/inverse_rendering.py svbrdf --normals --lights     # ... from ONE view under three lamps (PointLightIntegrator), beside the three-tilt run
    python examples/inverse_rendering.py svbrdf --normals --lights --stack     # ... and with the three lamps as one LightStageIntegrator: ms per step of both
    python examples/inverse_rendering.py svbrdf --normals --lights --distant   # ... and with the three lamps as distant lights (DistantLightIntegrator)
    python examples/inverse_rendering.py svbrdf --height      # ... of a quad with a relief: albedo, roughness and a height map
    python examples/inverse_rendering.py shape        # recover a displaced sphere's vertices, one by one, through psdr_cuda.LargeSteps

Needs an MI355X (the render path has no CPU fallback)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "psdr-cuda_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import enoki as ek  # noqa: E402
import psdr_cuda  # noqa: E402
from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD, Matrix4f as Matrix4fD  # noqa: E402
from psdr_cuda.fixtures import scene_path  # noqa: E402


def load(name, res=64, spp=16, sppe=0, sppse=0):
    sc = psdr_cuda.Scene()
    sc.load_file(scene_path(name), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    return sc


def loop(sc, integ, target, params, lr, steps, after_step=None, report=None):
    opt = torch.optim.Adam([p.t for p in params], lr=lr)
    t0 = time.perf_counter()
    for it in range(steps):
        opt.zero_grad()
        sc.configure()
        img = integ.renderD(sc)
        loss = ek.hmean(ek.hsum(ek.sqr(img - Vector3fD._wrap(target))))
        ek.backward(loss)
        opt.step()
        if after_step:
            after_step()
        if it % 10 == 0 or it == steps - 1:
            print("  step %3d  loss %.5f  %s" % (it, float(loss.t.item()), report() if report else ""))
    torch.cuda.synchronize()
    print("  %.1f ms per step" % ((time.perf_counter() - t0) / steps * 1e3))


def albedo():
    integ = psdr_cuda.PathTracer(max_depth=2)
    ref = load("cbox", spp=512); ref.configure()
    target = integ.renderC(ref).torch().clone()
    sc = load("cbox")
    refl = sc.param_map["BSDF[id=white]"].reflectance
    refl.data = Vector3fD([0.4, 0.6, 0.8])
    ek.set_requires_gradient(refl.data)
    loop(sc, integ, target, [refl.data], 0.05, 60, lambda: refl.data.t.data.clamp_(0.01, 0.99),
         lambda: "albedo %s (target 0.95 0.95 0.95)" % np.round(refl.data.numpy().reshape(3), 3))


def translation():
    integ = psdr_cuda.DirectIntegrator(1, 1)
    ref = load("cbox_occluder", spp=64); ref.configure()
    target = integ.renderC(ref).torch().clone()
    sc = load("cbox_occluder", spp=16, sppe=16, sppse=16)
    P = FloatD(12.0)
    ek.set_requires_gradient(P)
    mesh = sc.param_map["Mesh[1]"]

    def apply():
        mesh.set_transform(Matrix4fD.translate(Vector3fD([1.0, 0.0, 0.0]) * P))
    apply()
    loop(sc, integ, target, [P], 1.0, 50, apply, lambda: "offset %.3f (target 0)" % float(P.t.item()))


def envmap():
    integ = psdr_cuda.DirectIntegrator(1, 1)
    ref = load("bunny_env", spp=256); ref.configure()
    target = integ.renderC(ref).torch().clone()
    truth = ref.param_map["Emitter[0]"].radiance.data.numpy().copy()
    sc = load("bunny_env", spp=32)
    env = sc.param_map["Emitter[0]"]
    env.radiance.data = Vector3fD(torch.full((truth.shape[0], 3), 0.5, device="cuda"))
    ek.set_requires_gradient(env.radiance.data)
    loop(sc, integ, target, [env.radiance.data], 0.05, 80, lambda: env.radiance.data.t.data.clamp_(0.0, 100.0),
         lambda: "mean |map - truth| %.4f" % float(np.abs(env.radiance.data.numpy() - truth).mean()))


SVBRDF_XML = """<scene version="0.5.0">
<sensor type="perspective"><float name="fov" value="13"/><string name="fovAxis" value="x"/>
<transform name="toWorld"><lookAt origin="0, 125, 1000" target="0, 125, 0" up="0, 1, 0"/></transform>
<sampler type="independent"><integer name="sampleCount" value="4"/></sampler>
<film type="hdrfilm"><integer name="width" value="64"/><integer name="height" value="64"/><rfilter type="box"/></film></sensor>
<bsdf id="m" type="microfacet"><rgb name="specularReflectance" value="0.08, 0.08, 0.08"/></bsdf>
<shape type="obj"><string name="filename" value="./data/objects/cbox/floor_uv.obj"/>
<transform name="toWorld"><translate z="-50"/><scale x="0.9" z="0.6"/><rotate angle="90" x="1"/><rotate angle="%g" y="1"/><translate y="125"/></transform>
<boolean name="faceNormals" value="true"/><ref id="m"/></shape>
</scene>"""


def svbrdf(map_res=16, res=64, spp=8, steps=150, tilts=(0.0, 35.0, 65.0), normals=False, height=False, lights=False, stack=False, distant=False):
    """A quad with map_res x map_res kd and roughness maps (MicrofacetBSDF, F0 known) photographed with a flash at the camera under three tilts -- one quad
    transformed three times, the maps shared.  The diffuse lobe is seen at every tilt, the specular lobe only near normal incidence, so the two maps separate by
    angle.  Adam on both maps from a flat start; the flash's intensity brings the pixel values (1 / distance^2 = 1e-6) to order 0.1.
    normals (--normals): the target quad also carries a bumpy tangent-space normal map (leaning up to about 25 degrees) and the loop recovers kd, roughness AND
    the normal map, started flat.  Tilts about one axis leave the sign of the normal's component along that axis open, so the third view tilts about x.
    height (--height): the target quad carries a height map instead (texels in [0, 1], 2 world units per unit of height: slopes up to about 0.5 on the 16 x 16 cells of the
    160 x 160 quad) and the loop recovers kd, roughness and the height map, started flat, from a head-on view and one tilt about each axis.  A height field has one number per texel
    and its slopes are integrable by construction; a constant offset cannot be observed, so the error is reported with each map's mean removed.
    lights (--normals --lights): ONE camera, the quad head-on, and three lamps 120 degrees apart around the viewing axis, about 37 degrees off it
    (PointLightIntegrator, one per lamp: photometric stereo) instead of three tilts under the flash.
    stack (--normals --lights --stack): the three lamps as ONE LightStageIntegrator -- one renderD and one backward per step, the three photographs are the planes
    of its image.
    distant (--normals --lights --distant): the three lamps as DISTANT lights (DistantLightIntegrator): their directions are the lamps' seen from the quad's centre,
    their irradiance what the lamps give there (1e6 / 1000^2 = 1) -- the light model of calibrated photometric stereo.  Returns the final mean angular error of the normals, if any (with lights: that and the ms per step)."""
    rng = np.random.default_rng(3)
    kd_true = rng.uniform(0.2, 0.8, (map_res * map_res, 3)).astype(np.float32)
    r_true = rng.uniform(0.3, 0.6, map_res * map_res).astype(np.float32)
    integ = psdr_cuda.CollocatedIntegrator(1e6)
    integs = [integ] * 3
    if height:
        tilts = ((0.0, 0.0), (35.0, 0.0), (0.0, 35.0))          # head-on (the specular lobe: roughness), about y and about x (the sign of each slope)
        h_true = rng.uniform(0.0, 1.0, map_res * map_res).astype(np.float32)
    if normals:
        tilts = ((35.0, 0.0), (-35.0, 0.0), (0.0, 35.0))          # (about y, about x)
        v_true = np.concatenate([rng.uniform(-0.35, 0.35, (map_res * map_res, 2)), np.ones((map_res * map_res, 1))], axis=1)
        n_true = ((v_true + 1.0) / 2.0).astype(np.float32)          # the image encoding: texel = (v + 1) / 2
        if lights:
            tilts = ((0.0, 0.0),) * 3
            lamps = [(600.0 * np.cos(a), 125.0 + 600.0 * np.sin(a), 800.0) for a in np.radians([0.0, 120.0, 240.0])]
            integs = [psdr_cuda.PointLightIntegrator(p, 1e6) for p in lamps]
            if distant:
                integs = [psdr_cuda.DistantLightIntegrator((p[0], p[1] - 125.0, p[2]), 1.0) for p in lamps]
            if stack:
                tilts, integs = ((0.0, 0.0),), [psdr_cuda.LightStageIntegrator(lamps, 1e6)]

    def view(tilt, spp_, kd, rough, nm=None, hm=None):
        sc = psdr_cuda.Scene()
        if normals or height:
            sc.load_string((SVBRDF_XML % tilt[0]).replace('y="1"/><translate', 'y="1"/><rotate angle="%g" x="1"/><translate' % tilt[1]), False)
        else:
            sc.load_string(SVBRDF_XML % tilt, False)
        sc.opts.width = sc.opts.height = res
        sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp_, 0, 0, 0
        b = sc.param_map["BSDF[id=m]"]
        b.diffuse_reflectance.resolution = b.roughness.resolution = (map_res, map_res)
        b.diffuse_reflectance.data, b.roughness.data = kd, rough
        if nm is not None:
            b.normal_map = psdr_cuda.Bitmap3fD(map_res, map_res, nm)
        if hm is not None:
            b.height_map = psdr_cuda.Bitmap1fD(map_res, map_res, hm)
            b.height_scale = psdr_cuda.Bitmap1fD(2.0)
        return sc
    targets = []
    for tilt, integ in zip(tilts, integs):
        ref = view(tilt, 256, Vector3fD(torch.as_tensor(kd_true, device="cuda")), FloatD(torch.as_tensor(r_true, device="cuda")),
                   Vector3fD(torch.as_tensor(n_true, device="cuda")) if normals else None, FloatD(torch.as_tensor(h_true, device="cuda")) if height else None)
        ref.configure()
        targets.append(integ.renderC(ref).torch().clone())
    kd = Vector3fD(torch.full((map_res * map_res, 3), 0.5, device="cuda"))
    rough = FloatD(torch.full((map_res * map_res,), 0.45, device="cuda"))
    ek.set_requires_gradient(kd)
    ek.set_requires_gradient(rough)
    params = [kd.t, rough.t]
    nm = None
    if normals:
        nm = Vector3fD(torch.tensor([[0.5, 0.5, 1.0]], device="cuda").repeat(map_res * map_res, 1))
        ek.set_requires_gradient(nm)
        params.append(nm.t)
    hm = None
    if height:
        hm = FloatD(torch.full((map_res * map_res,), 0.5, device="cuda"))
        ek.set_requires_gradient(hm)
        params.append(hm.t)
    views = [view(tilt, spp, kd, rough, nm, hm) for tilt in tilts]
    opt = torch.optim.Adam(params, lr=0.03)

    def angle():
        a, b = 2.0 * nm.numpy().astype(np.float64) - 1.0, 2.0 * n_true.astype(np.float64) - 1.0
        a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
        return float(np.degrees(np.arccos(np.clip((a * b).sum(1), -1.0, 1.0))).mean())

    def relief():
        a, b = hm.numpy().reshape(-1).astype(np.float64), h_true.astype(np.float64)
        return float(np.abs((a - a.mean()) - (b - b.mean())).mean())

    def report():
        return "mean texel error: kd %.4f, roughness %.4f%s%s" % (float(np.abs(kd.numpy() - kd_true).mean()), float(np.abs(rough.numpy().reshape(-1) - r_true).mean()),
                                                                 ", mean angular error of the normals %.2f degrees" % angle() if normals else "",
                                                                 ", height (means removed) %.4f" % relief() if height else "")
    print("  start     %s" % report())
    t0 = time.perf_counter()
    for it in range(steps):
        opt.zero_grad()
        total = 0.0
        for sc, target, integ in zip(views, targets, integs):
            sc.configure()
            loss = ek.hmean(ek.hsum(ek.sqr(integ.renderD(sc) - Vector3fD._wrap(target))))
            if stack:
                loss = loss * 3.0          # the mean over the stack's three planes: three times that is the sum of the three lamps' means
            ek.backward(loss)
            total += float(loss.t.item())
        opt.step()
        kd.t.data.clamp_(0.01, 0.99)
        rough.t.data.clamp_(0.05, 1.0)
        if normals:
            nm.t.data.clamp_(0.0, 1.0)
        if it % 10 == 0 or it == steps - 1:
            print("  step %3d  loss %.5f  %s" % (it, total, report()))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print("  %.1f ms per step (%s)" % (ms, "one stack of three lamps" if stack else "three views"))
    if lights:
        return angle(), ms
    return angle() if normals else None


def icosphere(level):
    """unit icosphere: (vertices [V, 3], faces [F, 3])"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [np.array(p, np.float64) for p in ((-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1))]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, nf = {}, []
        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                v.append(v[a] + v[b])
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v)
    return v / np.linalg.norm(v, axis=1, keepdims=True), np.array(f, np.int32)


def shape():
    """Per-vertex shape optimisation.  Raw vertex gradients of a Monte Carlo boundary estimator tangle a mesh within a few Adam steps; the parameter is
    therefore u = (I + lambda L) x (psdr_cuda.LargeSteps), the positions are recovered by one solve per step, warm-started from the previous step's, and
    the backward pass turns the vertex gradient into (I + lambda L)^-1 g by a second solve."""
    integ = psdr_cuda.DirectIntegrator(1, 1)
    v, f = icosphere(3)

    def scene(verts, spp, sppe=0, sppse=0):
        sc = load("cbox_occluder", spp=spp, sppe=sppe, sppse=sppse)
        sc.param_map["Mesh[id=occluder]"].set_geometry(verts, f)
        return sc
    ref = scene(v * 35.0, 128); ref.configure()
    target = integ.renderC(ref).torch().clone()
    # start: the sphere squeezed and dented
    start = v * np.array([45.0, 25.0, 35.0]) * (1.0 + 0.15 * np.sin(4.0 * v[:, :1]))
    sc = scene(start, 16, 16, 16)
    mesh = sc.param_map["Mesh[id=occluder]"]
    ls = psdr_cuda.LargeSteps(mesh, lmbda=19.0)
    u = ls.to_differential(ek.detach(mesh.vertex_positions))
    ek.set_requires_gradient(u)
    truth = torch.as_tensor(v * 35.0, dtype=torch.float32, device="cuda")
    state = {"x": None}

    def apply():
        x = ls.from_differential(u, x0=state["x"])
        state["x"] = ek.detach(x)
        mesh.vertex_positions = x
    apply()
    loop(sc, integ, target, [u], 1.0, 120, apply,
         lambda: "mean vertex distance %.3f, %d CG iterations" % (float((state["x"].t - truth).norm(dim=1).mean()), ls.info()["iterations"]))


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "albedo"
    if which == "svbrdf" and "--height" in sys.argv[2:]:
        svbrdf(height=True)
    elif which == "svbrdf" and "--normals" in sys.argv[2:] and "--lights" in sys.argv[2:]:
        print("three tilts under the flash at the camera (CollocatedIntegrator):")
        tilted = svbrdf(normals=True)
        print("one view under three lamps (PointLightIntegrator):")
        lit, lit_ms = svbrdf(normals=True, lights=True)
        print("mean angular error of the normals: three lamps %.2f degrees, three tilts %.2f degrees" % (lit, tilted))
        if "--distant" in sys.argv[2:]:
            print("one view under three distant lamps (DistantLightIntegrator):")
            far, far_ms = svbrdf(normals=True, lights=True, distant=True)
            print("mean angular error of the normals: three distant lamps %.2f degrees (%.1f ms per step), three point lamps %.2f degrees (%.1f ms per step)" % (far, far_ms, lit, lit_ms))
        if "--stack" in sys.argv[2:]:
            print("one view under three lamps as one stack (LightStageIntegrator):")
            stacked, stacked_ms = svbrdf(normals=True, lights=True, stack=True)
            print("three lamps: one LightStageIntegrator %.1f ms per step (normals %.2f degrees), three PointLightIntegrators %.1f ms per step (normals %.2f degrees)" %
                  (stacked_ms, stacked, lit_ms, lit))
    elif which == "svbrdf" and "--normals" in sys.argv[2:]:
        svbrdf(normals=True)
    else:
        {"albedo": albedo, "translation": translation, "envmap": envmap, "svbrdf": svbrdf, "shape": shape}[which]()
