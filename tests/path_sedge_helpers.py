"""Front-end of tests/hostcheck/hostcheck_path_sedge.cpp: the PathTracer's secondary-edge term (csrc/psdr_path_sedge.h) run on the host."""
import ctypes as C

import numpy as np

from helpers import _grad_buffers, AD_KEYS
from hostlibs import cpu_desc, host_threads, load, tangents_struct
from psdr_cuda import _abi


def path_sedge_lib():
    return load("path_sedge")


def path_opts(max_depth, sppse, rng_offset=(0, 0, 0), sppse_range=None, spp=0, sppe=0):
    return _abi.make_opts(integrator=_abi.INTEGRATOR_PATH, max_depth=max_depth, spp=spp, sppe=sppe, sppse=sppse, sppse_range=sppse_range,
                          rng_offset=rng_offset, flags=_abi.FLAG_PATH_SEDGES)


def host_path_sedge_fwd(tb, opts, tangents, seg=3, walk=1, nthreads=None):
    """Forward mode (K = 1) on the host: the derivative image of the secondary-edge term alone."""
    tbc, desc, keep = cpu_desc(tb)
    dimg = np.zeros(tb["width"] * tb["height"] * 3, np.float32)
    tan = tangents_struct(tangents, keep)
    rc = path_sedge_lib().hostcheck_path_sedge_fwd(C.byref(desc), C.byref(opts), int(seg), int(walk), C.byref(tan), C.c_void_p(dimg.ctypes.data), nthreads or host_threads())
    assert rc == 0, rc
    return dimg.reshape(-1, 3)


def host_path_sedge_rev(tb, opts, adj, want=AD_KEYS, seg=3, walk=1):
    """Reverse mode on the host: {table: gradient} of the secondary-edge term alone."""
    tbc, desc, keep = cpu_desc(tb)
    bufs, g = _grad_buffers(tbc, want)
    adj = np.ascontiguousarray(adj, dtype=np.float32).reshape(-1)
    rc = path_sedge_lib().hostcheck_path_sedge_rev(C.byref(desc), C.byref(opts), int(seg), int(walk), C.c_void_p(adj.ctypes.data), C.byref(g))
    assert rc == 0, rc
    return bufs


def host_path_sedge_survivors(tb, opts):
    """(survivors of segment A's filter, of segment B's, slots) on the host"""
    tbc, desc, keep = cpu_desc(tb)
    out = (C.c_longlong * 3)()
    rc = path_sedge_lib().hostcheck_path_sedge_survivors(C.byref(desc), C.byref(opts), out)
    assert rc == 0, rc
    return int(out[0]), int(out[1]), int(out[2])


# ---------------------------------------------------------------- scenarios of the AD-against-FD tests (CPU and GPU)
_HEAD = """<scene version="0.5.0">
<sensor type="perspective">
<float name="fov" value="%(fov)g"/>
<string name="fovAxis" value="x"/>
<transform name="toWorld">
<lookAt origin="0, 125, 1000" target="%(target)s" up="%(up)s"/>
</transform>
<sampler type="independent"><integer name="sampleCount" value="8"/></sampler>
<film type="hdrfilm"><integer name="width" value="24"/><integer name="height" value="24"/><rfilter type="box"/></film>
</sensor>
<bsdf id="white" type="diffuse"><rgb name="reflectance" value="0.95, 0.95, 0.95"/></bsdf>
<bsdf id="red" type="diffuse"><rgb name="reflectance" value="0.9, 0.2, 0.2"/></bsdf>
<bsdf id="green" type="diffuse"><rgb name="reflectance" value="0.2, 0.9, 0.2"/></bsdf>
<bsdf id="black" type="diffuse"><rgb name="reflectance" value="0, 0, 0"/></bsdf>
<bsdf id="mirror" type="roughconductor"><float name="alpha" value="0.15"/><rgb name="eta" value="0.155, 0.117, 0.138"/><rgb name="k" value="4.83, 3.12, 2.15"/></bsdf>
"""


def _quad(obj, bsdf, transform="", emitter=None, shape_id=None):
    return ('<shape %stype="obj"><string name="filename" value="./data/objects/cbox/%s.obj"/>%s<boolean name="faceNormals" value="true"/><ref id="%s"/>%s</shape>\n'
            % ('id="%s" ' % shape_id if shape_id else "", obj, "<transform name=\"toWorld\">%s</transform>" % transform if transform else "", bsdf,
               '<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % emitter if emitter else ""))


# Only the surfaces a scenario needs: every edge of a static surface is drawn as often as one of the occluder's and adds nothing to the derivative.
# "uplight": the emitter (Mesh[0]) faces the ceiling, so the floor is lit by the ceiling alone; the occluder (Mesh[1]) hangs between the two.  Its shadow on
# the floor has no direct-source boundary segment at all: the indirect-source segment carries it.
UPLIGHT_XML = (_HEAD % dict(fov=13, target="0, 124.965, 999.001", up="0, 0.999388, -0.0349786") +
               _quad("emitter", "black", '<scale x="0.6" z="0.6"/><rotate angle="180" x="1"/><translate x="40" y="130" z="20"/>', emitter="60, 60, 40") +
               _quad("emitter", "white", '<scale x="0.75" z="0.75"/><rotate angle="180" x="1"/><translate x="-20" y="40" z="40"/>', shape_id="occluder") +
               _quad("floor", "white") + _quad("ceil", "white") + "</scene>\n")

# "mirror": the camera looks at a rough-conductor quad (Mesh[2], 45 degrees, alpha 0.15) over the back of the room and sees the floor under it, and the
# occluder's (Mesh[1]) shadow there, only in that quad -- a black blind (Mesh[3]) hides that part of the floor from the camera itself: the shadow boundary
# reaches the image through one bounce of the sensor-side walk.
MIRROR_XML = (_HEAD % dict(fov=20, target="0, 70, -40", up="0, 1, 0") +
              _quad("emitter", "black", '<translate x="0" y="190" z="160"/>', emitter="20, 20, 8") +
              _quad("emitter", "white", '<scale x="0.75" z="0.75"/><rotate angle="180" x="1"/><translate x="0" y="20" z="-10"/>', shape_id="occluder") +
              _quad("emitter", "mirror", '<rotate angle="-45" x="1"/><translate x="0" y="70" z="-40"/>') +
              _quad("emitter", "black", '<scale x="1.5" z="0.5"/><rotate angle="90" x="1"/><translate x="0" y="20" z="100"/>') +
              _quad("floor", "white", '<scale x="0.6"/>') + "</scene>\n")

SCENARIOS = {            # name: (fixture name or XML, max_depth, the direction Mesh[1] is translated along)
    "occluder": ("cbox_occluder", 3, (1.0, 0.5, 0.0)),
    "uplight": (UPLIGHT_XML, 2, (1.0, 0.0, 0.5)),
    "mirror": (MIRROR_XML, 2, (1.0, 0.0, 0.5)),
}


def scenario_scene(name, spp, sppe=0, sppse=0, offset=None, res=24):
    """The scenario's scene at res x res.  offset = None: Mesh[1] translated by direction * P, P a FloatD that requires a gradient -> (scene, P);
    offset = a number: translated by direction * offset (the finite-difference renders) -> (scene, None)."""
    import enoki as ek
    import psdr_cuda
    from enoki.cuda_autodiff import Float32 as FloatD, Vector3f as Vector3fD, Matrix4f as Matrix4fD
    from psdr_cuda.fixtures import scene_path
    src, _, direction = SCENARIOS[name]
    sc = psdr_cuda.Scene()
    if src.lstrip().startswith("<"):
        sc.load_string(src, False)
    else:
        sc.load_file(scene_path(src), False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, sppse, 0
    P = None
    if offset is None:
        P = FloatD(0.)
        ek.set_requires_gradient(P)
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(direction)) * P))
    else:
        sc.param_map["Mesh[1]"].set_transform(Matrix4fD.translate(Vector3fD(list(direction)) * FloatD(float(offset))))
    sc.configure()
    return sc, P
