"""Front-end of tests/hostcheck/hostcheck_collocated.cpp (the CollocatedIntegrator's estimator, csrc/psdr_collocated.h, run on the host) and the small scenes the
CollocatedIntegrator's tests share."""
import ctypes as C

import numpy as np

import hostlibs
import psdr_cuda
from helpers import _grad_buffers, AD_KEYS
from hostlibs import HC_DIR, cpu_desc, host_threads, tangents_struct
from psdr_cuda import _abi

HC_DEPS = hostlibs.deps("collocated")          # (what tests/test_collocated_host.py's stand-alone program is stale against, besides its own source)


def collocated_lib():
    return hostlibs.load("collocated")


def colloc_opts(spp, sppe=0, rng_offset=(0, 0, 0), spp_range=None, sppe_range=None, sppse=0):
    return _abi.make_opts(integrator=_abi.INTEGRATOR_COLLOCATED, spp=spp, sppe=sppe, sppse=sppse, spp_range=spp_range, sppe_range=sppe_range, rng_offset=rng_offset)


def host_colloc_render(tb, opts, mode=0, tangents=None, nthreads=None):
    """renderC (mode 0: image) or forward mode, K = 1 (mode 1: image, derivative image) of the product code on the host, unit intensity."""
    tbc, desc, keep = cpu_desc(tb)
    n = tb["width"] * tb["height"] * 3
    img, dimg = np.zeros(n, np.float32), np.zeros(n, np.float32)
    tan = tangents_struct(tangents, keep)
    rc = collocated_lib().hostcheck_collocated_render(C.byref(desc), C.byref(opts), int(mode), C.byref(tan), C.c_void_p(img.ctypes.data), C.c_void_p(dimg.ctypes.data), nthreads or host_threads())
    assert rc == 0, rc
    return (img.reshape(-1, 3), dimg.reshape(-1, 3)) if mode else img.reshape(-1, 3)


def host_colloc_rev(tb, opts, adj, want=AD_KEYS):
    """Reverse mode on the host: (image, {table: gradient})."""
    tbc, desc, keep = cpu_desc(tb)
    bufs, g = _grad_buffers(tbc, want)
    adj = np.ascontiguousarray(adj, dtype=np.float32).reshape(-1)
    img = np.zeros(adj.shape[0], np.float32)
    rc = collocated_lib().hostcheck_collocated_rev(C.byref(desc), C.byref(opts), C.c_void_p(adj.ctypes.data), C.c_void_p(img.ctypes.data), C.byref(g))
    assert rc == 0, rc
    return img.reshape(-1, 3), bufs


def host_film_samples(tb, opts):
    """(sx, sy) of every camera slot of renderC, slot order (pixel-major), as the harness draws them: [W H nsp, 2]"""
    tbc, desc, keep = cpu_desc(tb)
    n = tb["width"] * tb["height"] * (opts.spp_end - opts.spp_begin)
    out = np.zeros(2 * n, np.float32)
    assert collocated_lib().hostcheck_collocated_film_samples(C.byref(desc), C.byref(opts), C.c_void_p(out.ctypes.data)) == 0
    return out.reshape(-1, 2)


# ---------------------------------------------------------------- scenes
_HEAD = """<scene version="0.5.0">
<sensor type="perspective">
<float name="fov" value="13"/>
<string name="fovAxis" value="x"/>
<transform name="toWorld">
<lookAt origin="0, 125, 1000" target="0, 124.965, 999.001" up="0, 0.999388, -0.0349786"/>
</transform>
<sampler type="independent"><integer name="sampleCount" value="4"/></sampler>
<film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="16"/><rfilter type="box"/></film>
</sensor>
"""
DIFFUSE = '<bsdf id="m" type="diffuse"><rgb name="reflectance" value="0.7, 0.5, 0.3"/></bsdf>\n'
ROUGH = '<bsdf id="m" type="roughconductor"><float name="alpha" value="%g"/><rgb name="eta" value="0.2, 0.92, 1.1"/><rgb name="k" value="3.9, 2.45, 2.14"/></bsdf>\n'


def quad_xml(bsdf=DIFFUSE, tilt=0.0, emitter=False):
    """One 160 x 160 quad at the cbox camera's target, its normal turned from the viewing axis by `tilt` degrees about y: covers the middle of the film, the
    border pixels miss it.  No emitter unless asked for: the CollocatedIntegrator needs none."""
    em = '<emitter type="area"><rgb name="radiance" value="5, 5, 5"/></emitter>' if emitter else ""
    return (_HEAD + bsdf + '<shape type="obj"><string name="filename" value="./data/objects/cbox/emitter.obj"/><transform name="toWorld"><scale x="2" z="2"/>'
            '<rotate angle="-90" x="1"/><rotate angle="%g" y="1"/><translate x="0" y="125" z="0"/></transform><boolean name="faceNormals" value="true"/><ref id="m"/>%s</shape>\n</scene>\n'
            % (tilt, em))


def xml_scene(xml, res=16, spp=4, sppe=0, prepare=None):
    sc = psdr_cuda.Scene()
    sc.load_string(xml, False)
    sc.opts.width = sc.opts.height = res
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse, sc.opts.log_level = spp, sppe, 0, 0
    if prepare is not None:
        prepare(sc)
    sc.configure()
    return sc
