"""Integrators: the Python mirror of reference include/psdr/integrator/*.h, src/integrator/*.cpp.

`renderC` / `renderD` keep the reference's signatures and return conventions (src/psdr.cpp:282-294)
and run ENTIRELY on the HIP library behind include/psdr_hip.h.  There is no CPU fallback: without
libpsdr_hip.so or without a GPU the calls raise.

Multi-GPU: when torch.distributed is initialised, every rank renders the sample
slots s in [rank*spp/G, (rank+1)*spp/G) of every pixel and the image (and forward-mode
derivative image / reverse-mode gradient tables) is summed with ONE all-reduce per render call.
"""
import ctypes as C
import time

import numpy as np
import torch

import enoki as ek
from . import _abi
from .core import Object, psdr_assert, Vector3fC, Vector3fD, HyperCubeDistribution3f
from .scene import make_desc, MicrofacetBSDF, MICROFACET_COLLOCATED_ONLY, NORMAL_MAP_NEEDS_UV, HEIGHT_MAP_NEEDS_UV

_AD_KEYS = _abi.TANGENT_FIELDS


_SOLO = 0
_FORCE = False
_DECIDED = []          # innermost first: the collective decision a deferred render (renderD's lazy image, its backward) was created under


class solo:
    """`with integrator.solo():` -- render calls inside the block run on THIS rank alone: no spp sharding, no collective.  For work only one rank of a
    multi-rank job does while the others wait (bench.py: rank 0's counter passes and single-GPU side blocks at any world size).  A renderD issued inside
    the block keeps that decision when its image / gradient is evaluated later, outside the block (_RenderNode.collective)."""

    def __enter__(self):
        global _SOLO
        _SOLO += 1
        return self

    def __exit__(self, *exc):
        global _SOLO
        _SOLO -= 1
        return False


def force_collectives(on=True):
    """Developer switch (a function: the package reads no environment variable): the render calls issue their collectives at world size 1 too, so that every
    all-reduce of a render call EXECUTES on a one-GPU box -- over RCCL when the process group's backend is nccl (tests/test_rccl_single_rank_gpu.py; bench.py
    turns it on when ITS environment holds PSDR_FORCE_COLLECTIVES=1)."""
    global _FORCE
    _FORCE = bool(on)


class _decided:
    """Evaluate a deferred render under the collective decision taken when renderD was called."""

    def __init__(self, collective):
        self.collective = bool(collective)

    def __enter__(self):
        _DECIDED.append(self.collective)
        return self

    def __exit__(self, *exc):
        _DECIDED.pop()
        return False


def _dist():
    """torch.distributed when the render call takes part in the job's collectives: more than one rank (or force_collectives), not inside solo(), and -- for a
    deferred render -- what was decided when renderD was called."""
    import torch.distributed as dist
    if _DECIDED:
        return dist if (_DECIDED[-1] and dist.is_available() and dist.is_initialized()) else None
    if _SOLO:
        return None
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _FORCE):
        return dist
    return None


def shard_range(n, rank, world):
    """Slots [begin, end) of `n` per-pixel samples owned by `rank` (balanced, contiguous)."""
    base, rem = divmod(n, world)
    b = rank * base + min(rank, rem)
    return b, b + base + (1 if rank < rem else 0)


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _RenderNode:
    """What renderD remembers so that a tangent (ek.forward) or an adjoint (ek.backward) can be
    pushed through the renderer later: the table tensors (with their torch graph), the render
    options including the RNG offsets of the primal call, and the guiding grid."""

    def __init__(self, integrator, scene, sensor_id, tb, opts, guide):
        self.integrator, self.scene, self.sensor_id = integrator, scene, sensor_id
        self.tb, self.opts, self.guide = tb, opts, guide
        self.collective = _dist() is not None          # the sharding of `opts` was fixed under this decision: the deferred launches keep it

    def input_tensors(self):
        return [self.tb.get(k) for k in _AD_KEYS] if self.tb is not None else [None] * len(_AD_KEYS)

    def render_forward(self, tangents):
        with _decided(self.collective):
            img, dimgs = self.integrator._render_fwd(self.scene, self.tb, self.opts, self.guide, [tangents])
        self.primal = img.reshape(-1, 3)           # by-product of the forward-mode launch: renderD's value
        return dimgs[0].reshape(-1, 3)

    def release(self):
        pass


class _LazyImage(Vector3fD):
    """What renderD returns when a scene parameter requires a gradient: the image is rendered when it is first
    LOOKED AT.  `renderD(); enoki.forward(P); enoki.gradient(img)` -- the reference harness' sequence,
    examples/run_test.py:95-142 -- then costs ONE launch (the forward-mode kernel produces image and derivative image
    together) instead of a primal launch plus a forward-mode launch; any other use (numpy(), a torch loss for
    enoki.backward) renders the primal through the autograd bridge on first access of `.t`."""

    @classmethod
    def _make(cls, node, inputs):
        o = cls.__new__(cls)
        o._node, o._inputs, o._t = node, inputs, None
        return o

    @property
    def t(self):
        if self._t is None:
            primal = getattr(self._node, "primal", None)
            if primal is not None:
                self._t = primal
            else:
                with torch.enable_grad():          # a first look under no_grad() must not cache an image without autograd history
                    self._t = _RenderFn.apply(self._node, *self._inputs)
            self._inputs = None
        return self._t

    @t.setter
    def t(self, v):
        self._t = v


class _ReducingImage(Vector3fC):
    """renderC on several GPUs: the all-reduce of the image is issued asynchronously and joined when the image is first LOOKED AT, so
    that the next render call's kernel (the harness renders renderD right after renderC) runs while the ring moves the 3 W H floats."""

    @classmethod
    def _make(cls, t, work):
        o = cls.__new__(cls)
        o._t, o._work = t, work
        return o

    @property
    def t(self):
        if self._work is not None:
            self._work.wait()                     # nccl: the current stream waits for the collective; gloo: the host does
            self._work = None
        return self._t

    @t.setter
    def t(self, v):
        self._work, self._t = None, v


class _RenderFn(torch.autograd.Function):
    """torch.autograd bridge for reverse mode: forward = primal image, backward = psdr_render_d_rev."""

    @staticmethod
    def forward(ctx, node, *inputs):
        ctx.node = node
        ctx.present = [t is not None for t in inputs]
        # this primal render is going to be differentiated in reverse mode: where the reverse launch would repeat it as its value sweep (PathTracer on a
        # two-level scene), it runs with recording stages and the backward call below runs the adjoint kernel only (PSDR_FLAG_KEEP_RECORDS)
        geo = any(t is not None and t.requires_grad for t, k in zip(inputs, _AD_KEYS) if k in ("tri_info", "cam_to_world"))
        with _decided(node.collective):
            img = node.integrator._render_c(node.scene, node.tb, node.opts, node.guide, interior_only=True, keep_records=geo)
        return img.reshape(-1, 3)

    @staticmethod
    def backward(ctx, adj):
        node = ctx.node
        with _decided(node.collective):
            grads = node.integrator._render_rev(node.scene, node.tb, node.opts, node.guide, adj.contiguous().reshape(-1))
        out = [None]
        for k, present in zip(_AD_KEYS, ctx.present):
            out.append(grads.get(k) if present else None)
        return tuple(out)


class Integrator(Object):
    """reference include/psdr/integrator/integrator.h:8-28"""
    _type_name = "SamplingIntegrator"
    _kind = _abi.INTEGRATOR_DIRECT

    def __init__(self):
        super().__init__()
        self._guide = {}
        self._counters_src, self._counters_val, self._calls = None, None, 0

    @property
    def last_counters(self):
        """(rays traced, camera / primary-edge / secondary-edge slots) of the last render call; read from the device on
        first access (a host synchronisation -- the render calls themselves do not wait for the GPU)."""
        if self._counters_val is None and self._counters_src is not None:
            lib, scene = self._counters_src
            c = (C.c_uint64 * 4)()
            lib.psdr_get_counters(scene._native, c)
            self._counters_val = tuple(int(x) for x in c)
        return self._counters_val

    # ---- option block -----------------------------------------------------------
    def _opts(self, scene, with_edges):
        o = scene.opts
        dist = _dist()
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
        sppe = o.sppe if with_edges else 0
        path_sedges = self._kind == _abi.INTEGRATOR_PATH and getattr(self, "secondary_edges", False)
        sppse = o.sppse if (with_edges and (self._kind == _abi.INTEGRATOR_DIRECT or path_sedges)) else 0
        if sppse > 0 and path_sedges and self.max_depth > _abi.MAX_PATH_SEDGE_DEPTH:
            raise RuntimeError("PathTracer(secondary_edges=True): max_depth > %d is not supported for the secondary-edge term" % _abi.MAX_PATH_SEDGE_DEPTH)
        opts = _abi.make_opts(
            integrator=self._kind, bsdf_samples=getattr(self, "bsdf_samples", 1), light_samples=getattr(self, "light_samples", 1),
            max_depth=getattr(self, "max_depth", 1), hide_emitters=getattr(self, "hide_emitters", False),
            field=getattr(self, "_field_id", 0), spp=o.spp, sppe=sppe, sppse=sppse,
            spp_range=shard_range(o.spp, rank, world), sppe_range=shard_range(sppe, rank, world),
            sppse_range=shard_range(sppse, rank, world), rng_offset=scene._rng_offset,
            flags=_abi.FLAG_PATH_SEDGES if (path_sedges and sppse > 0) else 0)
        return opts

    def _advance_rng(self, scene, opts):
        d = _abi.draws_per_slot(opts)
        if opts.spp > 0:
            scene._rng_offset[0] += d[0]
        if opts.sppe > 0:
            scene._rng_offset[1] += d[1]
        if opts.sppse > 0:
            scene._rng_offset[2] += d[2]

    # ---- native plumbing ----------------------------------------------------------
    def _image_floats(self, tb):
        """floats of one image of this integrator (the LightStageIntegrator renders one plane per light)"""
        return tb["width"] * tb["height"] * 3

    def _prepare(self, scene, tb, guide):
        lib = _abi.load_hip()
        if not torch.cuda.is_available():
            raise RuntimeError("psdr_cuda: no GPU visible; the HIP render path has no CPU fallback")
        if scene._native is None:
            h = C.c_void_p()
            _abi.check(lib, lib.psdr_scene_create(C.byref(h)))
            scene._native = h
            for name, value in getattr(scene, "native_options", {}).items():
                _abi.check(lib, lib.psdr_scene_set_option(h, name.encode(), float(value)))
        desc, keep = make_desc(tb, guide)
        _abi.check(lib, lib.psdr_scene_set_tables(scene._native, C.byref(desc)))
        # the tree on the handle belongs to ONE set of tables: rebuild / refit whenever the tables submitted now are
        # not the ones it was built for (a renderD result differentiated after a later configure() brings its own,
        # older tables back -- and the next render call the newer ones again)
        stamp = tb.get("geo_version", scene._version)      # a material-only configure() keeps the geometry stamp
        if getattr(scene, "_bvh_version", None) != stamp:
            _abi.check(lib, lib.psdr_bvh_build(scene._native, _stream_ptr()))
            scene._bvh_version = stamp
        return lib, keep

    def _render_c(self, scene, tb, opts, guide, interior_only=False, defer_reduce=False, keep_records=False):
        lib, keep = self._prepare(scene, tb, guide)
        if keep_records and self._kind == _abi.INTEGRATOR_PATH:
            opts = type(opts).from_buffer_copy(opts)
            opts.flags |= _abi.FLAG_KEEP_RECORDS
        img = torch.empty(self._image_floats(tb), dtype=torch.float32, device="cuda")
        _abi.check(lib, lib.psdr_render_c(scene._native, C.byref(opts), img.data_ptr(), _stream_ptr()))
        self._counters(lib, scene)
        dist = _dist()
        if dist and defer_reduce:
            return img, dist.all_reduce(img, async_op=True)
        if dist:
            dist.all_reduce(img)
        return (img, None) if defer_reduce else img

    def _render_fwd(self, scene, tb, opts, guide, tangent_sets):
        lib, keep = self._prepare(scene, tb, guide)
        K = len(tangent_sets)
        n = self._image_floats(tb)
        buf = torch.empty((1 + K) * n, dtype=torch.float32, device="cuda")   # [image || derivative images]: one all-reduce
        tarr = (_abi.Tangents * K)()
        for k, ts in enumerate(tangent_sets):
            for name, t in zip(_abi.TANGENT_FIELDS, ts):
                if t is not None:
                    t = t.detach().to(torch.float32).contiguous()
                    keep.append(t)
                    setattr(tarr[k], "d_" + name, t.data_ptr())
        _abi.check(lib, lib.psdr_render_d_fwd(scene._native, C.byref(opts), K, tarr, buf.data_ptr(),
                                              buf.data_ptr() + 4 * n, _stream_ptr()))
        self._counters(lib, scene)
        dist = _dist()
        if dist:
            dist.all_reduce(buf)
        return buf[:n], [buf[(1 + k) * n:(2 + k) * n] for k in range(K)]

    def _render_rev(self, scene, tb, opts, guide, adj):
        lib, keep = self._prepare(scene, tb, guide)
        g = _abi.Grads()
        grads, flat = {}, []
        for name in _AD_KEYS:
            t = tb.get(name)
            if t is not None and t.requires_grad:
                flat.append((name, t.shape, t.numel()))
        total = sum(n for _, _, n in flat)
        gbuf = torch.zeros(max(total, 1), dtype=torch.float32, device="cuda")   # one flat buffer: one all-reduce
        off = 0
        for name, shape, n in flat:
            grads[name] = gbuf[off:off + n].view(shape)
            setattr(g, "g_" + name, gbuf.data_ptr() + 4 * off)
            off += n
        _abi.check(lib, lib.psdr_render_d_rev(scene._native, C.byref(opts), adj.data_ptr(), None, C.byref(g), _stream_ptr()))
        self._counters(lib, scene)
        dist = _dist()
        if dist:
            dist.all_reduce(gbuf)
        return grads

    def _counters(self, lib, scene):
        """The counters stay on the device until somebody looks (last_counters): no render call reads them back (the library's
        fused-vs-wavefront choice is a function of the scene and the options, not of earlier calls)."""
        self._counters_src, self._counters_val = (lib, scene), None
        self._calls += 1

    def _check_bsdfs(self, scene):
        """MicrofacetBSDF is an evaluation without sample / pdf: the integrators that sample a BSDF refuse the scene before any native call (the
        C ABI returns the same message)."""
        if self._kind in (_abi.INTEGRATOR_DIRECT, _abi.INTEGRATOR_PATH) and any(isinstance(b, MicrofacetBSDF) for b in scene.m_bsdfs):
            raise RuntimeError(MICROFACET_COLLOCATED_ONLY)
        # a normal map's tangent frame follows the texture coordinates: a mesh without them has no defined value (the C ABI refuses a scene without the table)
        if any(isinstance(m.bsdf, MicrofacetBSDF) and m.bsdf.normal_map is not None and not m.m_has_uv for m in scene.m_meshes):
            raise RuntimeError(NORMAL_MAP_NEEDS_UV)
        if any(isinstance(m.bsdf, MicrofacetBSDF) and m.bsdf.height_map is not None and not m.m_has_uv for m in scene.m_meshes):          # ... and so does a height map's basis
            raise RuntimeError(HEIGHT_MAP_NEEDS_UV)

    # ---- public API (src/psdr.cpp:282-285) -------------------------------------------
    def renderC(self, scene, sensor_id=0):
        self._check_bsdfs(scene)
        psdr_assert(scene.is_ready(), "Input scene must be configured!")
        psdr_assert(0 <= sensor_id < scene.num_sensors, "Invalid sensor id!")
        t0 = time.perf_counter()
        tb = scene.tables(sensor_id, capacity=True)
        opts = self._opts(scene, with_edges=False)
        img, work = self._render_c(scene, tb, opts, None, defer_reduce=True)
        self._advance_rng(scene, opts)
        if scene.opts.log_level:
            torch.cuda.synchronize()                     # only the log line needs the time; the image is stream-ordered
            self.log("Rendered in %g seconds." % (time.perf_counter() - t0))
        if work is not None:
            return _ReducingImage._make(img.reshape(-1, 3), work)
        return Vector3fC._wrap(img.reshape(-1, 3))

    def renderD(self, scene, sensor_id=0):
        self._check_bsdfs(scene)
        psdr_assert(scene.is_ready(), "Input scene must be configured!")
        psdr_assert(0 <= sensor_id < scene.num_sensors, "Invalid sensor id!")
        t0 = time.perf_counter()
        tb = scene.tables(sensor_id, capacity=True)
        opts = self._opts(scene, with_edges=True)
        if not (scene._sensor_tables[sensor_id]["num_prim_edges"] > 0):
            opts.sppe = opts.sppe_begin = opts.sppe_end = 0
        guide = self._guide.get(sensor_id)
        node = _RenderNode(self, scene, sensor_id, tb, opts, guide)
        inputs = node.input_tensors()
        if any(t is not None and t.requires_grad for t in inputs):
            img = _LazyImage._make(node, inputs)           # rendered on first use (see _LazyImage)
        else:
            img = Vector3fD._wrap(self._render_c(scene, tb, opts, guide, interior_only=True).reshape(-1, 3))
            img._node = node
        self._advance_rng(scene, opts)
        ek.register_render_node(img)
        if scene.opts.log_level:
            torch.cuda.synchronize()
            self.log("Rendered in %g seconds." % (time.perf_counter() - t0))
        return img

    def preprocess_secondary_edges(self, scene, sensor_id, resolution, nrounds=1):
        """DirectIntegrator::preprocess_secondary_edges, reference direct.cpp:166-204."""
        raise RuntimeError("preprocess_secondary_edges: only DirectIntegrator builds a guiding grid")


class FieldExtractionIntegrator(Integrator):
    """reference include/psdr/integrator/field.h, src/integrator/field.cpp"""
    _type_name = "FieldExtractionIntegrator"
    _kind = _abi.INTEGRATOR_FIELD

    def __init__(self, field):
        super().__init__()
        if field not in _abi.FIELDS:
            raise RuntimeError("Unsupported field: " + str(field))
        self.m_field = field
        self._field_id = _abi.FIELDS[field]


class DirectIntegrator(Integrator):
    """reference include/psdr/integrator/direct.h, src/integrator/direct.cpp"""
    _type_name = "DirectIntegrator"
    _kind = _abi.INTEGRATOR_DIRECT

    def __init__(self, bsdf_samples=1, light_samples=1):
        super().__init__()
        psdr_assert(bsdf_samples >= 0 and light_samples >= 0 and bsdf_samples + light_samples > 0)
        self.bsdf_samples, self.light_samples = int(bsdf_samples), int(light_samples)
        self.hide_emitters = False

    def preprocess_secondary_edges(self, scene, sensor_id, resolution, nrounds=1):
        self._check_bsdfs(scene)
        psdr_assert(nrounds > 0)
        psdr_assert(scene.is_ready(), "Scene needs to be configured!")
        reso = [int(r) for r in np.asarray(resolution).reshape(-1)]
        psdr_assert(len(reso) == 4)
        cells = reso[0] * reso[1] * reso[2]
        psdr_assert(cells * reso[3] < 2 ** 31 - 1)
        tb = scene.tables(sensor_id, capacity=True)
        lib, keep = self._prepare(scene, tb, None)
        mass = torch.zeros(cells, dtype=torch.float32, device="cuda")
        opts = self._opts(scene, with_edges=True)
        r = (C.c_int32 * 4)(*reso)
        _abi.check(lib, lib.psdr_guide_build(scene._native, C.byref(opts), r, int(nrounds), mass.data_ptr(), _stream_ptr()))
        dist = _dist()
        if dist:
            dist.all_reduce(mass)          # every rank evaluated all cells; keep replicas bit-identical
            mass /= dist.get_world_size()
        w = HyperCubeDistribution3f()
        w.set_resolution(reso[:3])
        w.set_mass(mass)
        torch.cuda.synchronize()
        self._guide[sensor_id] = (reso[:3], w.m_distrb.m_cmf, w.m_distrb.m_pmf, w.m_distrb.m_sum)
        return w


class PathTracer(Integrator):
    """Multi-bounce extension of DirectIntegrator::__Li.  NOT in the reference snapshot (SURVEY F2,
    App. F): defined so that PathTracer(max_depth=1) == DirectIntegrator(1, 1) sample for sample.

    secondary_edges=True: renderD also evaluates the secondary-edge boundary term (moving shadow and occlusion boundaries under global illumination,
    SURVEY App. F, F3) on scene.opts.sppse slots per pixel, in forward and reverse mode; max_depth <= 8.  Without it the geometry gradient of renderD
    holds the interior and the primary-edge term only and is wrong wherever a shadow edge moves.  The default is False because turning the term on
    changes the results of existing callers; a later change may flip it.

    The slots of the term are importance-sampled by up to two guiding grids per sensor, one per boundary segment of a slot, built by
    preprocess_path_secondary_edges (preprocess_secondary_edges stays DirectIntegrator's call: it builds one grid)."""
    _type_name = "PathTracer"
    _kind = _abi.INTEGRATOR_PATH

    def __init__(self, max_depth=3, secondary_edges=False):
        super().__init__()
        psdr_assert(max_depth >= 1)
        self.max_depth = int(max_depth)
        self.secondary_edges = bool(secondary_edges)
        self.bsdf_samples = self.light_samples = 1
        self.hide_emitters = False

    def _prepare(self, scene, tb, guide):
        """guide: None or (grid of segment A or None, grid of segment B or None).  Segment A's grid travels in the descriptor like DirectIntegrator's;
        segment B's lives on the handle, where psdr_scene_set_tables drops it: it is set again after every set_tables."""
        ga, gb = guide if guide is not None else (None, None)
        lib, keep = super()._prepare(scene, tb, ga)
        if gb is not None:
            reso, cmf, pmf, total = gb
            cmf, pmf = (t.detach().to(device="cuda", dtype=torch.float32).contiguous() for t in (cmf, pmf))
            keep += [cmf, pmf]
            _abi.check(lib, lib.psdr_scene_set_path_guide(scene._native, (C.c_int32 * 3)(*[int(r) for r in reso]), cmf.data_ptr(), pmf.data_ptr(), float(total)))
        return lib, keep

    def preprocess_path_secondary_edges(self, scene, sensor_id, resolution, resolution_indirect=None, nrounds=1):
        """Builds the guiding grids of the secondary-edge term for one sensor: `resolution` for the direct-source segment of a slot (over the slot's three
        numbers, as DirectIntegrator's grid), `resolution_indirect` for the indirect-source segment (over the edge number and the two direction numbers).
        Both are 4-vectors (cells along the three numbers, sample streams per cell) as in DirectIntegrator.preprocess_secondary_edges; None leaves that
        segment unguided.  Returns (HyperCubeDistribution3f or None, HyperCubeDistribution3f or None).  Every later renderD of the sensor uses the grids,
        in forward and reverse mode; calling the method again replaces them."""
        if not self.secondary_edges:
            raise RuntimeError("preprocess_path_secondary_edges: PathTracer(secondary_edges=False) never evaluates the slots the grids would guide")
        if self.max_depth > _abi.MAX_PATH_SEDGE_DEPTH:
            raise RuntimeError("preprocess_path_secondary_edges: max_depth > %d is not supported for the secondary-edge term" % _abi.MAX_PATH_SEDGE_DEPTH)
        self._check_bsdfs(scene)
        psdr_assert(nrounds > 0)
        psdr_assert(scene.is_ready(), "Scene needs to be configured!")
        psdr_assert(0 <= sensor_id < scene.num_sensors, "Invalid sensor id!")
        tb = scene.tables(sensor_id, capacity=True)
        lib, keep = self._prepare(scene, tb, None)
        opts = self._opts(scene, with_edges=True)
        dist = _dist()
        out, grids = [], []
        for segment, resolution_s in ((1, resolution), (2, resolution_indirect)):
            if resolution_s is None:
                out.append(None)
                grids.append(None)
                continue
            reso = [int(r) for r in np.asarray(resolution_s).reshape(-1)]
            psdr_assert(len(reso) == 4)
            cells = reso[0] * reso[1] * reso[2]
            psdr_assert(cells * reso[3] < 2 ** 31 - 1)
            mass = torch.zeros(cells, dtype=torch.float32, device="cuda")
            _abi.check(lib, lib.psdr_path_guide_build(scene._native, C.byref(opts), segment, (C.c_int32 * 4)(*reso), int(nrounds), mass.data_ptr(), _stream_ptr()))
            if dist:
                dist.all_reduce(mass)          # every rank evaluated all cells; keep replicas bit-identical
                mass /= dist.get_world_size()
            w = HyperCubeDistribution3f()
            w.set_resolution(reso[:3])
            w.set_mass(mass)
            out.append(w)
            grids.append((reso[:3], w.m_distrb.m_cmf, w.m_distrb.m_pmf, w.m_distrb.m_sum))
        torch.cuda.synchronize()
        if grids[0] is None and grids[1] is None:
            self._guide.pop(sensor_id, None)
        else:
            self._guide[sensor_id] = tuple(grids)
        return tuple(out)


class _CollocatedNode:
    """renderD of the CollocatedIntegrator: the unit-intensity render node (what the kernels compute) and the light's RGB intensity, which multiplies
    image and derivative image per channel on the host.  enoki.forward sees eight inputs: the seven tables and the intensity."""

    def __init__(self, unit, intensity):
        self.unit, self.intensity = unit, intensity

    def input_tensors(self):
        return self.unit.input_tensors() + [self.intensity.t]

    def render_forward(self, tangents):
        d_unit = self.unit.render_forward(list(tangents[:-1]))          # one forward-mode launch: unit image and its derivative
        unit, scale = self.unit.primal, self.intensity.t.detach().reshape(1, 3)
        self.primal = unit * scale
        d = d_unit * scale
        if tangents[-1] is not None:
            d = d + unit * tangents[-1].detach().reshape(1, 3)
        return d

    def render_primal(self):
        """image = unit image x intensity, with autograd history: torch's product rule hands the adjoint image, scaled per channel, to the reverse
        launch and the per-channel sum of adjoint x unit image to the intensity."""
        unit, inputs = self.unit, self.unit.input_tensors()
        with torch.enable_grad():
            if any(t is not None and t.requires_grad for t in inputs):
                img = _RenderFn.apply(unit, *inputs)
            else:
                with _decided(unit.collective):
                    img = unit.integrator._render_c(unit.scene, unit.tb, unit.opts, unit.guide, interior_only=True).reshape(-1, 3)
            return img * self.intensity.t.reshape(1, 3)

    def release(self):
        pass


class _CollocatedImage(Vector3fD):
    """What CollocatedIntegrator.renderD returns: rendered when first looked at, like _LazyImage (after enoki.forward the forward-mode launch has
    produced the image already)."""

    @classmethod
    def _make(cls, node):
        o = cls.__new__(cls)
        o._node, o._t = node, None
        return o

    @property
    def t(self):
        if self._t is None:
            primal = getattr(self._node, "primal", None)
            self._t = primal if primal is not None else self._node.render_primal()
        return self._t

    @t.setter
    def t(self, v):
        self._t = v


class CollocatedIntegrator(Integrator):
    """A point light at the camera position (a camera flash), the capture configuration in which albedo and roughness maps are recovered from
    photographs.  NOT in the reference snapshot: build-defined, like PathTracer.  For a camera ray with origin o that hits `its`

        Li = intensity * f(its; wi = its.wi, wo = its.wi) / |its.p - o|^2          (0 on a miss)

    with f the BSDF value, cosine included.  Emitters in the scene add nothing and a scene without any emitter is valid.  One ray per sample, no random
    numbers beyond the film jitter.  renderD's geometry gradient is the interior and the primary-edge term, and that is all of it: a point the camera
    sees is lit, so no shadow boundary is visible and scene.opts.sppse is ignored.

    intensity: a float, three floats (RGB) or a Vector3fD; kept as the differentiable attribute m_intensity.  The kernels render unit intensity
    (csrc/psdr_collocated.h); image, derivative image and adjoint image are scaled per channel here."""
    _type_name = "CollocatedIntegrator"
    _kind = _abi.INTEGRATOR_COLLOCATED

    def __init__(self, intensity=1.0):
        super().__init__()
        if isinstance(intensity, Vector3fD):
            psdr_assert(tuple(intensity.t.shape) == (1, 3), "intensity: one RGB triple expected")
            self.m_intensity = intensity
        else:
            v = [float(x) for x in np.asarray(intensity, dtype=np.float64).reshape(-1)]
            psdr_assert(len(v) in (1, 3), "intensity: a float or three floats expected")
            self.m_intensity = Vector3fD(v * 3 if len(v) == 1 else v)

    def renderC(self, scene, sensor_id=0):
        img = super().renderC(scene, sensor_id)          # unit intensity (joins the image's all-reduce)
        return Vector3fC._wrap(img.t * self.m_intensity.t.detach().reshape(1, 3).to(img.t.device))

    def renderD(self, scene, sensor_id=0):
        self._check_bsdfs(scene)          # (a normal map on a mesh without texture coordinates)
        psdr_assert(scene.is_ready(), "Input scene must be configured!")
        psdr_assert(0 <= sensor_id < scene.num_sensors, "Invalid sensor id!")
        t0 = time.perf_counter()
        tb = scene.tables(sensor_id, capacity=True)
        opts = self._opts(scene, with_edges=True)
        if not (scene._sensor_tables[sensor_id]["num_prim_edges"] > 0):
            opts.sppe = opts.sppe_begin = opts.sppe_end = 0
        img = _CollocatedImage._make(_CollocatedNode(_RenderNode(self, scene, sensor_id, tb, opts, None), self.m_intensity))
        self._advance_rng(scene, opts)
        ek.register_render_node(img)
        if scene.opts.log_level:
            img.t                                        # (the log line reports the render's time)
            torch.cuda.synchronize()
            self.log("Rendered in %g seconds." % (time.perf_counter() - t0))
        return img


class _PointRenderFn(torch.autograd.Function):
    """torch.autograd bridge of the PointLightIntegrator's reverse mode: _RenderFn with one more input, the light position, whose gradient
    psdr_render_d_rev adds into a device array of three floats."""

    @staticmethod
    def forward(ctx, node, pos, *inputs):
        ctx.node, ctx.present, ctx.pos_shape = node, [t is not None for t in inputs], pos.shape
        unit = node.unit
        with _decided(unit.collective), unit.integrator._light(node.pos):
            img = unit.integrator._render_c(unit.scene, unit.tb, unit.opts, unit.guide, interior_only=True)
        return img.reshape(-1, 3)

    @staticmethod
    def backward(ctx, adj):
        node, unit = ctx.node, ctx.node.unit
        g_pos = torch.zeros(3, dtype=torch.float32, device="cuda") if ctx.needs_input_grad[1] else None
        with _decided(unit.collective), unit.integrator._light(node.pos, g_pos=g_pos):
            grads = unit.integrator._render_rev(unit.scene, unit.tb, unit.opts, unit.guide, adj.contiguous().reshape(-1))
            dist = _dist()
            if dist and g_pos is not None:
                dist.all_reduce(g_pos)
            unit.integrator._forget_light(unit.scene)          # the handle must not keep the address of g_pos beyond this call
        out = [None, g_pos.reshape(ctx.pos_shape) if g_pos is not None else None]
        for k, present in zip(_AD_KEYS, ctx.present):
            out.append(grads.get(k) if present else None)
        return tuple(out)


class _PointLightNode(_CollocatedNode):
    """renderD of the PointLightIntegrator: _CollocatedNode with a ninth input, the light position (its value at the renderD call is the one every
    deferred launch of the node uses)."""

    def __init__(self, unit, intensity, position):
        super().__init__(unit, intensity)
        self.position = position
        self.pos = [float(x) for x in position.t.detach().reshape(-1).cpu()]

    def input_tensors(self):
        return super().input_tensors() + [self.position.t]

    def render_forward(self, tangents):
        d_pos = None if tangents[-1] is None else [float(x) for x in tangents[-1].detach().reshape(-1).cpu()]
        with self.unit.integrator._light(self.pos, d_pos=d_pos):
            return super().render_forward(list(tangents[:-1]))

    def render_primal(self):
        unit, inputs = self.unit, self.unit.input_tensors()
        with torch.enable_grad():
            pos = self.position.t
            if pos.requires_grad or any(t is not None and t.requires_grad for t in inputs):
                img = _PointRenderFn.apply(self, pos, *inputs)
            else:
                with _decided(unit.collective), unit.integrator._light(self.pos):
                    img = unit.integrator._render_c(unit.scene, unit.tb, unit.opts, unit.guide, interior_only=True).reshape(-1, 3)
            return img * self.intensity.t.reshape(1, 3).to(img.device)


class _light_scope:
    def __init__(self, integrator, pos, d_pos, g_pos):
        self.integrator, self.state = integrator, (pos, d_pos, g_pos)

    def __enter__(self):
        self.saved, self.integrator._light_state = self.integrator._light_state, self.state
        return self

    def __exit__(self, *exc):
        self.integrator._light_state = self.saved
        return False


class PointLightIntegrator(CollocatedIntegrator):
    """A point light at an arbitrary, differentiable world position: the set-up of photometric stereo, of a light stage, of a camera with an off-axis
    flash.  NOT in the reference snapshot: build-defined, like the CollocatedIntegrator it generalises.  For a camera ray that hits `its`, with the
    light at pL, dv = pL - its.p and r = |dv|

        Li = intensity * f(its; wi = its.wi, wo = to_local(dv / r)) * V(its.p, pL) / r^2          (0 on a miss)

    with f the BSDF value, cosine included (Diffuse, RoughConductor, MicrofacetBSDF with or without a normal or height map) and V the visibility of the
    light.  Emitters in the scene add nothing and a scene without any emitter is valid.  renderD's geometry gradient has three terms: the interior,
    the primary edges (scene.opts.sppe) and the boundary of the moving shadow outline (scene.opts.sppse slots of the secondary-edge table).

    position: three floats or a Vector3fD, kept as the differentiable attribute m_position; intensity: as CollocatedIntegrator's, m_intensity.  Both
    take part in enoki.forward and enoki.backward.  The kernels render ONE light of unit intensity (csrc/psdr_pointlight.h): several lights are
    several integrators whose images add."""
    _type_name = "PointLightIntegrator"
    _kind = _abi.INTEGRATOR_POINT
    _light_kind = _abi.LIGHT_POINT          # the model of m_position (DistantLightIntegrator: a direction)

    def __init__(self, position, intensity=1.0):
        super().__init__(intensity)
        if isinstance(position, Vector3fD):
            psdr_assert(tuple(position.t.shape) == (1, 3), "position: one point expected")
            self.m_position = position
        else:
            v = [float(x) for x in np.asarray(position, dtype=np.float64).reshape(-1)]
            psdr_assert(len(v) == 3 and all(np.isfinite(v)), "position: three finite floats expected")
            self.m_position = Vector3fD(v)
        self._light_state = None

    def _light(self, pos, d_pos=None, g_pos=None):
        """the light every native call inside the block renders with (position, its tangent in forward mode, its device gradient in reverse mode)"""
        return _light_scope(self, pos, d_pos, g_pos)

    def _opts(self, scene, with_edges):
        opts = super()._opts(scene, with_edges)
        if with_edges and scene.opts.sppse > 0:          # the shadow boundary: sppse slots, sharded like the other samplers
            dist = _dist()
            rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
            opts.sppse = scene.opts.sppse
            opts.sppse_begin, opts.sppse_end = shard_range(opts.sppse, rank, world)
        return opts

    def _prepare(self, scene, tb, guide):
        lib, keep = super()._prepare(scene, tb, guide)
        psdr_assert(self._light_state is not None, "PointLightIntegrator: no light in scope")
        pos, d_pos, g_pos = self._light_state
        args = ((C.c_float * 3)(*pos), 0 if d_pos is None else 1, None if d_pos is None else (C.c_float * 3)(*d_pos), None if g_pos is None else g_pos.data_ptr())
        if self._light_kind == _abi.LIGHT_POINT:
            _abi.check(lib, lib.psdr_scene_set_point_light(scene._native, *args))
        else:
            psdr_assert(not (tb.get("env_emitter", -1) >= 0), _abi.DISTANT_IN_ENV)
            _abi.check(lib, lib.psdr_scene_set_light(scene._native, self._light_kind, *args))
        if g_pos is not None:
            keep.append(g_pos)
        return lib, keep

    def _forget_light(self, scene):
        """removes the light from the scene's handle (with it the tangent and the gradient address of the last call); the next native call sets its own"""
        if scene._native is not None:
            lib = _abi.load_hip()
            _abi.check(lib, lib.psdr_scene_set_point_light(scene._native, None, 0, None, None))

    def renderC(self, scene, sensor_id=0):
        with self._light([float(x) for x in self.m_position.t.detach().reshape(-1).cpu()]):
            return super().renderC(scene, sensor_id)

    def renderD(self, scene, sensor_id=0):
        self._check_bsdfs(scene)
        psdr_assert(scene.is_ready(), "Input scene must be configured!")
        psdr_assert(0 <= sensor_id < scene.num_sensors, "Invalid sensor id!")
        t0 = time.perf_counter()
        tb = scene.tables(sensor_id, capacity=True)
        opts = self._opts(scene, with_edges=True)
        if not (scene._sensor_tables[sensor_id]["num_prim_edges"] > 0):
            opts.sppe = opts.sppe_begin = opts.sppe_end = 0
        if not (tb.get("num_sec_edges", 0) > 0):
            opts.sppse = opts.sppse_begin = opts.sppse_end = 0
        img = _CollocatedImage._make(_PointLightNode(_RenderNode(self, scene, sensor_id, tb, opts, None), self.m_intensity, self.m_position))
        self._advance_rng(scene, opts)
        ek.register_render_node(img)
        if scene.opts.log_level:
            img.t                                        # (the log line reports the render's time)
            torch.cuda.synchronize()
            self.log("Rendered in %g seconds." % (time.perf_counter() - t0))
        return img


class DistantLightIntegrator(PointLightIntegrator):
    """A distant (directional) light: a direction and an irradiance, the light model of calibrated and uncalibrated photometric stereo, or the sun.  NOT in
    the reference snapshot: build-defined.  direction points from the scene TOWARDS the light and need not be unit length; with u = direction / |direction|

        Li = irradiance * f(its; wi = its.wi, wo = to_local(u)) * V(its.p, u)          (0 on a miss)

    V the visibility along u to infinity; no 1 / r^2: irradiance is what a surface that faces the light receives, so a PointLightIntegrator at c + R u with
    intensity irradiance * R^2 tends to this image as R grows.  Everything else is the PointLightIntegrator's: renderC / renderD, the three gradient terms
    (the shadow boundary under parallel projection, csrc/psdr_pointlight.h), enoki.forward and enoki.backward, shards.

    direction: three floats or a Vector3fD, kept as the differentiable attribute m_direction -- its gradient is that of the vector as passed: tangential,
    and 1 / |direction| in size; irradiance: as CollocatedIntegrator's intensity, kept as m_intensity.  A scene inside an environment map's bounding mesh
    cannot be reached by a distant light: rendering it raises."""
    _type_name = "DistantLightIntegrator"
    _light_kind = _abi.LIGHT_DISTANT

    def __init__(self, direction, irradiance=1.0):
        if isinstance(direction, Vector3fD):
            psdr_assert(tuple(direction.t.shape) == (1, 3), "direction: one vector expected")
            v = [float(x) for x in direction.t.detach().reshape(-1).cpu()]
        else:
            v = [float(x) for x in np.asarray(direction, dtype=np.float64).reshape(-1)]
            psdr_assert(len(v) == 3, "direction: three finite floats expected")
        psdr_assert(all(np.isfinite(v)), "direction: three finite floats expected")
        psdr_assert(any(x != 0.0 for x in np.asarray(v, dtype=np.float32)), "direction: a vector that is not all zero expected")
        super().__init__(direction if isinstance(direction, Vector3fD) else v, irradiance)

    # the PointLightIntegrator reads m_position wherever it needs the light's vector: here that vector is m_direction
    @property
    def m_position(self):
        return self.m_direction

    @m_position.setter
    def m_position(self, value):
        self.m_direction = value


class _StackRenderFn(torch.autograd.Function):
    """torch.autograd bridge of the LightStageIntegrator's reverse mode: _PointRenderFn with the positions of all lights as the extra input; their
    gradients come back in a device array [L, 3]."""

    @staticmethod
    def forward(ctx, node, pos, *inputs):
        ctx.node, ctx.present, ctx.pos_shape = node, [t is not None for t in inputs], pos.shape
        unit = node.unit
        with _decided(unit.collective), unit.integrator._lights(node.pos):
            img = unit.integrator._render_c(unit.scene, unit.tb, unit.opts, unit.guide, interior_only=True)
        return img.reshape(-1, 3)

    @staticmethod
    def backward(ctx, adj):
        node, unit = ctx.node, ctx.node.unit
        g_pos = torch.zeros((len(node.pos), 3), dtype=torch.float32, device="cuda") if ctx.needs_input_grad[1] else None
        with _decided(unit.collective), unit.integrator._lights(node.pos, g_pos=g_pos):
            grads = unit.integrator._render_rev(unit.scene, unit.tb, unit.opts, unit.guide, adj.contiguous().reshape(-1))
            dist = _dist()
            if dist and g_pos is not None:
                dist.all_reduce(g_pos)
            unit.integrator._forget_lights(unit.scene)          # the handle must not keep the address of g_pos beyond this call
        out = [None, g_pos.reshape(ctx.pos_shape) if g_pos is not None else None]
        for k, present in zip(_AD_KEYS, ctx.present):
            out.append(grads.get(k) if present else None)
        return tuple(out)


class _LightStageNode:
    """renderD of the LightStageIntegrator: the unit-intensity render node of the whole stack ([L W H, 3], light-major), the intensities [L, 3] that scale
    plane l on the host and the positions [L, 3] (their values at the renderD call are the ones every deferred launch of the node uses).  enoki.forward
    sees nine inputs: the seven tables, the intensities and the positions.  combine: the image is sum_l intensity_l * unit_l, formed in torch."""

    def __init__(self, unit, intensities, positions, combine):
        self.unit, self.intensities, self.positions, self.combine = unit, intensities, positions, combine
        self.pos = [[float(x) for x in row] for row in positions.t.detach().reshape(-1, 3).cpu()]

    def input_tensors(self):
        return self.unit.input_tensors() + [self.intensities.t, self.positions.t]

    def _assemble(self, planes, scale):
        """planes [L W H, 3] x scale [L, 3] -> the stack [L W H, 3] or, combined, its sum over the lights [W H, 3]"""
        L = len(self.pos)
        stack = planes.reshape(L, -1, 3) * scale.reshape(L, 1, 3).to(planes.device)
        return stack.sum(dim=0) if self.combine else stack.reshape(-1, 3)

    def render_forward(self, tangents):
        d_int, d_pos = tangents[-2], tangents[-1]
        dp = None if d_pos is None else [[float(x) for x in row] for row in d_pos.detach().reshape(-1, 3).cpu()]
        with self.unit.integrator._lights(self.pos, d_pos=dp):
            d_unit = self.unit.render_forward(list(tangents[:-2]))          # one forward-mode launch: the unit stack and its derivative
        unit, scale = self.unit.primal, self.intensities.t.detach()
        self.primal = self._assemble(unit, scale)
        d = self._assemble(d_unit, scale)
        if d_int is not None:
            d = d + self._assemble(unit, d_int.detach())
        return d

    def render_primal(self):
        unit, inputs = self.unit, self.unit.input_tensors()
        with torch.enable_grad():
            pos = self.positions.t
            if pos.requires_grad or any(t is not None and t.requires_grad for t in inputs):
                img = _StackRenderFn.apply(self, pos, *inputs)
            else:
                with _decided(unit.collective), unit.integrator._lights(self.pos):
                    img = unit.integrator._render_c(unit.scene, unit.tb, unit.opts, unit.guide, interior_only=True).reshape(-1, 3)
            return self._assemble(img, self.intensities.t)

    def release(self):
        pass


class LightStageIntegrator(PointLightIntegrator):
    """L point lights rendered and differentiated in ONE call: the set-up of photometric stereo (3 to 12 lamps) and of a light stage (dozens).  NOT in the
    reference snapshot: build-defined.  Plane l is the PointLightIntegrator's image under light l -- the kernels (csrc/psdr_lightstage.h) find one hit per
    camera sample and loop over the lights from it, so the film jitter, the primary ray, the walk, the hit and, in reverse mode, the hit's adjoint chain
    are shared; the edge terms run per light.

    positions: an [L, 3] array (1 <= L <= 256) or a Vector3fD of L rows, kept as the differentiable attribute m_positions; intensities: a float, one RGB
    triple or [L, 3] (or a Vector3fD of L rows), kept as m_intensities.  combine=False: renderC / renderD return L*H*W rows, light-major, plane l scaled
    by intensity l.  combine=True: they return the one image sum_l intensity_l * unit_l (H*W rows), formed in torch from the stack.  The tables, the
    intensities and the positions take part in enoki.forward and enoki.backward.

    distant: None, or a sequence of L booleans (not differentiable).  A flagged row of m_positions is a DIRECTION towards a distant light
    (DistantLightIntegrator's model, its intensity an irradiance; the row's gradient is tangential and 1 / |row| in size); a stack may mix the two kinds
    in any order.  None is a stack of point lights."""
    _type_name = "LightStageIntegrator"
    _kind = _abi.INTEGRATOR_POINT_STACK

    def __init__(self, positions, intensities=1.0, combine=False, distant=None):
        Integrator.__init__(self)
        if isinstance(positions, Vector3fD):
            psdr_assert(positions.t.dim() == 2 and positions.t.shape[1] == 3, "positions: [L, 3] expected")
            self.m_positions = positions
        else:
            p = np.asarray(positions, dtype=np.float64)
            psdr_assert(p.ndim == 2 and p.shape[1] == 3 and np.isfinite(p).all(), "positions: an [L, 3] array of finite floats expected")
            self.m_positions = Vector3fD(torch.from_numpy(p.astype(np.float32)))
        L = int(self.m_positions.t.shape[0])
        psdr_assert(1 <= L <= _abi.POINT_LIGHTS_MAX, "positions: between 1 and %d lights expected" % _abi.POINT_LIGHTS_MAX)
        if isinstance(intensities, Vector3fD):
            psdr_assert(tuple(intensities.t.shape) == (L, 3), "intensities: [L, 3] expected")
            self.m_intensities = intensities
        else:
            v = np.asarray(intensities, dtype=np.float64)
            psdr_assert(v.size in (1, 3) or v.shape == (L, 3), "intensities: a float, three floats or [L, 3] expected")
            v = np.broadcast_to(v.reshape(1, -1) if v.size in (1, 3) else v, (L, 3))
            self.m_intensities = Vector3fD(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
        self.combine = bool(combine)
        self._light_state = None
        self.distant = None
        if distant is not None:
            flags = [bool(x) for x in distant]
            psdr_assert(len(flags) == L, "distant: %d flags expected, one per light" % L)
            rows = self.m_positions.t.detach().reshape(-1, 3).cpu().numpy()
            for l in range(L):
                if flags[l]:
                    psdr_assert(np.isfinite(rows[l]).all(), "positions: an [L, 3] array of finite floats expected")
                    psdr_assert((rows[l] != 0).any(), "positions: the direction of distant light %d is all zero" % l)
            self.distant = flags

    def _lights(self, pos, d_pos=None, g_pos=None):
        """the lights every native call inside the block renders with (positions [L][3], their tangents in forward mode, their device gradient in reverse mode)"""
        return _light_scope(self, pos, d_pos, g_pos)

    def _image_floats(self, tb):
        return len(self._light_state[0]) * tb["width"] * tb["height"] * 3

    def _prepare(self, scene, tb, guide):
        lib, keep = Integrator._prepare(self, scene, tb, guide)
        psdr_assert(self._light_state is not None, "LightStageIntegrator: no lights in scope")
        pos, d_pos, g_pos = self._light_state
        L = len(pos)
        flat = [x for row in pos for x in row]
        dflat = None if d_pos is None else [x for row in d_pos for x in row]
        args = ((C.c_float * (3 * L))(*flat), 0 if d_pos is None else 1, None if d_pos is None else (C.c_float * (3 * L))(*dflat), None if g_pos is None else g_pos.data_ptr())
        if self.distant is None:
            _abi.check(lib, lib.psdr_scene_set_point_lights(scene._native, L, *args))
        else:
            psdr_assert(not (any(self.distant) and tb.get("env_emitter", -1) >= 0), _abi.DISTANT_IN_ENV)
            kinds = (C.c_int32 * L)(*[_abi.LIGHT_DISTANT if f else _abi.LIGHT_POINT for f in self.distant])
            _abi.check(lib, lib.psdr_scene_set_lights(scene._native, L, kinds, *args))
        if g_pos is not None:
            keep.append(g_pos)
        return lib, keep

    def _forget_lights(self, scene):
        """removes the lights from the scene's handle (with them the tangents and the gradient address of the last call); the next native call sets its own"""
        if scene._native is not None:
            lib = _abi.load_hip()
            _abi.check(lib, lib.psdr_scene_set_point_lights(scene._native, 0, None, 0, None, None))

    def _positions_now(self):
        return [[float(x) for x in row] for row in self.m_positions.t.detach().reshape(-1, 3).cpu()]

    def renderC(self, scene, sensor_id=0):
        pos = self._positions_now()
        with self._lights(pos):
            img = Integrator.renderC(self, scene, sensor_id)          # unit intensities, [L W H, 3] (joins the image's all-reduce)
        L = len(pos)
        stack = img.t.reshape(L, -1, 3) * self.m_intensities.t.detach().reshape(L, 1, 3).to(img.t.device)
        return Vector3fC._wrap(stack.sum(dim=0) if self.combine else stack.reshape(-1, 3))

    def renderD(self, scene, sensor_id=0):
        self._check_bsdfs(scene)
        psdr_assert(scene.is_ready(), "Input scene must be configured!")
        psdr_assert(0 <= sensor_id < scene.num_sensors, "Invalid sensor id!")
        t0 = time.perf_counter()
        tb = scene.tables(sensor_id, capacity=True)
        opts = self._opts(scene, with_edges=True)
        if not (scene._sensor_tables[sensor_id]["num_prim_edges"] > 0):
            opts.sppe = opts.sppe_begin = opts.sppe_end = 0
        if not (tb.get("num_sec_edges", 0) > 0):
            opts.sppse = opts.sppse_begin = opts.sppse_end = 0
        img = _CollocatedImage._make(_LightStageNode(_RenderNode(self, scene, sensor_id, tb, opts, None), self.m_intensities, self.m_positions, self.combine))
        self._advance_rng(scene, opts)
        ek.register_render_node(img)
        if scene.opts.log_level:
            img.t                                        # (the log line reports the render's time)
            torch.cuda.synchronize()
            self.log("Rendered in %g seconds." % (time.perf_counter() - t0))
        return img
