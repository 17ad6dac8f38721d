// psdr_path_sedge.hip -- the kernels of the PathTracer's secondary-edge term (PSDR_FLAG_PATH_SEDGES, psdr_path_sedge.h) for the scene flag set
// PSDR_VARIANT_FLAGS, and their launches.  A translation unit of its own, compiled once per flag set like psdr_variant.hip: with the kernels inside
// psdr_kernels.h the units of psdr_variant.hip compiled their EXISTING kernels to other code (flag set 3 then tripped the build's spill guard in
// k_camera<Dual<3>, Dual<3>>, which this term never runs); kept apart, those units compile the device code they always did.  The C ABI calls
// path_sedge_ops_<flags>() after the variant's own render_fwd / render_rev (psdr_hip.hip).
#ifndef PSDR_WIDE_TREE
#if PSDR_VARIANT_FLAGS == 6
#define PSDR_WIDE_TREE 1
#else
#define PSDR_WIDE_TREE 0
#endif
#endif
#ifndef PSDR_LEAF_PAIR
#if PSDR_VARIANT_FLAGS == 6
#define PSDR_LEAF_PAIR 1
#else
#define PSDR_LEAF_PAIR 0
#endif
#endif
#include "psdr_kernels.h"
#include "psdr_path_sedge.h"

#ifndef PSDR_VARIANT_FLAGS
#error "compile with -DPSDR_VARIANT_FLAGS=0|1|2|3|4|6|8|10"
#endif
#define PSDR_CAT2(a, b) a##b
#define PSDR_CAT(a, b) PSDR_CAT2(a, b)

namespace {

// ---------------------------------------------------------------------- k_path_sedge
// The secondary-edge term of the PathTracer (PSDR_FLAG_PATH_SEDGES, psdr_path_sedge.h).  A slot evaluates two boundary segments; either is over after its
// first two rays for most slots, and a survivor then runs up to d-1 walk bounces (and, segment B, up to d-1 source bounces).  Split launch: per segment a
// filter over all slots (k_secondary_edge_filter for segment A: the very predicate of DirectIntegrator's term; k_path_sedge_filter for segment B), then this
// kernel over the compacted survivor list with po.seg naming the one segment the list belongs to.  Small launches run it once over all slots, both segments.
// Guided slots (psdr_path_sedge.h): segment A's grid is the descriptor's, which k_secondary_edge_filter warps by already; segment B's arrives as an argument of
// k_path_sedge_filter_g and in PathSedgeArgs<true> of the survivor kernels, which repeat the warp.  A launch with either grid runs the G = true instances; the
// G = false ones are the unguided kernels, compiled without the branch.
template <int FL, class Keep>
__device__ __forceinline__ void path_sedge_filter_loop(const LaunchCtx &cx, long long n, uint32_t *__restrict__ list, int *__restrict__ list_n, unsigned long long *counters, Keep &&keep_slot) {
    TraversalStack st; setup_lds(cx, st);
    uint32_t nrays = 0;
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    const int lane = threadIdx.x & 63;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        bool keep = false;
        if (j < n) keep = keep_slot(st, j, nrays);
        // (one atomic per wave and trip -- not the per-wave LDS buffer of k_secondary_edge_filter: 6-9 % of the slots pass this predicate, nearly every wave appends)
        const unsigned long long mask = __ballot(keep);
        if (mask != 0ull) {
            int base = 0;
            if (lane == 0) base = atomicAdd(list_n, (int) __popcll(mask));
            base = __shfl(base, 0, 64);
            if (keep) list[base + (int) __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t) j;          // base + rank < n: a slot appends at most once
        }
    }
    count_rays(counters, nrays);
}
template <int FL>
__global__ __launch_bounds__(kBlock, 4) void k_path_sedge_filter(LaunchCtx cx, long long i0, long long n, uint32_t *__restrict__ list, int *__restrict__ list_n, unsigned long long *counters) {
    path_sedge_filter_loop<FL>(cx, n, list, list_n, counters, [&](TraversalStack &st, long long j, uint32_t &nrays) {
        Rng rng; rng.init((uint64_t) (i0 + j), cx.jump);
        const float s0 = rng.next();
        (void) rng.next(); (void) rng.next();
        return path_sedge_survives_b<FL>(cx.sc, st, rng, s0, nrays);
    });
}
// ... of a launch with a grid on segment B: the warp of path_sedge_slot
template <int FL>
__global__ __launch_bounds__(kBlock, 4) void k_path_sedge_filter_g(LaunchCtx cx, long long i0, long long n, uint32_t *__restrict__ list, int *__restrict__ list_n, unsigned long long *counters,
                                                                    PathGuide gb) {
    path_sedge_filter_loop<FL>(cx, n, list, list_n, counters, [&](TraversalStack &st, long long j, uint32_t &nrays) {
        Rng rng; rng.init((uint64_t) (i0 + j), cx.jump);
        const float s0 = rng.next();
        (void) rng.next(); (void) rng.next();
        return path_sedge_survives_b<FL>(cx.sc, st, rng, s0, nrays, &gb);
    });
}

// ---------------------------------------------------------------------- guiding-grid build (psdr_path_guide_build)
// Slot j = (round r = j / gg.n, stream l = j % gg.n) of the gg.n = cells x per streams, as guide_launch numbers them.  STREAM LAYOUT of one evaluation:
//   stream l,        draws 3 r .. 3 r + 2   the cell sample, stratified into cell l / per (guide_slot_sample): s3 of segment A, (s3[0], u, v) of segment B
//   stream gg.n + j, draws 0 ..             every other number, laid out as a render slot's stream after s3: 2 skipped (the direction numbers) | 3 (d-1) walk
//                                           numbers of A | 3 (d-2) of B | 5 (d-1) source-bounce numbers
// Streams [0, gg.n) hold cell samples only and streams [gg.n, gg.n + gg.n * nrounds) the rest: disjoint.  tests/hostcheck/hostcheck_path_guide.cpp mirrors this.
// mass[cell] += path_sedge_mass * gg.scale, gg.scale = 1 / (per * nrounds).  Small builds: this kernel over all slots; large ones: a filter (segment A:
// k_secondary_edge_filter with the GuideGrid, segment B: k_path_guide_filter_b) and this kernel over the survivor list.
template <int FL>
__global__ __launch_bounds__(kBlock, 4) void k_path_guide_filter_b(LaunchCtx cx, GuideGrid gg, long long n, uint32_t *__restrict__ list, int *__restrict__ list_n, unsigned long long *counters) {
    path_sedge_filter_loop<FL>(cx, n, list, list_n, counters, [&](TraversalStack &st, long long j, uint32_t &nrays) {
        float c3[3]; int cell;
        guide_slot_sample(gg, j, c3, cell);
        return path_sedge_survives_b_at<FL>(cx.sc, st, c3[0], c3[1], c3[2], nrays);
    });
}

template <int FL>
__global__ __launch_bounds__(kBlock) void k_path_guide(LaunchCtx cx, GuideGrid gg, long long n, PathSedgeOpts po, float *__restrict__ mass, unsigned long long *counters,
                                                       const uint32_t *__restrict__ list, const int *__restrict__ list_n) {
    TraversalStack st; setup_lds(cx, st);
    uint32_t nrays = 0;
    const RngJump nojump{1ull, 0ull};
    if (list != nullptr) n = *list_n;
    for (long long jj = (long long) blockIdx.x * kBlock + threadIdx.x; jj < n; jj += (long long) gridDim.x * kBlock) {
        const long long j = list != nullptr ? (long long) list[jj] : jj;
        float c3[3]; int cell;
        guide_slot_sample(gg, j, c3, cell);          // cell < r0 r1 r2 = the length of mass: l < gg.n = cells * per
        Rng rest; rest.init((uint64_t) gg.n + (uint64_t) j, nojump);
        const float a = path_sedge_mass<FL>(cx.sc, st, rest, c3, po, nrays, list == nullptr) * gg.scale;
        if (a != 0.f) atomicAdd(mass + cell, a);
    }
    count_rays(counters, nrays);
}

template <int K, int FL, bool G>
__global__ __launch_bounds__(kBlock) void k_path_sedge(LaunchCtx cx, TangentView<K, FL> tv, long long i0, long long n, float inv_sppse, float *__restrict__ dimg, long long plane,
                                                       unsigned long long *counters, const uint32_t *__restrict__ list, const int *__restrict__ list_n, PathSedgeArgs<G> pa) {
    using R = Dual<K>;
    TraversalStack st; setup_lds(cx, st);
    uint32_t nrays = 0;
    const PathSedgeOpts po = pa.opts();
    if (list != nullptr) n = *list_n;
    for (long long jj = (long long) blockIdx.x * kBlock + threadIdx.x; jj < n; jj += (long long) gridDim.x * kBlock) {
        const long long j = list != nullptr ? (long long) list[jj] : jj;
        Rng rng; rng.init((uint64_t) (i0 + j), cx.jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        path_secondary_edge_sample<R, G>(cx.sc, tv, st, rng, s3, po, nrays, list == nullptr, [&](int pixel, const Vec3<R> &value) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float g[3] = {value.x.d[k] * inv_sppse, value.y.d[k] * inv_sppse, value.z.d[k] * inv_sppse};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (g[c] != 0.f) atomicAdd(dimg + (size_t) k * plane + (size_t) pixel * 3 + c, g[c]);
            }
        });
    }
    count_rays(counters, nrays);
}

template <int FL, bool G>
__global__ __launch_bounds__(kBlock) void k_path_sedge_rev(LaunchCtx cx, DeviceSink<FL> sink, long long i0, long long n, float inv_sppse, const float *__restrict__ adj_img,
                                                           unsigned long long *counters, const uint32_t *__restrict__ list, const int *__restrict__ list_n, PathSedgeArgs<G> pa) {
    TraversalStack st; setup_lds(cx, st);
    sink.begin(dyn_lds_floats(cx.off_sink));
    uint32_t nrays = 0;
    const PathSedgeOpts po = pa.opts();
    if (list != nullptr) n = *list_n;
    for (long long jj = (long long) blockIdx.x * kBlock + threadIdx.x; jj < n; jj += (long long) gridDim.x * kBlock) {
        const long long j = list != nullptr ? (long long) list[jj] : jj;
        Rng rng; rng.init((uint64_t) (i0 + j), cx.jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        path_secondary_edge_reverse<G>(sink, cx.sc, st, rng, s3, po, inv_sppse, adj_img, nrays, list == nullptr);
    }
    sink.end();
    count_rays(counters, nrays);
}


// ---- launches of the PathTracer's secondary-edge term (PSDR_FLAG_PATH_SEDGES)
inline bool path_sedges_wanted(const psdr_scene_s *h, const psdr_render_opts *o) {
    return o->sppse > 0 && o->sppse_end > o->sppse_begin && h->desc.num_sec_edges > 0 && o->integrator == PSDR_INTEGRATOR_PATH && (o->flags & PSDR_FLAG_PATH_SEDGES) != 0;
}
inline PathGuide path_guide_of(const psdr_scene_s *h) {
    PathGuide g;
    g.cmf = h->pg_cmf; g.pmf = h->pg_pmf; g.sum = h->pg_sum;
    g.r0 = h->pg_reso[0]; g.r1 = h->pg_reso[1]; g.r2 = h->pg_reso[2]; g.n = g.r0 * g.r1 * g.r2;
    return g;
}
// filter pass of segment B: the survivor list shares the handle's block with segment A's (the passes of one call follow each other on the stream)
template <int FL>
int path_sedge_filter_b(psdr_scene_s *h, const LaunchCtx &cx, long long i0, long long n, const uint32_t **list, const int **list_n, hipStream_t s, const PathGuide &gb, const GuideGrid *gg = nullptr) {
    const size_t need = 256 + (size_t) n * sizeof(uint32_t);
    if (int rc = scratch_reserve(&h->d_se_list, &h->se_list_bytes, need, s, "secondary-edge survivor list")) return rc;
    int *cnt = reinterpret_cast<int *>(h->d_se_list);
    uint32_t *lst = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(h->d_se_list) + 256);
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(int), s));
    if (gg != nullptr) hipLaunchKernelGGL(k_path_guide_filter_b<FL>, dim3(launch_blocks(h, n)), dim3(kBlock), lds_bytes(cx, h), s, cx, *gg, n, lst, cnt, h->d_counters);
    else if (gb.cmf != nullptr) hipLaunchKernelGGL(k_path_sedge_filter_g<FL>, dim3(launch_blocks(h, n)), dim3(kBlock), lds_bytes(cx, h), s, cx, i0, n, lst, cnt, h->d_counters, gb);
    else hipLaunchKernelGGL(k_path_sedge_filter<FL>, dim3(launch_blocks(h, n)), dim3(kBlock), lds_bytes(cx, h), s, cx, i0, n, lst, cnt, h->d_counters);
    HIP_TRY(hipGetLastError());
    *list = lst; *list_n = cnt;
    return 0;
}
// launch(list, list_n, grid slots, po, guided) starts the evaluating kernel (forward or reverse; guided: its G = true instance); cxf: the context the filters stage the scene with
template <int FL, class Launch>
int path_sedge_passes(psdr_scene_s *h, const psdr_render_opts *o, const LaunchCtx &cxf, long long i0, long long n, hipStream_t s, Launch &&launch) {
    PathSedgeOpts po{o->max_depth, h->opt.pt_sedge & 3, h->opt.pt_sedge_walk};
    if (po.max_depth < 2) po.seg &= 1;
    if ((po.seg & 2) && h->pg_cmf != nullptr) po.gb = path_guide_of(h);          // (a segment that is switched off ignores its grid)
    const bool ga = (po.seg & 1) && h->desc.guide_cmf != nullptr && h->desc.num_guide_cells > 0, gb = po.gb.cmf != nullptr;
    if (!path_sedge_split(h, n)) {
        if (po.seg != 0) { launch(nullptr, nullptr, n, po, ga || gb); HIP_TRY(hipGetLastError()); }
        return 0;
    }
    if (po.seg & 1) {
        const uint32_t *list = nullptr; const int *list_n = nullptr;
        if (int rc = secondary_edge_filter<FL>(h, cxf, i0, n, &list, &list_n, s)) return rc;
        PathSedgeOpts pa = po; pa.seg = 1;
        launch(list, list_n, list ? filter_grid_slots(n, 16) : n, pa, ga);
        HIP_TRY(hipGetLastError());
    }
    if (po.seg & 2) {
        const uint32_t *list = nullptr; const int *list_n = nullptr;
        if (int rc = path_sedge_filter_b<FL>(h, cxf, i0, n, &list, &list_n, s, po.gb)) return rc;
        PathSedgeOpts pb = po; pb.seg = 2;
        launch(list, list_n, filter_grid_slots(n, 4), pb, gb);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

template <int K, int FL>
int path_sedge_fwd_k(psdr_scene_s *h, const psdr_render_opts *o, const psdr_tangents *tangents, float *dimg, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    TangentView<K, FL> tv;
    for (int k = 0; k < K; ++k) tv.t[k] = tangents[k];
    EdgeLaunch e;
    if (int rc = begin_edge_term(h, o, 2, e, s)) return rc;
    return path_sedge_passes<FL>(h, o, e.cx, e.i0, e.n, s, [&](const uint32_t *list, const int *list_n, long long grid_slots, const PathSedgeOpts &po, bool guided) {
        if (guided)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_sedge<K, FL, true>), dim3(launch_blocks(h, grid_slots)), dim3(kBlock), lds_bytes(e.cx, h), s, e.cx, tv, e.i0, e.n, 1.f / (float) o->sppse,
                               dimg, WH * 3, h->d_counters, list, list_n, PathSedgeArgs<true>{po.max_depth, po.seg, po.walk, po.gb});
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_sedge<K, FL, false>), dim3(launch_blocks(h, grid_slots)), dim3(kBlock), lds_bytes(e.cx, h), s, e.cx, tv, e.i0, e.n, 1.f / (float) o->sppse,
                               dimg, WH * 3, h->d_counters, list, list_n, PathSedgeArgs<false>{po.max_depth, po.seg, po.walk});
    });
}
// forward mode: adds the term to the K derivative images psdr_render_d_fwd has rendered (same stream)
template <int FL>
int path_sedge_fwd(psdr_scene_s *h, const psdr_render_opts *o, int K, const psdr_tangents *tangents, float *dimg, hipStream_t s) {
    if (!path_sedges_wanted(h, o)) return 0;
    return K == 1 ? path_sedge_fwd_k<1, FL>(h, o, tangents, dimg, s) : path_sedge_fwd_k<3, FL>(h, o, tangents, dimg, s);
}
// reverse mode: scatters the term's adjoints into the tables psdr_render_d_rev has filled (same stream, same gradient cache layout)
template <int FL>
int path_sedge_rev(psdr_scene_s *h, const psdr_render_opts *o, const float *adj_img, const psdr_grads *grads, hipStream_t s) {
    if (!path_sedges_wanted(h, o)) return 0;
    DeviceSink<FL> sink{};
    if (int rc = make_device_sink(h, grads, sink)) return rc;
    EdgeLaunch e;
    if (int rc = begin_edge_term(h, o, 2, e, s)) return rc;
    const LaunchCtx cxf = e.cx;                                 // the filters stage the scene like a forward kernel (no gradient cache in LDS)
    int dyn_bytes = 0;
    if (int rc = plan_rev_one_vertex(h, e.cx, sink.L, &dyn_bytes)) return rc;
    if (int rc = allow_dynamic_lds(&k_path_sedge_rev<FL, false>, dyn_bytes)) return rc;
    if (int rc = allow_dynamic_lds(&k_path_sedge_rev<FL, true>, dyn_bytes)) return rc;
    return path_sedge_passes<FL>(h, o, cxf, e.i0, e.n, s, [&](const uint32_t *list, const int *list_n, long long grid_slots, const PathSedgeOpts &po, bool guided) {
        if (guided)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_sedge_rev<FL, true>), dim3(launch_blocks(h, grid_slots)), dim3(kBlock), dyn_bytes, s, e.cx, sink, e.i0, e.n, 1.f / (float) o->sppse, adj_img,
                               h->d_counters, list, list_n, PathSedgeArgs<true>{po.max_depth, po.seg, po.walk, po.gb});
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_path_sedge_rev<FL, false>), dim3(launch_blocks(h, grid_slots)), dim3(kBlock), dyn_bytes, s, e.cx, sink, e.i0, e.n, 1.f / (float) o->sppse, adj_img,
                               h->d_counters, list, list_n, PathSedgeArgs<false>{po.max_depth, po.seg, po.walk});
    });
}

// the guiding-grid build of one segment (the C ABI has checked the arguments and zeroed out_mass); evaluated unguided
template <int FL>
int path_guide_build(psdr_scene_s *h, const psdr_render_opts *o, int segment, const int32_t reso[4], int nrounds, float *out_mass, hipStream_t s) {
    LaunchCtx cx;
    if (int rc = make_ctx(h, o, 2, cx)) return rc;
    cx.sc.d.guide_cmf = nullptr; cx.sc.d.num_guide_cells = 0;
    const long long n = (long long) reso[0] * reso[1] * reso[2] * reso[3], total = n * nrounds;
    const GuideGrid gg{reso[0], reso[1], reso[2], reso[3], (int) n, 1.f / ((float) reso[3] * (float) nrounds)};
    const PathSedgeOpts po{o->max_depth, segment, h->opt.pt_sedge_walk};
    const uint32_t *list = nullptr; const int *list_n = nullptr;
    long long grid_slots = total;
    if (path_sedge_split(h, total)) {
        if (segment == 1) {
            if (int rc = secondary_edge_filter<FL>(h, cx, 0, total, &list, &list_n, s, &gg)) return rc;
            grid_slots = filter_grid_slots(total, 16);
        } else {
            if (int rc = path_sedge_filter_b<FL>(h, cx, 0, total, &list, &list_n, s, PathGuide{}, &gg)) return rc;
            grid_slots = filter_grid_slots(total, 4);
        }
    }
    hipLaunchKernelGGL(k_path_guide<FL>, dim3(launch_blocks(h, grid_slots)), dim3(kBlock), lds_bytes(cx, h), s, cx, gg, total, po, out_mass, h->d_counters, list, list_n);
    HIP_TRY(hipGetLastError());
    return 0;
}
}  // namespace

namespace psdr_host {
const PathSedgeOps *PSDR_CAT(path_sedge_ops_, PSDR_VARIANT_FLAGS)() {
    constexpr int FL = PSDR_VARIANT_FLAGS;
    static const PathSedgeOps ops{&path_sedge_fwd<FL>, &path_sedge_rev<FL>, &path_guide_build<FL>};
    return &ops;
}
}  // namespace psdr_host
