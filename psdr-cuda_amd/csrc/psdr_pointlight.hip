// psdr_pointlight.hip -- the kernels of the PointLightIntegrator (PSDR_INTEGRATOR_POINT, psdr_pointlight.h) for the scene flag set PSDR_VARIANT_FLAGS, and their
// launches.  A translation unit of its own, compiled once per flag set like psdr_collocated.hip and for the same reason: new kernels
// inside psdr_kernels.h change the code of the existing ones.  The C ABI picks point_light_ops_<flags>() for this integrator BEFORE the variant's own dispatch
// (psdr_hip.hip), so no other integrator kind comes here and this kind never reaches psdr_variant.hip or psdr_collocated.hip.
// Shared with the other kernels: primary_ray, closest_hit / intersect (every scene form), the film-sample and splat machinery of k_camera (wave_segmented_sum,
// the plain-store path of a wave that owns its pixels), wave_run_sum, Bsdf / BsdfRev, DeviceSink, PrimaryEdgeSink, begin_edge_term and the pixel-sorted slot
// order of the primary-edge launches.  The light travels as a kernel argument (PointLight: position + tangents), its gradient leaves through one atomic per
// wave and component (wave_total first).  Every kernel has the light model as its last template parameter (LK: PSDR_LIGHT_POINT / PSDR_LIGHT_DISTANT,
// psdr_pointlight.h); the host picks the family per launch from the light's kind (PSDR_BY_KIND).
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
#include "psdr_pointlight.h"

#ifndef PSDR_VARIANT_FLAGS
#error "compile with -DPSDR_VARIANT_FLAGS=0|1|2|3|4|6|8|10"
#endif
#define PSDR_CAT2(a, b) a##b
#define PSDR_CAT(a, b) PSDR_CAT2(a, b)

namespace {

// Resident waves per SIMD (workgroups of kBlock = 256 lanes per CU), chosen from the compiler's resource report of THESE kernels
// (profiles/pointlight_resources.txt: -Rpass-analysis=kernel-resource-usage).  No instance spills a VGPR at its bound: where the collocated kernel's
// count would spill here (the shadow ray keeps the BSDF value and the hit alive across a second walk), the count is lower.
// `rough`: the flag sets that carry the GGX code (RoughConductor, MicrofacetBSDF with wo != wi); the others evaluate a Lambertian only.
template <class G, class R, int FL> constexpr int point_camera_waves() {
    constexpr bool rough = (FL & kSceneRough) != 0;
    if (!is_ad<R>()) return rough ? 5 : 8;                                 // renderC
    constexpr int K = ad_traits<R>::K;
    if (!is_ad<G>()) return K == 1 ? (rough ? 4 : 6) : (rough ? 2 : 4);   // material duals
    return K == 1 ? (rough ? 3 : 4) : 2;                                  // geometry duals
}
template <int FL, bool GEO> constexpr int point_rev_waves() {
    constexpr bool rough = (FL & kSceneRough) != 0;
    return GEO ? 2 : (rough ? 3 : 5);
}
template <int K, int FL> constexpr int point_edge_waves() { return ((FL & kSceneRough) != 0) ? 3 : 4; }       // K = 0: the reverse kernel
// K = 0: the reverse kernel.  K = 3 at four waves (128 VGPRs) spills one VGPR on the two-level Lambertian set: three.  The distant family
// (profiles/distantlight_resources.txt) fits every bound of the point family but one: K = 1 on the plain sets 0 and 1 spills one VGPR at four waves: three
template <int K, int FL, int LK> constexpr int point_sedge_waves() {
    if (LK == PSDR_LIGHT_DISTANT && K == 1 && (FL & ~kSceneEnv) == 0) return 3;
    return ((FL & kSceneRough) != 0 || K == 3) ? 3 : 4;
}

__device__ __forceinline__ void add_light_grad(float *g_pos, const Vec3f &a) {
    // every lane of the wave arrives here: the wave's total, then one atomic per component
    const float x = wave_total(a.x), y = wave_total(a.y), z = wave_total(a.z);
    if ((threadIdx.x & 63) == 0 && g_pos != nullptr) {
        if (x != 0.f && isfinite(x)) atomicAdd(g_pos, x);
        if (y != 0.f && isfinite(y)) atomicAdd(g_pos + 1, y);
        if (z != 0.f && isfinite(z)) atomicAdd(g_pos + 2, z);
    }
}

// ---------------------------------------------------------------------- camera kernel (k_colloc_camera with this estimator)
template <class G, class R, int FL, int LK>
__global__ __launch_bounds__(kBlock, (point_camera_waves<G, R, FL>())) void k_point_camera(LaunchCtx cx, TV<R, FL> tv, PointLight pl, int spp, int s_begin, SlotDiv nsp, long long n, float inv_spp,
                                                                                        float *__restrict__ img, float *__restrict__ dimg, long long plane,
                                                                                        unsigned long long *counters, int own) {
    constexpr int K = ad_traits<R>::K;
    constexpr int NV = 3 * (1 + K);
    TraversalStack st; setup_lds(cx, st, tv);
    uint32_t nrays = 0;
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        const bool in = j < n;
        int pixel = 0x7fffffff, s_in = 0;
        if (in) slot_to_pixel(j, nsp, pixel, s_in);
        float v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = 0.f;
        if (in) {
            const uint64_t slot = (uint64_t) pixel * (uint64_t) spp + (uint64_t) (s_begin + s_in);
            const Vec3<R> r = point_camera_sample<G, R, LK>(cx.sc, tv, st, pl, cx.jump, pixel, slot, nrays);
            v[0] = val(r.x) * inv_spp; v[1] = val(r.y) * inv_spp; v[2] = val(r.z) * inv_spp;
#pragma unroll
            for (int k = 0; k < K; ++k) { v[3 + 3 * k] = tangent(r.x, k) * inv_spp; v[4 + 3 * k] = tangent(r.y, k) * inv_spp; v[5 + 3 * k] = tangent(r.z, k) * inv_spp; }
        }
        const bool head = wave_segmented_sum<NV>(pixel, v);
        if (head && in) {
            float *p = img + (size_t) pixel * 3;
            if (own) {
                // every sample of the pixel sits in this wave (run_camera's rule): plain stores
                p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
#pragma unroll
                for (int k = 0; k < K; ++k) { float *q = dimg + (size_t) k * plane + (size_t) pixel * 3; q[0] = v[3 + 3 * k]; q[1] = v[4 + 3 * k]; q[2] = v[5 + 3 * k]; }
            } else {
                if (v[0] != 0.f) atomicAdd(p, v[0]);
                if (v[1] != 0.f) atomicAdd(p + 1, v[1]);
                if (v[2] != 0.f) atomicAdd(p + 2, v[2]);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float *q = dimg + (size_t) k * plane + (size_t) pixel * 3;
                    if (v[3 + 3 * k] != 0.f) atomicAdd(q, v[3 + 3 * k]);
                    if (v[4 + 3 * k] != 0.f) atomicAdd(q + 1, v[4 + 3 * k]);
                    if (v[5 + 3 * k] != 0.f) atomicAdd(q + 2, v[5 + 3 * k]);
                }
            }
        }
    }
    count_rays(counters, nrays);
}

// ---------------------------------------------------------------------- reverse camera kernel
template <int FL, bool GEO, int LK>
__global__ __launch_bounds__(kBlock, (point_rev_waves<FL, GEO>())) void k_point_camera_rev(LaunchCtx cx, DeviceSink<FL> sink, PointLight pl, float *g_pos, int spp, int s_begin, SlotDiv nsp, long long n,
                                                                                        float inv_spp, const float *__restrict__ adj_img, float *__restrict__ img, unsigned long long *counters) {
    TraversalStack st; setup_lds(cx, st);
    sink.begin(dyn_lds_floats(cx.off_sink));
    uint32_t nrays = 0;
    Vec3f a_pl(0.f);
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        const bool in = j < n;
        int pixel = 0x7fffffff, s_in = 0;
        if (in) slot_to_pixel(j, nsp, pixel, s_in);
        float v[3] = {0.f, 0.f, 0.f};
        PrimaryGrad pg; pg.clear();
        if (in) {
            const uint64_t slot = (uint64_t) pixel * (uint64_t) spp + (uint64_t) (s_begin + s_in);
            const float *a = adj_img + (size_t) pixel * 3;
            const Vec3f r = point_sample_reverse<GEO, LK>(sink, pg, cx.sc, st, pl, cx.jump, pixel, slot, Vec3f{a[0] * inv_spp, a[1] * inv_spp, a[2] * inv_spp}, nrays, a_pl);
            v[0] = r.x * inv_spp; v[1] = r.y * inv_spp; v[2] = r.z * inv_spp;
        }
        // primary-triangle row: one add per run of lanes that hit the same triangle
        if (GEO && sink.g.g_tri_info != nullptr) {
            const bool head = wave_run_sum<kPrimaryWords, (FL & kSceneRough) == 0 || PSDR_DPP_ALWAYS>(pg.tri, pg.w);
            if (head && pg.tri >= 0) {
#pragma unroll
                for (int w = 0; w < kPrimaryWords; ++w) sink.add_tri(pg.tri, w, pg.w[w]);
            }
        }
        if (img != nullptr) {
            const bool head = wave_segmented_sum<3>(pixel, v);
            if (head && in) {
                float *p = img + (size_t) pixel * 3;
                if (v[0] != 0.f) atomicAdd(p, v[0]);
                if (v[1] != 0.f) atomicAdd(p + 1, v[1]);
                if (v[2] != 0.f) atomicAdd(p + 2, v[2]);
            }
        }
    }
    if (GEO) add_light_grad(g_pos, a_pl);
    sink.end();
    count_rays(counters, nrays);
}

// ---------------------------------------------------------------------- primary-edge kernels (k_colloc_edge / k_colloc_edge_rev with this Li)
template <int K, int FL, int LK>
__global__ __launch_bounds__(kBlock, (point_edge_waves<K, FL>())) void k_point_edge(LaunchCtx cx, TangentView<K, FL> tv, PointLight pl, long long i0, long long n, float inv_sppe,
                                                                              float *__restrict__ dimg, long long plane, unsigned long long *counters, const uint32_t *__restrict__ order) {
    TraversalStack st; setup_lds(cx, st);
    uint32_t nrays = 0;
    const PointLiOf<LK> li{pl};
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        float tan[K][3];
        int pixel = -1;
        if (j < n) {
            const long long jj = order ? (long long) order[j] : j;          // pixel-sorted evaluation order (psdr_hip.hip)
            pixel = collocated_edge_sample<K, FL>(cx.sc, tv, st, cx.jump, (uint64_t) (i0 + jj), inv_sppe, tan, nrays, li);
        }
        float v[3 * K];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * k + c] = pixel >= 0 ? tan[k][c] : 0.f;
        const bool head = wave_run_sum<3 * K>(pixel, v);          // one atomic per run of equal pixels
        if (head && pixel >= 0) {
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (v[3 * k + c] != 0.f) atomicAdd(dimg + (size_t) k * plane + (size_t) pixel * 3 + c, v[3 * k + c]);
        }
    }
    count_rays(counters, nrays);
}
template <int FL, int LK>
__global__ __launch_bounds__(kBlock, (point_edge_waves<0, FL>())) void k_point_edge_rev(LaunchCtx cx, PrimaryEdgeSink<FL> sink, PointLight pl, long long i0, long long n, float inv_sppe,
                                                                                  const float *__restrict__ adj_img, unsigned long long *counters, const uint32_t *__restrict__ order) {
    TraversalStack st; setup_lds(cx, st);
    uint32_t nrays = 0;
    const PointLiOf<LK> li{pl};
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        int edge = -1;
        if (j < n) edge = collocated_edge_reverse_values<FL>(cx.sc, st, cx.jump, (uint64_t) (i0 + (order ? (long long) order[j] : j)), inv_sppe, adj_img, nrays, w, li);
        const bool head = wave_run_sum<4>(edge, w);               // one atomic per run of equal edges
        if (head && edge >= 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sink.add_pedge(edge, i, w[i]);
        }
    }
    count_rays(counters, nrays);
}

// ---------------------------------------------------------------------- shadow-boundary kernels (slots of sampler 2)
template <int K, int FL, int LK>
__global__ __launch_bounds__(kBlock, (point_sedge_waves<K, FL, LK>())) void k_point_sedge(LaunchCtx cx, TangentView<K, FL> tv, PointLight pl, long long i0, long long n, float inv_sppse,
                                                                                float *__restrict__ dimg, long long plane, unsigned long long *counters) {
    TraversalStack st; setup_lds(cx, st);
    uint32_t nrays = 0;
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        float tan[K][3];
        int pixel = -1;
        if (j < n) {
            Rng rng; rng.init((uint64_t) (i0 + j), cx.jump);
            const float s3[3] = {rng.next(), rng.next(), rng.next()};
            pixel = point_sedge_sample<K, FL, LK>(cx.sc, tv, st, pl, s3, inv_sppse, tan, nrays);
        }
        float v[3 * K];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * k + c] = pixel >= 0 ? tan[k][c] : 0.f;
        const bool head = wave_run_sum<3 * K>(pixel, v);          // one atomic per run of equal pixels
        if (head && pixel >= 0) {
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (v[3 * k + c] != 0.f) atomicAdd(dimg + (size_t) k * plane + (size_t) pixel * 3 + c, v[3 * k + c]);
        }
    }
    count_rays(counters, nrays);
}
template <int FL, int LK>
__global__ __launch_bounds__(kBlock, (point_sedge_waves<0, FL, LK>())) void k_point_sedge_rev(LaunchCtx cx, DeviceSink<FL> sink, PointLight pl, float *g_pos, long long i0, long long n, float inv_sppse,
                                                                                    const float *__restrict__ adj_img, unsigned long long *counters) {
    TraversalStack st; setup_lds(cx, st);
    sink.begin(dyn_lds_floats(cx.off_sink));
    uint32_t nrays = 0;
    Vec3f a_pl(0.f);
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < n; j += (long long) gridDim.x * kBlock) {
        Rng rng; rng.init((uint64_t) (i0 + j), cx.jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        point_sedge_reverse<LK>(sink, cx.sc, st, pl, s3, inv_sppse, adj_img, nrays, a_pl);
    }
    add_light_grad(g_pos, a_pl);
    sink.end();
    count_rays(counters, nrays);
}

// ============================================================================ launches
// one statement for the light's kind: LK is the model inside it
#define PSDR_BY_KIND(kind, ...)                                                                                    \
    do { if ((kind) == PSDR_LIGHT_DISTANT) { constexpr int LK = PSDR_LIGHT_DISTANT; __VA_ARGS__; }                 \
         else { constexpr int LK = PSDR_LIGHT_POINT; __VA_ARGS__; } } while (0)
PointLight light_of(const psdr_scene_s *h, int K) {
    PointLight pl{};
    for (int c = 0; c < 3; ++c) pl.p[c] = h->point_pos[c];
    for (int k = 0; k < K && k < h->point_K; ++k)
        for (int c = 0; c < 3; ++c) pl.d[k][c] = h->point_dpos[k][c];
    return pl;
}
bool light_moves(const psdr_scene_s *h, int K) {
    for (int k = 0; k < K && k < h->point_K; ++k)
        for (int c = 0; c < 3; ++c) if (h->point_dpos[k][c] != 0.f) return true;
    return false;
}

template <class G, class R, int FL>
int point_run_camera(psdr_scene_s *h, const psdr_render_opts *o, const TV<R, FL> &tv, int kind, const PointLight &pl, float *img, float *dimg, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp <= 0 || nsp <= 0) return 0;
    LaunchCtx cx;
    if (int rc = make_ctx(h, o, 0, cx)) return rc;
    const long long n = WH * nsp;
    h->slots[0] += (uint64_t) n;
    const int own = wave_owns_pixels(h, nsp, n);
    PSDR_BY_KIND(kind, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_camera<G, R, FL, LK>), dim3(launch_blocks(h, n, camera_blocks_per_cu(h, n))), dim3(kBlock), lds_bytes(cx, h), s, cx, tv, pl, o->spp,
                                          o->spp_begin, SlotDiv(nsp), n, 1.f / (float) o->spp, img, dimg, WH * 3, h->d_counters, own));
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int FL>
int point_render_c(psdr_scene_s *h, const psdr_render_opts *o, float *out_img, hipStream_t s) {
    const TangentView<0, FL> tv0{};
    return point_run_camera<float, float, FL>(h, o, tv0, h->point_kind, light_of(h, 0), out_img, nullptr, s);
}

// The two edge terms of forward mode for one light: primary edges and the shadow boundary, added into dimg (K planes, `plane` floats apart)
template <int K, int FL>
int point_edges_fwd_k(psdr_scene_s *h, const psdr_render_opts *o, const TangentView<K, FL> &tv, int kind, const PointLight &pl, float *dimg, long long plane, hipStream_t s) {
    if (o->sppe > 0 && o->sppe_end > o->sppe_begin && h->desc.num_prim_edges > 0) {
        EdgeLaunch e;
        if (int rc = begin_edge_term(h, o, 1, e, s)) return rc;
        PSDR_BY_KIND(kind, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_edge<K, FL, LK>), dim3(launch_blocks(h, e.n)), dim3(kBlock), lds_bytes(e.cx, h), s, e.cx, tv, pl, e.i0, e.n, 1.f / (float) o->sppe,
                                              dimg, plane, h->d_counters, e.order));
        HIP_TRY(hipGetLastError());
    }
    if (o->sppse > 0 && o->sppse_end > o->sppse_begin && h->desc.num_sec_edges > 0) {
        EdgeLaunch e;
        if (int rc = begin_edge_term(h, o, 2, e, s)) return rc;
        PSDR_BY_KIND(kind, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_sedge<K, FL, LK>), dim3(launch_blocks(h, e.n)), dim3(kBlock), lds_bytes(e.cx, h), s, e.cx, tv, pl, e.i0, e.n, 1.f / (float) o->sppse,
                                              dimg, plane, h->d_counters));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

template <int K, int FL>
int point_render_fwd_k(psdr_scene_s *h, const psdr_render_opts *o, const psdr_tangents *tangents, float *img, float *dimg, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    TangentView<K, FL> tv;
    for (int k = 0; k < K; ++k) tv.t[k] = tangents[k];
    const PointLight pl = light_of(h, K);
    HIP_TRY(hipMemsetAsync(img, 0, sizeof(float) * WH * 3, s));
    HIP_TRY(hipMemsetAsync(dimg, 0, sizeof(float) * WH * 3 * K, s));
    if (tangents_move_geometry(tangents, K) || light_moves(h, K)) { if (int rc = point_run_camera<Dual<K>, Dual<K>, FL>(h, o, tv, h->point_kind, pl, img, dimg, s)) return rc; }
    else { if (int rc = point_run_camera<float, Dual<K>, FL>(h, o, tv, h->point_kind, pl, img, dimg, s)) return rc; }
    return point_edges_fwd_k<K, FL>(h, o, tv, h->point_kind, pl, dimg, WH * 3, s);
}
template <int FL>
int point_render_fwd(psdr_scene_s *h, const psdr_render_opts *o, int K, const psdr_tangents *tangents, float *img, float *dimg, hipStream_t s) {
    switch (K) {
        case 1: return point_render_fwd_k<1, FL>(h, o, tangents, img, dimg, s);
        case 3: return point_render_fwd_k<3, FL>(h, o, tangents, img, dimg, s);
        default: return fail("psdr_render_d_fwd: K must be 1 or 3");
    }
}

// The two edge terms of reverse mode for one light (gradient of its position: g_pos, +=, or null)
template <int FL>
int point_edges_rev(psdr_scene_s *h, const psdr_render_opts *o, const float *adj_img, const psdr_grads *grads, DeviceSink<FL> &sink, int kind, const PointLight &pl, float *g_pos, hipStream_t s) {
    if (o->sppe > 0 && o->sppe_end > o->sppe_begin && h->desc.num_prim_edges > 0 && grads->g_prim_edge) {
        EdgeLaunch e;
        if (int rc = begin_edge_term(h, o, 1, e, s)) return rc;
        PrimaryEdgeSink<FL> pe_sink;
        if (int rc = begin_pe_replicas(h, grads, e, pe_sink, s)) return rc;
        PSDR_BY_KIND(kind, hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_edge_rev<FL, LK>), dim3(launch_blocks(h, e.n, big_launch_per_cu(h, e.n))), dim3(kBlock), lds_bytes(e.cx, h), s, e.cx, pe_sink, pl, e.i0, e.n,
                                              1.f / (float) o->sppe, adj_img, h->d_counters, e.order));
        HIP_TRY(hipGetLastError());
        if (int rc = end_pe_replicas(h, grads, pe_sink, s)) return rc;
    }
    if (o->sppse > 0 && o->sppse_end > o->sppse_begin && h->desc.num_sec_edges > 0 && (grads->g_sec_edge != nullptr || grads->g_tri_info != nullptr || g_pos != nullptr)) {
        EdgeLaunch e;
        if (int rc = begin_edge_term(h, o, 2, e, s)) return rc;
        int dyn_bytes = 0;
        if (int rc = plan_rev_one_vertex(h, e.cx, sink.L, &dyn_bytes)) return rc;
        PSDR_BY_KIND(kind, if (int rc = allow_dynamic_lds(&k_point_sedge_rev<FL, LK>, dyn_bytes)) return rc;
                     hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_sedge_rev<FL, LK>), dim3(launch_blocks(h, e.n)), dim3(kBlock), dyn_bytes, s, e.cx, sink, pl, g_pos, e.i0, e.n, 1.f / (float) o->sppse, adj_img,
                                        h->d_counters));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

template <int FL>
int point_render_rev(psdr_scene_s *h, const psdr_render_opts *o, const float *adj_img, float *out_img, const psdr_grads *grads, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    if (out_img) HIP_TRY(hipMemsetAsync(out_img, 0, sizeof(float) * WH * 3, s));
    DeviceSink<FL> sink{};
    if (int rc = make_device_sink(h, grads, sink)) return rc;
    const PointLight pl = light_of(h, 0);
    float *g_pos = h->point_gpos;
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp > 0 && nsp > 0) {
        LaunchCtx cx;
        if (int rc = make_ctx(h, o, 0, cx)) return rc;
        const long long n = WH * nsp;
        h->slots[0] += (uint64_t) n;
        const bool geo = grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr || g_pos != nullptr;
        int dyn_bytes = 0;          // no light samples: no private emitter rows; one vertex per slot: nothing deferred
        if (int rc = plan_rev_one_vertex(h, cx, sink.L, &dyn_bytes)) return rc;
        rev_layout_of_sink(h, sink.L, false);
        h->rev_layout[8] = kRevFused;
#define PSDR_LAUNCH_POINT_REV(GEO)                                                                                                                                       \
        PSDR_BY_KIND(h->point_kind, if (int rc = allow_dynamic_lds(&k_point_camera_rev<FL, GEO, LK>, dyn_bytes)) return rc;                                               \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_camera_rev<FL, GEO, LK>), dim3(launch_blocks(h, n)), dim3(kBlock), dyn_bytes, s, cx, sink, pl, g_pos, o->spp, o->spp_begin, SlotDiv(nsp), n,   \
                           1.f / (float) o->spp, adj_img, out_img, h->d_counters))
        if (geo) PSDR_LAUNCH_POINT_REV(true); else PSDR_LAUNCH_POINT_REV(false);
#undef PSDR_LAUNCH_POINT_REV
        HIP_TRY(hipGetLastError());
    }
    return point_edges_rev<FL>(h, o, adj_img, grads, sink, h->point_kind, pl, g_pos, s);
}

// The edge terms for a light given by value, as the LightStageIntegrator (psdr_lightstage.hip) launches them once per light of its stack:
// pos [3], d_pos [K][3] or null; dimg: the light's first derivative plane, `plane` floats to the next tangent's
template <int FL>
int point_edges_fwd_of(psdr_scene_s *h, const psdr_render_opts *o, int K, const psdr_tangents *tangents, int kind, const float *pos, const float *d_pos, float *dimg, long long plane, hipStream_t s) {
    PointLight pl{};
    for (int c = 0; c < 3; ++c) pl.p[c] = pos[c];
    for (int k = 0; k < K && d_pos; ++k) for (int c = 0; c < 3; ++c) pl.d[k][c] = d_pos[3 * k + c];
    if (K == 1) { TangentView<1, FL> tv; tv.t[0] = tangents[0]; return point_edges_fwd_k<1, FL>(h, o, tv, kind, pl, dimg, plane, s); }
    TangentView<3, FL> tv;
    for (int k = 0; k < 3; ++k) tv.t[k] = tangents[k];
    return point_edges_fwd_k<3, FL>(h, o, tv, kind, pl, dimg, plane, s);
}
template <int FL>
int point_edges_rev_of(psdr_scene_s *h, const psdr_render_opts *o, const float *adj_img, const psdr_grads *grads, int kind, const float *pos, float *g_pos, hipStream_t s) {
    PointLight pl{};
    for (int c = 0; c < 3; ++c) pl.p[c] = pos[c];
    DeviceSink<FL> sink{};
    if (int rc = make_device_sink(h, grads, sink)) return rc;
    return point_edges_rev<FL>(h, o, adj_img, grads, sink, kind, pl, g_pos, s);
}
#undef PSDR_BY_KIND
}  // namespace

namespace psdr_host {
const PointLightOps *PSDR_CAT(point_light_ops_, PSDR_VARIANT_FLAGS)() {
    constexpr int FL = PSDR_VARIANT_FLAGS;
    static const PointLightOps ops{&point_render_c<FL>, &point_render_fwd<FL>, &point_render_rev<FL>, &point_edges_fwd_of<FL>, &point_edges_rev_of<FL>};
    return &ops;
}
}  // namespace psdr_host
