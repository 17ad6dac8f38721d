// psdr_lightstage.hip -- the camera kernels of the LightStageIntegrator (PSDR_INTEGRATOR_POINT_STACK, psdr_lightstage.h) for the scene flag set
// PSDR_VARIANT_FLAGS, and the launches of the integrator.  A translation unit of its own, compiled once per flag set like psdr_pointlight.hip and for the same
// reason: the PointLightIntegrator's units keep their code.  One hit per sample slot, then a run-time, wave-uniform loop over the lights
// of the handle's device table (LightTable: read with a wave-uniform index); every light has its own wave_segmented_sum and its own plane of the output.
// The primary-edge and shadow-boundary terms are the PointLightIntegrator's kernels (PointLightOps::edges_fwd / edges_rev), launched once per light with the
// light's planes: the same rng_offset for every light, so every plane is the single-light launch's plane.
// Light models (psdr_pointlight.h): the camera kernels have a last template parameter MIXED.  false: every light of the stack is a point light -- the loop
// holds the point instantiation alone.  true: a light of the table is distant -- the loop branches, wave-uniformly, on the light's kind to one of the two
// instantiations; a stack may mix the kinds in any order.  The host picks per launch (upload_lights).
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
#include "psdr_lightstage.h"

#ifndef PSDR_VARIANT_FLAGS
#error "compile with -DPSDR_VARIANT_FLAGS=0|1|2|3|4|6|8|10"
#endif
#define PSDR_CAT2(a, b) a##b
#define PSDR_CAT(a, b) PSDR_CAT2(a, b)

namespace {

// Resident waves per SIMD, chosen from the compiler's resource report of THESE kernels (profiles/lightstage_resources.txt): no instance spills a VGPR or
// uses scratch at its bound.  The hit stays alive across the loop over the lights, so some counts are below k_point_camera's.
// MIXED (the loop branches on the light's kind, profiles/distantlight_resources.txt): the point-only instances keep every count; the mixed ones fit them
// all but two -- renderC on the two-level Lambertian set (8 VGPRs spilt at eight waves: seven) and the K = 3 material duals on the plain sets 0 and 1
// (one VGPR spilt at four waves: three).
template <class G, class R, int FL, bool MIXED> constexpr int stack_camera_waves() {
    constexpr bool rough = (FL & kSceneRough) != 0, forest = (FL & kSceneForest) != 0;
    if (!is_ad<R>()) return rough ? (forest ? 4 : 5) : ((MIXED && forest) ? 7 : 8);                  // renderC
    constexpr int K = ad_traits<R>::K;
    if (!is_ad<G>() && MIXED && K == 3 && (FL & ~kSceneEnv) == 0) return 3;
    if (!is_ad<G>()) return K == 1 ? (rough ? 3 : 6) : (rough ? 2 : 4);   // material duals
    return K == 1 ? (rough ? (forest ? 2 : 3) : 4) : (rough ? 1 : 2);     // geometry duals
}
template <int FL, bool GEO> constexpr int stack_rev_waves() {
    constexpr bool rough = (FL & kSceneRough) != 0;
    return GEO ? (rough ? 1 : 2) : (rough ? 3 : 5);
}

// ---------------------------------------------------------------------- camera kernel: img [L][plane], dimg [K][L][plane]
template <class G, class R, int FL, bool MIXED>
__global__ __launch_bounds__(kBlock, (stack_camera_waves<G, R, FL, MIXED>())) void k_stack_camera(LaunchCtx cx, TV<R, FL> tv, LightTable lt, int spp, int s_begin, SlotDiv nsp, long long n, float inv_spp,
                                                                                        float *__restrict__ img, float *__restrict__ dimg, long long plane,
                                                                                        unsigned long long *counters, int own) {
    constexpr int K = ad_traits<R>::K;
    constexpr int KG = K > 0 ? K : 1;
    constexpr int NV = 3 * (1 + K);
    TraversalStack st; setup_lds(cx, st, tv);
    uint32_t nrays = 0;
    const int L = lt.L;
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        const bool in = j < n;
        int pixel = 0x7fffffff, s_in = 0;
        if (in) slot_to_pixel(j, nsp, pixel, s_in);
        StackHit<G> hit;
        hit.ok = false; hit.bsdf_id = -1;
        if (in) hit = stack_camera_hit<G>(cx.sc, tv, st, cx.jump, pixel, (uint64_t) pixel * (uint64_t) spp + (uint64_t) (s_begin + s_in), nrays);
        const Bsdf<G, R> bsdf(cx.sc, tv, hit.ok ? hit.bsdf_id : 0);
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            float v[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = 0.f;
            if (hit.ok) {
                const PointLight pl = stack_light<KG>(lt, l);
                const Vec3<R> r = (MIXED && stack_light_distant(lt, l)) ? stack_light_value<G, R, kLightDistant>(cx.sc, tv, st, bsdf, hit.its, pl, nrays)
                                                                        : stack_light_value<G, R, kLightPoint>(cx.sc, tv, st, bsdf, hit.its, pl, nrays);
                v[0] = val(r.x) * inv_spp; v[1] = val(r.y) * inv_spp; v[2] = val(r.z) * inv_spp;
#pragma unroll
                for (int k = 0; k < K; ++k) { v[3 + 3 * k] = tangent(r.x, k) * inv_spp; v[4 + 3 * k] = tangent(r.y, k) * inv_spp; v[5 + 3 * k] = tangent(r.z, k) * inv_spp; }
            }
            const bool head = wave_segmented_sum<NV>(pixel, v);
            if (head && in) {
                float *p = img + (size_t) l * plane + (size_t) pixel * 3;
                if (own) {
                    // every sample of the pixel sits in this wave (run_camera's rule): plain stores
                    p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
#pragma unroll
                    for (int k = 0; k < K; ++k) { float *q = dimg + ((size_t) k * L + l) * plane + (size_t) pixel * 3; q[0] = v[3 + 3 * k]; q[1] = v[4 + 3 * k]; q[2] = v[5 + 3 * k]; }
                } else {
                    if (v[0] != 0.f) atomicAdd(p, v[0]);
                    if (v[1] != 0.f) atomicAdd(p + 1, v[1]);
                    if (v[2] != 0.f) atomicAdd(p + 2, v[2]);
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        float *q = dimg + ((size_t) k * L + l) * plane + (size_t) pixel * 3;
                        if (v[3 + 3 * k] != 0.f) atomicAdd(q, v[3 + 3 * k]);
                        if (v[4 + 3 * k] != 0.f) atomicAdd(q + 1, v[4 + 3 * k]);
                        if (v[5 + 3 * k] != 0.f) atomicAdd(q + 2, v[5 + 3 * k]);
                    }
                }
            }
        }
    }
    count_rays(counters, nrays);
}

// ---------------------------------------------------------------------- reverse camera kernel: adj_img [L][plane], img [L][plane] or null, g_pos [L][3] or null
// The lights' gradients: the wave's total per light and component (wave_total), added to a column of 3 L floats in LDS (off_gpos: behind the gradient
// cache); one global atomic per workgroup, light and component at the end.
template <int FL, bool GEO, bool MIXED>
__global__ __launch_bounds__(kBlock, (stack_rev_waves<FL, GEO>())) void k_stack_camera_rev(LaunchCtx cx, DeviceSink<FL> sink, LightTable lt, float *g_pos, int off_gpos, int spp, int s_begin, SlotDiv nsp,
                                                                                        long long n, float inv_spp, const float *__restrict__ adj_img, float *__restrict__ img, long long plane,
                                                                                        unsigned long long *counters) {
    using CamSink = typename CameraSinkOf<GEO, DeviceSink<FL>>::type;
    TraversalStack st; setup_lds(cx, st);
    sink.begin(dyn_lds_floats(cx.off_sink));
    const int L = lt.L;
    float *lds_gpos = dyn_lds_floats(off_gpos);
    const bool want_gpos = GEO && g_pos != nullptr;
    if (want_gpos) {
        for (int i = threadIdx.x; i < 3 * L; i += kBlock) lds_gpos[i] = 0.f;
        __syncthreads();
    }
    uint32_t nrays = 0;
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long j = (long long) blockIdx.x * kBlock + threadIdx.x; j < nceil; j += (long long) gridDim.x * kBlock) {
        const bool in = j < n;
        int pixel = 0x7fffffff, s_in = 0;
        if (in) slot_to_pixel(j, nsp, pixel, s_in);
        PrimaryGrad pg; pg.clear();
        StackRevHit H;
        H.ok = H.lit = false; H.bsdf_id = -1;
        if (in) stack_rev_begin<GEO, FL>(H, cx.sc, st, cx.jump, pixel, (uint64_t) pixel * (uint64_t) spp + (uint64_t) (s_begin + s_in), nrays);
        CamSink csink(sink, pg);
        const BsdfRev<CamSink> brev(cx.sc, H.ok ? H.bsdf_id : 0);
#pragma unroll 1
        for (int l = 0; l < L; ++l) {
            Vec3f r(0.f), a_pl(0.f);
            if (H.ok) {
                const float *a = adj_img + (size_t) l * plane + (size_t) pixel * 3;
                const PointLight pl = stack_light<1>(LightTable{lt.pos, nullptr, L, nullptr}, l);
                const Vec3f adj{a[0] * inv_spp, a[1] * inv_spp, a[2] * inv_spp};
                r = (MIXED && stack_light_distant(lt, l)) ? stack_rev_light<GEO, kLightDistant>(csink, pg, cx.sc, st, brev, H, pl, adj, nrays, a_pl)
                                                          : stack_rev_light<GEO, kLightPoint>(csink, pg, cx.sc, st, brev, H, pl, adj, nrays, a_pl);
            }
            if (want_gpos) {
                // every lane of the wave arrives here
                const float x = wave_total(a_pl.x), y = wave_total(a_pl.y), z = wave_total(a_pl.z);
                if ((threadIdx.x & 63) == 0) {
                    if (x != 0.f && isfinite(x)) atomicAdd(lds_gpos + 3 * l, x);
                    if (y != 0.f && isfinite(y)) atomicAdd(lds_gpos + 3 * l + 1, y);
                    if (z != 0.f && isfinite(z)) atomicAdd(lds_gpos + 3 * l + 2, z);
                }
            }
            if (img != nullptr) {
                float v[3] = {r.x * inv_spp, r.y * inv_spp, r.z * inv_spp};
                const bool head = wave_segmented_sum<3>(pixel, v);
                if (head && in) {
                    float *p = img + (size_t) l * plane + (size_t) pixel * 3;
                    if (v[0] != 0.f) atomicAdd(p, v[0]);
                    if (v[1] != 0.f) atomicAdd(p + 1, v[1]);
                    if (v[2] != 0.f) atomicAdd(p + 2, v[2]);
                }
            }
        }
        stack_rev_end<GEO>(csink, cx.sc, H);          // the hit's adjoint chain, once, on the sums over the lights
        // primary-triangle row: one add per run of lanes that hit the same triangle
        if (GEO && sink.g.g_tri_info != nullptr) {
            const bool head = wave_run_sum<kPrimaryWords, (FL & kSceneRough) == 0 || PSDR_DPP_ALWAYS>(pg.tri, pg.w);
            if (head && pg.tri >= 0) {
#pragma unroll
                for (int w = 0; w < kPrimaryWords; ++w) sink.add_tri(pg.tri, w, pg.w[w]);
            }
        }
    }
    if (want_gpos) {
        __syncthreads();
        for (int i = threadIdx.x; i < 3 * L; i += kBlock) {
            const float x = lds_gpos[i];
            if (x != 0.f && isfinite(x)) atomicAdd(g_pos + i, x);
        }
    }
    sink.end();
    count_rays(counters, nrays);
}

// ============================================================================ launches
// The handle's lights onto the device table, on the call's stream: positions [L][3], then K tangent sets [K][L][3] (missing sets are zero); behind room for
// three sets the kinds [L], uploaded only when a light is distant (lt.kind != null: the MIXED kernels)
int upload_lights(psdr_scene_s *h, int K, hipStream_t s, LightTable &lt, bool &moves) {
    const int L = (int) (h->stack_pos.size() / 3);
    const size_t n3 = (size_t) L * 3;
    HIP_TRY(hipMemcpyAsync(h->d_stack_lights, h->stack_pos.data(), sizeof(float) * n3, hipMemcpyHostToDevice, s));
    lt.pos = h->d_stack_lights; lt.dpos = nullptr; lt.L = L; lt.kind = nullptr;
    if (std::find(h->stack_kind.begin(), h->stack_kind.end(), PSDR_LIGHT_DISTANT) != h->stack_kind.end()) {
        int32_t *d_kind = reinterpret_cast<int32_t *>(h->d_stack_lights + 4 * n3);
        HIP_TRY(hipMemcpyAsync(d_kind, h->stack_kind.data(), sizeof(int32_t) * (size_t) L, hipMemcpyHostToDevice, s));
        lt.kind = d_kind;
    }
    moves = false;
    const int Kh = std::min(K, h->stack_K);
    for (size_t i = 0; i < n3 * (size_t) Kh; ++i) moves = moves || h->stack_dpos[i] != 0.f;
    if (K > 0 && moves) {
        if (Kh < K) HIP_TRY(hipMemsetAsync(h->d_stack_lights + n3, 0, sizeof(float) * n3 * K, s));
        HIP_TRY(hipMemcpyAsync(h->d_stack_lights + n3, h->stack_dpos.data(), sizeof(float) * n3 * Kh, hipMemcpyHostToDevice, s));
        lt.dpos = h->d_stack_lights + n3;
    }
    return 0;
}

template <class G, class R, int FL>
int stack_run_camera(psdr_scene_s *h, const psdr_render_opts *o, const TV<R, FL> &tv, const LightTable &lt, float *img, float *dimg, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp <= 0 || nsp <= 0) return 0;
    LaunchCtx cx;
    if (int rc = make_ctx(h, o, 0, cx)) return rc;
    const long long n = WH * nsp;
    h->slots[0] += (uint64_t) n;
    const int own = wave_owns_pixels(h, nsp, n);
    if (lt.kind != nullptr)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stack_camera<G, R, FL, true>), dim3(launch_blocks(h, n, camera_blocks_per_cu(h, n))), dim3(kBlock), lds_bytes(cx, h), s, cx, tv, lt, o->spp, o->spp_begin,
                           SlotDiv(nsp), n, 1.f / (float) o->spp, img, dimg, WH * 3, h->d_counters, own);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stack_camera<G, R, FL, false>), dim3(launch_blocks(h, n, camera_blocks_per_cu(h, n))), dim3(kBlock), lds_bytes(cx, h), s, cx, tv, lt, o->spp, o->spp_begin,
                           SlotDiv(nsp), n, 1.f / (float) o->spp, img, dimg, WH * 3, h->d_counters, own);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int FL>
int stack_render_c(psdr_scene_s *h, const psdr_render_opts *o, float *out_img, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    LightTable lt; bool moves;
    if (int rc = upload_lights(h, 0, s, lt, moves)) return rc;
    HIP_TRY(hipMemsetAsync(out_img, 0, sizeof(float) * WH * 3 * lt.L, s));
    const TangentView<0, FL> tv0{};
    return stack_run_camera<float, float, FL>(h, o, tv0, lt, out_img, nullptr, s);
}

template <int K, int FL>
int stack_render_fwd_k(psdr_scene_s *h, const psdr_render_opts *o, const psdr_tangents *tangents, float *img, float *dimg, const psdr_host::PointLightOps *point, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    TangentView<K, FL> tv;
    for (int k = 0; k < K; ++k) tv.t[k] = tangents[k];
    LightTable lt; bool moves;
    if (int rc = upload_lights(h, K, s, lt, moves)) return rc;
    const int L = lt.L;
    HIP_TRY(hipMemsetAsync(img, 0, sizeof(float) * WH * 3 * L, s));
    HIP_TRY(hipMemsetAsync(dimg, 0, sizeof(float) * WH * 3 * L * K, s));
    if (tangents_move_geometry(tangents, K) || moves) { if (int rc = stack_run_camera<Dual<K>, Dual<K>, FL>(h, o, tv, lt, img, dimg, s)) return rc; }
    else { if (int rc = stack_run_camera<float, Dual<K>, FL>(h, o, tv, lt, img, dimg, s)) return rc; }
    // the edge terms: the PointLightIntegrator's kernels, once per light, into the light's planes
    const int Kh = std::min(K, h->stack_K);
    for (int l = 0; l < L; ++l) {
        float dp[3][3] = {};
        for (int k = 0; k < Kh; ++k) for (int c = 0; c < 3; ++c) dp[k][c] = h->stack_dpos[((size_t) k * L + l) * 3 + c];
        if (int rc = point->edges_fwd(h, o, K, tangents, h->stack_kind[(size_t) l], h->stack_pos.data() + 3 * l, &dp[0][0], dimg + (size_t) l * WH * 3, (long long) L * WH * 3, s)) return rc;
    }
    return 0;
}
template <int FL>
int stack_render_fwd(psdr_scene_s *h, const psdr_render_opts *o, int K, const psdr_tangents *tangents, float *img, float *dimg, const psdr_host::PointLightOps *point, hipStream_t s) {
    switch (K) {
        case 1: return stack_render_fwd_k<1, FL>(h, o, tangents, img, dimg, point, s);
        case 3: return stack_render_fwd_k<3, FL>(h, o, tangents, img, dimg, point, s);
        default: return fail("psdr_render_d_fwd: K must be 1 or 3");
    }
}

template <int FL>
int stack_render_rev(psdr_scene_s *h, const psdr_render_opts *o, const float *adj_img, float *out_img, const psdr_grads *grads, const psdr_host::PointLightOps *point, hipStream_t s) {
    const long long WH = (long long) h->desc.width * h->desc.height;
    LightTable lt; bool moves;
    if (int rc = upload_lights(h, 0, s, lt, moves)) return rc;
    const int L = lt.L;
    if (out_img) HIP_TRY(hipMemsetAsync(out_img, 0, sizeof(float) * WH * 3 * L, s));
    DeviceSink<FL> sink{};
    if (int rc = make_device_sink(h, grads, sink)) return rc;
    float *g_pos = h->stack_gpos;
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
        // the column of the lights' gradients behind the gradient cache
        const int off_gpos = (dyn_bytes + 15) / 16 * 16;
        dyn_bytes = off_gpos + (geo && g_pos ? 3 * L * (int) sizeof(float) : 0);
        if (dyn_bytes > h->lds_limit) return fail("psdr_render_d_rev: the LightStageIntegrator's launch needs " + std::to_string(dyn_bytes) + " bytes of LDS per workgroup, the device offers " +
                                                  std::to_string(h->lds_limit));
#define PSDR_LAUNCH_STACK_REV(GEO, MIXED)                                                                                                                                \
        do { if (int rc = allow_dynamic_lds(&k_stack_camera_rev<FL, GEO, MIXED>, dyn_bytes)) return rc;                                                                  \
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stack_camera_rev<FL, GEO, MIXED>), dim3(launch_blocks(h, n)), dim3(kBlock), dyn_bytes, s, cx, sink, lt, g_pos, off_gpos, o->spp, o->spp_begin, SlotDiv(nsp), n, \
                           1.f / (float) o->spp, adj_img, out_img, WH * 3, h->d_counters); } while (0)
        if (lt.kind != nullptr) { if (geo) PSDR_LAUNCH_STACK_REV(true, true); else PSDR_LAUNCH_STACK_REV(false, true); }
        else { if (geo) PSDR_LAUNCH_STACK_REV(true, false); else PSDR_LAUNCH_STACK_REV(false, false); }
#undef PSDR_LAUNCH_STACK_REV
        HIP_TRY(hipGetLastError());
    }
    for (int l = 0; l < L; ++l)
        if (int rc = point->edges_rev(h, o, adj_img + (size_t) l * WH * 3, grads, h->stack_kind[(size_t) l], h->stack_pos.data() + 3 * l, g_pos ? g_pos + 3 * l : nullptr, s)) return rc;
    return 0;
}
}  // namespace

namespace psdr_host {
const LightStageOps *PSDR_CAT(light_stage_ops_, PSDR_VARIANT_FLAGS)() {
    constexpr int FL = PSDR_VARIANT_FLAGS;
    static const LightStageOps ops{&stack_render_c<FL>, &stack_render_fwd<FL>, &stack_render_rev<FL>};
    return &ops;
}
}  // namespace psdr_host
