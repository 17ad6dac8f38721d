// psdr_path_lean.h -- the PathTracer camera kernels of flag set 8 (plain diffuse, no tree) for the launch the headline makes: every wave sits on ONE pixel and every
// kernel-argument primitive is a slab-form rectangle.  One vertex body for renderC (K = 0) and the log-derivative renderD (K >= 1): the estimator of
// Li<float, float, PATH> / li_path_logd_lean (same draws, same arithmetic forms, the same bits) without the work those two repeat or carry for other launches:
//   * the vertex' reflectance is looked up ONCE (K >= 1: one dual lookup, its value part is the plain texel) and answers both BSDF evaluations and the
//     log-derivative quotient -- Bsdf::eval fetches it per call, albedo_logd a third time, and the fences of the parking columns keep the compiler from merging them;
//   * the film position, the pixel's address and the splat are wave-uniform (scalar unit); the wave's total is wave_total directly, lane 0 stores; no atomic
//     epilogue, no segmented path;
//   * the ray test holds the slab-form rows only (lean_closest_hit: aa_prim_test / resolve_tiny_hit as closest_hit calls them, no plane-form loop).
// Every other launch (another sample count, a chunk, a primitive in plane form, columns that do not fit) runs the kernels it ran before: psdr_plan.h
// path_lean_form is the rule.  Included behind psdr_kernels.h by the two units that instantiate it (psdr_path_lean.hip: K = 0, psdr_logd_lean.hip: K = 1).
#pragma once
#include "psdr_logd_lean.h"

// A/B builds (tools/build_variant_lib.sh -DPSDR_PATH_LEAN_AB=n): the twins WITHOUT one of their parts, each replaced by what the kernels of before do in its place --
// bit 0: the reflectance per evaluation (Bsdf::eval, albedo_logd); bit 1: film position, reduction and splat per lane (wave_segmented_sum, the atomic epilogue compiled
// in); bit 2: the shared ray test (closest_hit with its plane-form loop).  Same bits in every combination.  The product is 0.
#ifndef PSDR_PATH_LEAN_AB
#define PSDR_PATH_LEAN_AB 0
#endif

namespace psdr {

// columns of the parked form: those of ParkLayout<K> and three more for the vertex' reflectance (PARKED = false: no columns, everything in registers)
template <int K> struct LeanLayout {
    static constexpr int result = 0, beta = 3, rd = 6, s = 6 + 3 * K, rng = 6 + 6 * K, vtx = 10 + 6 * K, rho = 13 + 6 * K, cols = 16 + 6 * K;
};

// closest_hit<false, 2, MASKED> of a launch whose rows are all in slab form (aa_cnt covers n_tiny: the plane-form loop has no trip)
template <bool MASKED>
__device__ __forceinline__ Hit lean_closest_hit(const SceneView &sc, const Vec3f &o, const Vec3f &d, uint32_t rows) {
    Hit best; best.tri = -1; best.u = best.v = -1.f; best.t = INFINITY;
    const Vec3f inv{1.f / d.x, 1.f / d.y, 1.f / d.z};
    int best_i = kNoPrim;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const float4 kernarg_float4;
    const kernarg_float4 *prim_rows = (kernarg_float4 *) ((__attribute__((address_space(4))) const char *) __builtin_amdgcn_kernarg_segment_ptr() + offsetof(SceneView, tiny));
    const int aa_cnt = sc.aa_cnt;
    float4 ra[kAaSlots]; float hb[kAaSlots]; int pk[kAaSlots];
#pragma unroll
    for (int i = 0; i < kAaSlots; ++i) {
        ra[i] = prim_rows[i * 4];
        const float2 r = *(__attribute__((address_space(4))) const float2 *) &prim_rows[i * 4 + 1];
        hb[i] = r.x; pk[i] = __float_as_int_hd(r.y);
    }
    const int cx = aa_cnt & 255, cy = (aa_cnt >> 8) & 255, cz = aa_cnt >> 16;
#define PSDR_AA(AX, S) do { if (!MASKED || ((rows >> (S)) & 1u) != 0u) aa_prim_test<AX, false>(ra[S], hb[S], pk[S], 0, o, d, inv, best, best_i, -1, -1); } while (0)
    if (cx > 0) { PSDR_AA(0, 0); if (cx > 1) { PSDR_AA(0, 1); if (cx > 2) PSDR_AA(0, 2); } }
    if (cy > 0) { PSDR_AA(1, 3); if (cy > 1) { PSDR_AA(1, 4); if (cy > 2) PSDR_AA(1, 5); } }
    if (cz > 0) { PSDR_AA(2, 6); if (cz > 1) { PSDR_AA(2, 7); if (cz > 2) PSDR_AA(2, 8); } }
#undef PSDR_AA
#else
    (void) rows; (void) o; (void) inv;
#endif
    resolve_tiny_hit(sc, best, best_i);
    return best;
}
// intersect<float, TVT, MASKED> (kDetached) on it
template <bool MASKED, class TVT>
__device__ __forceinline__ Its<float> lean_intersect(const SceneView &sc, const TVT &tv, TraversalStack &st, const RayT<float> &ray, bool active, uint32_t &nrays, int pre_slot, uint32_t rows = 0xffffffffu) {
    if constexpr ((PSDR_PATH_LEAN_AB & 4) != 0) return intersect<float, TVT, MASKED>(sc, tv, st, ray, active, kDetached, nrays, -1, -1, pre_slot, rows);
    Its<float> its;
    its.valid = false; its.tri = its.mesh = -1; its.J = 1.f; its.t = INFINITY;
    if (!active) return its;
    nrays++;
    Hit h;
    if constexpr (MASKED) h = lean_closest_hit<true>(sc, ray.o, ray.d, wave_or_hd(rows));
    else h = lean_closest_hit<false>(sc, ray.o, ray.d, rows);
    if (h.tri < 0) return its;
    fill_its_from_hit<float>(its, sc, tv, h, ray, kDetached);
    return its;
}
// Bsdf<float, float>::eval of the flag set (diffuse) on the reflectance the vertex holds
__device__ __forceinline__ Vec3f lean_eval(const Vec3f &rho, const Its<float> &its, const Vec3f &wo) {
    if (!(its.wi.z > 0.f && wo.z > 0.f)) return Vec3f(0.f);
    return rho * (wo.z * kInvPi);
}

template <int K> struct LeanValue { float v[3 * (1 + K)]; };          // result, then K tangents of it

// li_path_logd_lean for K >= 0 tangent sets on albedo texels, every lane on a live slot.  PARKED: the state that idles across the two ray tests of a vertex sits in
// the LDS columns of LeanLayout<K> (psdr_logd_lean.h on why and how).
template <int K, bool PARKED, class TVT>
__device__ __forceinline__ LeanValue<K> li_path_lean(const SceneView &sc, const TVT &tv, TraversalStack &st, const LiParams &lp, Rng &rng, const RayT<float> &ray, uint32_t &nrays, const Park &pk) {
    using L = LeanLayout<K>;
    using TV0 = TangentView<0, TVT::flags>;
    static_assert(TVT::tiny && !TVT::has_env && !TVT::has_rough && TVT::k == K, "the twins serve the plain diffuse flag set of scenes without a tree");
    constexpr int KA = K > 0 ? K : 1;
    const TV0 tv0{};
    auto fence = [] { if constexpr (PARKED) Park::fence(); };
    constexpr bool ONCE = (PSDR_PATH_LEAN_AB & 1) == 0;
    Its<float> its = lean_intersect<false>(sc, tv0, st, ray, true, nrays, kPrePrimaryRay);
    bool active = its.valid;
    Vec3f result = lp.hide_emitters ? Vec3f(0.f) : Le<float>(sc, tv0, its, active);
    float rd[KA][3], s[KA][3];
#pragma unroll
    for (int k = 0; k < KA; ++k) { rd[k][0] = rd[k][1] = rd[k][2] = 0.f; s[k][0] = s[k][1] = s[k][2] = 0.f; }
    Vec3f beta(1.f);
    for (int depth = 0; depth < lp.max_depth; ++depth) {
        int bsdf_id = active ? Tab<TVT::flags>::mesh_bsdf(sc, its.mesh) : 0;
        bool act = active;
        if (bsdf_id < 0) { act = false; bsdf_id = 0; }
        const Bsdf<float, float> bsdf(sc, tv0, bsdf_id);
        // the vertex' material, once: the reflectance for both evaluations and (K >= 1) its quotient d rho / rho for the running sums, as albedo_logd forms it
        Vec3f rho(0.f);
        if constexpr (!ONCE && K > 0) {
            if (active) {
                float g[KA][3];
                albedo_logd<KA>(sc, tv, its, g);
#pragma unroll
                for (int k = 0; k < K; ++k) { s[k][0] += g[k][0]; s[k][1] += g[k][1]; s[k][2] += g[k][2]; }
            }
        }
        if (ONCE && act) {
            if constexpr (K == 0) rho = bsdf.tex3(sc, tv0, PSDR_SLOT_REFLECTANCE, its);
            else {
                const Bsdf<float, Dual<KA>> bsdf_d(sc, tv, bsdf_id);
                const Vec3<Dual<KA>> r = bsdf_d.tex3(sc, tv, PSDR_SLOT_REFLECTANCE, its);
                rho = Vec3f(r.x.v, r.y.v, r.z.v);
                const float ix = r.x.v != 0.f ? 1.f / r.x.v : 0.f, iy = r.y.v != 0.f ? 1.f / r.y.v : 0.f, iz = r.z.v != 0.f ? 1.f / r.z.v : 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) { s[k][0] += r.x.d[k] * ix; s[k][1] += r.y.d[k] * iy; s[k][2] += r.z.d[k] * iz; }
            }
        }
        const float sb0 = rng.next(), sb1 = rng.next(), sb2 = rng.next();
        const float s0 = rng.next(), s1 = rng.next();
        float sb1k = sb1, sb2k = sb2;
        if constexpr (PARKED) {
            pk.put3(L::result, result); pk.put3(L::beta, beta);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pk.put(L::rd + 3 * k, rd[k][0]); pk.put(L::rd + 3 * k + 1, rd[k][1]); pk.put(L::rd + 3 * k + 2, rd[k][2]);
                pk.put(L::s + 3 * k, s[k][0]); pk.put(L::s + 3 * k + 1, s[k][1]); pk.put(L::s + 3 * k + 2, s[k][2]);
            }
            pk.put64(L::rng, rng.state); pk.put64(L::rng + 2, rng.inc);
            pk.put(L::vtx, sb1); pk.put(L::vtx + 1, sb2);
            if constexpr (ONCE) pk.put3(L::rho, rho);
        }
        fence();
        Vec3f c(0.f);
        if (act) {
            // the emitter sample (direct_step's light_sample)
            const PosSample<float> ps = sample_emitter_position<float>(sc, tv0, its.p, s0, s1, false);
            Vec3f wo = ps.p - its.p;
            const float d2 = dot(wo, wo), dist = safe_sqrt(d2);
            wo = wo / dist;
            const RayT<float> ray1{its.p, wo};
            const Vec3f wl = its.sh.to_local(wo);
            const bool lit = PSDR_SKIP_UNLIT ? (wl.z > 0.f && its.wi.z > 0.f) : true;
            auto trace_light = [&]() {
                if constexpr (PSDR_OCC_ROWS) return lean_intersect<true>(sc, tv0, st, ray1, ps.valid && lit, nrays, kPreLightRay, occ_rows(sc, its.tri, ps.tri));
                else return lean_intersect<false>(sc, tv0, st, ray1, ps.valid && lit, nrays, kPreLightRay);
            };
            const Its<float> its1 = trace_light();
            if (its1.valid && its1.t > dist - kShadowEpsilon && emitter_of(sc, tv0, its1) >= 0) {
                Vec3f rho_l = rho;
                if constexpr (PARKED && ONCE) rho_l = pk.get3(L::rho);
                const float Gv = abs_(dot(its1.n, -wo)) / d2;
                const Vec3f bsdf_val = (ONCE ? lean_eval(rho_l, its, wl) : bsdf.eval(sc, tv0, its, wl, true)) * to_m<float>(Gv * ps.J / ps.pdf);
                float pdf1 = bsdf.pdf(sc, tv0, its, wl, true);
                pdf1 = pdf1 * Gv;
                const float w = mis_weight(float(ps.pdf), pdf1);
                c = c + Le<float>(sc, tv0, its1, true) * bsdf_val * w;
            }
        }
        if constexpr (PARKED) {
            Park::fence();
            sb1k = pk.get(L::vtx); sb2k = pk.get(L::vtx + 1);
            Park::fence();
            pk.put3(L::vtx, c);
            Park::fence();
        }
        const float sb[3] = {sb0, sb1k, sb2k};
        Its<float> nits; Vec3f nf(0.f); bool nvalid = false;
        Vec3f lb(0.f); float wb = 0.f; bool a1b = false;          // the BSDF sample's emitter hit: added behind the reload, in direct_step's own form
        if (act) {
            // the BSDF sample (direct_step's bsdf_sample); its hit is the path's next vertex
            Vec3f wo_s; float pdf_s;
            bool a1 = bsdf.sample(sc, tv0, its, sb, true, wo_s, pdf_s);
            // (the shading tangents rebuilt from the normal: psdr_logd_lean.h)
            Vec3f shn = its.sh.n;
            asm volatile("" : "+v"(shn.x), "+v"(shn.y), "+v"(shn.z));
            const Frame<float> fr(shn);
            const Vec3f dir1 = fr.s * wo_s.x + fr.t * wo_s.y + shn * wo_s.z;
            const RayT<float> ray1{its.p, dir1};
            const Its<float> its1 = lean_intersect<false>(sc, tv0, st, ray1, a1, nrays, kPreBsdfRay);
            const bool a_hit = a1 && its1.valid;
            a1 = a_hit && emitter_of(sc, tv0, its1) >= 0;
            Vec3f bsdf_val(0.f); float pdf0(0.f);
            if (a_hit) {
                Vec3f rho_b = rho;
                if constexpr (PARKED && ONCE) rho_b = pk.get3(L::rho);
                bsdf_val = ONCE ? lean_eval(rho_b, its, wo_s) : bsdf.eval(sc, tv0, its, wo_s, true);
                const float Gv = abs_(dot(its1.n, -ray1.d)) / sqr(its1.t);
                pdf0 = pdf_s * Gv;
                bsdf_val = bsdf_val / pdf_s;
            }
            if (a1) {
                wb = mis_weight(pdf0, float(emitter_position_pdf(sc, tv0, its.p, its1)));
                lb = Le<float>(sc, tv0, its1, true) * bsdf_val;
            }
            a1b = a1;
            nits = its1; nf = bsdf_val; nvalid = a_hit;
        }
        if constexpr (PARKED) {
            Park::fence();
            c = pk.get3(L::vtx);
            result = pk.get3(L::result); beta = pk.get3(L::beta);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                rd[k][0] = pk.get(L::rd + 3 * k); rd[k][1] = pk.get(L::rd + 3 * k + 1); rd[k][2] = pk.get(L::rd + 3 * k + 2);
                s[k][0] = pk.get(L::s + 3 * k); s[k][1] = pk.get(L::s + 3 * k + 1); s[k][2] = pk.get(L::s + 3 * k + 2);
            }
            rng.state = pk.get64(L::rng); rng.inc = pk.get64(L::rng + 2);
            Park::fence();
        }
        if (a1b) c = c + lb * wb;
        // ---- the path's update (Li / li_path_logd)
        if (active) {
            if constexpr (K == 0) result = result + beta * c;
            else {
                const Vec3f bc = beta * c;
                result = result + bc;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    rd[k][0] = fmaf(bc.x, s[k][0], rd[k][0]); rd[k][1] = fmaf(bc.y, s[k][1], rd[k][1]); rd[k][2] = fmaf(bc.z, s[k][2], rd[k][2]);
                }
            }
            active = nvalid;
            if (active) {
                beta = beta * nf;
                if (!(beta.x != 0.f || beta.y != 0.f || beta.z != 0.f)) active = false;
            }
        }
        its = nits;          // for every lane (psdr_logd_lean.h)
    }
    // zero_nonfinite of the sample
    LeanValue<K> out;
    const bool fx = isfinite(result.x), fy = isfinite(result.y), fz = isfinite(result.z);
    out.v[0] = fx ? result.x : 0.f; out.v[1] = fy ? result.y : 0.f; out.v[2] = fz ? result.z : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        out.v[3 + 3 * k] = (fx && isfinite(rd[k][0])) ? rd[k][0] : 0.f;
        out.v[4 + 3 * k] = (fy && isfinite(rd[k][1])) ? rd[k][1] : 0.f;
        out.v[5 + 3 * k] = (fz && isfinite(rd[k][2])) ? rd[k][2] : 0.f;
    }
    return out;
}

}  // namespace psdr

namespace {

// columns per K: the compile-only table of profiles/path_lean_ab.txt decides
template <int K> constexpr bool path_lean_parked() { return psdr_host::path_lean_cols(K) > 0; }

// One wave = one pixel, 64 samples of it (psdr_plan.h path_lean_form).  wdiv: the division by the image width.  K >= 1 runs behind the gate of the log-derivative
// launches like k_camera_logd_lean; SEEDED: the slot's stream comes from the handle's seed table.  The body of the two kernels below, which differ in their names:
// tools that sort kernels into renderC and renderD by name (bench.py's counter passes) look for "k_camera_logd" in a log-derivative kernel's.
template <int K, bool SEEDED>
__device__ __forceinline__ void camera_path_lean(const LaunchCtx &cx, const TangentView<K, kSceneTiny> &tv, int spp, int s_begin, const SlotDiv &wdiv, int n_pixels, float inv_spp,
                                                 float *__restrict__ img, float *__restrict__ dimg, long long plane, unsigned long long *counters, const ulonglong2 *__restrict__ seed) {
    constexpr int NV = 3 * (1 + K);
    constexpr bool PARKED = path_lean_parked<K>();
    if constexpr (K > 0) { if (counters[kLogdGateWord] != 1ull) return; }
    TraversalStack st; setup_lds(cx, st, tv);
    Park pk{nullptr};
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (PARKED) pk.base = reinterpret_cast<float *>(psdr_dyn_lds + cx.off_park) + threadIdx.x;
#endif
    uint32_t nrays = 0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    constexpr int kWaves = kBlock / 64;
    for (int pb = (int) blockIdx.x * kWaves; pb < n_pixels; pb += (int) gridDim.x * kWaves) {          // (uniform: a wave is whole or absent)
        const int pixel = pb + wave;
        if (pixel >= n_pixels) continue;
        Rng rng;
        if constexpr (SEEDED) {
            const ulonglong2 sd = (seed + (size_t) pixel * 64)[lane];
            rng.init_seeded(sd.x, sd.y, cx.jump);
        } else {
            rng.init((uint64_t) pixel * (uint64_t) spp + (uint64_t) (s_begin + lane), cx.jump);
        }
        const float j0 = rng.next(), j1 = rng.next();
        const TangentView<0, kSceneTiny> tv0{};
        if constexpr ((PSDR_PATH_LEAN_AB & 2) != 0) {
            // A/B: the pixel as a per-lane value, the film arithmetic and the splat of k_camera_logd_lean on it
            int pl = pixel;
            asm volatile("" : "+v"(pl));
            const int W = cx.sc.d.width;
            const float sx = ((float) (pl % W) + j0) / (float) W, sy = ((float) (pl / W) + j1) / (float) cx.sc.d.height;
            const RayT<float> ray = primary_ray<float>(cx.sc, tv0, sx, sy);
            const LeanValue<K> r = li_path_lean<K, PARKED>(cx.sc, tv, st, cx.lp, rng, ray, nrays, pk);
            float v[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = r.v[i] * inv_spp;
            const bool head = wave_segmented_sum<NV>(pl, v);
            if (head) {
                float *p = img + (size_t) pl * 3;
                if (cx.lp.max_depth >= 0) {          // (`own`, as a value the compiler cannot fold)
                    p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
#pragma unroll
                    for (int k = 0; k < K; ++k) { float *q = dimg + (size_t) k * plane + (size_t) pl * 3; q[0] = v[3 + 3 * k]; q[1] = v[4 + 3 * k]; q[2] = v[5 + 3 * k]; }
                } else {
#pragma unroll
                    for (int i = 0; i < 3; ++i) if (v[i] != 0.f) atomicAdd(p + i, v[i]);
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        for (int i = 0; i < 3; ++i) if (v[3 + 3 * k + i] != 0.f) atomicAdd(dimg + (size_t) k * plane + (size_t) pl * 3 + i, v[3 + 3 * k + i]);
                }
            }
            continue;
        }
        int py, px;
        slot_to_pixel(pixel, wdiv, py, px);
        const float sx = ((float) px + j0) / (float) cx.sc.d.width, sy = ((float) py + j1) / (float) cx.sc.d.height;
        const RayT<float> ray = primary_ray<float>(cx.sc, tv0, sx, sy);
        const LeanValue<K> r = li_path_lean<K, PARKED>(cx.sc, tv, st, cx.lp, rng, ray, nrays, pk);
        float v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = wave_total(r.v[i] * inv_spp);
        if (lane == 0) {
            float *p = img + (size_t) pixel * 3;
            p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
#pragma unroll
            for (int k = 0; k < K; ++k) { float *q = dimg + (size_t) k * plane + (size_t) pixel * 3; q[0] = v[3 + 3 * k]; q[1] = v[4 + 3 * k]; q[2] = v[5 + 3 * k]; }
        }
    }
    count_rays(counters, nrays);
}
template <bool SEEDED>
__global__ __launch_bounds__(kBlock, kPathLeanWaves) void k_camera_path_lean(LaunchCtx cx, TangentView<0, kSceneTiny> tv, int spp, int s_begin, SlotDiv wdiv, int n_pixels, float inv_spp,
                                                                              float *__restrict__ img, float *__restrict__ dimg, long long plane, unsigned long long *counters,
                                                                              const ulonglong2 *__restrict__ seed) {
    camera_path_lean<0, SEEDED>(cx, tv, spp, s_begin, wdiv, n_pixels, inv_spp, img, dimg, plane, counters, seed);
}
template <int K, bool SEEDED>
__global__ __launch_bounds__(kBlock, kPathLeanWaves) void k_camera_logd_path_lean(LaunchCtx cx, TangentView<K, kSceneTiny> tv, int spp, int s_begin, SlotDiv wdiv, int n_pixels, float inv_spp,
                                                                                   float *__restrict__ img, float *__restrict__ dimg, long long plane, unsigned long long *counters,
                                                                                   const ulonglong2 *__restrict__ seed) {
    static_assert(K >= 1, "the renderC twin is k_camera_path_lean");
    camera_path_lean<K, SEEDED>(cx, tv, spp, s_begin, wdiv, n_pixels, inv_spp, img, dimg, plane, counters, seed);
}

}  // namespace

namespace psdr_host {
// Launches the twin of K tangent sets where path_lean_form chooses it (*ran), in the grid and with the seed table of the launch it replaces.  K >= 1: behind the gate
// kernels of run_camera.  cx0: the launch context of run_camera (off_park is set on a copy).
template <int K>
int path_lean_launch(psdr_scene_s *h, const psdr_render_opts *o, const LaunchCtx &cx0, const psdr::TangentView<K, psdr::kSceneTiny> &tv, float *img, float *dimg, hipStream_t s, bool *ran) {
    *ran = false;
    const long long WH = (long long) h->desc.width * h->desc.height;
    const int nsp = o->spp_end - o->spp_begin;
    const long long n = WH * nsp;
    const int lds = (lds_bytes(cx0, h) + 15) / 16 * 16, park = path_lean_cols(K) * kBlock * 4;
    // (K >= 1: run_camera calls behind its texels-only test)
    if (path_lean_form(h, kSceneTiny, K, o->integrator, true, nsp, n, lds) != kPathLeanOwnSlab) { h->path_lean_fallbacks[K > 0]++; return 0; }
    LaunchCtx cx = cx0;
    cx.off_park = lds;
    const dim3 grid(launch_blocks(h, n, camera_blocks_per_cu(h, n)));
    const ulonglong2 *seed = seed_table(h, o, WH, nsp, n, s);
    const SlotDiv wdiv(h->desc.width);
    const float inv_spp = 1.f / (float) o->spp;
#define PSDR_LAUNCH_LEAN(...) hipLaunchKernelGGL(HIP_KERNEL_NAME(__VA_ARGS__), grid, dim3(kBlock), lds + park, s, cx, tv, o->spp, o->spp_begin, wdiv, (int) WH, inv_spp, img, dimg, WH * 3, h->d_counters, seed)
    if constexpr (K == 0) { if (seed != nullptr) PSDR_LAUNCH_LEAN(k_camera_path_lean<true>); else PSDR_LAUNCH_LEAN(k_camera_path_lean<false>); }
    else { if (seed != nullptr) PSDR_LAUNCH_LEAN(k_camera_logd_path_lean<K, true>); else PSDR_LAUNCH_LEAN(k_camera_logd_path_lean<K, false>); }
#undef PSDR_LAUNCH_LEAN
    h->path_lean_launches[K > 0]++;
    if (seed != nullptr) h->seed_launches++;
    if (K > 0) {          // a lean launch of the log-derivative kernel like the one it stands in for (psdr_scene_logd_info)
        h->logd_lean_launches++;
        if (seed != nullptr) h->logd_lean_seeded++;
        h->logd_lean_lds = lds; h->logd_lean_park = park;
    }
    *ran = true;
    return 0;
}
}  // namespace psdr_host
