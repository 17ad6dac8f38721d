// psdr_logd_lean.h -- the lean twin of the log-derivative camera kernel (psdr_kernels.h k_camera_logd) for scenes without a tree.
//
// k_camera_logd<1, FL, true> runs at six waves per SIMD (80 VGPRs) and does not fit: 37 VGPRs spilled, 71 scratch instructions, 712 MB of counter
// traffic per launch of the headline, and its time follows the spill count (profiles/seed_cache_ab.txt section 6).  The twin evaluates the same
// estimator (li_path_logd / direct_step's PathTracer vertex: same draws, same arithmetic forms, bit-identical images) with the state that idles
// across the two ray tests of a path vertex PARKED in per-lane LDS columns (column i of lane t at park[i * kBlock + t]: conflict-free, one ds_
// instruction each way) instead of wherever the register allocator spills it.
//
// What makes parking work (and what defeated parking the accumulators around direct_step inside the old kernel body):
//   * store and reload sit at the SAME control-flow level, outside every divergent branch.  A value reloaded inside `if (in)` / `if (active)` is
//     merged with its old value at the join, so the old value's register stays allocated across the branch for the lanes that skip it and
//     nothing is freed.  The twin therefore runs a slot with `active = in` instead of under `if (in)`, and parks / reloads for all lanes;
//   * a compiler fence (empty asm with a memory clobber) behind the stores and in front of the loads keeps store-to-load forwarding from
//     handing the register copy on;
//   * plain LDS pointers (address space inferred after inlining), not volatile ones.
#pragma once
#include "psdr_device.h"

namespace psdr {

// columns: 0-2 result, 3-5 beta, 6 .. 6+3K-1 rd, then s, then the stream (state, inc: 4 words), then 3 words that change hands inside a
// vertex (the BSDF sample's two numbers across the light ray; the light sample's contribution across the BSDF ray).  19 KiB per workgroup at K = 1.
template <int K> struct ParkLayout {
    static constexpr int result = 0, beta = 3, rd = 6, s = 6 + 3 * K, rng = 6 + 6 * K, vtx = 10 + 6 * K, cols = 13 + 6 * K;
};
struct Park {
    float *base;          // this lane's word of column 0
    __device__ __forceinline__ void put(int col, float v) const { base[col * kBlock] = v; }
    __device__ __forceinline__ float get(int col) const { return base[col * kBlock]; }
    __device__ __forceinline__ void put3(int col, const Vec3f &v) const { put(col, v.x); put(col + 1, v.y); put(col + 2, v.z); }
    __device__ __forceinline__ Vec3f get3(int col) const { Vec3f v; v.x = get(col); v.y = get(col + 1); v.z = get(col + 2); return v; }
    __device__ __forceinline__ void put64(int col, uint64_t v) const { put(col, __uint_as_float((uint32_t) v)); put(col + 1, __uint_as_float((uint32_t) (v >> 32))); }
    __device__ __forceinline__ uint64_t get64(int col) const { return (uint64_t) __float_as_uint(get(col)) | ((uint64_t) __float_as_uint(get(col + 1)) << 32); }
    static __device__ __forceinline__ void fence() { asm volatile("" ::: "memory"); }
};

// li_path_logd with the vertex step of direct_step (its PathTracer branch, G = M = float: emitter sample first, then the BSDF sample) written out
// so that the parked state can change hands between the two ray tests.  active0: the slot exists (the caller does not branch around the path).
template <int K, class TVT>
__device__ __forceinline__ Vec3<Dual<K>> li_path_logd_lean(const SceneView &sc, const TVT &tv, TraversalStack &st, const LiParams &lp, Rng &rng, const RayT<float> &ray,
                                                         bool active0, uint32_t &nrays, const Park &pk) {
    using L = ParkLayout<K>;
    using TV0 = TangentView<0, TVT::flags>;
    static_assert(TVT::tiny && !TVT::has_env && !TVT::has_rough, "the twin serves the plain diffuse flag set of scenes without a tree");
    const TV0 tv0{};
    Its<float> its = intersect<float>(sc, tv0, st, ray, active0, kDetached, nrays, -1, -1, kPrePrimaryRay);
    bool active = active0 && its.valid;
    Vec3f result = lp.hide_emitters ? Vec3f(0.f) : Le<float>(sc, tv0, its, active);
    float rd[K][3], s[K][3];
#pragma unroll
    for (int k = 0; k < K; ++k) { rd[k][0] = rd[k][1] = rd[k][2] = 0.f; s[k][0] = s[k][1] = s[k][2] = 0.f; }
    Vec3f beta(1.f);
    for (int depth = 0; depth < lp.max_depth; ++depth) {
        if (active) {
            float g[K][3];
            albedo_logd<K>(sc, tv, its, g);
#pragma unroll
            for (int k = 0; k < K; ++k) { s[k][0] += g[k][0]; s[k][1] += g[k][1]; s[k][2] += g[k][2]; }
        }
        // ---- direct_step<float, float>(.., its, active, 1, 1, .., &nits, &nf, &nvalid, nullptr, last)
        int bsdf_id = active ? Tab<TVT::flags>::mesh_bsdf(sc, its.mesh) : 0;
        bool act = active;
        if (bsdf_id < 0) { act = false; bsdf_id = 0; }
        const Bsdf<float, float> bsdf(sc, tv0, bsdf_id);
        const float sb0 = rng.next(), sb1 = rng.next(), sb2 = rng.next();
        const float s0 = rng.next(), s1 = rng.next();
        // everything the two ray tests do not touch leaves the registers (all lanes, no branch around it)
        pk.put3(L::result, result); pk.put3(L::beta, beta);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            pk.put(L::rd + 3 * k, rd[k][0]); pk.put(L::rd + 3 * k + 1, rd[k][1]); pk.put(L::rd + 3 * k + 2, rd[k][2]);
            pk.put(L::s + 3 * k, s[k][0]); pk.put(L::s + 3 * k + 1, s[k][1]); pk.put(L::s + 3 * k + 2, s[k][2]);
        }
        pk.put64(L::rng, rng.state); pk.put64(L::rng + 2, rng.inc);
        pk.put(L::vtx, sb1); pk.put(L::vtx + 1, sb2);
        Park::fence();
        Vec3f c(0.f);
        if (act) {
            // the emitter sample (direct.cpp:120-160)
            const PosSample<float> ps = sample_emitter_position<float>(sc, tv0, its.p, s0, s1, false);
            Vec3f wo = ps.p - its.p;
            const float d2 = dot(wo, wo), dist = safe_sqrt(d2);
            wo = wo / dist;
            const RayT<float> ray1{its.p, wo};
            const Vec3f wl = its.sh.to_local(wo);
            const bool lit = PSDR_SKIP_UNLIT ? (wl.z > 0.f && its.wi.z > 0.f) : true;
            auto trace_light = [&]() {
                if constexpr (TVT::tiny && PSDR_OCC_ROWS) return intersect<float, TV0, true>(sc, tv0, st, ray1, ps.valid && lit, kDetached, nrays, -1, -1, kPreLightRay, occ_rows(sc, its.tri, ps.tri));
                else return intersect<float>(sc, tv0, st, ray1, ps.valid && lit, kDetached, nrays, -1, -1, kPreLightRay);
            };
            const Its<float> its1 = trace_light();
            if (its1.valid && its1.t > dist - kShadowEpsilon && emitter_of(sc, tv0, its1) >= 0) {
                const float Gv = abs_(dot(its1.n, -wo)) / d2;
                const Vec3f bsdf_val = bsdf.eval(sc, tv0, its, wl, true) * to_m<float>(Gv * ps.J / ps.pdf);
                float pdf1 = bsdf.pdf(sc, tv0, its, wl, true);
                pdf1 = pdf1 * Gv;
                const float w = mis_weight(float(ps.pdf), pdf1);
                c = c + Le<float>(sc, tv0, its1, true) * bsdf_val * w;
            }
        }
        Park::fence();
        const float sb[3] = {sb0, pk.get(L::vtx), pk.get(L::vtx + 1)};
        Park::fence();
        pk.put3(L::vtx, c);
        Park::fence();
        Its<float> nits; Vec3f nf(0.f); bool nvalid = false;
        Vec3f lb(0.f); float wb = 0.f; bool a1b = false;          // the BSDF sample's emitter hit: added behind the reload, in direct_step's own form
        if (act) {
            // the BSDF sample (direct.cpp:64-118); its hit is the path's next vertex
            Vec3f wo_s; float pdf_s;
            bool a1 = bsdf.sample(sc, tv0, its, sb, true, wo_s, pdf_s);
            // the shading tangents are rebuilt from the normal (Frame's own arithmetic on its own input: the same bits) instead of living across the light ray;
            // the normal passes through an empty asm so that the two frames are not merged into one again
            Vec3f shn = its.sh.n;
            asm volatile("" : "+v"(shn.x), "+v"(shn.y), "+v"(shn.z));
            const Frame<float> fr(shn);
            const Vec3f dir1 = fr.s * wo_s.x + fr.t * wo_s.y + shn * wo_s.z;
            const RayT<float> ray1{its.p, dir1};
            const Its<float> its1 = intersect<float>(sc, tv0, st, ray1, a1, kDetached, nrays, -1, -1, kPreBsdfRay);
            const bool a_hit = a1 && its1.valid;
            a1 = a_hit && emitter_of(sc, tv0, its1) >= 0;
            Vec3f bsdf_val(0.f); float pdf0(0.f);
            if (a_hit) {
                bsdf_val = bsdf.eval(sc, tv0, its, wo_s, true);
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
        if (a1b) c = c + lb * wb;
        // ---- li_path_logd's update
        if (active) {
            const Vec3f bc = beta * c;
            result = result + bc;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                rd[k][0] = fmaf(bc.x, s[k][0], rd[k][0]); rd[k][1] = fmaf(bc.y, s[k][1], rd[k][1]); rd[k][2] = fmaf(bc.z, s[k][2], rd[k][2]);
            }
            active = nvalid;
            if (active) {
                beta = beta * nf;
                if (!(beta.x != 0.f || beta.y != 0.f || beta.z != 0.f)) active = false;
            }
        }
        its = nits;          // for every lane: a lane whose path has ended never reads it again, and a merge with the old record would keep all of it alive across both ray tests
    }
    Vec3<Dual<K>> out;
    out.x.v = result.x; out.y.v = result.y; out.z.v = result.z;
#pragma unroll
    for (int k = 0; k < K; ++k) { out.x.d[k] = rd[k][0]; out.y.d[k] = rd[k][1]; out.z.d[k] = rd[k][2]; }
    return out;
}

}  // namespace psdr
