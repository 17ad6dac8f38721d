// psdr_lightstage.h -- LightStageIntegrator (PSDR_INTEGRATOR_POINT_STACK, include/psdr_hip.h): L point lights rendered from ONE camera hit per sample slot.
// Plane l of the result is the PointLightIntegrator's image under light l (psdr_pointlight.h: Li = f(wi, wo_l) V(p, pL_l) / r_l^2, unit intensity); what the
// lights share -- the film jitter, the primary ray, the walk, the hit, the Bsdf record and, in reverse mode, the adjoint chain of the hit -- is done once.
// The estimator is split where the sharing ends:
//   forward   stack_camera_hit (once per slot)   -> stack_light_value (once per light: the light part of li_point)
//   reverse   stack_rev_begin  (once per slot)   -> stack_rev_light   (once per light: value, BSDF adjoint, a_wo chain to the light; the adjoints of its.p, the
//             shading frame, wi, uv and of a mapped record's frame ADD UP in StackRevHit) -> stack_rev_end (once per slot: the part of point_sample_reverse
//             behind the a_wo chain, on the sums)
// The loop over the lights belongs to the caller (the kernels of psdr_lightstage.hip, the host harness tests/hostcheck/hostcheck_lightstage.cpp): it is a
// run-time, wave-uniform loop with a wave reduction per light, which a per-lane function cannot hold.  colloc_bsdf_eval_vjp scatters the texel adjoints itself
// (bitmap_vjp inside BsdfRev::eval_vjp and the microfacet adjoints), so the BSDF parameters' adjoints leave per light; everything behind them is summed.
// The primary-edge and shadow-boundary terms share nothing between lights but the edge draw: they run as the PointLightIntegrator's own kernels, once per light.
#pragma once
#include "psdr_pointlight.h"

namespace psdr {

// The lights as the kernels read them: positions [L][3] (a distant light's row: its direction), in forward mode tangents [K][L][3] (null: none) and the
// light models [L] (PSDR_LIGHT_*; null: every light is a point light); read with a wave-uniform index, so the branch on a light's kind is wave-uniform
struct LightTable { const float *pos; const float *dpos; int L; const int32_t *kind; };
PSDR_HD bool stack_light_distant(const LightTable &lt, int l) { return lt.kind != nullptr && lt.kind[l] == PSDR_LIGHT_DISTANT; }
template <int K> PSDR_HD PointLight stack_light(const LightTable &lt, int l) {
    PointLight pl{};
    for (int c = 0; c < 3; ++c) pl.p[c] = lt.pos[3 * l + c];
    if (lt.dpos != nullptr) {
        for (int k = 0; k < K; ++k)
            for (int c = 0; c < 3; ++c) pl.d[k][c] = lt.dpos[((size_t) k * lt.L + l) * 3 + c];
    }
    return pl;
}

// ---------------------------------------------------------------------------------------------------------------------- forward
// What the lights of one slot share: the hit and its BSDF id.  ok: a hit on a mesh with a BSDF.
template <class G> struct StackHit { Its<G> its; int bsdf_id; bool ok; };
// seeded as point_camera_sample, the same two jitter draws
template <class G, class TVT>
PSDR_HD StackHit<G> stack_camera_hit(const SceneView &sc, const TVT &tv, TraversalStack &st, const RngJump &jump, int pixel, uint64_t slot, uint32_t &nrays) {
    Rng rng; rng.init(slot, jump);
    const float j0 = rng.next(), j1 = rng.next();
    const int W = sc.d.width;
    const float sx = ((float) (pixel % W) + j0) / (float) W, sy = ((float) (pixel / W) + j1) / (float) sc.d.height;
    const RayT<G> ray = primary_ray<G>(sc, tv, sx, sy);
    StackHit<G> h;
    h.its = known_or_traced<false, G>(sc, tv, st, ray, true, nrays, nullptr);
    h.bsdf_id = h.its.valid ? Tab<TVT::flags>::mesh_bsdf(sc, h.its.mesh) : -1;
    h.ok = h.its.valid && h.bsdf_id >= 0;
    return h;
}
// the light part of li_point, non-finite components zeroed as point_camera_sample does
template <class G, class M, int LK = kLightPoint, class TVT>
PSDR_HD Vec3<M> stack_light_value(const SceneView &sc, const TVT &tv, TraversalStack &st, const Bsdf<G, M> &bsdf, const Its<G> &its, const PointLight &pl, uint32_t &nrays) {
    Vec3<G> dv, dn; G r2, r;
    light_from<LK>(pl, its.p, dv, dn, r2, r);
    const Vec3<G> wo = its.sh.to_local(dn);
    const Vec3<M> f = colloc_bsdf_eval<TVT::has_rough>(sc, tv, bsdf, its, wo);
    if (!point_light_visible<TVT::flags>(sc, st, val(its.p), val(dn), val(r), nrays)) return zero3<M>();
    if constexpr (LK == kLightDistant) return zero_nonfinite(f);
    else return zero_nonfinite(f * to_m<M>(1.f / r2));
}

// ---------------------------------------------------------------------------------------------------------------------- reverse
// The hit of one slot and the adjoints the lights add up in it
struct StackRevHit {
    bool ok, face0, lit;
    Hit h0;
    TriRow<float> T0;
    Its<float> its;
    ShNormal sn0;
    RayT<float> ray;
    float bu, bv, sx, sy;
    const float *q;
    int bsdf_id;
    VertexAdj va0;
    NormalMapAdj nx;
};
// point_sample_reverse up to the light: the primary ray, the walk and the hit (GEO: in its solid-angle form)
template <bool GEO, int FL>
PSDR_HD void stack_rev_begin(StackRevHit &H, const SceneView &sc, TraversalStack &st, const RngJump &jump, int pixel, uint64_t slot, uint32_t &nrays) {
    const TangentView<0, FL> tv0{};
    H.ok = H.lit = false; H.bsdf_id = -1;
    H.va0.clear(); H.nx.clear();
    Rng rng; rng.init(slot, jump);
    const float j0 = rng.next(), j1 = rng.next();
    const int W = sc.d.width;
    H.sx = ((float) (pixel % W) + j0) / (float) W; H.sy = ((float) (pixel / W) + j1) / (float) sc.d.height;
    H.ray = primary_ray<float>(sc, tv0, H.sx, H.sy);
    nrays++;
    H.h0 = closest_hit<false, tree_mode<FL>()>(sc, st, H.ray.o, H.ray.d, INFINITY, -1, -1, kPrePrimaryRay);
    if (H.h0.tri < 0) return;
    const int tm0 = Tab<FL>::tri_mesh(sc, H.h0.tri);
    H.face0 = (tm0 & PSDR_TRI_FACE_NORMALS) != 0;
    H.T0 = load_tri<float>(sc, tv0, H.h0.tri);
    float t0;
    Its<float> &its = H.its;
    if (GEO) {
        moeller_trumbore(H.T0.p0, H.T0.e1, H.T0.e2, H.ray, H.bu, H.bv, t0);          // solid-angle form (fill_its_from_hit)
        its.p = bary_point(H.T0.p0, H.T0.e1, H.T0.e2, H.bu, H.bv);
    } else {
        H.bu = H.h0.u; H.bv = H.h0.v;
        its.p = bary_point(H.T0.p0, H.T0.e1, H.T0.e2, H.bu, H.bv);
        t0 = norm(its.p - H.ray.o);
    }
    its.valid = true; its.tri = H.h0.tri; its.mesh = tm0 & ~PSDR_TRI_FACE_NORMALS; its.hu = H.h0.u; its.hv = H.h0.v;
    its.n = H.T0.fn; its.J = 1.f; its.t = t0;
    H.sn0 = shading_normal(H.T0, H.face0, H.bu, H.bv);
    its.sh = Frame<float>(H.sn0.n);
    its.wi = GEO ? its.sh.to_local(-H.ray.d) : its.sh.to_local(-((its.p - H.ray.o) / t0));
    H.q = sc.d.tri_uv ? Tab<FL>::tri_uv(sc, H.h0.tri) : nullptr;
    const float *q = H.q;
    its.uvx = q ? (q[2] - q[0]) * H.bu + ((q[4] - q[0]) * H.bv + q[0]) : 0.f;
    its.uvy = q ? (q[3] - q[1]) * H.bu + ((q[5] - q[1]) * H.bv + q[1]) : 0.f;
    H.bsdf_id = Tab<FL>::mesh_bsdf(sc, its.mesh);
    H.ok = H.bsdf_id >= 0;
}
// One light of a slot with H.ok.  adj = dLoss / d(pixel of this light's plane) / spp; returns the primal sample value; a_pl (+=): the light's gradient.
// sink: CameraSinkOf<GEO, RealSink> over the slot's PrimaryGrad pg (pg.tri: the hit's row, once a light reaches it); brev: BsdfRev<Sink> of H.bsdf_id.
template <bool GEO, int LK = kLightPoint, class Sink>
PSDR_HD Vec3f stack_rev_light(Sink &sink, PrimaryGrad &pg, const SceneView &sc, TraversalStack &st, const BsdfRev<Sink> &brev, StackRevHit &H, const PointLight &pl, const Vec3f &adj, uint32_t &nrays,
                              Vec3f &a_pl) {
    const TangentView<0, Sink::flags> tv0{};
    const Its<float> &its = H.its;
    Vec3f dv, dn; float r2, r;
    light_from<LK>(pl, its.p, dv, dn, r2, r);
    const float inv_r2 = LK == kLightDistant ? 1.f : 1.f / r2;
    const Vec3f wo = its.sh.to_local(dn);
    const Vec3f f = colloc_bsdf_eval<(Sink::flags & kSceneRough) != 0>(sc, tv0, brev.b, its, wo);
    if (!point_light_visible<Sink::flags>(sc, st, its.p, dn, r, nrays)) return Vec3f(0.f);
    H.lit = true;
    pg.tri = H.h0.tri;
    const Vec3f result = f * inv_r2;
    // masked(value, ~isfinite(value)) = 0, per component: a zeroed component has no gradient either
    const Vec3f a{isfinite(result.x) ? adj.x : 0.f, isfinite(result.y) ? adj.y : 0.f, isfinite(result.z) ? adj.z : 0.f};
    Vec3f a_wo(0.f);
    colloc_bsdf_eval_vjp(sink, sc, tv0, brev, its, wo, a * inv_r2, H.va0.wi, a_wo, H.va0.u, H.va0.v, H.nx);
    if (GEO) {
        // 1 / r^2 and wo = to_local(dn), dn = dv / r, dv = pL - p (distant: dn = dv / |dv|, dv = d)
        Vec3f a_dv(0.f);
        if constexpr (LK != kLightDistant) {
            const float a_r2 = -dot(a, zero_nonfinite(f)) * inv_r2 * inv_r2;
            a_dv = dv * (2.f * a_r2);
        }
        const Vec3f a_dn = its.sh.s * a_wo.x + its.sh.t * a_wo.y + its.sh.n * a_wo.z;
        acc(H.va0.s, dn * a_wo.x); acc(H.va0.t, dn * a_wo.y); acc(H.va0.n, dn * a_wo.z);
        acc_finite(a_dv, normalize_vjp(dv, dn, a_dn));
        acc_finite(a_pl, a_dv);
        if constexpr (LK != kLightDistant) acc(H.va0.p, -a_dv);
    }
    return zero_nonfinite(result);
}
// The hit's adjoint chain, once, on what the lights added up (the part of point_sample_reverse behind the a_wo chain)
template <bool GEO, class Sink>
PSDR_HD void stack_rev_end(Sink &sink, const SceneView &sc, StackRevHit &H) {
    if (!GEO || !(H.ok && H.lit)) return;
    constexpr bool kNormalMaps = (Sink::flags & kSceneRough) != 0;
    const Its<float> &its = H.its;
    VertexAdj &va0 = H.va0;
    const NormalMapAdj &nx = H.nx;
    const float *q = H.q;
    // the primary vertex: wi = to_local(-d), frame(sh_n(bu, bv)), uv(bu, bv), p = p0 + bu e1 + bv e2, (bu, bv, t) = MT(tri0, ray)
    const Vec3f dcam = camera_space_dir(sc, H.sx, H.sy);
    const Vec3f a_d = -(its.sh.s * va0.wi.x + its.sh.t * va0.wi.y + its.sh.n * va0.wi.z);
    acc(va0.s, H.ray.d * (-va0.wi.x)); acc(va0.t, H.ray.d * (-va0.wi.y)); acc(va0.n, H.ray.d * (-va0.wi.z));
    if constexpr (kNormalMaps) { if (nx.on) { acc(va0.s, nx.s); acc(va0.t, nx.t); acc(va0.n, nx.n); } }
    const Vec3f a_shn = va0.n + frame_vjp(H.sn0.n, va0.s, va0.t);
    float abu = dot(va0.p, H.T0.e1), abv = dot(va0.p, H.T0.e2);
    shading_normal_vjp(sink, H.h0.tri, H.T0, H.sn0, H.bu, H.bv, a_shn, abu, abv);
    if (q) { abu += va0.u * (q[2] - q[0]) + va0.v * (q[3] - q[1]); abv += va0.u * (q[4] - q[0]) + va0.v * (q[5] - q[1]); }
    const MtAdj ma = mt_vjp(H.T0.p0, H.T0.e1, H.T0.e2, H.ray, abu, abv, 0.f);
    Vec3f a_e1 = ma.e1 + va0.p * H.bu, a_e2 = ma.e2 + va0.p * H.bv;
    if constexpr (kNormalMaps) { if (nx.on) { acc(a_e1, nx.e1); acc(a_e2, nx.e2); } }          // ... and dp_du of the tangent frame
    scatter_vec(sink, H.h0.tri, 0, ma.p0 + va0.p); scatter_vec(sink, H.h0.tri, 3, a_e1); scatter_vec(sink, H.h0.tri, 6, a_e2);
    camera_ray_vjp(sink, sc, dcam, ma.o, a_d + ma.d);
}

}  // namespace psdr
