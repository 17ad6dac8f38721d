// psdr_collocated.h -- CollocatedIntegrator (PSDR_INTEGRATOR_COLLOCATED, include/psdr_hip.h): a point light at the camera position.  Build-defined, like the
// PathTracer: the reference snapshot has no such integrator.  For a camera ray with origin o that hits `its`
//     Li = f(its; wi = its.wi, wo = its.wi) / |its.p - o|^2          (0 on a miss)
// with f = Bsdf::eval as the other integrators call it (cosine included), in the shading frame the hit carries.  Unit intensity: the caller scales the
// images (psdr_cuda/integrator.py).  Emitters add nothing -- no Le, no emitter sampling -- and no number is drawn beyond the film jitter: two per camera
// slot, one per primary-edge slot.  A point seen from the camera is seen from the light, so no shadow boundary is ever visible: the geometry gradient is
// the interior term and the primary-edge term, there is no secondary-edge term.
// ONE copy of the estimator: the forward kernels (value and dual numbers), the reverse kernels (psdr_collocated.hip) and the host harness
// (tests/hostcheck/hostcheck_collocated.cpp) instantiate the functions below.
#pragma once
#include "psdr_reverse.h"
#include "psdr_colloc_microfacet.h"

namespace psdr {

// Li of one camera ray.  G: geometry type (Dual<K>: the solid-angle form of the hit, as Li's), M: material / result type.
template <class G, class M, bool KNOWN = false, class TVT>
PSDR_HD Vec3<M> li_collocated(const SceneView &sc, const TVT &tv, TraversalStack &st, const RayT<G> &ray, bool active, uint32_t &nrays, const Hit *primary = nullptr) {
    const Its<G> its = known_or_traced<KNOWN, G>(sc, tv, st, ray, active, nrays, primary);
    if (!(active && its.valid)) return zero3<M>();
    const int bsdf_id = Tab<TVT::flags>::mesh_bsdf(sc, its.mesh);
    if (bsdf_id < 0) return zero3<M>();          // the bounding mesh of an environment map has no BSDF
    const Bsdf<G, M> bsdf(sc, tv, bsdf_id);
    const Vec3<M> f = colloc_bsdf_eval<TVT::has_rough>(sc, tv, bsdf, its, its.wi);          // MicrofacetBSDF by the record's type (psdr_colloc_microfacet.h)
    const Vec3<G> dv = its.p - ray.o;
    const G inv_d2 = 1.f / dot(dv, dv);
    return f * to_m<M>(inv_d2);
}

// One camera sample slot (camera_sample's counterpart)
template <class G, class M, class TVT>
PSDR_HD Vec3<M> collocated_camera_sample(const SceneView &sc, const TVT &tv, TraversalStack &st, const RngJump &jump, int pixel, uint64_t slot, uint32_t &nrays) {
    Rng rng; rng.init(slot, jump);
    const float j0 = rng.next(), j1 = rng.next();
    const int W = sc.d.width;
    const float sx = ((float) (pixel % W) + j0) / (float) W, sy = ((float) (pixel / W) + j1) / (float) sc.d.height;
    const RayT<G> ray = primary_ray<G>(sc, tv, sx, sy);
    return zero_nonfinite(li_collocated<G, M>(sc, tv, st, ray, true, nrays));
}

// One primary-edge slot up to the difference of Li across the edge (primary_edge_sample / primary_edge_reverse_values with this estimator): what forward and
// reverse mode share.  false: the slot contributes nothing.
// LiOf: the estimator on the two sides, at<KNOWN>(...) = Li of one camera ray -- this integrator's, or the PointLightIntegrator's (psdr_pointlight.h)
struct CollocatedEdge { int k, pixel; float u, nx, ny, xdn; float dL[3]; };
struct CollocatedLi {
    template <bool KNOWN, class TVT>
    PSDR_HD Vec3f at(const SceneView &sc, const TVT &tv0, TraversalStack &st, const RayT<float> &ray, bool active, uint32_t &nrays, const Hit *primary) const {
        return li_collocated<float, float, KNOWN>(sc, tv0, st, ray, active, nrays, primary);
    }
};
template <int FL, class LiOf = CollocatedLi>
PSDR_HD bool collocated_edge_values(const SceneView &sc, TraversalStack &st, const RngJump &jump, uint64_t slot, uint32_t &nrays, CollocatedEdge &e, const LiOf &li = LiOf()) {
    Rng rng; rng.init(slot, jump);
    float u = rng.next(), pmf;
    const int k = sample_reuse(sc.d.prim_cmf, sc.d.prim_pmf, sc.d.prim_sum, sc.d.num_prim_edges, u, pmf);
    const float *pe = sc.d.prim_edge + (size_t) k * PSDR_PEDGE_STRIDE;
    const float nx = pe[4], ny = pe[5], pdf = pmf / pe[6];
    const float px = pe[0] * (1.f - u) + pe[2] * u, py = pe[1] * (1.f - u) + pe[3] * u;
    const int W = sc.d.width, H = sc.d.height;
    const int ix = (int) floorf(px * (float) W), iy = (int) floorf(py * (float) H);
    bool valid = ix >= 0 && ix < W && iy >= 0 && iy < H && pmf > 0.f && pe[6] > 0.f;          // (pmf > 0, length > 0: see primary_edge_sample)
    const TangentView<0, FL> tv0{};
    if (sc.d.prim_edge_z != nullptr && valid) valid = primary_edge_point_visible(sc, tv0, st, k, u, px, py, nrays);
    // Li on the two sides of the edge (ray_n first, then ray_p); one loop body, so the estimator is instantiated once
    Vec3f Ln(0.f), Lp(0.f);
    Hit hp0, hp1;
    hp0.tri = hp1.tri = -1; hp0.u = hp0.v = hp0.t = hp1.u = hp1.v = hp1.t = 0.f;
    // two-level scenes: both camera rays through ONE walk (closest_hit_pair), then the estimator on each side's known hit
    if constexpr (pair_walk_ok<FL>()) { if (valid) primary_edge_camera_hits(sc, tv0, st, px, py, nx, ny, hp0, hp1); }
#pragma unroll 1
    for (int side = 0; side < 2; ++side) {
        const float sg = side == 0 ? -kEdgeEpsilon : kEdgeEpsilon;
        const RayT<float> ray = primary_ray<float>(sc, tv0, px + sg * nx, py + sg * ny);
        Vec3f L;
        // (this integrator's own Li is called as it always was: through the functor the two-level rough unit compiled to other code)
        if constexpr (std::is_same<LiOf, CollocatedLi>::value) {
            if constexpr (pair_walk_ok<FL>()) { const Hit hs = side == 0 ? hp0 : hp1; L = li_collocated<float, float, true>(sc, tv0, st, ray, valid, nrays, &hs); }
            else L = li_collocated<float, float>(sc, tv0, st, ray, valid, nrays);
        } else {
            if constexpr (pair_walk_ok<FL>()) { const Hit hs = side == 0 ? hp0 : hp1; L = li.template at<true>(sc, tv0, st, ray, valid, nrays, &hs); }
            else L = li.template at<false>(sc, tv0, st, ray, valid, nrays, nullptr);
        }
        if (side == 0) Ln = L; else Lp = L;
    }
    if (!valid) return false;
    e.k = k; e.pixel = iy * W + ix; e.u = u; e.nx = nx; e.ny = ny; e.xdn = px * nx + py * ny;
    e.dL[0] = (Ln.x - Lp.x) / pdf; e.dL[1] = (Ln.y - Lp.y) / pdf; e.dL[2] = (Ln.z - Lp.z) / pdf;
    return true;
}
// forward mode: returns the pixel (or -1), tan[k][c] = d value / d P_k
template <int K, int FL, class LiOf = CollocatedLi>
PSDR_HD int collocated_edge_sample(const SceneView &sc, const TangentView<K, FL> &tv, TraversalStack &st, const RngJump &jump, uint64_t slot, float inv_sppe,
                                   float tan[K][3], uint32_t &nrays, const LiOf &li = LiOf()) {
    CollocatedEdge e;
    if (!collocated_edge_values<FL>(sc, st, jump, slot, nrays, e, li)) return -1;
    const bool fin[3] = {isfinite(e.xdn * e.dL[0]), isfinite(e.xdn * e.dL[1]), isfinite(e.xdn * e.dL[2])};
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const float *dp = tv.t[t].d_prim_edge ? tv.t[t].d_prim_edge + (size_t) e.k * PSDR_PEDGE_STRIDE : nullptr;
        const float dxdn = dp ? ((dp[0] * (1.f - e.u) + dp[2] * e.u) * e.nx + (dp[1] * (1.f - e.u) + dp[3] * e.u) * e.ny) : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float g = dxdn * e.dL[c]; tan[t][c] = (fin[c] && isfinite(g)) ? g * inv_sppe : 0.f; }
    }
    return e.pixel;
}
// reverse mode: returns the edge (or -1) and w[4] = the gradient of its (p0.x, p0.y, p1.x, p1.y) words
template <int FL, class LiOf = CollocatedLi>
PSDR_HD int collocated_edge_reverse_values(const SceneView &sc, TraversalStack &st, const RngJump &jump, uint64_t slot, float inv_sppe,
                                           const float *__restrict__ adj_img, uint32_t &nrays, float w[4], const LiOf &li = LiOf()) {
    w[0] = w[1] = w[2] = w[3] = 0.f;
    CollocatedEdge e;
    if (!collocated_edge_values<FL>(sc, st, jump, slot, nrays, e, li)) return -1;
    const float *a = adj_img + (size_t) e.pixel * 3;
    float g = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) if (isfinite(e.xdn * e.dL[c])) g += a[c] * e.dL[c];
    g *= inv_sppe;
    if (g == 0.f || !isfinite(g)) return -1;
    w[0] = g * (1.f - e.u) * e.nx; w[1] = g * (1.f - e.u) * e.ny; w[2] = g * e.u * e.nx; w[3] = g * e.u * e.ny;
    return e.k;
}

// One camera sample in reverse mode (camera_sample_reverse's counterpart).  adj = dLoss / d(pixel) / spp; returns the primal sample value.
//   GEO: a geometry gradient (triangle table / camera) is wanted -> the solid-angle form of the hit and its adjoint chain; otherwise the on-surface
//        form, exactly like forward mode, and every geometry adjoint is compiled out (MaterialSink)
// The primary triangle's row adjoint comes back in pg (PrimarySink), for the caller to sum across the lanes that share the triangle.
template <bool GEO, class RealSink>
PSDR_HD Vec3f collocated_sample_reverse(RealSink &real_sink, PrimaryGrad &pg, const SceneView &sc, TraversalStack &st, const RngJump &jump, int pixel, uint64_t slot,
                                        const Vec3f &adj, uint32_t &nrays) {
    pg.clear();
    using Sink = typename CameraSinkOf<GEO, RealSink>::type;
    Sink sink(real_sink, pg);
    const TangentView<0, Sink::flags> tv0{};
    Rng rng; rng.init(slot, jump);
    const float j0 = rng.next(), j1 = rng.next();
    const int W = sc.d.width;
    const float sx = ((float) (pixel % W) + j0) / (float) W, sy = ((float) (pixel / W) + j1) / (float) sc.d.height;
    const RayT<float> ray = primary_ray<float>(sc, tv0, sx, sy);
    nrays++;
    const Hit h0 = closest_hit<false, tree_mode<RealSink::flags>()>(sc, st, ray.o, ray.d, INFINITY, -1, -1, kPrePrimaryRay);
    if (h0.tri < 0) return Vec3f(0.f);
    pg.tri = h0.tri;
    const int tm0 = Tab<RealSink::flags>::tri_mesh(sc, h0.tri);
    const bool face0 = (tm0 & PSDR_TRI_FACE_NORMALS) != 0;
    const TriRow<float> T0 = load_tri<float>(sc, tv0, h0.tri);
    float bu, bv, t0;
    Its<float> its;
    if (GEO) {
        moeller_trumbore(T0.p0, T0.e1, T0.e2, ray, bu, bv, t0);          // solid-angle form (fill_its_from_hit)
        its.p = bary_point(T0.p0, T0.e1, T0.e2, bu, bv);
    } else {
        bu = h0.u; bv = h0.v;
        its.p = bary_point(T0.p0, T0.e1, T0.e2, bu, bv);
        t0 = norm(its.p - ray.o);
    }
    its.valid = true; its.tri = h0.tri; its.mesh = tm0 & ~PSDR_TRI_FACE_NORMALS; its.hu = h0.u; its.hv = h0.v;
    its.n = T0.fn; its.J = 1.f; its.t = t0;
    const ShNormal sn0 = shading_normal(T0, face0, bu, bv);
    its.sh = Frame<float>(sn0.n);
    its.wi = GEO ? its.sh.to_local(-ray.d) : its.sh.to_local(-((its.p - ray.o) / t0));
    const float *q = sc.d.tri_uv ? Tab<RealSink::flags>::tri_uv(sc, h0.tri) : nullptr;
    its.uvx = q ? (q[2] - q[0]) * bu + ((q[4] - q[0]) * bv + q[0]) : 0.f;
    its.uvy = q ? (q[3] - q[1]) * bu + ((q[5] - q[1]) * bv + q[1]) : 0.f;

    const int bsdf_id = Tab<RealSink::flags>::mesh_bsdf(sc, its.mesh);
    if (bsdf_id < 0) return Vec3f(0.f);
    BsdfRev<Sink> brev(sc, bsdf_id);
    const Vec3f f = colloc_bsdf_eval<(Sink::flags & kSceneRough) != 0>(sc, tv0, brev.b, its, its.wi);
    const Vec3f dv = its.p - ray.o;
    const float inv_d2 = 1.f / dot(dv, dv);
    const Vec3f result = f * inv_d2;
    // masked(value, ~isfinite(value)) = 0, per component: a zeroed component has no gradient either
    const Vec3f a{isfinite(result.x) ? adj.x : 0.f, isfinite(result.y) ? adj.y : 0.f, isfinite(result.z) ? adj.z : 0.f};
    VertexAdj va0; va0.clear();
    Vec3f a_wo(0.f);
    NormalMapAdj nx; nx.clear();                                         // a normal- or height-mapped MicrofacetBSDF: adjoints of the shading frame and of e1, e2 (dp_du / p_u, p_v)
    colloc_bsdf_eval_vjp(sink, sc, tv0, brev, its, its.wi, a * inv_d2, va0.wi, a_wo, va0.u, va0.v, nx);
    acc(va0.wi, a_wo);                                                   // wo = wi
    constexpr bool kNormalMaps = (Sink::flags & kSceneRough) != 0;       // (the type is compiled into the rough flag sets only)
    if (GEO) {
        // 1 / |p - o|^2, then the primary vertex: wi = to_local(-d), frame(sh_n(bu, bv)), uv(bu, bv), p = p0 + bu e1 + bv e2, (bu, bv, t) = MT(tri0, ray)
        const float a_d2 = -dot(a, zero_nonfinite(f)) * inv_d2 * inv_d2;
        const Vec3f a_dv = dv * (2.f * a_d2);
        acc(va0.p, a_dv);
        const Vec3f dcam = camera_space_dir(sc, sx, sy);
        const Vec3f a_d = -(its.sh.s * va0.wi.x + its.sh.t * va0.wi.y + its.sh.n * va0.wi.z);
        acc(va0.s, ray.d * (-va0.wi.x)); acc(va0.t, ray.d * (-va0.wi.y)); acc(va0.n, ray.d * (-va0.wi.z));
        if constexpr (kNormalMaps) { if (nx.on) { acc(va0.s, nx.s); acc(va0.t, nx.t); acc(va0.n, nx.n); } }
        const Vec3f a_shn = va0.n + frame_vjp(sn0.n, va0.s, va0.t);
        float abu = dot(va0.p, T0.e1), abv = dot(va0.p, T0.e2);
        shading_normal_vjp(sink, h0.tri, T0, sn0, bu, bv, a_shn, abu, abv);
        if (q) { abu += va0.u * (q[2] - q[0]) + va0.v * (q[3] - q[1]); abv += va0.u * (q[4] - q[0]) + va0.v * (q[5] - q[1]); }
        const MtAdj ma = mt_vjp(T0.p0, T0.e1, T0.e2, ray, abu, abv, 0.f);
        if constexpr (kNormalMaps) {          // ... and dp_du of the tangent frame
            Vec3f a_e1 = ma.e1 + va0.p * bu, a_e2 = ma.e2 + va0.p * bv;
            if (nx.on) { acc(a_e1, nx.e1); acc(a_e2, nx.e2); }
            scatter_vec(sink, h0.tri, 0, ma.p0 + va0.p); scatter_vec(sink, h0.tri, 3, a_e1); scatter_vec(sink, h0.tri, 6, a_e2);
        } else {
            scatter_vec(sink, h0.tri, 0, ma.p0 + va0.p); scatter_vec(sink, h0.tri, 3, ma.e1 + va0.p * bu); scatter_vec(sink, h0.tri, 6, ma.e2 + va0.p * bv);
        }
        camera_ray_vjp(sink, sc, dcam, ma.o - a_dv, a_d + ma.d);
    }
    return zero_nonfinite(result);
}

}  // namespace psdr
