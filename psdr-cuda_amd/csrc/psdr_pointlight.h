// psdr_pointlight.h -- PointLightIntegrator (PSDR_INTEGRATOR_POINT, include/psdr_hip.h): a point light at an arbitrary, differentiable world position pL.
// Build-defined, like the CollocatedIntegrator it generalises: the reference snapshot has no such integrator.  For a camera ray that hits `its`, with
// dv = pL - its.p, r^2 = dot(dv, dv) and wo = its.sh.to_local(dv / r)
//     Li = f(its; wi = its.wi, wo) * V(its.p, pL) / r^2          (0 on a miss)
// with f = colloc_bsdf_eval (cosine included) and V = 1 unless the walk finds a hit with t in [RayEpsilon, r - ShadowEpsilon) on the ray from its.p towards pL.
// Unit intensity: the caller scales the images (psdr_cuda/integrator.py).  Emitters add nothing.  Draws per slot: two per camera slot, one per primary-edge
// slot, three per shadow-boundary slot (the first is used).
// The geometry gradient has three terms: the interior (dual numbers through its.p, the frame, wi, wo, r^2 and pL), the primary edges (collocated_edge_values
// with this Li on both sides) and the boundary of the moving shadow outline (point_sedge_*), which the collocated configuration never sees.
// ONE copy of the estimator: the forward kernels, the reverse kernels (psdr_pointlight.hip) and the host harnesses (tests/hostcheck/hostcheck_pointlight.cpp,
// hostcheck_distantlight.cpp) instantiate the functions below.
// The light model is a compile-time parameter LK of them (include/psdr_hip.h: PSDR_LIGHT_POINT, the default, is the text above).  PSDR_LIGHT_DISTANT: the
// PointLight's vector is a direction d from the scene TOWARDS the light, of any length; with u = d / |d| and wo = its.sh.to_local(u)
//     Li = f(its; wi = its.wi, wo) * V(its.p, u)                 (0 on a miss)
// V = 1 unless the walk finds a hit with t in [RayEpsilon, inf) on the ray (its.p, u); no falloff: unit IRRADIANCE on a surface that faces the light, so a
// point light at c + R u with intensity R^2 tends to this model.  The gradient is that of d as passed: tangential, and 1 / |d| in size.  The shadow
// boundary is a parallel projection (point_sedge_values).
#pragma once
#include "psdr_collocated.h"

namespace psdr {

// The light as the kernels receive it: position (PSDR_LIGHT_DISTANT: direction towards the light) and, in forward mode, its K tangents (zero otherwise)
struct PointLight { float p[3]; float d[3][3]; };
constexpr int kLightPoint = PSDR_LIGHT_POINT, kLightDistant = PSDR_LIGHT_DISTANT;
template <class G> PSDR_HD Vec3<G> point_light_pos(const PointLight &pl) {
    Vec3<G> p = lift<G>(Vec3f{pl.p[0], pl.p[1], pl.p[2]});
    if constexpr (is_ad<G>()) {
#pragma unroll
        for (int k = 0; k < ad_traits<G>::K; ++k) { p.x.d[k] = pl.d[k][0]; p.y.d[k] = pl.d[k][1]; p.z.d[k] = pl.d[k][2]; }
    }
    return p;
}
// V(p, pL) for the unit direction d0 = (pL - p) / r: nothing in [RayEpsilon, r - ShadowEpsilon) (the tmax form of primary_edge_point_visible)
template <int FL>
PSDR_HD bool point_light_visible(const SceneView &sc, TraversalStack &st, const Vec3f &p, const Vec3f &d0, float r, uint32_t &nrays) {
    nrays++;
    return closest_hit<false, tree_mode<FL>()>(sc, st, p, d0, r - kShadowEpsilon).tri < 0;
}

// The light seen from p: the unit direction dn towards it, the far end tmax of the visibility ray and, for the point model alone, dv = pL - p and r^2
// (the distant model leaves dv = d, for normalize_vjp, and r2 unset)
template <int LK, class G> PSDR_HD void light_from(const PointLight &pl, const Vec3<G> &p, Vec3<G> &dv, Vec3<G> &dn, G &r2, G &r) {
    if constexpr (LK == kLightDistant) {
        dv = point_light_pos<G>(pl);
        dn = normalize(dv);
        r = G(INFINITY);
    } else {
        dv = point_light_pos<G>(pl) - p;
        r2 = dot(dv, dv);
        r = sqrt_(r2);
        dn = dv / r;
    }
}

// Li of one camera ray.  G: geometry type (Dual<K>: the solid-angle form of the hit, and the light's tangents), M: material / result type.
template <class G, class M, bool KNOWN = false, int LK = kLightPoint, class TVT>
PSDR_HD Vec3<M> li_point(const SceneView &sc, const TVT &tv, TraversalStack &st, const PointLight &pl, const RayT<G> &ray, bool active, uint32_t &nrays, const Hit *primary = nullptr) {
    const Its<G> its = known_or_traced<KNOWN, G>(sc, tv, st, ray, active, nrays, primary);
    if (!(active && its.valid)) return zero3<M>();
    const int bsdf_id = Tab<TVT::flags>::mesh_bsdf(sc, its.mesh);
    if (bsdf_id < 0) return zero3<M>();          // the bounding mesh of an environment map has no BSDF
    Vec3<G> dv, dn; G r2, r;
    light_from<LK>(pl, its.p, dv, dn, r2, r);
    const Vec3<G> wo = its.sh.to_local(dn);
    const Bsdf<G, M> bsdf(sc, tv, bsdf_id);
    const Vec3<M> f = colloc_bsdf_eval<TVT::has_rough>(sc, tv, bsdf, its, wo);
    if (!point_light_visible<TVT::flags>(sc, st, val(its.p), val(dn), val(r), nrays)) return zero3<M>();
    if constexpr (LK == kLightDistant) return f;
    else return f * to_m<M>(1.f / r2);
}

// One camera sample slot (collocated_camera_sample's counterpart)
template <class G, class M, int LK = kLightPoint, class TVT>
PSDR_HD Vec3<M> point_camera_sample(const SceneView &sc, const TVT &tv, TraversalStack &st, const PointLight &pl, const RngJump &jump, int pixel, uint64_t slot, uint32_t &nrays) {
    Rng rng; rng.init(slot, jump);
    const float j0 = rng.next(), j1 = rng.next();
    const int W = sc.d.width;
    const float sx = ((float) (pixel % W) + j0) / (float) W, sy = ((float) (pixel / W) + j1) / (float) sc.d.height;
    const RayT<G> ray = primary_ray<G>(sc, tv, sx, sy);
    return zero_nonfinite(li_point<G, M, false, LK>(sc, tv, st, pl, ray, true, nrays));
}

// The Li of the primary-edge term: collocated_edge_values / _sample / _reverse_values (psdr_collocated.h) take it as their LiOf
template <int LK> struct PointLiOf {
    PointLight pl;
    template <bool KNOWN, class TVT>
    PSDR_HD Vec3f at(const SceneView &sc, const TVT &tv0, TraversalStack &st, const RayT<float> &ray, bool active, uint32_t &nrays, const Hit *primary) const {
        return li_point<float, float, KNOWN, LK>(sc, tv0, st, pl, ray, active, nrays, primary);
    }
};
using PointLi = PointLiOf<kLightPoint>;

// One camera sample in reverse mode (collocated_sample_reverse's sibling).  adj = dLoss / d(pixel) / spp; returns the primal sample value.
//   GEO: a geometry gradient (triangle table / camera / light position) is wanted -> the solid-angle form of the hit and its adjoint chain
// The a_wo that colloc_bsdf_eval_vjp returns goes through wo = to_local(dv / r) to its.p, the frame and pL (a_pl, +=); under the distant model through
// wo = to_local(d / |d|) to the frame and d (a_pl, +=: tangential, 1 / |d| in size), and nothing reaches its.p.
template <bool GEO, int LK = kLightPoint, class RealSink>
PSDR_HD Vec3f point_sample_reverse(RealSink &real_sink, PrimaryGrad &pg, const SceneView &sc, TraversalStack &st, const PointLight &pl, const RngJump &jump, int pixel, uint64_t slot,
                                   const Vec3f &adj, uint32_t &nrays, Vec3f &a_pl) {
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
    Vec3f dv, dn; float r2, r;
    light_from<LK>(pl, its.p, dv, dn, r2, r);
    const float inv_r2 = LK == kLightDistant ? 1.f : 1.f / r2;
    const Vec3f wo = its.sh.to_local(dn);
    BsdfRev<Sink> brev(sc, bsdf_id);
    const Vec3f f = colloc_bsdf_eval<(Sink::flags & kSceneRough) != 0>(sc, tv0, brev.b, its, wo);
    if (!point_light_visible<RealSink::flags>(sc, st, its.p, dn, r, nrays)) return Vec3f(0.f);
    pg.tri = h0.tri;
    const Vec3f result = f * inv_r2;
    // masked(value, ~isfinite(value)) = 0, per component: a zeroed component has no gradient either
    const Vec3f a{isfinite(result.x) ? adj.x : 0.f, isfinite(result.y) ? adj.y : 0.f, isfinite(result.z) ? adj.z : 0.f};
    VertexAdj va0; va0.clear();
    Vec3f a_wo(0.f);
    NormalMapAdj nx; nx.clear();                                         // a normal- or height-mapped MicrofacetBSDF: adjoints of the shading frame and of e1, e2
    colloc_bsdf_eval_vjp(sink, sc, tv0, brev, its, wo, a * inv_r2, va0.wi, a_wo, va0.u, va0.v, nx);
    constexpr bool kNormalMaps = (Sink::flags & kSceneRough) != 0;       // (the type is compiled into the rough flag sets only)
    if (GEO) {
        // 1 / r^2 and wo = to_local(dn), dn = dv / r, dv = pL - p (distant: dn = dv / |dv|, dv = d)
        Vec3f a_dv(0.f);
        if constexpr (LK != kLightDistant) {
            const float a_r2 = -dot(a, zero_nonfinite(f)) * inv_r2 * inv_r2;
            a_dv = dv * (2.f * a_r2);
        }
        const Vec3f a_dn = its.sh.s * a_wo.x + its.sh.t * a_wo.y + its.sh.n * a_wo.z;
        acc(va0.s, dn * a_wo.x); acc(va0.t, dn * a_wo.y); acc(va0.n, dn * a_wo.z);
        acc_finite(a_dv, normalize_vjp(dv, dn, a_dn));
        acc_finite(a_pl, a_dv);
        if constexpr (LK != kLightDistant) acc(va0.p, -a_dv);
        // the primary vertex: wi = to_local(-d), frame(sh_n(bu, bv)), uv(bu, bv), p = p0 + bu e1 + bv e2, (bu, bv, t) = MT(tri0, ray)
        const Vec3f dcam = camera_space_dir(sc, sx, sy);
        const Vec3f a_d = -(its.sh.s * va0.wi.x + its.sh.t * va0.wi.y + its.sh.n * va0.wi.z);
        acc(va0.s, ray.d * (-va0.wi.x)); acc(va0.t, ray.d * (-va0.wi.y)); acc(va0.n, ray.d * (-va0.wi.z));
        if constexpr (kNormalMaps) { if (nx.on) { acc(va0.s, nx.s); acc(va0.t, nx.t); acc(va0.n, nx.n); } }
        const Vec3f a_shn = va0.n + frame_vjp(sn0.n, va0.s, va0.t);
        float abu = dot(va0.p, T0.e1), abv = dot(va0.p, T0.e2);
        shading_normal_vjp(sink, h0.tri, T0, sn0, bu, bv, a_shn, abu, abv);
        if (q) { abu += va0.u * (q[2] - q[0]) + va0.v * (q[3] - q[1]); abv += va0.u * (q[4] - q[0]) + va0.v * (q[5] - q[1]); }
        const MtAdj ma = mt_vjp(T0.p0, T0.e1, T0.e2, ray, abu, abv, 0.f);
        Vec3f a_e1 = ma.e1 + va0.p * bu, a_e2 = ma.e2 + va0.p * bv;
        if constexpr (kNormalMaps) { if (nx.on) { acc(a_e1, nx.e1); acc(a_e2, nx.e2); } }          // ... and dp_du of the tangent frame
        scatter_vec(sink, h0.tri, 0, ma.p0 + va0.p); scatter_vec(sink, h0.tri, 3, a_e1); scatter_vec(sink, h0.tri, 6, a_e2);
        camera_ray_vjp(sink, sc, dcam, ma.o, a_d + ma.d);
    }
    return zero_nonfinite(result);
}

// ---------------------------------------------------------------------------------------------------------------------- the shadow boundary
// One slot of sampler 2.  Edge k and the point xB = p0 + s1 e1 by sample_reuse over sec_cmf / sec_pmf (pdf = pmf / |e1|); the boundary segment runs from pL
// through xB onto the surface point xD, which the camera must see.  The outline of the shadow on the receiver is the projection of the edge from pL:
// an edge element dl maps to (rD / rB) (sinphi / sinphi2) dl of outline, and the outline moves along n (in the receiver's plane) with d dot(n, x(u, v)),
// (u, v) = Moeller-Trumbore of the ray pL -> xB against the triangle at xD.  What crosses the outline is the image's density per receiver area,
//     sensor_val * |dot(to camera, nD)| * f(xD; wi = to the camera, wo = to pL) / rD^2
// (sample_direct's sensor_val is per solid angle of the camera: the cosine at xD turns it into a density per area; f carries the shading cosine to the
// light, as in Li, so the shading-normal factor of secondary_edge_sample reduces to that geometric cosine).
// PSDR_LIGHT_DISTANT: the projection is parallel, along -u.  The segment runs from infinity through xB onto xD; an edge element maps to (sinphi / sinphi2) dl
// of outline (rD / rB -> 1, and the 1 / rD^2 is gone with the falloff); (u, v) = Moeller-Trumbore of the ray (xB, -u), so the outline moves with the edge
// row through the ray's ORIGIN and with d through its direction -- a different Jacobian and a different motion term, not a limit of the ones above.
// What forward and reverse mode share; false: the slot contributes nothing.
struct PointSedge { int k, pixel, tri; float s1; Vec3f xB, n; float value0[3]; };
template <int FL, int LK = kLightPoint>
PSDR_HD bool point_sedge_values(const SceneView &sc, TraversalStack &st, const PointLight &pl, const float s3[3], uint32_t &nrays, PointSedge &r) {
    const TangentView<0, FL> tv0{};
    float s1 = s3[0], pmf;
    const int k = sample_reuse(sc.d.sec_cmf, sc.d.sec_pmf, sc.d.sec_sum, sc.d.num_sec_edges, s1, pmf);
    const float *se = sc.d.sec_edge + (size_t) k * PSDR_SEDGE_STRIDE;
    const Vec3f ep0{se[0], se[1], se[2]}, ee1{se[3], se[4], se[5]}, n0{se[6], se[7], se[8]}, n1{se[9], se[10], se[11]}, ep2{se[12], se[13], se[14]};
    const bool is_boundary = se[15] != 0.f;
    const Vec3f xB = ee1 * s1 + ep0;
    const float e1len = norm(ee1);
    if (!(pmf > 0.f && e1len > 0.f)) return false;          // a dropped row of a capacity table
    const Vec3f edge = ee1 / e1len, edge2 = ep2 - ep0;
    const float pdf = pmf / e1len;
    const Vec3f pL = point_light_pos<float>(pl);          // (distant: d)
    Vec3f dir; float rB;
    if constexpr (LK == kLightDistant) { dir = -normalize(pL); rB = INFINITY; }
    else { const Vec3f wv = xB - pL; rB = norm(wv); dir = wv / rB; }
    // the silhouette test of boundary_segment_direct with e = -dir
    const Vec3f e = -dir;
    const float d0n = dot(n0, e), d1n = dot(n1, e);
    const int sgn0 = d0n > kEdgeEpsilon ? 1 : (d0n < -kEdgeEpsilon ? -1 : 0), sgn1 = d1n > kEdgeEpsilon ? 1 : (d1n < -kEdgeEpsilon ? -1 : 0);
    if (!(rB > kShadowEpsilon && (is_boundary ? sgn0 != 0 : sgn0 * sgn1 < 0))) return false;
    const bool skip = sc.d.sec_edge_faces != nullptr;
    const int f0 = skip ? sc.d.sec_edge_faces[2 * k] : -1, f1 = skip ? sc.d.sec_edge_faces[2 * k + 1] : -1;
    // pL -> xB unoccluded (the edge's own faces left out; distant: xB towards the light, to infinity), then on from xB onto a surface
    nrays++;
    const Vec3f bo = LK == kLightDistant ? xB : pL, bd = LK == kLightDistant ? e : dir;
    const Hit hb = (f0 >= 0 || f1 >= 0) ? closest_hit<true, tree_mode<FL>()>(sc, st, bo, bd, rB - kShadowEpsilon, f0, f1)
                                        : closest_hit<false, tree_mode<FL>()>(sc, st, bo, bd, rB - kShadowEpsilon);
    if (hb.tri >= 0) return false;
    const Its<float> itsD = intersect<float>(sc, tv0, st, RayT<float>{xB, dir}, true, kDetached, nrays, f0, f1);
    if (!itsD.valid) return false;
    const Vec3f xD = itsD.p;
    int pixel; float qx, qy, sensor_val;
    if (!sample_direct(sc, xD, pixel, qx, qy, sensor_val)) return false;
    // the camera sees xD (secondary_edge_sample's test, in double)
    const RayT<float> cam = primary_ray<float>(sc, tv0, qx, qy);
    nrays++;
    const Hit hc = closest_hit<false, tree_mode<FL>()>(sc, st, cam.o, cam.d, INFINITY);
    if (hc.tri < 0) return false;
    if (!(camera_return_distance(sc, itsD.tri, itsD.hu, itsD.hv, hc.tri) < (double) kShadowEpsilon)) return false;
    const Vec3f nD = itsD.n;
    const Vec3f ev = cross(edge, dir);
    const float sinphi = norm(ev);
    const Vec3f proj = normalize(cross(ev, nD));
    const float sinphi2 = norm(cross(dir, proj));
    if (!(sinphi > kEpsilon && sinphi2 > kEpsilon)) return false;
    const int bsdf_id = Tab<FL>::mesh_bsdf(sc, itsD.mesh);
    if (bsdf_id < 0) return false;
    const Vec3f d0 = -cam.d;
    Its<float> itsC = itsD;
    itsC.wi = itsD.sh.to_local(d0);
    const Vec3f wo = itsD.sh.to_local(-dir);
    const Bsdf<float, float> bsdf(sc, tv0, bsdf_id);
    const Vec3f f = colloc_bsdf_eval<(FL & kSceneRough) != 0>(sc, tv0, bsdf, itsC, wo);
    const float correction = fabsf(dot(d0, nD));
    const Vec3f n = normalize(cross(nD, proj));
    const float sign = copysignf(1.f, dot(ev, edge2)) * copysignf(1.f, dot(ev, n));
    float wgt;
    if constexpr (LK == kLightDistant) wgt = sensor_val * correction * (sinphi / sinphi2) / pdf * sign;
    else { const float rD = norm(xD - pL); wgt = sensor_val * correction / (rD * rD) * (rD / rB) * (sinphi / sinphi2) / pdf * sign; }
    r.k = k; r.pixel = pixel; r.tri = itsD.tri; r.s1 = s1; r.xB = xB; r.n = n;
    r.value0[0] = f.x * wgt; r.value0[1] = f.y * wgt; r.value0[2] = f.z * wgt;
    return true;
}
// forward mode: returns the pixel (or -1), tan[k][c] = d value / d P_k.  The triangle row at xD, the edge row and pL are differentiable; x(u, v) is
// rebuilt from the DETACHED row (the u2 construction of secondary_edge_sample).  Distant: the ray (bp0, -normalize(d)), origin and direction differentiable.
template <int K, int FL, int LK = kLightPoint>
PSDR_HD int point_sedge_sample(const SceneView &sc, const TangentView<K, FL> &tv, TraversalStack &st, const PointLight &pl, const float s3[3], float inv_sppse,
                               float tan[K][3], uint32_t &nrays) {
    using R = Dual<K>;
    PointSedge e;
    if (!point_sedge_values<FL, LK>(sc, st, pl, s3, nrays, e)) return -1;
    const size_t off = (size_t) e.k * PSDR_SEDGE_STRIDE;
    constexpr auto sm = &psdr_tangents::d_sec_edge;
    const Vec3<R> ep0 = ld3<R>(sc.d.sec_edge, tv, sm, off), ee1 = ld3<R>(sc.d.sec_edge, tv, sm, off + 3);
    const Vec3<R> bp0 = ee1 * R(e.s1) + ep0;
    const Vec3<R> pL = point_light_pos<R>(pl);
    const TriRow<R> T = load_tri<R>(sc, tv, e.tri);
    RayT<R> shadow;
    if constexpr (LK == kLightDistant) shadow = RayT<R>{bp0, -normalize(pL)};
    else shadow = RayT<R>{pL, normalize(bp0 - pL)};
    R u, v, t;
    moeller_trumbore(T.p0, T.e1, T.e2, shadow, u, v, t);
    const Vec3<R> u2 = bary_point(detach(T.p0), detach(T.e1), detach(T.e2), u, v);
    const R dn = dot(lift<R>(e.n), u2);
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) { const float g = dn.d[k] * e.value0[c]; tan[k][c] = (isfinite(e.value0[c] * dn.v) && isfinite(g)) ? g * inv_sppse : 0.f; }
    return e.pixel;
}
// reverse mode: adjoints to g_sec_edge (p0, e1) and g_tri_info (the row at xD) through the sink, to the light position through a_pl (+=).  Distant: the
// ray's origin adjoint goes to the edge row, its direction adjoint through -normalize_vjp to d; the point light routes both through xB - pL.
template <int LK = kLightPoint, class Sink>
PSDR_HD void point_sedge_reverse(Sink &sink, const SceneView &sc, TraversalStack &st, const PointLight &pl, const float s3[3], float inv_sppse,
                                 const float *__restrict__ adj_img, uint32_t &nrays, Vec3f &a_pl) {
    const TangentView<0, Sink::flags> tv0{};
    PointSedge e;
    if (!point_sedge_values<Sink::flags, LK>(sc, st, pl, s3, nrays, e)) return;
    const Vec3f pL = point_light_pos<float>(pl);
    const TriRow<float> TA = load_tri<float>(sc, tv0, e.tri);
    const Vec3f wv = LK == kLightDistant ? pL : e.xB - pL;
    const Vec3f wn = normalize(wv);
    const RayT<float> shadow = LK == kLightDistant ? RayT<float>{e.xB, -wn} : RayT<float>{pL, wn};
    float su, sv, stt;
    moeller_trumbore(TA.p0, TA.e1, TA.e2, shadow, su, sv, stt);
    const Vec3f u2 = bary_point(TA.p0, TA.e1, TA.e2, su, sv);
    const float dn = dot(e.n, u2);
    const float *a = adj_img + (size_t) e.pixel * 3;
    float a_dn = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) if (isfinite(e.value0[c] * dn)) a_dn += a[c] * e.value0[c];
    a_dn *= inv_sppse;
    if (a_dn == 0.f || !isfinite(a_dn)) return;
    const Vec3f a_u2 = e.n * a_dn;
    const MtAdj ma = mt_vjp(TA.p0, TA.e1, TA.e2, shadow, dot(a_u2, TA.e1), dot(a_u2, TA.e2), 0.f);
    scatter_vec(sink, e.tri, 0, ma.p0); scatter_vec(sink, e.tri, 3, ma.e1); scatter_vec(sink, e.tri, 6, ma.e2);
    const Vec3f a_wn = normalize_vjp(wv, wn, ma.d);
    const Vec3f a_w = LK == kLightDistant ? ma.o : a_wn;
    // xB = e1 * s1 + p0 (edge table)
    sink.add_sedge(e.k, 0, a_w.x); sink.add_sedge(e.k, 1, a_w.y); sink.add_sedge(e.k, 2, a_w.z);
    sink.add_sedge(e.k, 3, a_w.x * e.s1); sink.add_sedge(e.k, 4, a_w.y * e.s1); sink.add_sedge(e.k, 5, a_w.z * e.s1);
    acc_finite(a_pl, LK == kLightDistant ? -a_wn : ma.o - a_w);
}

}  // namespace psdr
