// psdr_path_sedge.h -- the secondary-edge boundary term of the PathTracer (PSDR_FLAG_PATH_SEDGES).  Build-defined: the reference
// has no PathTracer.  Anchored at max_depth = 1 to DirectIntegrator::eval_secondary_edge (secondary_edge_sample / secondary_edge_reverse), draw for draw.
//
// One slot of sampler 2 evaluates two boundary segments through one edge point p0:
//   A  direct source:   the segment ends on the emitter sample (boundary_segment_direct, the reference's draw); source = Le.
//   B  indirect source: the segment's direction is uniform on the sphere and ends on any surface; source = the radiance that surface REFLECTS towards the
//                       edge after exactly k = 1 .. d-1 further direct steps (Li's loop body without Le: A and B partition the integrand, no MIS).
// The sensor side of both is a random walk from p1 (the segment continued backwards onto a surface): every walk vertex y_j connects to the camera.
// Everything is detached; the tangent / adjoint flows through dn = dot(n, u2) only, once per segment and FORM: the connection at y_0 measures u2 from
// the camera ray's hit (solid-angle form, as the reference), the connections at y_1.. from the material point of p1 on its triangle (path-space form).
// The functions are mode-agnostic templates over two callables (the camera connection at y_0 and the sink of a connection's value), so forward mode,
// reverse mode and the host harness run ONE copy of the estimator.
//
// Guiding.  The three numbers that decide a segment before its first ray -- A: s3[0..2] (edge point, emitter sample: DirectIntegrator's draw),
// B: (s3[0], u, v) (edge point, sphere direction) -- are warped by an optional 3-D grid per segment with the semantics of HyperCubeDistribution3f
// (cube_sample_reuse<3>), and the returned pdf divides the segment's contribution by the rule of k_secondary_edge (pdf > kEpsilon ? 1 / pdf : 1).  Grid A is
// the scene descriptor's grid (guide_*), grid B travels in PathSedgeOpts.  The grids are independent: B warps the RAW s3[0], never what grid A made of it.
// No draw moves: a guided slot warps numbers, it never redraws them.  The template flag G = false compiles the grids out (the kernels of unguided launches: the
// guided branch cost k_path_sedge_rev<4> its second wave per SIMD); G = true looks at run time, so one host build serves both.
#pragma once
#include "psdr_reverse.h"

namespace psdr {

constexpr int kMaxPathSedgeDepth = PSDR_PATH_SEDGES_MAX_DEPTH;              // per-slot source sums live in registers: d - 1 <= 7 entries
// the grid of one segment: n = r0 r1 r2 cells, cell (c0, c1, c2) at (c0 r1 + c1) r2 + c2; cmf == nullptr: the segment is not guided
struct PathGuide { const float *cmf = nullptr, *pmf = nullptr; float sum = 0.f; int n = 0, r0 = 1, r1 = 1, r2 = 1; };
struct PathSedgeOpts { int max_depth, seg, walk; PathGuide gb = {}; };          // seg: bit 0 = segment A, bit 1 = segment B; walk = 0: the walk stops at y_0; gb: segment B's grid
// ... as a kernel argument: an unguided launch carries no grid
template <bool G> struct PathSedgeArgs;
template <> struct PathSedgeArgs<false> { int max_depth, seg, walk; PSDR_HD PathSedgeOpts opts() const { return PathSedgeOpts{max_depth, seg, walk}; } };
template <> struct PathSedgeArgs<true> { int max_depth, seg, walk; PathGuide gb; PSDR_HD PathSedgeOpts opts() const { return PathSedgeOpts{max_depth, seg, walk, gb}; } };
// warps s by the grid and returns what the segment's density is multiplied by (1 where k_secondary_edge's rule leaves the value alone)
PSDR_HD float path_guide_warp(const PathGuide &g, float s[3]) {
    const float pdf = cube_sample_reuse<3>(g.cmf, g.pmf, g.sum, g.n, g.r0, g.r1, g.r2, s);
    return pdf > kEpsilon ? pdf : 1.f;
}
PSDR_HD bool guided_a(const SceneView &sc) { return sc.d.guide_cmf != nullptr && sc.d.num_guide_cells > 0; }

// draws of one slot of sampler 2: s3 | 2 direction numbers | 3 (d-1) walk numbers of A | 3 (d-2) of B | 5 (d-1) source-bounce numbers
PSDR_HD int path_sedge_draws(int d) { return d >= 2 ? 11 * d - 9 : 3; }
PSDR_HD void rng_skip(Rng &rng, int n) { for (int i = 0; i < n; ++i) (void) rng.next_u32(); }

struct SourceSums { Vec3f c[kMaxPathSedgeDepth - 1]; };          // c[i] = L_1 + .. + L_{i+1}
// (no run-time indexing: the array stays in registers)
PSDR_HD Vec3f source_pick(const SourceSums &P, int i) {
    Vec3f r(0.f);
#pragma unroll
    for (int q = 0; q < kMaxPathSedgeDepth - 1; ++q) if (q == i) r = P.c[q];
    return r;
}

// L_k, k = 1 .. d-1: the radiance leaving `its` towards its.wi after exactly k direct steps (the loop body of Li started at a known vertex, without Le(its))
template <class TVT>
PSDR_HD void path_sedge_source(const SceneView &sc, const TVT &tv0, TraversalStack &st, Rng &rng, Its<float> its, int d, SourceSums &P, uint32_t &nrays) {
    Vec3f beta(1.f), cum(0.f);
    bool active = true;
#pragma unroll
    for (int q = 0; q < kMaxPathSedgeDepth - 1; ++q) P.c[q] = Vec3f(0.f);
#pragma unroll 1
    for (int k = 1; k < d; ++k) {
        Its<float> nits; Vec3f nf(0.f); bool nvalid = false;
        const Vec3f c = direct_step<float, float>(sc, tv0, st, rng, its, active, 1, 1, nrays, &nits, &nf, &nvalid, nullptr, k + 1 >= d);
        if (active) {
            cum = cum + beta * c;
            active = nvalid;
            if (active) {
                beta = beta * nf;
                its = nits;
                if (!(beta.x != 0.f || beta.y != 0.f || beta.z != 0.f)) active = false;
            }
        }
#pragma unroll
        for (int q = 0; q < kMaxPathSedgeDepth - 1; ++q) if (q == k - 1) P.c[q] = cum;
    }
}

// The edge point of a slot for segment B (segment A takes it from boundary_segment_direct, which keeps the edge normals to itself)
struct SedgePoint { int k; float s1, pdf_len; Vec3f p0, edge, edge2, n0, n1; bool is_boundary; };
PSDR_HD SedgePoint sedge_point(const SceneView &sc, float s0) {
    SedgePoint r;
    float s1 = s0, pdf0;
    r.k = sample_reuse(sc.d.sec_cmf, sc.d.sec_pmf, sc.d.sec_sum, sc.d.num_sec_edges, s1, pdf0);
    const float *se = sc.d.sec_edge + (size_t) r.k * PSDR_SEDGE_STRIDE;
    const Vec3f ep0{se[0], se[1], se[2]}, ee1{se[3], se[4], se[5]}, ep2{se[12], se[13], se[14]};
    r.n0 = Vec3f{se[6], se[7], se[8]}; r.n1 = Vec3f{se[9], se[10], se[11]};
    r.is_boundary = se[15] != 0.f;
    r.p0 = ee1 * s1 + ep0;
    const float e1len = norm(ee1);
    r.edge = ee1 / e1len; r.edge2 = ep2 - ep0; r.s1 = s1; r.pdf_len = pdf0 / e1len;
    return r;
}
PSDR_HD Vec3f uniform_sphere(float u, float v) {
    const float z = 1.f - 2.f * u, r = sqrtf(fmaxf(1.f - z * z, 0.f)), phi = 6.28318530717958647692f * v;
    return {r * cosf(phi), r * sinf(phi), z};
}
PSDR_HD void sedge_skip_faces(const SceneView &sc, int k, int &f0, int &f1) {
    const bool skip = sc.d.sec_edge_faces != nullptr && !sc.literal_forms;
    f0 = skip ? sc.d.sec_edge_faces[2 * k] : -1; f1 = skip ? sc.d.sec_edge_faces[2 * k + 1] : -1;
}

// The two rays of a segment: forwards from the edge point (A: must reach the emitter sample p2; B: any surface with a BSDF), then backwards onto a surface.
template <int FL>
PSDR_HD bool path_sedge_rays_a(const SceneView &sc, TraversalStack &st, const BoundarySeg &bs, Vec3f &dir, Its<float> &its2, Its<float> &its1c, uint32_t &nrays) {
    const TangentView<0, FL> tv0{};
    bool valid = bs.valid;
    dir = normalize(bs.p2 - bs.p0);
    int f0, f1; sedge_skip_faces(sc, bs.k, f0, f1);
    its2 = intersect<float>(sc, tv0, st, RayT<float>{bs.p0, dir}, valid, kDetached, nrays, f0, f1);
    valid = valid && its2.valid && norm(its2.p - bs.p2) < kShadowEpsilon;
    its1c = intersect<float>(sc, tv0, st, RayT<float>{bs.p0, -dir}, valid, kDetached, nrays, f0, f1);
    return valid && its1c.valid;
}
template <int FL>
PSDR_HD bool path_sedge_rays_b(const SceneView &sc, TraversalStack &st, const SedgePoint &ep, const Vec3f &dir, Its<float> &its2, Its<float> &its1c, uint32_t &nrays) {
    const TangentView<0, FL> tv0{};
    const float d0n = dot(ep.n0, dir), d1n = dot(ep.n1, dir);
    const int sgn0 = d0n > kEdgeEpsilon ? 1 : (d0n < -kEdgeEpsilon ? -1 : 0), sgn1 = d1n > kEdgeEpsilon ? 1 : (d1n < -kEdgeEpsilon ? -1 : 0);
    bool valid = ep.pdf_len > 0.f && (ep.is_boundary ? sgn0 != 0 : sgn0 * sgn1 < 0);
    int f0, f1; sedge_skip_faces(sc, ep.k, f0, f1);
    its2 = intersect<float>(sc, tv0, st, RayT<float>{ep.p0, dir}, valid, kDetached, nrays, f0, f1);
    valid = valid && its2.valid && Tab<FL>::mesh_bsdf(sc, its2.mesh) >= 0;
    its1c = intersect<float>(sc, tv0, st, RayT<float>{ep.p0, -dir}, valid, kDetached, nrays, f0, f1);
    return valid && its1c.valid;
}
// the filter predicate of segment B: the two rays of the segment that (s0, u, v) decide
template <int FL>
PSDR_HD bool path_sedge_survives_b_at(const SceneView &sc, TraversalStack &st, float s0, float u, float v, uint32_t &nrays) {
    const SedgePoint ep = sedge_point(sc, s0);
    Its<float> its2, its1c;
    return path_sedge_rays_b<FL>(sc, st, ep, uniform_sphere(u, v), its2, its1c, nrays);
}
// ... in a split launch: the slot's direction draw, warped by segment B's grid exactly as path_sedge_slot re-derives it for the survivors
template <int FL>
PSDR_HD bool path_sedge_survives_b(const SceneView &sc, TraversalStack &st, Rng &rng /* after s3 */, float s0, uint32_t &nrays, const PathGuide *gb = nullptr) {
    const float u = rng.next(), v = rng.next();
    float sb[3] = {s0, u, v};
    if (gb != nullptr && gb->cmf != nullptr) (void) path_guide_warp(*gb, sb);
    return path_sedge_survives_b_at<FL>(sc, st, sb[0], sb[1], sb[2], nrays);
}

// What one segment hands to the mode-specific code: the edge, its two hits and the geometry of the boundary
struct SedgeSegment { int k; float s1; Vec3f p0, dir, n; Its<float> its2, its1c; float base_v, bpdf, sgn; bool geom_ok; Vec3f src_a; };
// base_v, the normal dn is measured along and the sign factors of eval_secondary_edge (direct.cpp:270-300) for a segment that ends at p2 on a surface with normal bn
PSDR_HD void sedge_geom(SedgeSegment &sg, const Vec3f &edge, const Vec3f &edge2, const Vec3f &bn, const Vec3f &p2) {
    const float dist = norm(p2 - sg.its1c.p), cos2 = fabsf(dot(bn, sg.dir));
    const Vec3f ev = cross(edge, sg.dir);
    const float sinphi = norm(ev);
    const Vec3f proj = normalize(cross(ev, bn));
    const float sinphi2 = norm(cross(sg.dir, proj));
    sg.base_v = (sg.its1c.t / dist) * (sinphi / sinphi2) * cos2;
    sg.geom_ok = sinphi > kEpsilon && sinphi2 > kEpsilon;
    sg.n = normalize(cross(bn, proj));
    sg.sgn = copysignf(1.f, dot(ev, edge2)) * copysignf(1.f, dot(ev, sg.n));
}

// The sensor side of one segment: the walk y_0 = its1c, y_1, .. with a camera connection at every vertex.
//   cam0(qx, qy, d0, tri) -> bool   the connection at y_0: traces the camera ray in the caller's mode (dual numbers / adjoint records), reports its
//                                   direction back towards the camera and the triangle it meets; false: nothing met
//   emit(form, pixel, value)        one connection's detached value (form 0: y_0, form 1: y_1 ..)
// src_a: the constant source of segment A (Le); otherwise connection j uses the source sums of segment B within the depth budget.
template <int FL, class Cam0, class Emit>
PSDR_HD void path_sedge_walk(const SceneView &sc, TraversalStack &st, Rng &rng, const PathSedgeOpts &po, bool seg_a, const Vec3f &src_a, const SourceSums &P,
                             Its<float> its, Vec3f dw, float base_v, float bpdf, float sgn, bool geom_ok, Cam0 &&cam0, Emit &&emit, uint32_t &nrays) {
    const TangentView<0, FL> tv0{};
    const int d = po.max_depth, jmax = seg_a ? d : d - 1;
    Vec3f T(1.f);
#pragma unroll 1
    for (int j = 0; j < jmax; ++j) {
        const int bsdf_id = Tab<FL>::mesh_bsdf(sc, its.mesh);
        const Bsdf<float, float> bsdf(sc, tv0, bsdf_id < 0 ? 0 : bsdf_id);
        const Vec3f p1 = its.p;
        int pixel; float qx, qy, sensor_val;
        if (sample_direct(sc, p1, pixel, qx, qy, sensor_val)) {
            Vec3f d0(0.f); int tri = -1; bool seen;
            if (j == 0) seen = cam0(qx, qy, d0, tri);
            else {
                const RayT<float> cam = primary_ray<float>(sc, tv0, qx, qy);
                nrays++;
                tri = closest_hit<false, tree_mode<FL>()>(sc, st, cam.o, cam.d, INFINITY).tri;
                d0 = -cam.d; seen = tri >= 0;
            }
            // "the camera sees the vertex" (direct.cpp:262), in double: see secondary_edge_sample
            if (seen && !(j == 0 && sc.literal_forms)) seen = camera_return_distance(sc, its.tri, its.hu, its.hv, tri) < (double) kShadowEpsilon;
            if (seen && geom_ok && bsdf_id >= 0) {
                const Vec3f d0_local = its.sh.to_local(d0);
                Vec3f bsdf_val = bsdf.eval(sc, tv0, its, d0_local, true);
                const float correction = fabsf((its.wi.z * dot(d0, its.n)) / (d0_local.z * dot(dw, its.n)));
                bsdf_val = bsdf_val * correction;
                const Vec3f src = seg_a ? src_a : source_pick(P, d - 2 - j);
                Vec3f value0 = bsdf_val * (j == 0 ? src : src * T) * (base_v * sensor_val / bpdf);
                value0 = value0 * sgn;
                emit(j == 0 ? 0 : 1, pixel, value0);
            }
        }
        if (bsdf_id < 0) return;                                        // bounding mesh: null BSDF evaluates to zero
        if (!geom_ok || po.walk == 0 || j + 1 >= jmax) return;
        // extend: wo ~ bsdf.sample(y_j; wi_j); T carries eval / pdf and the shading / geometric cosine ratios of both directions at y_j
        const float s[3] = {rng.next(), rng.next(), rng.next()};
        Vec3f wo; float pdf;
        if (!bsdf.sample(sc, tv0, its, s, true, wo, pdf)) return;
        const Vec3f f = bsdf.eval(sc, tv0, its, wo, true);
        const Vec3f dir1 = its.sh.s * wo.x + its.sh.t * wo.y + its.sh.n * wo.z;
        const float ratio = fabsf((its.wi.z * dot(dir1, its.n)) / (dot(dw, its.n) * wo.z));
        T = T * f * (ratio / pdf);
        if (!(T.x != 0.f || T.y != 0.f || T.z != 0.f) || !(isfinite(T.x) && isfinite(T.y) && isfinite(T.z))) return;
        const Its<float> nits = intersect<float>(sc, tv0, st, RayT<float>{p1, dir1}, true, kDetached, nrays);
        if (!nits.valid) return;
        its = nits; dw = dir1;
    }
}

// dn = dot(n, u2): u2 = where the line from the receiver point x through the edge point bp0 meets the plane of triangle tri2 (detached triangle, moving (u, v))
template <class R, class TVT>
PSDR_HD R sedge_dn(const SceneView &sc, const TVT &tv, const Vec3<R> &x, const Vec3<R> &bp0, int tri2, const Vec3f &n) {
    const TriRow<R> T = load_tri<R>(sc, tv, tri2);
    const RayT<R> shadow{x, normalize(bp0 - x)};
    R u, v, t;
    moeller_trumbore(T.p0, T.e1, T.e2, shadow, u, v, t);
    const Vec3<R> u2 = bary_point(detach(T.p0), detach(T.e1), detach(T.e2), u, v);
    return dot(lift<R>(n), u2);
}
// its adjoint: scatters into triangle tri2 and the edge row, returns the adjoint of the receiver point
template <class Sink>
PSDR_HD Vec3f sedge_dn_vjp(Sink &sink, const SceneView &sc, const Vec3f &x, const Vec3f &p0, int tri2, const Vec3f &n, float a_dn, int k, float s1) {
    const TangentView<0, Sink::flags> tv0{};
    const TriRow<float> TA = load_tri<float>(sc, tv0, tri2);
    const Vec3f wv = p0 - x;
    const RayT<float> shadow{x, normalize(wv)};
    const Vec3f a_u2 = n * a_dn;
    const MtAdj ma = mt_vjp(TA.p0, TA.e1, TA.e2, shadow, dot(a_u2, TA.e1), dot(a_u2, TA.e2), 0.f);
    scatter_vec(sink, tri2, 0, ma.p0); scatter_vec(sink, tri2, 3, ma.e1); scatter_vec(sink, tri2, 6, ma.e2);
    const Vec3f a_w = normalize_vjp(wv, shadow.d, ma.d);
    // bp0 = e1 * s1 + p0 (edge table)
    sink.add_sedge(k, 0, a_w.x); sink.add_sedge(k, 1, a_w.y); sink.add_sedge(k, 2, a_w.z);
    sink.add_sedge(k, 3, a_w.x * s1); sink.add_sedge(k, 4, a_w.y * s1); sink.add_sedge(k, 5, a_w.z * s1);
    return ma.o - a_w;
}

// Runs both segments of a slot.  begin(seg) -> bool prepares the mode's per-segment state (dn of the material form ..), cam0 / emit as in path_sedge_walk,
// end(seg) finishes the segment (reverse mode: the two VJP chains).  rng: the slot's stream after s3.  count_first: the slot's first two rays per segment
// are counted here (false: the filter of a split launch traced and counted them).  uv: the direction numbers of segment B when they are not the stream's (the
// guiding-grid build: the cell sample); the stream advances past its two all the same.
template <int FL, bool G = true, class Begin, class Cam0, class Emit, class End>
PSDR_HD void path_sedge_slot(const SceneView &sc, TraversalStack &st, Rng rng, const float s3[3], const PathSedgeOpts &po, uint32_t &nrays, bool count_first,
                             Begin &&begin, Cam0 &&cam0, Emit &&emit, End &&end, const float *uv = nullptr) {
    const TangentView<0, FL> tv0{};
    const int d = po.max_depth;
    float u = 0.f, v = 0.f;
    if (d >= 2) { u = rng.next(); v = rng.next(); }
    if (uv != nullptr) { u = uv[0]; v = uv[1]; }
    Rng rng_a = rng, rng_b = rng;
    if (d >= 2) rng_skip(rng_b, 3 * (d - 1));
    Rng rng_s = rng_b;
    if (d >= 2) rng_skip(rng_s, 3 * (d - 2));
    uint32_t counted_before = 0;
    uint32_t &n12 = count_first ? nrays : counted_before;
    SedgeSegment sg;
    SourceSums P;
#pragma unroll
    for (int q = 0; q < kMaxPathSedgeDepth - 1; ++q) P.c[q] = Vec3f(0.f);
    if (po.seg & 1) {
        float sa[3] = {s3[0], s3[1], s3[2]}, ga = 1.f;
        if (G && guided_a(sc)) { const float pdf = guide_sample_reuse(sc, sa); ga = pdf > kEpsilon ? pdf : 1.f; }
        const BoundarySeg bs = boundary_segment_direct<FL>(sc, sa);
        if (path_sedge_rays_a<FL>(sc, st, bs, sg.dir, sg.its2, sg.its1c, n12)) {
            sg.k = bs.k; sg.s1 = bs.s1; sg.p0 = bs.p0; sg.bpdf = bs.pdf * ga;
            sedge_geom(sg, bs.edge, bs.edge2, bs.n, bs.p2);
            sg.src_a = Le<float>(sc, tv0, sg.its2, true);
            if (begin(sg)) {
                path_sedge_walk<FL>(sc, st, rng_a, po, true, sg.src_a, P, sg.its1c, sg.dir, sg.base_v, sg.bpdf, sg.sgn, sg.geom_ok, cam0, emit, nrays);
                end(sg);
            }
        }
    }
    if ((po.seg & 2) && d >= 2) {
        float sb[3] = {s3[0], u, v}, gb = 1.f;          // the RAW s3[0]: the grids are independent
        if (G && po.gb.cmf != nullptr) gb = path_guide_warp(po.gb, sb);
        const SedgePoint ep = sedge_point(sc, sb[0]);
        sg.dir = uniform_sphere(sb[1], sb[2]);
        if (path_sedge_rays_b<FL>(sc, st, ep, sg.dir, sg.its2, sg.its1c, n12)) {
            sg.k = ep.k; sg.s1 = ep.s1; sg.p0 = ep.p0; sg.bpdf = ep.pdf_len * 0.07957747154594767f * gb;          // density of (edge point, direction): 1 / (4 pi) per solid angle, times the grid's
            sedge_geom(sg, ep.edge, ep.edge2, sg.its2.n, sg.its2.p);
            sg.src_a = Vec3f(0.f);
            if (sg.geom_ok) {
                path_sedge_source(sc, tv0, st, rng_s, sg.its2, d, P, nrays);
                const Vec3f all = source_pick(P, d - 2);
                if ((all.x != 0.f || all.y != 0.f || all.z != 0.f) && begin(sg)) {
                    path_sedge_walk<FL>(sc, st, rng_b, po, false, sg.src_a, P, sg.its1c, sg.dir, sg.base_v, sg.bpdf, sg.sgn, true, cam0, emit, nrays);
                    end(sg);
                }
            }
        }
    }
}

// ---- forward mode: out(pixel, value) receives one connection's tangent-only value (R = Dual<K>), to be scaled and added to the derivative image
template <class R, bool G = true, class TVT, class Out>
PSDR_HD void path_secondary_edge_sample(const SceneView &sc, const TVT &tv, TraversalStack &st, const Rng &rng, const float s3[3], const PathSedgeOpts &po, uint32_t &nrays,
                                        bool count_first, Out &&out) {
    constexpr int FL = TVT::flags;
    R dn0(0.f), dn1(0.f);          // per form (two names, not an array: `form` is a run-time value and an indexed array would live in scratch)
    Vec3<R> bp0 = zero3<R>();
    const SedgeSegment *cur = nullptr;
    auto begin = [&](const SedgeSegment &sg) {
        cur = &sg;
        const size_t off = (size_t) sg.k * PSDR_SEDGE_STRIDE;
        constexpr auto sm = &psdr_tangents::d_sec_edge;
        const Vec3<R> ep0 = ld3<R>(sc.d.sec_edge, tv, sm, off), ee1 = ld3<R>(sc.d.sec_edge, tv, sm, off + 3);
        bp0 = ee1 * R(sg.s1) + ep0;
        if (po.max_depth >= 2 && po.walk != 0) {
            // the material point of p1: p0_T + hu e1_T + hv e2_T with (hu, hv) detached
            const TriRow<R> T1 = load_tri<R>(sc, tv, sg.its1c.tri);
            const Vec3<R> x = bary_point(T1.p0, T1.e1, T1.e2, R(sg.its1c.hu), R(sg.its1c.hv));
            dn1 = sedge_dn<R>(sc, tv, x, bp0, sg.its2.tri, sg.n);
        }
        return true;
    };
    auto cam0 = [&](float qx, float qy, Vec3f &d0, int &tri) {
        const RayT<R> camera_ray = primary_ray<R>(sc, tv, qx, qy);
        const Its<R> its1 = intersect<R>(sc, tv, st, camera_ray, true, kSolidAngle, nrays);
        if (!its1.valid) return false;
        if (sc.literal_forms && !(norm(val(its1.p) - cur->its1c.p) < kShadowEpsilon)) return false;          // direct.cpp:262 as written
        d0 = -val(camera_ray.d); tri = its1.tri;
        dn0 = sedge_dn<R>(sc, tv, its1.p, bp0, cur->its2.tri, cur->n);
        return true;
    };
    auto emit = [&](int form, int pixel, const Vec3f &value0) {
        const R d = form == 0 ? dn0 : dn1;
        const Vec3<R> res{d * value0.x, d * value0.y, d * value0.z};
        out(pixel, zero_nonfinite(res - detach(res)));
    };
    auto end = [&](const SedgeSegment &) {};
    path_sedge_slot<FL, G>(sc, st, rng, s3, po, nrays, count_first, begin, cam0, emit, end);
}

// ---- reverse mode: the connections of one segment add <adj_pixel, value> into one seed per form; the VJP chain of dn then runs once per form
template <bool G = true, class Sink>
PSDR_HD void path_secondary_edge_reverse(Sink &sink, const SceneView &sc, TraversalStack &st, const Rng &rng, const float s3[3], const PathSedgeOpts &po, float scale,
                                         const float *__restrict__ adj_img, uint32_t &nrays, bool count_first) {
    constexpr int FL = Sink::flags;
    const TangentView<0, FL> tv0{};
    float dn0 = 0.f, dn1 = 0.f, a_dn0 = 0.f, a_dn1 = 0.f;          // per form (see path_secondary_edge_sample)
    Vec3f xm(0.f), x1(0.f), dcam(0.f);
    RayT<float> cam{Vec3f(0.f), Vec3f(0.f)};
    TriRow<float> Tc{};
    float cu = 0.f, cv = 0.f; int ctri = -1;
    const SedgeSegment *cur = nullptr;
    auto begin = [&](const SedgeSegment &sg) {
        cur = &sg; a_dn0 = a_dn1 = 0.f; ctri = -1;
        if (po.max_depth >= 2 && po.walk != 0) {
            const TriRow<float> T1 = load_tri<float>(sc, tv0, sg.its1c.tri);
            xm = bary_point(T1.p0, T1.e1, T1.e2, sg.its1c.hu, sg.its1c.hv);
            dn1 = sedge_dn<float>(sc, tv0, xm, sg.p0, sg.its2.tri, sg.n);
        }
        return true;
    };
    auto cam0 = [&](float qx, float qy, Vec3f &d0, int &tri) {
        dcam = camera_space_dir(sc, qx, qy);
        cam = primary_ray<float>(sc, tv0, qx, qy);
        nrays++;
        const Hit hc = closest_hit<false, tree_mode<FL>()>(sc, st, cam.o, cam.d, INFINITY);
        if (hc.tri < 0) return false;
        Tc = load_tri<float>(sc, tv0, hc.tri);
        float ct;
        moeller_trumbore(Tc.p0, Tc.e1, Tc.e2, cam, cu, cv, ct);
        x1 = bary_point(Tc.p0, Tc.e1, Tc.e2, cu, cv);            // its1.p (solid-angle form, on the triangle)
        ctri = hc.tri; tri = hc.tri; d0 = -cam.d;
        dn0 = sedge_dn<float>(sc, tv0, x1, cur->p0, cur->its2.tri, cur->n);
        return true;
    };
    auto emit = [&](int form, int pixel, const Vec3f &value0) {
        const float *a = adj_img + (size_t) pixel * 3;
        const float v0[3] = {value0.x, value0.y, value0.z};
        const float dnf = form == 0 ? dn0 : dn1;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) if (isfinite(v0[c] * dnf)) acc += a[c] * v0[c];
        if (form == 0) a_dn0 += acc; else a_dn1 += acc;
    };
    auto end = [&](const SedgeSegment &sg) {
        const float a0 = a_dn0 * scale, a1 = a_dn1 * scale;
        if (a0 != 0.f && isfinite(a0) && ctri >= 0) {
            const Vec3f a_x1 = sedge_dn_vjp(sink, sc, x1, sg.p0, sg.its2.tri, sg.n, a0, sg.k, sg.s1);
            // x1 = p0 + u e1 + v e2 with (u, v, .) = MT(triangle C, camera ray)
            const MtAdj mc = mt_vjp(Tc.p0, Tc.e1, Tc.e2, cam, dot(a_x1, Tc.e1), dot(a_x1, Tc.e2), 0.f);
            scatter_vec(sink, ctri, 0, mc.p0 + a_x1); scatter_vec(sink, ctri, 3, mc.e1 + a_x1 * cu); scatter_vec(sink, ctri, 6, mc.e2 + a_x1 * cv);
            camera_ray_vjp(sink, sc, dcam, mc.o, mc.d);
        }
        if (a1 != 0.f && isfinite(a1)) {
            // the material point rides on its triangle: the receiver's adjoint goes to the three rows of its1c.tri
            const Vec3f a_x = sedge_dn_vjp(sink, sc, xm, sg.p0, sg.its2.tri, sg.n, a1, sg.k, sg.s1);
            scatter_vec(sink, sg.its1c.tri, 0, a_x); scatter_vec(sink, sg.its1c.tri, 3, a_x * sg.its1c.hu); scatter_vec(sink, sg.its1c.tri, 6, a_x * sg.its1c.hv);
        }
    };
    path_sedge_slot<FL, G>(sc, st, rng, s3, po, nrays, count_first, begin, cam0, emit, end);
}

// ---- guiding-grid build (psdr_path_guide_build): what ONE unguided evaluation of segment po.seg (1 = A, 2 = B) adds to its cell before the division by the
// streams per cell and the rounds: hmax over the colour channels of the sum over the segment's camera connections of |value0|.  c3: the cell sample -- s3 of
// segment A, (s3[0], u, v) of segment B; rest: the stream of every other number of the evaluation, laid out as a render slot's stream after s3 (its two direction
// numbers are skipped).  The caller's scene view carries no grid and po.gb is empty: like psdr_guide_build, the build ignores any grid that is set.
template <int FL>
PSDR_HD float path_sedge_mass(const SceneView &sc, TraversalStack &st, const Rng &rest, const float c3[3], const PathSedgeOpts &po, uint32_t &nrays, bool count_first) {
    const TangentView<0, FL> tv0{};
    Vec3f acc(0.f);
    const SedgeSegment *cur = nullptr;
    auto begin = [&](const SedgeSegment &sg) { cur = &sg; return true; };
    auto cam0 = [&](float qx, float qy, Vec3f &d0, int &tri) {
        const RayT<float> cam = primary_ray<float>(sc, tv0, qx, qy);
        const Its<float> its1 = intersect<float>(sc, tv0, st, cam, true, kDetached, nrays);
        if (!its1.valid) return false;
        if (sc.literal_forms && !(norm(its1.p - cur->its1c.p) < kShadowEpsilon)) return false;
        d0 = -cam.d; tri = its1.tri;
        return true;
    };
    auto emit = [&](int, int, const Vec3f &value0) {
        const Vec3f v = zero_nonfinite(value0);
        acc = acc + Vec3f{fabsf(v.x), fabsf(v.y), fabsf(v.z)};
    };
    auto end = [&](const SedgeSegment &) {};
    path_sedge_slot<FL, false>(sc, st, rest, c3, po, nrays, count_first, begin, cam0, emit, end, po.seg == 2 ? c3 + 1 : nullptr);
    return fmaxf(acc.x, fmaxf(acc.y, acc.z));
}

}  // namespace psdr
