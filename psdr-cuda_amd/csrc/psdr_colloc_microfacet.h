// psdr_colloc_microfacet.h -- MicrofacetBSDF (PSDR_BSDF_MICROFACET, include/psdr_hip.h): a Lambertian diffuse lobe plus an isotropic
// GGX specular lobe with a Schlick Fresnel term.  Build-defined: the reference snapshot has no such BSDF.  For local directions with wi.z > 0 and wo.z > 0
// (zero otherwise), cosine included like Bsdf::eval:
//     h = normalize(wi + wo)
//     f cos(theta_o) = kd / pi * wo.z  +  F(wi.h) D(h) G1(wi, h) G1(wo, h) / (4 wi.z),      F(c) = F0 + (1 - F0) (1 - c)^5
// with D and G1 the project's GGX<M>{alpha, alpha} (psdr_device.h, their cut-offs included) and alpha = r^2.  Record slots: kd = PSDR_SLOT_REFLECTANCE,
// r = PSDR_SLOT_ALPHA_U, F0 = PSDR_SLOT_ETA.  Where D's cut-off answers zero -- alpha = 0 among the cases -- the specular lobe is zero and the value is
// the diffuse lobe.
// The model is an evaluation and its adjoint, no sample / pdf: the CollocatedIntegrator (psdr_collocated.h) evaluates f at ONE direction pair, wo = wi (there
// h = wi and F = F0), and is the only integrator that serves the type.  The value (microfacet_any_eval) and its adjoint
// (microfacet_eval_vjp, microfacet_mapped_eval_vjp) take a general wo all the same.
// PSDR_BSDF_MICROFACET_NORMAL is the same record plus a tangent-space normal map in PSDR_SLOT_K: the lobes are evaluated about a
// normal n' turned away from the shading normal in a frame whose tangent follows the texture's u axis (normal_map_frame below).
// PSDR_BSDF_MICROFACET_HEIGHT is the same record plus a 1-channel height map in PSDR_SLOT_K and its scale in PSDR_SLOT_ALPHA_V: n' is the
// normal of the surface displaced by scale x height along the shading normal, to first order (height_map_frame below).
// Compiled only into the flag sets that carry the GGX code (kSceneRough); the Lambertian ones keep their text.
#pragma once
#include "psdr_reverse.h"

namespace psdr {

// G: geometry type of the hit and the directions, M: material / result type -- plain floats, Dual<1> and Dual<3> go through this one copy.  The two lobes for
// local directions that passed the side test (its: the texture coordinates of the lookups)
template <class G, class M, class TVT>
PSDR_HD Vec3<M> microfacet_lobes(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its, const Vec3<M> &wi_m, const Vec3<M> &wo_m) {
    const Vec3<M> diffuse = b.tex3(sc, tv, PSDR_SLOT_REFLECTANCE, its) * (wo_m.z * kInvPi);
    const M alpha = sqr(b.tex1(sc, tv, PSDR_SLOT_ALPHA_U, its));
    const GGX<M> g{alpha, alpha};
    const Vec3<M> H = normalize(wo_m + wi_m);
    const M D = g.eval(H);
    if (val(D) == 0.f) return diffuse;
    const M res = D * (g.smith_g1(wi_m, H) * g.smith_g1(wo_m, H)) / (4.f * wi_m.z);
    const Vec3<M> F0 = b.tex3(sc, tv, PSDR_SLOT_ETA, its);
    const M t = 1.f - dot(wi_m, H);
    const M w = sqr(sqr(t)) * t;
    return {diffuse.x + (F0.x + (1.f - F0.x) * w) * res, diffuse.y + (F0.y + (1.f - F0.y) * w) * res, diffuse.z + (F0.z + (1.f - F0.z) * w) * res};
}

// Adjoint of value = microfacet_lobes(its, wi, wo): af (RGB) -> awi, awo, the texels of the three maps (through the sink), a_uv.
// The geometric part D G1 G1 / (4 wi.z) and the Fresnel cosine go through ggx_geo_vjp (psdr_reverse.h), the rough conductor's own.  An adjoint that is not
// finite (alpha at the edge of fp32) is dropped like the sample's value is (zero_nonfinite).
template <class Sink, class TVT>
PSDR_HD void microfacet_lobes_vjp(Sink &sink, const SceneView &sc, const TVT &tv0, const Bsdf<float, float> &b, const Its<float> &its, const Vec3f &wi, const Vec3f &wo,
                                  const Vec3f &af, Vec3f &awi, Vec3f &awo, float &auvx, float &auvy) {
    {   // kd / pi * wo.z
        const Vec3f kd = b.tex3(sc, tv0, PSDR_SLOT_REFLECTANCE, its);
        const float c = wo.z * kInvPi;
        const float a_kd[3] = {af.x * c, af.y * c, af.z * c};
        bitmap_vjp<Sink, 3>(sink, sc, b.slot(PSDR_SLOT_REFLECTANCE), its.uvx, its.uvy, a_kd, auvx, auvy);
        awo.z += dot(af, kd) * kInvPi;
    }
    const float r = b.tex1(sc, tv0, PSDR_SLOT_ALPHA_U, its), alpha = r * r;
    const GgxAdj v0 = ggx_geo_vjp<true>(wi, wo, alpha, alpha, 0.f, 0.f);          // value pass: geo = D G1 G1 / (4 wi.z), c = wi.h
    if (v0.zero || !isfinite(v0.geo)) return;
    const Vec3f F0 = b.tex3(sc, tv0, PSDR_SLOT_ETA, its);
    const float t = 1.f - v0.c, t4 = sqr(sqr(t)), w = t4 * t;
    // value_ch = (F0 + (1 - F0) w) geo,  w = (1 - c)^5
    const float *f0 = &F0.x, *afp = &af.x;
    float a_geo = 0.f, a_c = 0.f, a_f0[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        a_f0[ch] = finite_or_zero(afp[ch] * v0.geo * (1.f - w));
        a_geo += afp[ch] * (f0[ch] + (1.f - f0[ch]) * w);
        a_c += afp[ch] * v0.geo * (1.f - f0[ch]) * (-5.f * t4);
    }
    const GgxAdj ga = ggx_geo_vjp<true>(wi, wo, alpha, alpha, a_geo, a_c);
    acc_finite(awi, ga.wi); acc_finite(awo, ga.wo);
    const float a_r = finite_or_zero((ga.au + ga.av) * (2.f * r));          // alpha_u = alpha_v = r^2
    bitmap_vjp<Sink, 1>(sink, sc, b.slot(PSDR_SLOT_ALPHA_U), its.uvx, its.uvy, &a_r, auvx, auvy);
    bitmap_vjp<Sink, 3>(sink, sc, b.slot(PSDR_SLOT_ETA), its.uvx, its.uvy, a_f0, auvx, auvy);
}
// ... with BsdfRev::eval_vjp's signature
template <class Sink, class TVT>
PSDR_HD void microfacet_eval_vjp(Sink &sink, const SceneView &sc, const TVT &tv0, const Bsdf<float, float> &b, const Its<float> &its, const Vec3f &wo,
                                 const Vec3f &af, Vec3f &awi, Vec3f &awo, float &auvx, float &auvy) {
    if (!(its.wi.z > 0.f && wo.z > 0.f)) return;
    microfacet_lobes_vjp(sink, sc, tv0, b, its, its.wi, wo, af, awi, awo, auvx, auvy);
}

// ------------------------------------------------------------------ tangent-space normal map (PSDR_BSDF_MICROFACET_NORMAL)
// The perturbed normal n' of a hit and the intermediate values its adjoint reads:
//     v = 2 c - 1 (c: the map's texel at the hit's uv),   dp_du = e1 c1 + e2 c2,  c1 = dv2 / det,  c2 = -dv1 / det  (the triangle's three UVs),
//     p = dp_du - n (n . dp_du),  s = normalize(p),  t = n x s,  m = s v.x + t v.y + n v.z,  n' = normalize(m)
// zero: |v|^2 <= 1e-12, the BSDF value is zero; flat: no UV-aligned tangent exists (det == 0, |p|^2 <= 1e-20, or a scene without texture coordinates), n' = n.
template <class M> struct NormalMap { Vec3<M> n, v, dp, p, s, t, m, n1; M ndp; float c1, c2; bool zero, flat; };
template <class G, class M, class TVT>
PSDR_HD NormalMap<M> normal_map_frame(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its) {
    NormalMap<M> r;
    const Vec3<M> c = b.tex3(sc, tv, PSDR_SLOT_K, its);
    r.v = {2.f * c.x - 1.f, 2.f * c.y - 1.f, 2.f * c.z - 1.f};
    r.n = r.n1 = to_m3<M>(its.sh.n);
    r.zero = !(val(dot(r.v, r.v)) > 1e-12f);
    r.flat = true;
    if (r.zero || sc.d.tri_uv == nullptr) return r;
    const float *q = Tab<TVT::flags>::tri_uv(sc, its.tri);
    const float du1 = q[2] - q[0], dv1 = q[3] - q[1], du2 = q[4] - q[0], dv2 = q[5] - q[1], det = du1 * dv2 - du2 * dv1;
    if (det == 0.f) return r;
    const TriRow<G> T = load_tri<G>(sc, tv, its.tri);
    r.c1 = dv2 / det; r.c2 = -dv1 / det;
    r.dp = to_m3<M>(T.e1) * r.c1 + to_m3<M>(T.e2) * r.c2;
    r.ndp = dot(r.n, r.dp);
    r.p = r.dp - r.n * r.ndp;
    if (!(val(dot(r.p, r.p)) > 1e-20f)) return r;
    r.flat = false;
    r.s = normalize(r.p);
    r.t = cross(r.n, r.s);
    r.m = r.s * r.v.x + r.t * r.v.y + r.n * r.v.z;
    r.n1 = normalize(r.m);
    return r;
}

// ------------------------------------------------------------------ height map (PSDR_BSDF_MICROFACET_HEIGHT)
// The gradient (h_u, h_v) of a 1-channel bilinear map at (u, v): the exact derivative of what bitmap_eval<., 1> returns there, from the same cell and the same
// weights (v flipped, x - floor(x), scaled by (w - 1, h - 1), px / py clamped to w - 2 / h - 2):
//     h_u = (w - 1) [w0y (h10 - h00) + w1y (h11 - h01)],     h_v = -(h - 1) [w0x (h01 - h00) + w1x (h11 - h10)]      (the minus: the v flip)
// U = type of the texture coordinates, M = type of the texels, as bitmap_eval; a 1 x 1 map has no slope.
template <class M, bool LDS, class U, class TVT>
PSDR_HD void bitmap_grad_from(const SceneView &sc, const TVT &tv, const int32_t *slot, U u, U v, M &hu, M &hv) {
    const int off = slot[0], w = slot[1], h = slot[2];
    if (w == 1 && h == 1) { hu = hv = M(0.f); return; }
    v = -v;
    u = u - floorf(val(u)); v = v - floorf(val(v));
    u = u * (float) (w - 1); v = v * (float) (h - 1);
    int px = (int) floorf(val(u)), py = (int) floorf(val(v));
    const U w1x = u - (float) px, w1y = v - (float) py;
    const U w0x = 1.f - w1x, w0y = 1.f - w1y;
    px = px < w - 2 ? px : w - 2; py = py < h - 2 ? py : h - 2;
    const size_t idx = (size_t) off + (size_t) py * w + px;
    const M h00 = texel<M, LDS>(sc, tv, idx), h10 = texel<M, LDS>(sc, tv, idx + 1), h01 = texel<M, LDS>(sc, tv, idx + w), h11 = texel<M, LDS>(sc, tv, idx + w + 1);
    hu = ((h10 - h00) * w0y + (h11 - h01) * w1y) * (float) (w - 1);
    hv = ((h01 - h00) * w0x + (h11 - h10) * w1x) * (-(float) (h - 1));
}
template <class M, class U, class TVT>
PSDR_HD void bitmap_grad(const SceneView &sc, const TVT &tv, const int32_t *slot, U u, U v, M &hu, M &hv) {
    if constexpr (Tab<TVT::flags>::lds_small) {
        if (sc.lt_tex >= 0) { bitmap_grad_from<M, true>(sc, tv, slot, u, v, hu, hv); return; }
    }
    bitmap_grad_from<M, false>(sc, tv, slot, u, v, hu, hv);
}
// ... and its adjoint: (a_hu, a_hv) to the four texels with the signed weights above, and to (u, v) through the patch's one second derivative, the cross term
//     d h_u / dv = d h_v / du = -(w - 1) (h - 1) (h11 - h10 - h01 + h00)
template <class Sink>
PSDR_HD void bitmap_grad_vjp(Sink &sink, const SceneView &sc, const int32_t *slot, float u, float v, float a_hu, float a_hv, float &au, float &av) {
    const int off = slot[0], w = slot[1], h = slot[2];
    if (w == 1 && h == 1) return;
    const float *tx = sc.d.texels;
    v = -v;
    u = u - floorf(u); v = v - floorf(v);
    u = u * (float) (w - 1); v = v * (float) (h - 1);
    int px = (int) floorf(u), py = (int) floorf(v);
    const float w1x = u - (float) px, w1y = v - (float) py, w0x = 1.f - w1x, w0y = 1.f - w1y;
    px = px < w - 2 ? px : w - 2; py = py < h - 2 ? py : h - 2;
    const size_t i00 = (size_t) off + (size_t) py * w + px, i10 = i00 + 1, i01 = i00 + w, i11 = i01 + 1;
    const float gu = a_hu * (float) (w - 1), gv = -a_hv * (float) (h - 1);
    sink.add_texel((int) i00, -gu * w0y - gv * w0x); sink.add_texel((int) i10, gu * w0y - gv * w1x);
    sink.add_texel((int) i01, -gu * w1y + gv * w0x); sink.add_texel((int) i11, gu * w1y + gv * w1x);
    const float c = -(tx[i11] - tx[i10] - tx[i01] + tx[i00]) * ((float) (w - 1) * (float) (h - 1));
    au += a_hv * c; av += a_hu * c;
}

// The perturbed normal n' of a height-mapped hit and the intermediate values its adjoint reads:
//     p_u = e1 c1 + e2 c2,  p_v = e1 c3 + e2 c4   (the surface's derivatives along u and v, from the triangle's three UVs: c1 = dv2 / det, c2 = -dv1 / det,
//     c3 = -du2 / det, c4 = du1 / det),   a = p_u - n (n . p_u),  b = p_v - n (n . p_v),  J = n . (a x b),
//     g_u = (b x n) / J,  g_v = (n x a) / J   (the dual basis of (a, b) in the shading plane: it need not be orthogonal),
//     m = n - sigma (h_u g_u + h_v g_v),  n' = normalize(m)
// m . n = 1: n' never points below the shading plane.  flat: no such basis exists (det == 0, !(|J| > 1e-20), or a scene without texture coordinates), n' = n.
template <class M> struct HeightMap { Vec3<M> n, pu, pv, a, b, gu, gv, q, m, n1; M npu, npv, J, hu, hv, sigma; float c1, c2, c3, c4; bool flat; };
template <class G, class M, class TVT>
PSDR_HD HeightMap<M> height_map_frame(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its) {
    HeightMap<M> r;
    r.n = r.n1 = to_m3<M>(its.sh.n);
    r.flat = true;
    if (sc.d.tri_uv == nullptr) return r;
    const float *q = Tab<TVT::flags>::tri_uv(sc, its.tri);
    const float du1 = q[2] - q[0], dv1 = q[3] - q[1], du2 = q[4] - q[0], dv2 = q[5] - q[1], det = du1 * dv2 - du2 * dv1;
    if (det == 0.f) return r;
    const TriRow<G> T = load_tri<G>(sc, tv, its.tri);
    r.c1 = dv2 / det; r.c2 = -dv1 / det; r.c3 = -du2 / det; r.c4 = du1 / det;
    const Vec3<M> e1 = to_m3<M>(T.e1), e2 = to_m3<M>(T.e2);
    r.pu = e1 * r.c1 + e2 * r.c2; r.pv = e1 * r.c3 + e2 * r.c4;
    r.npu = dot(r.n, r.pu); r.npv = dot(r.n, r.pv);
    r.a = r.pu - r.n * r.npu; r.b = r.pv - r.n * r.npv;
    r.J = dot(r.n, cross(r.a, r.b));
    if (!(fabsf(val(r.J)) > 1e-20f)) return r;
    r.flat = false;
    r.gu = cross(r.b, r.n) / r.J; r.gv = cross(r.n, r.a) / r.J;
    r.sigma = b.tex1(sc, tv, PSDR_SLOT_ALPHA_V, its);
    bitmap_grad<M>(sc, tv, b.slot(PSDR_SLOT_K), its.uvx, its.uvy, r.hu, r.hv);
    r.q = r.gu * r.hu + r.gv * r.hv;
    r.m = r.n - r.q * r.sigma;
    r.n1 = normalize(r.m);
    return r;
}

// value = microfacet_lobes(wi', wo') with wi' = Frame(n').to_local(world wi), wo' likewise, where wi.z > 0, wo.z > 0 (the unperturbed side test stays) and
// wi'.z > 0, wo'.z > 0; zero otherwise.  Frame(n') is the project's constructor: the lobes are isotropic, so how the frame is completed around n' does not
// change the value (it depends on wi'.z, wo'.z and wi'.wo' alone).  The two mapped record types differ in how n' is made, nothing else.
template <class G, class M, class TVT>
PSDR_HD bool mapped_directions(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its, const Vec3<G> &wo, bool height, Vec3<M> &wi1, Vec3<M> &wo1) {
    Vec3<M> n1;
    if (height) n1 = height_map_frame<G, M>(sc, tv, b, its).n1;
    else {
        const NormalMap<M> nm = normal_map_frame<G, M>(sc, tv, b, its);
        if (nm.zero) return false;
        n1 = nm.n1;
    }
    const Frame<M> f1(n1);
    wi1 = f1.to_local(to_m3<M>(its.sh.to_world(its.wi))); wo1 = f1.to_local(to_m3<M>(its.sh.to_world(wo)));
    return val(wi1.z) > 0.f && val(wo1.z) > 0.f;
}
// one body for the three record types, so that an instance holds ONE copy of the lobes
template <class G, class M, class TVT>
PSDR_HD Vec3<M> microfacet_any_eval(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its, const Vec3<G> &wo, int type) {
    if (!(val(its.wi.z) > 0.f && val(wo.z) > 0.f)) return zero3<M>();
    Vec3<M> wi_m = to_m3<M>(its.wi), wo_m = to_m3<M>(wo);
    if (type != PSDR_BSDF_MICROFACET) { if (!mapped_directions<G, M>(sc, tv, b, its, wo, type == PSDR_BSDF_MICROFACET_HEIGHT, wi_m, wo_m)) return zero3<M>(); }
    return microfacet_lobes<G, M>(sc, tv, b, its, wi_m, wo_m);
}

// What the adjoint of a normal- or height-mapped record adds to BsdfRev::eval_vjp's outputs: the adjoints of the hit's shading frame (the value reads the WORLD
// directions sh.to_world(wi), sh.to_world(wo) and the shading normal) and of the triangle's two edges (through dp_du / p_u, p_v).  on: the record was of such a type --
// collocated_sample_reverse adds nothing otherwise, so every other record keeps its arithmetic.
struct NormalMapAdj {
    Vec3f s, t, n, e1, e2; bool on;
    PSDR_HD void clear() { s = t = n = e1 = e2 = Vec3f(0.f); on = false; }
};
// a_n' of a normal-mapped hit -> the normal texels (2 a_v: v = 2 c - 1), a_uv, and x: the shading normal, e1, e2 (through dp_du).  Not called where n' = n.
template <class Sink>
PSDR_HD void normal_map_frame_vjp(Sink &sink, const SceneView &sc, const Bsdf<float, float> &b, const Its<float> &its, const NormalMap<float> &nm, const Vec3f &an1,
                                  NormalMapAdj &x, float &auvx, float &auvy) {
    const Vec3f am = normalize_vjp(nm.m, nm.n1, an1);
    const float a_c[3] = {finite_or_zero(2.f * dot(am, nm.s)), finite_or_zero(2.f * dot(am, nm.t)), finite_or_zero(2.f * dot(am, nm.n))};
    bitmap_vjp<Sink, 3>(sink, sc, b.slot(PSDR_SLOT_K), its.uvx, its.uvy, a_c, auvx, auvy);
    // m = s v.x + t v.y + n v.z,  t = n x s,  s = normalize(p),  p = dp - n (n . dp),  dp = e1 c1 + e2 c2
    const Vec3f a_t = am * nm.v.y;
    const Vec3f a_s = am * nm.v.x + cross(a_t, nm.n);
    const Vec3f a_p = normalize_vjp(nm.p, nm.s, a_s);
    const float nap = dot(nm.n, a_p);
    const Vec3f a_dp = a_p - nm.n * nap;
    acc_finite(x.n, am * nm.v.z + cross(nm.s, a_t) - a_p * nm.ndp - nm.dp * nap);
    acc_finite(x.e1, a_dp * nm.c1); acc_finite(x.e2, a_dp * nm.c2);
}
// a_n' of a height-mapped hit -> the scale texel, the height texels and a_uv (bitmap_grad_vjp), and x: the shading normal, e1, e2 (through the dual basis).
// Not called where n' = n.
template <class Sink>
PSDR_HD void height_map_frame_vjp(Sink &sink, const SceneView &sc, const Bsdf<float, float> &b, const Its<float> &its, const HeightMap<float> &hm, const Vec3f &an1,
                                  NormalMapAdj &x, float &auvx, float &auvy) {
    const Vec3f am = normalize_vjp(hm.m, hm.n1, an1);
    // m = n - sigma q,  q = h_u g_u + h_v g_v
    const float a_sigma = finite_or_zero(-dot(am, hm.q));
    bitmap_vjp<Sink, 1>(sink, sc, b.slot(PSDR_SLOT_ALPHA_V), its.uvx, its.uvy, &a_sigma, auvx, auvy);
    bitmap_grad_vjp(sink, sc, b.slot(PSDR_SLOT_K), its.uvx, its.uvy, finite_or_zero(-hm.sigma * dot(am, hm.gu)), finite_or_zero(-hm.sigma * dot(am, hm.gv)), auvx, auvy);
    // g_u = (b x n) / J,  g_v = (n x a) / J,  J = n . (a x b)
    const float invJ = 1.f / hm.J;
    const Vec3f a_gu = am * (-hm.sigma * hm.hu), a_gv = am * (-hm.sigma * hm.hv);
    const Vec3f a_cu = a_gu * invJ, a_cv = a_gv * invJ;
    const float a_J = -(dot(a_gu, hm.gu) + dot(a_gv, hm.gv)) * invJ;
    const Vec3f a_a = cross(a_cv, hm.n) + cross(hm.b, hm.n) * a_J;
    const Vec3f a_b = cross(hm.n, a_cu) + cross(hm.n, hm.a) * a_J;
    // a = p_u - n (n . p_u),  b = p_v - n (n . p_v),  p_u = e1 c1 + e2 c2,  p_v = e1 c3 + e2 c4
    const float naa = dot(hm.n, a_a), nab = dot(hm.n, a_b);
    const Vec3f a_pu = a_a - hm.n * naa, a_pv = a_b - hm.n * nab;
    acc_finite(x.n, am + cross(a_cu, hm.b) + cross(hm.a, a_cv) + cross(hm.a, hm.b) * a_J - a_a * hm.npu - hm.pu * naa - a_b * hm.npv - hm.pv * nab);
    acc_finite(x.e1, a_pu * hm.c1 + a_pv * hm.c3); acc_finite(x.e2, a_pu * hm.c2 + a_pv * hm.c4);
}
// Adjoint of value = microfacet_any_eval(its, wo) of a mapped record (height: type 4, otherwise type 3): af -> awi, awo, the texels of the record's maps, a_uv, x.
// Nothing where the value is defined as zero, nothing to the map's texels (and to the scale, e1, e2) where n' = n.  One body, as the value's.
template <class Sink, class TVT>
PSDR_HD void microfacet_mapped_eval_vjp(Sink &sink, const SceneView &sc, const TVT &tv0, const Bsdf<float, float> &b, const Its<float> &its, const Vec3f &wo,
                                        const Vec3f &af, bool height, Vec3f &awi, Vec3f &awo, NormalMapAdj &x, float &auvx, float &auvy) {
    x.on = true;
    if (!(its.wi.z > 0.f && wo.z > 0.f)) return;
    NormalMap<float> nm; HeightMap<float> hm;
    Vec3f n1; bool flat;
    if (height) { hm = height_map_frame<float, float>(sc, tv0, b, its); n1 = hm.n1; flat = hm.flat; }
    else {
        nm = normal_map_frame<float, float>(sc, tv0, b, its);
        if (nm.zero) return;
        n1 = nm.n1; flat = nm.flat;
    }
    const Frame<float> f1(n1);
    const Vec3f Wi = its.sh.to_world(its.wi), Wo = its.sh.to_world(wo);
    const Vec3f wi1 = f1.to_local(Wi), wo1 = f1.to_local(Wo);
    if (!(wi1.z > 0.f && wo1.z > 0.f)) return;
    Vec3f awi1(0.f), awo1(0.f);
    microfacet_lobes_vjp(sink, sc, tv0, b, its, wi1, wo1, af, awi1, awo1, auvx, auvy);
    // wi' = (Wi . s1, Wi . t1, Wi . n'), (s1, t1, n') = Frame(n')
    // ... and Wi = sh.s wi.x + sh.t wi.y + sh.n wi.z, as forward mode evaluates it (Wo likewise)
    const Vec3f aWi = f1.to_world(awi1), aWo = f1.to_world(awo1);
    acc_finite(awi, its.sh.to_local(aWi)); acc_finite(awo, its.sh.to_local(aWo));
    acc_finite(x.s, aWi * its.wi.x + aWo * wo.x); acc_finite(x.t, aWi * its.wi.y + aWo * wo.y); acc_finite(x.n, aWi * its.wi.z + aWo * wo.z);
    const Vec3f an1 = Wi * awi1.z + Wo * awo1.z + frame_vjp(n1, Wi * awi1.x + Wo * awo1.x, Wi * awi1.y + Wo * awo1.y);
    if (flat) { acc_finite(x.n, an1); return; }
    if (height) height_map_frame_vjp(sink, sc, b, its, hm, an1, x, auvx, auvy);
    else normal_map_frame_vjp(sink, sc, b, its, nm, an1, x, auvx, auvy);
}

// The collocated estimator's BSDF value and its adjoint: MicrofacetBSDF by the record's type where the instance carries the GGX code (ROUGH), Bsdf::eval /
// BsdfRev::eval_vjp for every other record and in every other instance
template <bool ROUGH, class G, class M, class TVT>
PSDR_HD Vec3<M> colloc_bsdf_eval(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its, const Vec3<G> &wo) {
    if constexpr (ROUGH) {
        const int type = b.type();
        if (type >= PSDR_BSDF_MICROFACET && type <= PSDR_BSDF_MICROFACET_HEIGHT) return microfacet_any_eval<G, M>(sc, tv, b, its, wo, type);
    }
    return b.eval(sc, tv, its, wo, true);
}
// x: what a normal- or height-mapped record adds (NormalMapAdj); untouched by every other record
template <class Sink, class TVT>
PSDR_HD void colloc_bsdf_eval_vjp(Sink &sink, const SceneView &sc, const TVT &tv0, const BsdfRev<Sink> &brev, const Its<float> &its, const Vec3f &wo, const Vec3f &af,
                                  Vec3f &awi, Vec3f &awo, float &auvx, float &auvy, NormalMapAdj &x) {
    if constexpr ((Sink::flags & kSceneRough) != 0) {
        if (brev.b.type() == PSDR_BSDF_MICROFACET) { microfacet_eval_vjp(sink, sc, tv0, brev.b, its, wo, af, awi, awo, auvx, auvy); return; }
        const int type = brev.b.type();
        if (type == PSDR_BSDF_MICROFACET_NORMAL || type == PSDR_BSDF_MICROFACET_HEIGHT) {
            microfacet_mapped_eval_vjp(sink, sc, tv0, brev.b, its, wo, af, type == PSDR_BSDF_MICROFACET_HEIGHT, awi, awo, x, auvx, auvy);
            return;
        }
    }
    brev.eval_vjp(sink, tv0, its, wo, af, awi, awo, auvx, auvy);
}

}  // namespace psdr
