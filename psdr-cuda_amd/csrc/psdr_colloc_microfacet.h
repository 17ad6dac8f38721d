// psdr_colloc_microfacet.h -- MicrofacetBSDF (PSDR_BSDF_MICROFACET, include/psdr_hip.h): a Lambertian diffuse lobe plus an isotropic
// GGX specular lobe with a Schlick Fresnel term.  Build-defined: the reference snapshot has no such BSDF.  For local directions with wi.z > 0 and wo.z > 0
// (zero otherwise), cosine included like Bsdf::eval:
//     h = normalize(wi + wo)
//     f cos(theta_o) = kd / pi * wo.z  +  F(wi.h) D(h) G1(wi, h) G1(wo, h) / (4 wi.z),      F(c) = F0 + (1 - F0) (1 - c)^5
// with D and G1 the project's GGX<M>{alpha, alpha} (psdr_device.h, their cut-offs included) and alpha = r^2.  Record slots: kd = PSDR_SLOT_REFLECTANCE,
// r = PSDR_SLOT_ALPHA_U, F0 = PSDR_SLOT_ETA.  Where D's cut-off answers zero -- alpha = 0 among the cases -- the specular lobe is zero and the value is
// the diffuse lobe.
// The model is an evaluation and its adjoint, no sample / pdf: the CollocatedIntegrator (psdr_collocated.h) evaluates f at ONE direction pair, wo = wi (there
// h = wi and F = F0), and is the only integrator that serves the type.  Both functions take a general wo all the same.
// Compiled only into the flag sets that carry the GGX code (kSceneRough); the Lambertian ones keep their text.
#pragma once
#include "psdr_reverse.h"

namespace psdr {

// G: geometry type of the hit and the directions, M: material / result type -- plain floats, Dual<1> and Dual<3> go through this one copy
template <class G, class M, class TVT>
PSDR_HD Vec3<M> microfacet_eval(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its, const Vec3<G> &wo, bool active) {
    if (!(active && val(its.wi.z) > 0.f && val(wo.z) > 0.f)) return zero3<M>();
    const Vec3<M> diffuse = b.tex3(sc, tv, PSDR_SLOT_REFLECTANCE, its) * (wo.z * kInvPi);
    const M alpha = sqr(b.tex1(sc, tv, PSDR_SLOT_ALPHA_U, its));
    const GGX<M> g{alpha, alpha};
    const Vec3<M> wi_m = to_m3<M>(its.wi), wo_m = to_m3<M>(wo);
    const Vec3<M> H = normalize(wo_m + wi_m);
    const M D = g.eval(H);
    if (val(D) == 0.f) return diffuse;
    const M res = D * (g.smith_g1(wi_m, H) * g.smith_g1(wo_m, H)) / (4.f * wi_m.z);
    const Vec3<M> F0 = b.tex3(sc, tv, PSDR_SLOT_ETA, its);
    const M t = 1.f - dot(wi_m, H);
    const M w = sqr(sqr(t)) * t;
    return {diffuse.x + (F0.x + (1.f - F0.x) * w) * res, diffuse.y + (F0.y + (1.f - F0.y) * w) * res, diffuse.z + (F0.z + (1.f - F0.z) * w) * res};
}

// Adjoint of value = microfacet_eval(its, wo), with BsdfRev::eval_vjp's signature: af (RGB) -> awi, awo, the texels of the three maps (through the sink), a_uv.
// The geometric part D G1 G1 / (4 wi.z) and the Fresnel cosine go through ggx_geo_vjp (psdr_reverse.h), the rough conductor's own.  An adjoint that is not
// finite (alpha at the edge of fp32) is dropped like the sample's value is (zero_nonfinite).
template <class Sink, class TVT>
PSDR_HD void microfacet_eval_vjp(Sink &sink, const SceneView &sc, const TVT &tv0, const Bsdf<float, float> &b, const Its<float> &its, const Vec3f &wo,
                                 const Vec3f &af, Vec3f &awi, Vec3f &awo, float &auvx, float &auvy) {
    if (!(its.wi.z > 0.f && wo.z > 0.f)) return;
    {   // kd / pi * wo.z
        const Vec3f kd = b.tex3(sc, tv0, PSDR_SLOT_REFLECTANCE, its);
        const float c = wo.z * kInvPi;
        const float a_kd[3] = {af.x * c, af.y * c, af.z * c};
        bitmap_vjp<Sink, 3>(sink, sc, b.slot(PSDR_SLOT_REFLECTANCE), its.uvx, its.uvy, a_kd, auvx, auvy);
        awo.z += dot(af, kd) * kInvPi;
    }
    const float r = b.tex1(sc, tv0, PSDR_SLOT_ALPHA_U, its), alpha = r * r;
    const GgxAdj v0 = ggx_geo_vjp<true>(its.wi, wo, alpha, alpha, 0.f, 0.f);          // value pass: geo = D G1 G1 / (4 wi.z), c = wi.h
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
    const GgxAdj ga = ggx_geo_vjp<true>(its.wi, wo, alpha, alpha, a_geo, a_c);
    acc_finite(awi, ga.wi); acc_finite(awo, ga.wo);
    const float a_r = finite_or_zero((ga.au + ga.av) * (2.f * r));          // alpha_u = alpha_v = r^2
    bitmap_vjp<Sink, 1>(sink, sc, b.slot(PSDR_SLOT_ALPHA_U), its.uvx, its.uvy, &a_r, auvx, auvy);
    bitmap_vjp<Sink, 3>(sink, sc, b.slot(PSDR_SLOT_ETA), its.uvx, its.uvy, a_f0, auvx, auvy);
}

// The collocated estimator's BSDF value and its adjoint: MicrofacetBSDF by the record's type where the instance carries the GGX code (ROUGH), Bsdf::eval /
// BsdfRev::eval_vjp for every other record and in every other instance
template <bool ROUGH, class G, class M, class TVT>
PSDR_HD Vec3<M> colloc_bsdf_eval(const SceneView &sc, const TVT &tv, const Bsdf<G, M> &b, const Its<G> &its, const Vec3<G> &wo) {
    if constexpr (ROUGH) { if (b.type() == PSDR_BSDF_MICROFACET) return microfacet_eval<G, M>(sc, tv, b, its, wo, true); }
    return b.eval(sc, tv, its, wo, true);
}
template <class Sink, class TVT>
PSDR_HD void colloc_bsdf_eval_vjp(Sink &sink, const SceneView &sc, const TVT &tv0, const BsdfRev<Sink> &brev, const Its<float> &its, const Vec3f &wo, const Vec3f &af,
                                  Vec3f &awi, Vec3f &awo, float &auvx, float &auvy) {
    if constexpr ((Sink::flags & kSceneRough) != 0) {
        if (brev.b.type() == PSDR_BSDF_MICROFACET) { microfacet_eval_vjp(sink, sc, tv0, brev.b, its, wo, af, awi, awo, auvx, auvy); return; }
    }
    brev.eval_vjp(sink, tv0, its, wo, af, awi, awo, auvx, auvy);
}

}  // namespace psdr
