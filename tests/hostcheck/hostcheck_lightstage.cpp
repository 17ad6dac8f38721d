// hostcheck_lightstage.cpp -- TEST-ONLY harness: the LightStageIntegrator's estimator (csrc/psdr_lightstage.h, PSDR_HD functions) run on the host, slot by slot,
// with the loop over the lights the kernels of csrc/psdr_lightstage.hip run: one hit per slot, then every light.  The edge terms run per light, as the launches
// do, through the PointLightIntegrator's functions (csrc/psdr_pointlight.h).  A library of its own (libhostcheck_lightstage.so), as hostcheck_pointlight.cpp is
// for its header.  Never imported by the psdr_cuda package and not a fallback: the render path only ever executes these functions inside HIP kernels.
// tests/hostcheck/lightstage_san.cpp includes this file into a stand-alone program for the host sanitizers.
#include "host_common.h"
#include "../../psdr-cuda_amd/csrc/psdr_lightstage.h"

namespace {
// mode 0: renderC (unit intensities); mode 1: renderD forward with K tangent sets (tan: [K], d_pos: [K][L][3] or null): interior + primary edges + shadow
// boundary, each under its own sample count; img: [L][W H 3], dimg: [K][L][W H 3].  Per-thread images in double, summed in thread order.
template <int K>
int render_k(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, const psdr_tangents *tan, int L, const float *pos, const float *d_pos, float *img, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const LightTable lt{pos, mode ? d_pos : nullptr, L};
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    ThreadImages acc(nthreads, n3 * L), dacc(nthreads, mode ? n3 * L * K : 0);
    TangentView<K, kSceneAll> tvk;
    bool geo = mode && d_pos;
    for (int k = 0; k < K; ++k) { tvk.t[k] = tan ? tan[k] : psdr_tangents{}; geo = geo || tvk.t[k].d_tri_info || tvk.t[k].d_cam_to_world; }
    const TangentView<0, kSceneAll> tv0{};
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp > 0 && nsp > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[0]);
        pfor(WH * nsp, nthreads, [&](long long a, long long b, int t) {
            TraversalStack st; uint32_t nr = 0;
            for (long long j = a; j < b; ++j) {
                const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
                const uint64_t slot = (uint64_t) pixel * o->spp + s;
                if (mode == 0) {
                    const StackHit<float> h = stack_camera_hit<float>(hs.sc, tv0, st, jump, pixel, slot, nr);
                    if (!h.ok) continue;
                    const Bsdf<float, float> bsdf(hs.sc, tv0, h.bsdf_id);
                    for (int l = 0; l < L; ++l) {
                        const Vec3f r = stack_light_value<float, float>(hs.sc, tv0, st, bsdf, h.its, stack_light<1>(lt, l), nr);
                        acc.add3(t, (int) (l * WH) + pixel, r.x / o->spp, r.y / o->spp, r.z / o->spp);
                    }
                } else {
                    const auto one = [&](auto gtag) {
                        using G = decltype(gtag);
                        const StackHit<G> h = stack_camera_hit<G>(hs.sc, tvk, st, jump, pixel, slot, nr);
                        if (!h.ok) return;
                        const Bsdf<G, Dual<K>> bsdf(hs.sc, tvk, h.bsdf_id);
                        for (int l = 0; l < L; ++l) {
                            const Vec3<Dual<K>> r = stack_light_value<G, Dual<K>>(hs.sc, tvk, st, bsdf, h.its, stack_light<K>(lt, l), nr);
                            acc.add3(t, (int) (l * WH) + pixel, r.x.v / o->spp, r.y.v / o->spp, r.z.v / o->spp);
                            for (int k = 0; k < K; ++k) dacc.add3(t, (int) (((long long) k * L + l) * WH) + pixel, r.x.d[k] / o->spp, r.y.d[k] / o->spp, r.z.d[k] / o->spp);
                        }
                    };
                    if (geo) one(Dual<K>(0.f)); else one(0.f);
                }
            }
        });
    }
    // the edge terms, per light (the launches run the PointLightIntegrator's kernels once per light)
    for (int l = 0; l < L && mode == 1; ++l) {
        const PointLight pl = stack_light<K>(lt, l);
        const auto splat = [&](int t, int pix, const float tg[K][3]) { for (int k = 0; k < K; ++k) dacc.add3(t, (int) (((long long) k * L + l) * WH) + pix, tg[k][0], tg[k][1], tg[k][2]); };
        if (o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0) {
            const RngJump jump = make_rng_jump(o->rng_offset[1]);
            const long long i0 = WH * o->sppe_begin, n = WH * (o->sppe_end - o->sppe_begin);
            const PointLi li{pl};
            pfor(n, nthreads, [&](long long a, long long b, int t) {
                TraversalStack st; uint32_t nr = 0;
                for (long long j = a; j < b; ++j) {
                    float tg[K][3];
                    const int pix = collocated_edge_sample<K, kSceneAll>(hs.sc, tvk, st, jump, (uint64_t) (i0 + j), 1.f / o->sppe, tg, nr, li);
                    if (pix >= 0) splat(t, pix, tg);
                }
            });
        }
        if (o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0) {
            const RngJump jump = make_rng_jump(o->rng_offset[2]);
            const long long i0 = WH * o->sppse_begin, n = WH * (o->sppse_end - o->sppse_begin);
            pfor(n, nthreads, [&](long long a, long long b, int t) {
                TraversalStack st; uint32_t nr = 0;
                for (long long j = a; j < b; ++j) {
                    Rng rng; rng.init((uint64_t) (i0 + j), jump);
                    const float s3[3] = {rng.next(), rng.next(), rng.next()};
                    float tg[K][3];
                    const int pix = point_sedge_sample<K, kSceneAll>(hs.sc, tvk, st, pl, s3, 1.f / o->sppse, tg, nr);
                    if (pix >= 0) splat(t, pix, tg);
                }
            });
        }
    }
    acc.reduce(img);
    if (mode && dimg) dacc.reduce(dimg);
    return 0;
}
}  // namespace

extern "C" {

// mode 0: renderC; mode 1: forward mode with K = 1 or 3 tangent sets.  pos [L][3]; tan [K] or null; d_pos [K][L][3] or null; img [L][W H 3]; dimg [K][L][W H 3]
int hostcheck_lightstage_render(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, int K, const psdr_tangents *tan, int L, const float *pos, const float *d_pos,
                                float *img, float *dimg, int nthreads) {
    if (L < 1 || (K != 1 && K != 3)) return 2;
    return K == 1 ? render_k<1>(d, o, mode, tan, L, pos, d_pos, img, dimg, nthreads) : render_k<3>(d, o, mode, tan, L, pos, d_pos, img, dimg, nthreads);
}

// reverse mode: adj [L][W H 3]; the gradient tables `grads` names (zeroed by the caller), the lights' gradients g_pos [L][3] (+=, or null), and the images
// [L][W H 3] if img is not null
int hostcheck_lightstage_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int L, const float *pos, const float *adj, float *img, const psdr_grads *grads, float *g_pos) {
    if (L < 1) return 2;
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const LightTable lt{pos, nullptr, L};
    HostSink sink; sink.g = *grads;
    const bool geo = grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr || g_pos != nullptr;
    const long long WH = (long long) d->width * d->height;
    TraversalStack st; uint32_t nr = 0;
    std::vector<double> acc((size_t) WH * 3 * L, 0.0), gp((size_t) 3 * L, 0.0);
    const int nsp = o->spp_end - o->spp_begin;
    const auto camera = [&](auto geo_tag) {
        constexpr bool GEO = decltype(geo_tag)::value;
        using CamSink = typename CameraSinkOf<GEO, HostSink>::type;
        const RngJump jump = make_rng_jump(o->rng_offset[0]);
        const float inv = 1.f / o->spp;
        for (long long j = 0; j < WH * nsp; ++j) {
            const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
            PrimaryGrad pg; pg.clear();
            StackRevHit H;
            stack_rev_begin<GEO, kSceneAll>(H, hs.sc, st, jump, pixel, (uint64_t) pixel * o->spp + s, nr);
            if (!H.ok) continue;
            CamSink csink(sink, pg);
            const BsdfRev<CamSink> brev(hs.sc, H.bsdf_id);
            for (int l = 0; l < L; ++l) {
                const float *a = adj + ((size_t) l * WH + pixel) * 3;
                Vec3f apl(0.f);
                const Vec3f r = stack_rev_light<GEO>(csink, pg, hs.sc, st, brev, H, stack_light<1>(lt, l), Vec3f{a[0] * inv, a[1] * inv, a[2] * inv}, nr, apl);
                gp[3 * l] += apl.x; gp[3 * l + 1] += apl.y; gp[3 * l + 2] += apl.z;
                double *p = &acc[((size_t) l * WH + pixel) * 3];
                p[0] += r.x * inv; p[1] += r.y * inv; p[2] += r.z * inv;
            }
            stack_rev_end<GEO>(csink, hs.sc, H);
            if (pg.tri >= 0) for (int w = 0; w < kPrimaryWords; ++w) sink.add_tri(pg.tri, w, pg.w[w]);
        }
    };
    if (o->spp > 0 && nsp > 0) { if (geo) camera(std::true_type{}); else camera(std::false_type{}); }
    for (int l = 0; l < L; ++l) {
        const PointLight pl = stack_light<1>(lt, l);
        const float *adj_l = adj + (size_t) l * WH * 3;
        if (o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0 && grads->g_prim_edge) {
            const RngJump jump = make_rng_jump(o->rng_offset[1]);
            const PointLi li{pl};
            for (long long j = WH * o->sppe_begin; j < WH * o->sppe_end; ++j) {
                float w[4];
                const int k = collocated_edge_reverse_values<kSceneAll>(hs.sc, st, jump, (uint64_t) j, 1.f / o->sppe, adj_l, nr, w, li);
                if (k >= 0) for (int i = 0; i < 4; ++i) sink.add_pedge(k, i, w[i]);
            }
        }
        if (o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0 && (grads->g_sec_edge || grads->g_tri_info || g_pos)) {
            const RngJump jump = make_rng_jump(o->rng_offset[2]);
            for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
                Rng rng; rng.init((uint64_t) j, jump);
                const float s3[3] = {rng.next(), rng.next(), rng.next()};
                Vec3f apl(0.f);
                point_sedge_reverse(sink, hs.sc, st, pl, s3, 1.f / o->sppse, adj_l, nr, apl);
                gp[3 * l] += apl.x; gp[3 * l + 1] += apl.y; gp[3 * l + 2] += apl.z;
            }
        }
    }
    if (g_pos) for (int i = 0; i < 3 * L; ++i) g_pos[i] += (float) gp[i];
    if (img) for (size_t i = 0; i < acc.size(); ++i) img[i] = (float) acc[i];
    return 0;
}
}
