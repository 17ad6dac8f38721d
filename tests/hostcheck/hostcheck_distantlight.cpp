// hostcheck_distantlight.cpp -- TEST-ONLY harness: the estimators of the PointLightIntegrator and the LightStageIntegrator (csrc/psdr_pointlight.h,
// csrc/psdr_lightstage.h, PSDR_HD functions) run on the host, slot by slot, with a LIGHT MODEL PER LIGHT (PSDR_LIGHT_POINT / PSDR_LIGHT_DISTANT): the single
// light through the functions the kernels of csrc/psdr_pointlight.hip instantiate, the stack with the loop the kernels of csrc/psdr_lightstage.hip run (one hit
// per slot, then every light, a branch on the light's kind) and the edge terms per light.  A library of its own (libhostcheck_distantlight.so), beside
// hostcheck_pointlight.cpp and hostcheck_lightstage.cpp, which keep the point model.  Never imported by the psdr_cuda package and not a fallback: the render
// path only ever executes these functions inside HIP kernels.  tests/hostcheck/distantlight_san.cpp includes this file into a stand-alone program for the
// host sanitizers.
#include "host_common.h"
#include "../../psdr-cuda_amd/csrc/psdr_lightstage.h"

namespace {
template <int LK> using Kind = std::integral_constant<int, LK>;
// f(Kind<LK>{}) for the light's kind
template <class F> auto by_kind(int kind, F &&f) { return kind == PSDR_LIGHT_DISTANT ? f(Kind<kLightDistant>{}) : f(Kind<kLightPoint>{}); }
bool kind_ok(int kind) { return kind == PSDR_LIGHT_POINT || kind == PSDR_LIGHT_DISTANT; }

// the light with K tangents (d_v: [K][3] or null)
PointLight make_light(const float *v, const float *d_v, int K = 1) {
    PointLight pl{};
    for (int c = 0; c < 3; ++c) pl.p[c] = v[c];
    for (int k = 0; k < K && d_v; ++k) for (int c = 0; c < 3; ++c) pl.d[k][c] = d_v[3 * k + c];
    return pl;
}

// The two edge terms of forward mode for one light: splat(thread, pixel, tg[K][3])
template <int K, int LK, class Splat>
void edges_fwd(const HostScene &hs, const psdr_scene_desc *d, const psdr_render_opts *o, const TangentView<K, kSceneAll> &tvk, const PointLight &pl, int nthreads, const Splat &splat) {
    const long long WH = (long long) d->width * d->height;
    if (o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[1]);
        const long long i0 = WH * o->sppe_begin, n = WH * (o->sppe_end - o->sppe_begin);
        const PointLiOf<LK> li{pl};
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
                const int pix = point_sedge_sample<K, kSceneAll, LK>(hs.sc, tvk, st, pl, s3, 1.f / o->sppse, tg, nr);
                if (pix >= 0) splat(t, pix, tg);
            }
        });
    }
}
// ... and of reverse mode: adj: the light's plane; gp [3]: the gradient of the light's vector (+=)
template <int LK>
void edges_rev(const HostScene &hs, const psdr_scene_desc *d, const psdr_render_opts *o, HostSink &sink, const psdr_grads *grads, const PointLight &pl, const float *adj, bool want_gv, double *gp) {
    const long long WH = (long long) d->width * d->height;
    TraversalStack st; uint32_t nr = 0;
    if (o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0 && grads->g_prim_edge) {
        const RngJump jump = make_rng_jump(o->rng_offset[1]);
        const PointLiOf<LK> li{pl};
        for (long long j = WH * o->sppe_begin; j < WH * o->sppe_end; ++j) {
            float w[4];
            const int k = collocated_edge_reverse_values<kSceneAll>(hs.sc, st, jump, (uint64_t) j, 1.f / o->sppe, adj, nr, w, li);
            if (k >= 0) for (int i = 0; i < 4; ++i) sink.add_pedge(k, i, w[i]);
        }
    }
    if (o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0 && (grads->g_sec_edge || grads->g_tri_info || want_gv)) {
        const RngJump jump = make_rng_jump(o->rng_offset[2]);
        for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
            Rng rng; rng.init((uint64_t) j, jump);
            const float s3[3] = {rng.next(), rng.next(), rng.next()};
            Vec3f apl(0.f);
            point_sedge_reverse<LK>(sink, hs.sc, st, pl, s3, 1.f / o->sppse, adj, nr, apl);
            gp[0] += apl.x; gp[1] += apl.y; gp[2] += apl.z;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------ one light (kind 4)
// mode 0: renderC (unit intensity / irradiance); mode 1: renderD forward with K tangent sets (tan: [K], d_v: [K][3] or null); dimg: [K][W H 3]
template <int K, int LK>
int render_one(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, const psdr_tangents *tan, const float *v, const float *d_v, float *img, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const PointLight pl = make_light(v, mode ? d_v : nullptr, K);
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    ThreadImages acc(nthreads, n3), dacc(nthreads, mode ? n3 * K : 0);
    TangentView<K, kSceneAll> tvk;
    bool geo = mode && d_v;
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
                    const Vec3f r = point_camera_sample<float, float, LK>(hs.sc, tv0, st, pl, jump, pixel, slot, nr);
                    acc.add3(t, pixel, r.x / o->spp, r.y / o->spp, r.z / o->spp);
                } else {
                    const Vec3<Dual<K>> r = geo ? point_camera_sample<Dual<K>, Dual<K>, LK>(hs.sc, tvk, st, pl, jump, pixel, slot, nr)
                                                : point_camera_sample<float, Dual<K>, LK>(hs.sc, tvk, st, pl, jump, pixel, slot, nr);
                    acc.add3(t, pixel, r.x.v / o->spp, r.y.v / o->spp, r.z.v / o->spp);
                    for (int k = 0; k < K; ++k) dacc.add3(t, (int) (k * WH) + pixel, r.x.d[k] / o->spp, r.y.d[k] / o->spp, r.z.d[k] / o->spp);
                }
            }
        });
    }
    if (mode == 1)
        edges_fwd<K, LK>(hs, d, o, tvk, pl, nthreads, [&](int t, int pix, const float tg[K][3]) { for (int k = 0; k < K; ++k) dacc.add3(t, (int) (k * WH) + pix, tg[k][0], tg[k][1], tg[k][2]); });
    acc.reduce(img);
    if (mode && dimg) dacc.reduce(dimg);
    return 0;
}

template <int LK>
int rev_one(const psdr_scene_desc *d, const psdr_render_opts *o, const float *v, const float *adj, float *img, const psdr_grads *grads, float *g_v) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const PointLight pl = make_light(v, nullptr);
    HostSink sink; sink.g = *grads;
    const bool geo = grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr || g_v != nullptr;
    const long long WH = (long long) d->width * d->height;
    TraversalStack st; uint32_t nr = 0;
    std::vector<double> acc((size_t) WH * 3, 0.0);
    double gp[3] = {0.0, 0.0, 0.0};
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp > 0 && nsp > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[0]);
        for (long long j = 0; j < WH * nsp; ++j) {
            const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
            const float inv = 1.f / o->spp;
            const Vec3f a{adj[pixel * 3] * inv, adj[pixel * 3 + 1] * inv, adj[pixel * 3 + 2] * inv};
            PrimaryGrad pg;
            Vec3f apl(0.f);
            const uint64_t slot = (uint64_t) pixel * o->spp + s;
            const Vec3f r = geo ? point_sample_reverse<true, LK>(sink, pg, hs.sc, st, pl, jump, pixel, slot, a, nr, apl) : point_sample_reverse<false, LK>(sink, pg, hs.sc, st, pl, jump, pixel, slot, a, nr, apl);
            if (pg.tri >= 0) for (int w = 0; w < kPrimaryWords; ++w) sink.add_tri(pg.tri, w, pg.w[w]);
            gp[0] += apl.x; gp[1] += apl.y; gp[2] += apl.z;
            acc[pixel * 3] += r.x * inv; acc[pixel * 3 + 1] += r.y * inv; acc[pixel * 3 + 2] += r.z * inv;
        }
    }
    edges_rev<LK>(hs, d, o, sink, grads, pl, adj, g_v != nullptr, gp);
    if (g_v) for (int c = 0; c < 3; ++c) g_v[c] += (float) gp[c];
    if (img) for (size_t i = 0; i < acc.size(); ++i) img[i] = (float) acc[i];
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------ a stack (kind 5)
// img: [L][W H 3], dimg: [K][L][W H 3]; v [L][3], d_v [K][L][3] or null, kinds [L]
template <int K>
int render_stack(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, const psdr_tangents *tan, int L, const int32_t *kinds, const float *v, const float *d_v, float *img, float *dimg,
                 int nthreads) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const LightTable lt{v, mode ? d_v : nullptr, L, kinds};
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    ThreadImages acc(nthreads, n3 * L), dacc(nthreads, mode ? n3 * L * K : 0);
    TangentView<K, kSceneAll> tvk;
    bool geo = mode && d_v;
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
                        const PointLight pl = stack_light<1>(lt, l);
                        const Vec3f r = stack_light_distant(lt, l) ? stack_light_value<float, float, kLightDistant>(hs.sc, tv0, st, bsdf, h.its, pl, nr)
                                                                   : stack_light_value<float, float, kLightPoint>(hs.sc, tv0, st, bsdf, h.its, pl, nr);
                        acc.add3(t, (int) (l * WH) + pixel, r.x / o->spp, r.y / o->spp, r.z / o->spp);
                    }
                } else {
                    const auto one = [&](auto gtag) {
                        using G = decltype(gtag);
                        const StackHit<G> h = stack_camera_hit<G>(hs.sc, tvk, st, jump, pixel, slot, nr);
                        if (!h.ok) return;
                        const Bsdf<G, Dual<K>> bsdf(hs.sc, tvk, h.bsdf_id);
                        for (int l = 0; l < L; ++l) {
                            const PointLight pl = stack_light<K>(lt, l);
                            const Vec3<Dual<K>> r = stack_light_distant(lt, l) ? stack_light_value<G, Dual<K>, kLightDistant>(hs.sc, tvk, st, bsdf, h.its, pl, nr)
                                                                               : stack_light_value<G, Dual<K>, kLightPoint>(hs.sc, tvk, st, bsdf, h.its, pl, nr);
                            acc.add3(t, (int) (l * WH) + pixel, r.x.v / o->spp, r.y.v / o->spp, r.z.v / o->spp);
                            for (int k = 0; k < K; ++k) dacc.add3(t, (int) (((long long) k * L + l) * WH) + pixel, r.x.d[k] / o->spp, r.y.d[k] / o->spp, r.z.d[k] / o->spp);
                        }
                    };
                    if (geo) one(Dual<K>(0.f)); else one(0.f);
                }
            }
        });
    }
    // the edge terms, per light (the launches run the PointLightIntegrator's kernels of the light's kind once per light)
    for (int l = 0; l < L && mode == 1; ++l) {
        const PointLight pl = stack_light<K>(lt, l);
        const auto splat = [&](int t, int pix, const float tg[K][3]) { for (int k = 0; k < K; ++k) dacc.add3(t, (int) (((long long) k * L + l) * WH) + pix, tg[k][0], tg[k][1], tg[k][2]); };
        by_kind(kinds[l], [&](auto kind) { edges_fwd<K, decltype(kind)::value>(hs, d, o, tvk, pl, nthreads, splat); return 0; });
    }
    acc.reduce(img);
    if (mode && dimg) dacc.reduce(dimg);
    return 0;
}
}  // namespace

extern "C" {

// One light.  mode 0: renderC; mode 1: forward mode with K = 1 or 3 tangent sets.  v [3]: position or direction by kind; tan [K] or null; d_v [K][3] or null;
// img [W H 3]; dimg [K][W H 3]
int hostcheck_distantlight_render(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, int K, const psdr_tangents *tan, int kind, const float *v, const float *d_v, float *img,
                                  float *dimg, int nthreads) {
    if (!kind_ok(kind) || (K != 1 && K != 3)) return 2;
    return by_kind(kind, [&](auto k) {
        constexpr int LK = decltype(k)::value;
        return K == 1 ? render_one<1, LK>(d, o, mode, tan, v, d_v, img, dimg, nthreads) : render_one<3, LK>(d, o, mode, tan, v, d_v, img, dimg, nthreads);
    });
}
// reverse mode: the gradient tables `grads` names (zeroed by the caller), the gradient of the light's vector g_v [3] (+=, or null), and the image if img is not null
int hostcheck_distantlight_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int kind, const float *v, const float *adj, float *img, const psdr_grads *grads, float *g_v) {
    if (!kind_ok(kind)) return 2;
    return by_kind(kind, [&](auto k) { return rev_one<decltype(k)::value>(d, o, v, adj, img, grads, g_v); });
}

// A stack.  kinds [L]; v [L][3]; tan [K] or null; d_v [K][L][3] or null; img [L][W H 3]; dimg [K][L][W H 3]
int hostcheck_distantstack_render(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, int K, const psdr_tangents *tan, int L, const int32_t *kinds, const float *v, const float *d_v,
                                  float *img, float *dimg, int nthreads) {
    if (L < 1 || (K != 1 && K != 3)) return 2;
    for (int l = 0; l < L; ++l) if (!kind_ok(kinds[l])) return 2;
    return K == 1 ? render_stack<1>(d, o, mode, tan, L, kinds, v, d_v, img, dimg, nthreads) : render_stack<3>(d, o, mode, tan, L, kinds, v, d_v, img, dimg, nthreads);
}
// reverse mode: adj [L][W H 3]; the gradient tables `grads` names (zeroed by the caller), the lights' gradients g_v [L][3] (+=, or null), and the images
// [L][W H 3] if img is not null
int hostcheck_distantstack_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int L, const int32_t *kinds, const float *v, const float *adj, float *img, const psdr_grads *grads, float *g_v) {
    if (L < 1) return 2;
    for (int l = 0; l < L; ++l) if (!kind_ok(kinds[l])) return 2;
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const LightTable lt{v, nullptr, L, kinds};
    HostSink sink; sink.g = *grads;
    const bool geo = grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr || g_v != nullptr;
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
                const Vec3f al{a[0] * inv, a[1] * inv, a[2] * inv};
                const PointLight pl = stack_light<1>(lt, l);
                Vec3f apl(0.f);
                const Vec3f r = stack_light_distant(lt, l) ? stack_rev_light<GEO, kLightDistant>(csink, pg, hs.sc, st, brev, H, pl, al, nr, apl)
                                                           : stack_rev_light<GEO, kLightPoint>(csink, pg, hs.sc, st, brev, H, pl, al, nr, apl);
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
        by_kind(kinds[l], [&](auto kind) { edges_rev<decltype(kind)::value>(hs, d, o, sink, grads, pl, adj + (size_t) l * WH * 3, g_v != nullptr, &gp[3 * (size_t) l]); return 0; });
    }
    if (g_v) for (int i = 0; i < 3 * L; ++i) g_v[i] += (float) gp[i];
    if (img) for (size_t i = 0; i < acc.size(); ++i) img[i] = (float) acc[i];
    return 0;
}
}
