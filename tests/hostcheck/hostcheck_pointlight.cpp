// hostcheck_pointlight.cpp -- TEST-ONLY harness: the PointLightIntegrator's estimator (csrc/psdr_pointlight.h, PSDR_HD functions) run on the host, slot by slot,
// so that `-m "not gpu"` tests can check it where no GPU exists and the GPU tests have a reference the oracle does not offer (the reference snapshot has no such
// integrator).  A library of its own (libhostcheck_pointlight.so), as hostcheck_collocated.cpp is for its header.  Never imported by the psdr_cuda package and
// not a fallback: the render path only ever executes these functions inside HIP kernels.  tests/hostcheck/pointlight_san.cpp includes this file into a
// stand-alone program for the host sanitizers.
#include "host_common.h"
#include "../../psdr-cuda_amd/csrc/psdr_pointlight.h"

namespace {
// the light with K tangents (d_pos: [K][3] or null)
PointLight make_light(const float *pos, const float *d_pos, int K = 1) {
    PointLight pl{};
    for (int c = 0; c < 3; ++c) pl.p[c] = pos[c];
    for (int k = 0; k < K && d_pos; ++k) for (int c = 0; c < 3; ++c) pl.d[k][c] = d_pos[3 * k + c];
    return pl;
}

// mode 0: renderC (unit intensity); mode 1: renderD forward with K tangent sets (tan: [K], d_pos: [K][3] or null): interior + primary edges + shadow boundary,
// each under its own sample count (spp, sppe, sppse of *o); dimg: [K][W H 3].  Per-thread images in double, summed in thread order.
template <int K>
int render_k(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, const psdr_tangents *tan, const float *pos, const float *d_pos, float *img, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const PointLight pl = make_light(pos, mode ? d_pos : nullptr, K);
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    ThreadImages acc(nthreads, n3), dacc(nthreads, mode ? n3 * K : 0);
    TangentView<K, kSceneAll> tvk;
    bool geo = mode && d_pos;
    for (int k = 0; k < K; ++k) { tvk.t[k] = tan ? tan[k] : psdr_tangents{}; geo = geo || tvk.t[k].d_tri_info || tvk.t[k].d_cam_to_world; }
    const TangentView<0, kSceneAll> tv0{};
    const auto splat = [&](int t, int pix, const float tg[K][3]) { for (int k = 0; k < K; ++k) dacc.add3(t, (int) (k * WH) + pix, tg[k][0], tg[k][1], tg[k][2]); };
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp > 0 && nsp > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[0]);
        pfor(WH * nsp, nthreads, [&](long long a, long long b, int t) {
            TraversalStack st; uint32_t nr = 0;
            for (long long j = a; j < b; ++j) {
                const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
                const uint64_t slot = (uint64_t) pixel * o->spp + s;
                if (mode == 0) {
                    const Vec3f r = point_camera_sample<float, float>(hs.sc, tv0, st, pl, jump, pixel, slot, nr);
                    acc.add3(t, pixel, r.x / o->spp, r.y / o->spp, r.z / o->spp);
                } else {
                    const Vec3<Dual<K>> r = geo ? point_camera_sample<Dual<K>, Dual<K>>(hs.sc, tvk, st, pl, jump, pixel, slot, nr)
                                                : point_camera_sample<float, Dual<K>>(hs.sc, tvk, st, pl, jump, pixel, slot, nr);
                    acc.add3(t, pixel, r.x.v / o->spp, r.y.v / o->spp, r.z.v / o->spp);
                    for (int k = 0; k < K; ++k) dacc.add3(t, (int) (k * WH) + pixel, r.x.d[k] / o->spp, r.y.d[k] / o->spp, r.z.d[k] / o->spp);
                }
            }
        });
    }
    if (mode == 1 && o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0) {
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
    if (mode == 1 && o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0) {
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
    acc.reduce(img);
    if (mode && dimg) dacc.reduce(dimg);
    return 0;
}
}  // namespace

extern "C" {

// mode 0: renderC; mode 1: forward mode, K = 1 (tan: one set or null, d_pos: [3] or null, dimg: [W H 3])
int hostcheck_pointlight_render(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, const psdr_tangents *tan, const float *pos, const float *d_pos, float *img,
                                float *dimg, int nthreads) {
    return render_k<1>(d, o, mode, tan, pos, d_pos, img, dimg, nthreads);
}
// forward mode, K = 3: tan [3], d_pos [3][3] or null, dimg [3][W H 3]
int hostcheck_pointlight_render_k3(const psdr_scene_desc *d, const psdr_render_opts *o, const psdr_tangents *tan, const float *pos, const float *d_pos, float *img, float *dimg,
                                   int nthreads) {
    return render_k<3>(d, o, 1, tan, pos, d_pos, img, dimg, nthreads);
}

// reverse mode: the gradient tables `grads` names (zeroed by the caller), the light-position gradient g_pos[3] (+=, or null), and the image if img is not null
int hostcheck_pointlight_rev(const psdr_scene_desc *d, const psdr_render_opts *o, const float *pos, const float *adj, float *img, const psdr_grads *grads, float *g_pos) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const PointLight pl = make_light(pos, nullptr);
    HostSink sink; sink.g = *grads;
    const bool geo = grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr || g_pos != nullptr;
    const long long WH = (long long) d->width * d->height;
    TraversalStack st; uint32_t nr = 0;
    std::vector<double> acc((size_t) WH * 3, 0.0);
    double gp[3] = {0.0, 0.0, 0.0};
    const auto take = [&](const Vec3f &a) { gp[0] += a.x; gp[1] += a.y; gp[2] += a.z; };
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
            const Vec3f r = geo ? point_sample_reverse<true>(sink, pg, hs.sc, st, pl, jump, pixel, slot, a, nr, apl) : point_sample_reverse<false>(sink, pg, hs.sc, st, pl, jump, pixel, slot, a, nr, apl);
            if (pg.tri >= 0) for (int w = 0; w < kPrimaryWords; ++w) sink.add_tri(pg.tri, w, pg.w[w]);
            take(apl);
            acc[pixel * 3] += r.x * inv; acc[pixel * 3 + 1] += r.y * inv; acc[pixel * 3 + 2] += r.z * inv;
        }
    }
    if (o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0 && grads->g_prim_edge) {
        const RngJump jump = make_rng_jump(o->rng_offset[1]);
        const PointLi li{pl};
        for (long long j = WH * o->sppe_begin; j < WH * o->sppe_end; ++j) {
            float w[4];
            const int k = collocated_edge_reverse_values<kSceneAll>(hs.sc, st, jump, (uint64_t) j, 1.f / o->sppe, adj, nr, w, li);
            if (k >= 0) for (int i = 0; i < 4; ++i) sink.add_pedge(k, i, w[i]);
        }
    }
    if (o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0 && (grads->g_sec_edge || grads->g_tri_info || g_pos)) {
        const RngJump jump = make_rng_jump(o->rng_offset[2]);
        for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
            Rng rng; rng.init((uint64_t) j, jump);
            const float s3[3] = {rng.next(), rng.next(), rng.next()};
            Vec3f apl(0.f);
            point_sedge_reverse(sink, hs.sc, st, pl, s3, 1.f / o->sppse, adj, nr, apl);
            take(apl);
        }
    }
    if (g_pos) for (int c = 0; c < 3; ++c) g_pos[c] += (float) gp[c];
    if (img) for (size_t i = 0; i < acc.size(); ++i) img[i] = (float) acc[i];
    return 0;
}
}
