// hostcheck_collocated.cpp -- TEST-ONLY harness: the CollocatedIntegrator's estimator (csrc/psdr_collocated.h, PSDR_HD functions) run on the host, slot by slot,
// so that `-m "not gpu"` tests can check it where no GPU exists and the GPU tests have a reference the oracle does not offer (the reference snapshot has no such
// integrator).  A library of its own (libhostcheck_collocated.so), as hostcheck_path_sedge.cpp is for its header.  Never imported by the psdr_cuda package and
// not a fallback: the render path only ever executes these functions inside HIP kernels.  tests/hostcheck/colloc_san.cpp includes this file into a
// stand-alone program for the host sanitizers.
#include "host_common.h"
#include "../../psdr-cuda_amd/csrc/psdr_collocated.h"

extern "C" {

// mode 0: renderC (unit intensity); mode 1: renderD forward (K = 1), interior + primary edges.  Per-thread images in double, summed in thread order.
int hostcheck_collocated_render(const psdr_scene_desc *d, const psdr_render_opts *o, int mode, const psdr_tangents *tan, float *img, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    ThreadImages acc(nthreads, n3), dacc(nthreads, mode ? n3 : 0);
    TangentView<1, kSceneAll> tv1; tv1.t[0] = tan ? *tan : psdr_tangents{};
    const TangentView<0, kSceneAll> tv0{};
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp > 0 && nsp > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[0]);
        const bool geo = tv1.t[0].d_tri_info || tv1.t[0].d_cam_to_world;
        pfor(WH * nsp, nthreads, [&](long long a, long long b, int t) {
            TraversalStack st; uint32_t nr = 0;
            for (long long j = a; j < b; ++j) {
                const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
                const uint64_t slot = (uint64_t) pixel * o->spp + s;
                if (mode == 0) {
                    const Vec3f r = collocated_camera_sample<float, float>(hs.sc, tv0, st, jump, pixel, slot, nr);
                    acc[t][pixel * 3] += r.x / o->spp; acc[t][pixel * 3 + 1] += r.y / o->spp; acc[t][pixel * 3 + 2] += r.z / o->spp;
                } else {
                    const Vec3<Dual<1>> r = geo ? collocated_camera_sample<Dual<1>, Dual<1>>(hs.sc, tv1, st, jump, pixel, slot, nr)
                                                : collocated_camera_sample<float, Dual<1>>(hs.sc, tv1, st, jump, pixel, slot, nr);
                    acc[t][pixel * 3] += r.x.v / o->spp; acc[t][pixel * 3 + 1] += r.y.v / o->spp; acc[t][pixel * 3 + 2] += r.z.v / o->spp;
                    dacc[t][pixel * 3] += r.x.d[0] / o->spp; dacc[t][pixel * 3 + 1] += r.y.d[0] / o->spp; dacc[t][pixel * 3 + 2] += r.z.d[0] / o->spp;
                }
            }
        });
    }
    if (mode == 1 && o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[1]);
        const long long i0 = WH * o->sppe_begin, n = WH * (o->sppe_end - o->sppe_begin);
        pfor(n, nthreads, [&](long long a, long long b, int t) {
            TraversalStack st; uint32_t nr = 0;
            for (long long j = a; j < b; ++j) {
                float tg[1][3];
                const int pix = collocated_edge_sample<1, kSceneAll>(hs.sc, tv1, st, jump, (uint64_t) (i0 + j), 1.f / o->sppe, tg, nr);
                if (pix >= 0) for (int c = 0; c < 3; ++c) dacc[t][pix * 3 + c] += tg[0][c];
            }
        });
    }
    acc.reduce(img);
    if (mode && dimg) dacc.reduce(dimg);
    return 0;
}

// reverse mode: the gradient tables `grads` names (zeroed by the caller), and the image if img is not null
int hostcheck_collocated_rev(const psdr_scene_desc *d, const psdr_render_opts *o, const float *adj, float *img, const psdr_grads *grads) {
    HostScene hs;
    if (!setup(hs, d, Grid::keep)) return 1;
    HostSink sink; sink.g = *grads;
    const bool geo = grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr;
    const long long WH = (long long) d->width * d->height;
    TraversalStack st; uint32_t nr = 0;
    std::vector<double> acc((size_t) WH * 3, 0.0);
    const int nsp = o->spp_end - o->spp_begin;
    if (o->spp > 0 && nsp > 0) {
        const RngJump jump = make_rng_jump(o->rng_offset[0]);
        for (long long j = 0; j < WH * nsp; ++j) {
            const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
            const float inv = 1.f / o->spp;
            const Vec3f a{adj[pixel * 3] * inv, adj[pixel * 3 + 1] * inv, adj[pixel * 3 + 2] * inv};
            PrimaryGrad pg;
            const uint64_t slot = (uint64_t) pixel * o->spp + s;
            const Vec3f r = geo ? collocated_sample_reverse<true>(sink, pg, hs.sc, st, jump, pixel, slot, a, nr) : collocated_sample_reverse<false>(sink, pg, hs.sc, st, jump, pixel, slot, a, nr);
            if (pg.tri >= 0) for (int w = 0; w < kPrimaryWords; ++w) sink.add_tri(pg.tri, w, pg.w[w]);
            acc[pixel * 3] += r.x * inv; acc[pixel * 3 + 1] += r.y * inv; acc[pixel * 3 + 2] += r.z * inv;
        }
    }
    if (o->sppe > 0 && o->sppe_end > o->sppe_begin && d->num_prim_edges > 0 && grads->g_prim_edge) {
        const RngJump jump = make_rng_jump(o->rng_offset[1]);
        for (long long j = WH * o->sppe_begin; j < WH * o->sppe_end; ++j) {
            float w[4];
            const int k = collocated_edge_reverse_values<kSceneAll>(hs.sc, st, jump, (uint64_t) j, 1.f / o->sppe, adj, nr, w);
            if (k >= 0) for (int i = 0; i < 4; ++i) sink.add_pedge(k, i, w[i]);
        }
    }
    if (img) for (size_t i = 0; i < acc.size(); ++i) img[i] = (float) acc[i];
    return 0;
}

// the film samples of renderC, in slot order: (sx, sy) of slot j = pixel * nsp + s -- what a closed-form evaluation needs (tests/test_collocated_host.py
// cross-checks them against oracle.rng)
int hostcheck_collocated_film_samples(const psdr_scene_desc *d, const psdr_render_opts *o, float *sxy) {
    const long long WH = (long long) d->width * d->height;
    const int nsp = o->spp_end - o->spp_begin;
    const RngJump jump = make_rng_jump(o->rng_offset[0]);
    for (long long j = 0; j < WH * nsp; ++j) {
        const int pixel = (int) (j / nsp), s = o->spp_begin + (int) (j % nsp);
        Rng rng; rng.init((uint64_t) pixel * o->spp + s, jump);
        const float j0 = rng.next(), j1 = rng.next();
        sxy[2 * j] = ((float) (pixel % d->width) + j0) / (float) d->width; sxy[2 * j + 1] = ((float) (pixel / d->width) + j1) / (float) d->height;
    }
    return 0;
}
}
