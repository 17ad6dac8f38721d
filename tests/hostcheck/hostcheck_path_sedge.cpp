// hostcheck_path_sedge.cpp -- TEST-ONLY harness, a sibling of hostcheck.cpp: runs the PathTracer's secondary-edge estimator (csrc/psdr_path_sedge.h, PSDR_HD
// functions) on the host, slot by slot, so that `-m "not gpu"` tests can check the term (depth-1 anchor, forward = reverse, AD against finite
// differences) where no GPU exists.  Never imported by the psdr_cuda package and not a fallback.
#include "../../psdr-cuda_amd/csrc/psdr_bvh_build.h"
#include "../../psdr-cuda_amd/csrc/psdr_path_sedge.h"

#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

using namespace psdr;

namespace {
struct HostScene {
    SceneView sc{};
    Builder b;
};
// as hostcheck.cpp sets a scene up (tiny scenes take the all-triangles path of closest_hit)
bool setup(HostScene &hs, const psdr_scene_desc *d) {
    hs.sc.d = *d;
    if (!hs.sc.d.env_f) hs.sc.d.env_emitter = -1;
    hs.sc.d.guide_cmf = nullptr; hs.sc.d.num_guide_cells = 0;          // (PathTracer slots are not guided)
    int32_t root = 0;
    if (hs.b.run(d->tri_info, d->num_tris, root)) return false;
    hs.sc.nodes = hs.b.nodes.data(); hs.sc.btris = hs.b.btris.data(); hs.sc.root = root;
    const char *e = std::getenv("PSDR_TINY_SCENE");
    if (d->num_tris <= kTinyTris && !(e && std::atoi(e) == 0)) {
        std::vector<float4> prims;
        pack_tiny_prims(hs.b.btris, prims);
        hs.sc.n_tiny = tiny_plane_form(prims, hs.sc.tiny, hs.sc.tiny_meta, &hs.sc.aa_cnt);
    }
    return true;
}
template <class F> void pfor(long long n, int nt, F f) {
    std::vector<std::thread> th;
    long long chunk = (n + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        long long a = t * chunk, b = std::min(n, a + chunk);
        if (a >= b) break;
        th.emplace_back([=] { f(a, b, t); });
    }
    for (auto &x : th) x.join();
}
struct HostSink {
    static constexpr int flags = kSceneAll;
    static constexpr bool has_env = true;
    psdr_grads g;
    static void put(float *b, size_t i, float v) { if (b && v != 0.f && std::isfinite(v)) b[i] += v; }
    void add_env(int w, float v) const { put(g.g_env_f, w, v); }
    void add_tri(int tri, int word, float v) const { put(g.g_tri_info, (size_t) tri * PSDR_TRI_STRIDE + word, v); }
    void add_texel(int idx, float v) const { put(g.g_texels, idx, v); }
    void add_rad(int e, int c, float v) const { put(g.g_emitter_rad, (size_t) e * 3 + c, v); }
    void add_cam(int w, float v) const { put(g.g_cam_to_world, w, v); }
    void add_sedge(int e, int w, float v) const { put(g.g_sec_edge, (size_t) e * PSDR_SEDGE_STRIDE + w, v); }
    void add_pedge(int e, int w, float v) const { put(g.g_prim_edge, (size_t) e * PSDR_PEDGE_STRIDE + w, v); }
};
bool wanted(const psdr_scene_desc *d, const psdr_render_opts *o) {
    return o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0 && o->integrator == PSDR_INTEGRATOR_PATH && (o->flags & PSDR_FLAG_PATH_SEDGES) &&
           o->max_depth >= 1 && o->max_depth <= kMaxPathSedgeDepth;
}
}  // namespace

extern "C" {

// forward mode (K = 1): the derivative image of the PathTracer's secondary-edge term ALONE (slots [W H sppse_begin, W H sppse_end) of sampler 2);
// seg / walk: the scene options pt_sedge / pt_sedge_walk
int hostcheck_path_sedge_fwd(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const psdr_tangents *tan, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (!wanted(d, o)) return 2;
    hs.sc.literal_forms = (o->flags & PSDR_FLAG_LITERAL_FORMS) ? 1 : 0;
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    std::vector<std::vector<double>> dacc(nthreads, std::vector<double>(n3, 0.0));
    TangentView<1, kSceneAll> tv1; tv1.t[0] = tan ? *tan : psdr_tangents{};
    const PathSedgeOpts po{o->max_depth, seg, walk};
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    const long long i0 = WH * o->sppse_begin, n = WH * (o->sppse_end - o->sppse_begin);
    pfor(n, nthreads, [&](long long a, long long b, int t) {
        TraversalStack st; uint32_t nr = 0;
        for (long long j = a; j < b; ++j) {
            Rng rng; rng.init((uint64_t) (i0 + j), jump);
            const float s3[3] = {rng.next(), rng.next(), rng.next()};
            const float scale = 1.f / o->sppse;
            path_secondary_edge_sample<Dual<1>>(hs.sc, tv1, st, rng, s3, po, nr, true, [&](int pix, const Vec3<Dual<1>> &v) {
                dacc[t][pix * 3] += v.x.d[0] * scale; dacc[t][pix * 3 + 1] += v.y.d[0] * scale; dacc[t][pix * 3 + 2] += v.z.d[0] * scale;
            });
        }
    });
    for (size_t i = 0; i < n3; ++i) {
        double ds = 0;
        for (int t = 0; t < nthreads; ++t) ds += dacc[t][i];
        dimg[i] = (float) ds;
    }
    return 0;
}

// reverse mode: the same slots scattered into the caller's gradient tables (accumulated with +=, one thread: the summation order is fixed)
int hostcheck_path_sedge_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const float *adj, const psdr_grads *grads) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (!wanted(d, o)) return 2;
    HostSink sink; sink.g = *grads;
    const long long WH = (long long) d->width * d->height;
    const PathSedgeOpts po{o->max_depth, seg, walk};
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    TraversalStack st; uint32_t nr = 0;
    for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
        Rng rng; rng.init((uint64_t) j, jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        path_secondary_edge_reverse(sink, hs.sc, st, rng, s3, po, 1.f / o->sppse, adj, nr, true);
    }
    return 0;
}

// how many of the slots get past the first two rays of segment A / segment B (the survivor lists of a split launch): out[0], out[1]; returns the slot count in out[2]
int hostcheck_path_sedge_survivors(const psdr_scene_desc *d, const psdr_render_opts *o, long long *out) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (!wanted(d, o)) return 2;
    const long long WH = (long long) d->width * d->height;
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    TraversalStack st; uint32_t nr = 0;
    out[0] = out[1] = 0; out[2] = WH * (o->sppse_end - o->sppse_begin);
    for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
        Rng rng; rng.init((uint64_t) j, jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        if (secondary_edge_survives<kSceneAll>(hs.sc, st, s3, nr)) out[0]++;
        if (o->max_depth >= 2 && path_sedge_survives_b<kSceneAll>(hs.sc, st, rng, s3[0], nr)) out[1]++;
    }
    return 0;
}

int hostcheck_path_sedge_draws(int max_depth) { return path_sedge_draws(max_depth); }
}
