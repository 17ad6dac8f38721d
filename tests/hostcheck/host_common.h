// host_common.h -- TEST-ONLY: what the estimator harnesses of this directory share (hostcheck.cpp, hostcheck_path_sedge.cpp, hostcheck_path_guide.cpp,
// hostcheck_collocated.cpp): the scene set-up, the thread loop, the gradient sink, the per-thread images, the slot loops of the PathTracer's secondary-edge term
// and the reader of the stand-alone programs' tables file.  Each harness is one translation unit, so everything here sits in an unnamed namespace.
#pragma once
#include "../../psdr-cuda_amd/csrc/psdr_bvh_build.h"
#include "../../psdr-cuda_amd/csrc/psdr_path_sedge.h"

#include <cstdio>
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
// what becomes of the descriptor's guiding grid (guide_*)
enum class Grid { keep, drop, keep_valid };          // as given | PathTracer slots that are not guided | segment A's grid, if it is one
// one tree, or the all-triangles path of closest_hit for a tiny scene, as psdr_bvh_build arranges on the device
bool setup(HostScene &hs, const psdr_scene_desc *d, Grid grid) {
    hs.sc.d = *d;
    if (!hs.sc.d.env_f) hs.sc.d.env_emitter = -1;
    if (grid == Grid::drop || (grid == Grid::keep_valid && !guided_a(hs.sc))) { hs.sc.d.guide_cmf = nullptr; hs.sc.d.num_guide_cells = 0; }
    int32_t root = 0;
    if (hs.b.run(d->tri_info, d->num_tris, root)) return false;
    hs.sc.nodes = hs.b.nodes.data(); hs.sc.btris = hs.b.btris.data(); hs.sc.root = root;
    const char *e = std::getenv("PSDR_TINY_SCENE");
    if (d->num_tris <= kTinyTris && !(e && std::atoi(e) == 0)) {
        std::vector<float4> prims;
        pack_tiny_prims(hs.b.btris, prims);
        hs.sc.n_tiny = tiny_plane_form(prims, hs.sc.tiny, hs.sc.tiny_meta, &hs.sc.aa_cnt);
        // SceneView::emit_rows as psdr_bvh_build sets it (the estimators' emitter pre-test; the host check's TangentView flags carry neither kSceneTiny nor
        // kSceneForest, so the estimators here do not USE it -- hostcheck_emitter_rows hands it to the tests)
        std::vector<char> is_em((size_t) d->num_tris, 0);
        for (int e = 0; e < d->num_emitters && d->emitter_i; ++e) {
            const int32_t *ei = d->emitter_i + (size_t) e * PSDR_EMITTER_I_STRIDE;
            for (int f = 0; f < ei[2]; ++f) if (ei[1] + f >= 0 && ei[1] + f < d->num_tris) is_em[(size_t) (ei[1] + f)] = 1;
        }
        hs.sc.emit_rows = tiny_emitter_rows(hs.sc.tiny_meta, hs.sc.n_tiny, hs.sc.aa_cnt, is_em);
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
// one double image per thread of a pfor; reduce() sums them in thread order
struct ThreadImages {
    std::vector<std::vector<double>> img;
    ThreadImages(int nthreads, size_t n) : img((size_t) nthreads, std::vector<double>(n, 0.0)) {}
    std::vector<double> &operator[](int t) { return img[(size_t) t]; }
    void add3(int t, int pix, double x, double y, double z) { double *p = &img[(size_t) t][(size_t) pix * 3]; p[0] += x; p[1] += y; p[2] += z; }
    void reduce(float *out) const {
        for (size_t i = 0; i < img[0].size(); ++i) {
            double s = 0;
            for (const auto &a : img) s += a[i];
            out[i] = (float) s;
        }
    }
};
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

// ---------------------------------------------------------------- the PathTracer's secondary-edge term: slots [W H sppse_begin, W H sppse_end) of sampler 2
// (hostcheck_path_sedge.cpp and hostcheck_path_guide.cpp: each forms its own PathSedgeOpts and says what becomes of the descriptor's grid)
bool path_sedge_wanted(const psdr_scene_desc *d, const psdr_render_opts *o) {
    return o->sppse > 0 && o->sppse_end > o->sppse_begin && d->num_sec_edges > 0 && o->integrator == PSDR_INTEGRATOR_PATH && (o->flags & PSDR_FLAG_PATH_SEDGES) &&
           o->max_depth >= 1 && o->max_depth <= kMaxPathSedgeDepth;
}
// forward mode (K = 1): the derivative image of the term alone
int path_sedge_fwd(const psdr_scene_desc *d, const psdr_render_opts *o, Grid grid, const PathSedgeOpts &po, const psdr_tangents *tan, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d, grid)) return 1;
    if (!path_sedge_wanted(d, o)) return 2;
    hs.sc.literal_forms = (o->flags & PSDR_FLAG_LITERAL_FORMS) ? 1 : 0;
    const long long WH = (long long) d->width * d->height;
    nthreads = std::max(1, nthreads);
    ThreadImages dacc(nthreads, (size_t) WH * 3);
    TangentView<1, kSceneAll> tv1; tv1.t[0] = tan ? *tan : psdr_tangents{};
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    const long long i0 = WH * o->sppse_begin, n = WH * (o->sppse_end - o->sppse_begin);
    pfor(n, nthreads, [&](long long a, long long b, int t) {
        TraversalStack st; uint32_t nr = 0;
        for (long long j = a; j < b; ++j) {
            Rng rng; rng.init((uint64_t) (i0 + j), jump);
            const float s3[3] = {rng.next(), rng.next(), rng.next()};
            const float scale = 1.f / o->sppse;
            path_secondary_edge_sample<Dual<1>>(hs.sc, tv1, st, rng, s3, po, nr, true, [&](int pix, const Vec3<Dual<1>> &v) {
                dacc.add3(t, pix, v.x.d[0] * scale, v.y.d[0] * scale, v.z.d[0] * scale);
            });
        }
    });
    dacc.reduce(dimg);
    return 0;
}
// reverse mode: the same slots scattered into the caller's gradient tables (accumulated with +=, one thread: the summation order is fixed)
int path_sedge_rev(const psdr_scene_desc *d, const psdr_render_opts *o, Grid grid, const PathSedgeOpts &po, const float *adj, const psdr_grads *grads) {
    HostScene hs;
    if (!setup(hs, d, grid)) return 1;
    if (!path_sedge_wanted(d, o)) return 2;
    HostSink sink; sink.g = *grads;
    const long long WH = (long long) d->width * d->height;
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    TraversalStack st; uint32_t nr = 0;
    for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
        Rng rng; rng.init((uint64_t) j, jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        path_secondary_edge_reverse(sink, hs.sc, st, rng, s3, po, 1.f / o->sppse, adj, nr, true);
    }
    return 0;
}
// how many of the slots get past the first two rays of segment A / segment B (the survivor lists of a split launch) under the scene's grid A and *gb (null: no
// grid B): out[0], out[1]; the slot count in out[2]
int path_sedge_survivors(const psdr_scene_desc *d, const psdr_render_opts *o, Grid grid, const PathGuide *gb, long long *out) {
    HostScene hs;
    if (!setup(hs, d, grid)) return 1;
    if (!path_sedge_wanted(d, o)) return 2;
    const long long WH = (long long) d->width * d->height;
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    TraversalStack st; uint32_t nr = 0;
    out[0] = out[1] = 0; out[2] = WH * (o->sppse_end - o->sppse_begin);
    for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
        Rng rng; rng.init((uint64_t) j, jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        float sa[3] = {s3[0], s3[1], s3[2]};
        if (guided_a(hs.sc)) (void) guide_sample_reuse(hs.sc, sa);          // as k_secondary_edge_filter warps
        if (secondary_edge_survives<kSceneAll>(hs.sc, st, sa, nr)) out[0]++;
        if (o->max_depth >= 2 && path_sedge_survives_b<kSceneAll>(hs.sc, st, rng, s3[0], nr, gb)) out[1]++;
    }
    return 0;
}

// ---------------------------------------------------------------- the tables file of the stand-alone programs (tests/hostlibs.py write_tables_file):
//   int64 sizeof(desc) | desc bytes | int64 m | m x (int64 offset of a pointer member in desc, int64 bytes, data) | opts bytes | the program's own arrays
struct TablesFile {
    psdr_scene_desc d{};
    psdr_render_opts o{};
    std::vector<std::vector<double>> blocks;          // (double: every table aligned for any element type)
    std::FILE *f = nullptr;
    ~TablesFile() { if (f) std::fclose(f); }
    bool rd(void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
    template <class T> bool rd(std::vector<T> &v) { return rd(v.data(), sizeof(T) * v.size()); }
    // header, table records patched into d, options; false (after a message) if the file is not one
    bool open(const char *prog, const char *path) {
        const auto fail = [&](const char *what) { std::fprintf(stderr, "%s: %s\n", prog, what); return false; };
        if (!(f = std::fopen(path, "rb"))) return fail("cannot open the tables file");
        long long sz = 0, m = 0;
        if (!rd(&sz, 8) || sz != (long long) sizeof(d) || !rd(&d, sizeof(d)) || !rd(&m, 8) || m < 0 || m > 64) return fail("bad header");
        blocks.resize((size_t) m);
        for (auto &blk : blocks) {
            long long off = 0, bytes = 0;
            if (!rd(&off, 8) || !rd(&bytes, 8) || off < 0 || off + 8 > (long long) sizeof(d) || bytes < 0) return fail("bad table record");
            blk.assign((size_t) bytes / 8 + 1, 0.0);
            if (!rd(blk.data(), (size_t) bytes)) return fail("short table");
            const void *p = blk.data();
            std::memcpy(reinterpret_cast<char *>(&d) + off, &p, sizeof(p));
        }
        return rd(&o, sizeof(o)) || fail("short options");
    }
};
}  // namespace
