// hostcheck_path_guide.cpp -- TEST-ONLY harness, a sibling of hostcheck_path_sedge.cpp: the GUIDED secondary-edge estimator of the PathTracer and the guiding-grid
// build of either segment (csrc/psdr_path_sedge.h, the PSDR_HD functions the kernels run) on the host.  Grid A is the descriptor's grid (guide_*), grid B comes as
// arguments.  Never imported by the psdr_cuda package and not a fallback.  With -DPATH_GUIDE_MAIN the file is a stand-alone program over a tables file (built with
// the host sanitizers by tests/test_path_guide_host.py, never loaded into Python).
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
// as hostcheck_path_sedge.cpp sets a scene up, but the descriptor's grid stays (segment A's)
bool setup(HostScene &hs, const psdr_scene_desc *d) {
    hs.sc.d = *d;
    if (!hs.sc.d.env_f) hs.sc.d.env_emitter = -1;
    if (!hs.sc.d.guide_cmf || hs.sc.d.num_guide_cells <= 0) { hs.sc.d.guide_cmf = nullptr; hs.sc.d.num_guide_cells = 0; }
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
PathGuide grid_b(const int32_t *reso, const float *cmf, const float *pmf, float sum) {
    PathGuide g;
    if (reso && cmf && pmf) { g.cmf = cmf; g.pmf = pmf; g.sum = sum; g.r0 = reso[0]; g.r1 = reso[1]; g.r2 = reso[2]; g.n = reso[0] * reso[1] * reso[2]; }
    return g;
}
// what path_sedge_passes makes of the options: depth 1 has no segment B, a segment that is off ignores its grid
PathSedgeOpts slot_opts(const psdr_render_opts *o, int seg, int walk, const PathGuide &gb) {
    PathSedgeOpts po{o->max_depth, seg & 3, walk};
    if (po.max_depth < 2) po.seg &= 1;
    if (po.seg & 2) po.gb = gb;
    return po;
}
// guide_slot_sample of the build kernels (csrc/psdr_kernels.h), mirrored: slot j = (round j / n, stream j % n), draws 3 r .. 3 r + 2 of stream l stratified into its cell
void cell_sample(const int32_t reso[4], long long n, long long j, float c3[3], int &cell) {
    const int r = (int) (j / n), l = (int) (j - (long long) r * n);
    cell = l / reso[3];
    const int c0 = cell / (reso[1] * reso[2]), rem = cell - c0 * reso[1] * reso[2], c1 = rem / reso[2], c2 = rem - c1 * reso[2];
    Rng rng; rng.init((uint64_t) l, rng_jump_hd(3ull * (uint64_t) r));
    c3[0] = rng.next(); c3[1] = rng.next(); c3[2] = rng.next();
    c3[0] = (c3[0] + (float) c0) * (1.f / (float) reso[0]);
    c3[1] = (c3[1] + (float) c1) * (1.f / (float) reso[1]);
    c3[2] = (c3[2] + (float) c2) * (1.f / (float) reso[2]);
}
}  // namespace

extern "C" {

// forward mode (K = 1): the derivative image of the guided term alone; seg / walk: the scene options pt_sedge / pt_sedge_walk; b_reso == NULL: no grid B
int hostcheck_path_guide_fwd(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const int32_t *b_reso, const float *b_cmf, const float *b_pmf, float b_sum,
                             const psdr_tangents *tan, float *dimg, int nthreads) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (!wanted(d, o)) return 2;
    hs.sc.literal_forms = (o->flags & PSDR_FLAG_LITERAL_FORMS) ? 1 : 0;
    const long long WH = (long long) d->width * d->height;
    const size_t n3 = (size_t) WH * 3;
    nthreads = std::max(1, nthreads);
    std::vector<std::vector<double>> dacc(nthreads, std::vector<double>(n3, 0.0));
    TangentView<1, kSceneAll> tv1; tv1.t[0] = tan ? *tan : psdr_tangents{};
    const PathSedgeOpts po = slot_opts(o, seg, walk, grid_b(b_reso, b_cmf, b_pmf, b_sum));
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

// reverse mode: the same slots scattered into the caller's gradient tables (+=, one thread: the summation order is fixed)
int hostcheck_path_guide_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const int32_t *b_reso, const float *b_cmf, const float *b_pmf, float b_sum,
                             const float *adj, const psdr_grads *grads) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (!wanted(d, o)) return 2;
    HostSink sink; sink.g = *grads;
    const long long WH = (long long) d->width * d->height;
    const PathSedgeOpts po = slot_opts(o, seg, walk, grid_b(b_reso, b_cmf, b_pmf, b_sum));
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    TraversalStack st; uint32_t nr = 0;
    for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
        Rng rng; rng.init((uint64_t) j, jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        path_secondary_edge_reverse(sink, hs.sc, st, rng, s3, po, 1.f / o->sppse, adj, nr, true);
    }
    return 0;
}

// survivors of segment A's filter / segment B's under the grids (the lists of a split launch): out[0], out[1]; slots in out[2]
int hostcheck_path_guide_survivors(const psdr_scene_desc *d, const psdr_render_opts *o, const int32_t *b_reso, const float *b_cmf, const float *b_pmf, float b_sum, long long *out) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (!wanted(d, o)) return 2;
    const long long WH = (long long) d->width * d->height;
    const RngJump jump = make_rng_jump(o->rng_offset[2]);
    const PathGuide gb = grid_b(b_reso, b_cmf, b_pmf, b_sum);
    TraversalStack st; uint32_t nr = 0;
    out[0] = out[1] = 0; out[2] = WH * (o->sppse_end - o->sppse_begin);
    for (long long j = WH * o->sppse_begin; j < WH * o->sppse_end; ++j) {
        Rng rng; rng.init((uint64_t) j, jump);
        const float s3[3] = {rng.next(), rng.next(), rng.next()};
        float sa[3] = {s3[0], s3[1], s3[2]};
        if (guided_a(hs.sc)) (void) guide_sample_reuse(hs.sc, sa);          // as k_secondary_edge_filter warps
        if (secondary_edge_survives<kSceneAll>(hs.sc, st, sa, nr)) out[0]++;
        if (o->max_depth >= 2 && path_sedge_survives_b<kSceneAll>(hs.sc, st, rng, s3[0], nr, &gb)) out[1]++;
    }
    return 0;
}

// the guiding-grid build of psdr_path_guide_build (segment 1 = A, 2 = B; reso [4]; unguided: any grid of the descriptor is ignored), summed in double
int hostcheck_path_guide_mass(const psdr_scene_desc *d, const psdr_render_opts *o, int segment, int walk, const int32_t *reso, int nrounds, float *out_mass, int nthreads) {
    HostScene hs;
    if (!setup(hs, d)) return 1;
    if (d->num_sec_edges <= 0 || o->max_depth < 1 || o->max_depth > kMaxPathSedgeDepth || (segment != 1 && segment != 2) || (segment == 2 && o->max_depth < 2) || nrounds <= 0) return 2;
    hs.sc.d.guide_cmf = nullptr; hs.sc.d.num_guide_cells = 0;
    hs.sc.literal_forms = (o->flags & PSDR_FLAG_LITERAL_FORMS) ? 1 : 0;
    const long long cells = (long long) reso[0] * reso[1] * reso[2], n = cells * reso[3], total = n * nrounds;
    nthreads = std::max(1, nthreads);
    std::vector<std::vector<double>> acc(nthreads, std::vector<double>((size_t) cells, 0.0));
    const PathSedgeOpts po{o->max_depth, segment, walk};
    const RngJump nojump{1ull, 0ull};
    const double scale = 1.0 / ((double) reso[3] * (double) nrounds);
    pfor(total, nthreads, [&](long long a, long long b, int t) {
        TraversalStack st; uint32_t nr = 0;
        for (long long j = a; j < b; ++j) {
            float c3[3]; int cell;
            cell_sample(reso, n, j, c3, cell);
            Rng rest; rest.init((uint64_t) n + (uint64_t) j, nojump);          // k_path_guide's stream layout
            acc[t][(size_t) cell] += (double) path_sedge_mass<kSceneAll>(hs.sc, st, rest, c3, po, nr, true) * scale;
        }
    });
    for (long long c = 0; c < cells; ++c) {
        double s = 0;
        for (int t = 0; t < nthreads; ++t) s += acc[t][(size_t) c];
        out_mass[c] = (float) s;
    }
    return 0;
}
}

#ifdef PATH_GUIDE_MAIN
// Stand-alone run over a tables file (tests/test_path_guide_host.py writes it):
//   int64 sizeof(desc) | desc bytes | int64 m | m x (int64 offset of a pointer member in desc, int64 bytes, data) | opts bytes | int32 b_reso[3] | float b_sum |
//   b_cmf, b_pmf [cells] | int32 mass_reso[4] | int32 nrounds | float d_sec_edge [num_sec_edges x 16] | float adj [W H 3]
// Prints: the sums of |derivative image| and |g_sec_edge|, the survivor counts, the sums of both masses.
namespace {
bool rd(std::FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
}
int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: path_guide_san <tables file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "path_guide_san: cannot open %s\n", argv[1]); return 2; }
    long long sz = 0, m = 0;
    psdr_scene_desc d{};
    if (!rd(f, &sz, 8) || sz != (long long) sizeof(d) || !rd(f, &d, sizeof(d)) || !rd(f, &m, 8) || m < 0 || m > 64) { std::fprintf(stderr, "path_guide_san: bad header\n"); return 2; }
    std::vector<std::vector<double>> blocks((size_t) m);          // (double: every table aligned for any element type)
    for (long long i = 0; i < m; ++i) {
        long long off = 0, bytes = 0;
        if (!rd(f, &off, 8) || !rd(f, &bytes, 8) || off < 0 || off + 8 > (long long) sizeof(d) || bytes < 0) { std::fprintf(stderr, "path_guide_san: bad table record\n"); return 2; }
        blocks[(size_t) i].assign((size_t) bytes / 8 + 1, 0.0);
        if (!rd(f, blocks[(size_t) i].data(), (size_t) bytes)) { std::fprintf(stderr, "path_guide_san: short table\n"); return 2; }
        const void *p = blocks[(size_t) i].data();
        std::memcpy(reinterpret_cast<char *>(&d) + off, &p, sizeof(p));
    }
    psdr_render_opts o{};
    int32_t b_reso[3], mass_reso[4], nrounds = 0;
    float b_sum = 0.f;
    if (!rd(f, &o, sizeof(o)) || !rd(f, b_reso, sizeof(b_reso)) || !rd(f, &b_sum, 4)) { std::fprintf(stderr, "path_guide_san: short options\n"); return 2; }
    const long long cells_b = (long long) b_reso[0] * b_reso[1] * b_reso[2];
    if (cells_b <= 0 || cells_b > (1 << 20)) return 2;
    std::vector<float> b_cmf((size_t) cells_b), b_pmf((size_t) cells_b);
    if (!rd(f, b_cmf.data(), 4 * (size_t) cells_b) || !rd(f, b_pmf.data(), 4 * (size_t) cells_b) || !rd(f, mass_reso, sizeof(mass_reso)) || !rd(f, &nrounds, 4)) return 2;
    const long long cells_m = (long long) mass_reso[0] * mass_reso[1] * mass_reso[2];
    if (cells_m <= 0 || cells_m > (1 << 20) || d.num_sec_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    std::vector<float> d_se((size_t) d.num_sec_edges * PSDR_SEDGE_STRIDE), adj((size_t) d.width * d.height * 3), dimg(adj.size(), 0.f), g_se(d_se.size(), 0.f);
    if (!rd(f, d_se.data(), 4 * d_se.size()) || !rd(f, adj.data(), 4 * adj.size())) { std::fprintf(stderr, "path_guide_san: short tangents\n"); return 2; }
    std::fclose(f);
    psdr_tangents tan{}; tan.d_sec_edge = d_se.data();
    psdr_grads g{}; g.g_sec_edge = g_se.data();
    if (int rc = hostcheck_path_guide_fwd(&d, &o, 3, 1, b_reso, b_cmf.data(), b_pmf.data(), b_sum, &tan, dimg.data(), 2)) return 10 + rc;
    if (int rc = hostcheck_path_guide_rev(&d, &o, 3, 1, b_reso, b_cmf.data(), b_pmf.data(), b_sum, adj.data(), &g)) return 20 + rc;
    long long surv[3] = {0, 0, 0};
    if (int rc = hostcheck_path_guide_survivors(&d, &o, b_reso, b_cmf.data(), b_pmf.data(), b_sum, surv)) return 30 + rc;
    std::vector<float> mass((size_t) cells_m);
    double sums[4] = {0, 0, 0, 0};
    for (float v : dimg) sums[0] += std::fabs(v);
    for (float v : g_se) sums[1] += std::fabs(v);
    for (int seg = 1; seg <= 2; ++seg) {
        if (int rc = hostcheck_path_guide_mass(&d, &o, seg, 1, mass_reso, nrounds, mass.data(), 2)) return 40 + rc;
        for (float v : mass) sums[1 + seg] += v;
    }
    std::printf("%.9g %.9g %lld %lld %lld %.9g %.9g\n", sums[0], sums[1], surv[0], surv[1], surv[2], sums[2], sums[3]);
    return 0;
}
#endif
