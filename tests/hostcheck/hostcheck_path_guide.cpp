// hostcheck_path_guide.cpp -- TEST-ONLY harness, a sibling of hostcheck_path_sedge.cpp: the GUIDED secondary-edge estimator of the PathTracer and the guiding-grid
// build of either segment (csrc/psdr_path_sedge.h, the PSDR_HD functions the kernels run) on the host.  Grid A is the descriptor's grid (guide_*), grid B comes as
// arguments.  Never imported by the psdr_cuda package and not a fallback.  With -DPATH_GUIDE_MAIN the file is a stand-alone program over a tables file (built with
// the host sanitizers by tests/test_path_guide_host.py, never loaded into Python).
#include "host_common.h"

namespace {
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
    return path_sedge_fwd(d, o, Grid::keep_valid, slot_opts(o, seg, walk, grid_b(b_reso, b_cmf, b_pmf, b_sum)), tan, dimg, nthreads);
}

// reverse mode: the same slots scattered into the caller's gradient tables (+=, one thread: the summation order is fixed)
int hostcheck_path_guide_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const int32_t *b_reso, const float *b_cmf, const float *b_pmf, float b_sum,
                             const float *adj, const psdr_grads *grads) {
    return path_sedge_rev(d, o, Grid::keep_valid, slot_opts(o, seg, walk, grid_b(b_reso, b_cmf, b_pmf, b_sum)), adj, grads);
}

// survivors of segment A's filter / segment B's under the grids (the lists of a split launch): out[0], out[1]; slots in out[2]
int hostcheck_path_guide_survivors(const psdr_scene_desc *d, const psdr_render_opts *o, const int32_t *b_reso, const float *b_cmf, const float *b_pmf, float b_sum, long long *out) {
    const PathGuide gb = grid_b(b_reso, b_cmf, b_pmf, b_sum);
    return path_sedge_survivors(d, o, Grid::keep_valid, &gb, out);
}

// the guiding-grid build of psdr_path_guide_build (segment 1 = A, 2 = B; reso [4]; unguided: any grid of the descriptor is ignored), summed in double
int hostcheck_path_guide_mass(const psdr_scene_desc *d, const psdr_render_opts *o, int segment, int walk, const int32_t *reso, int nrounds, float *out_mass, int nthreads) {
    HostScene hs;
    if (!setup(hs, d, Grid::drop)) return 1;
    if (d->num_sec_edges <= 0 || o->max_depth < 1 || o->max_depth > kMaxPathSedgeDepth || (segment != 1 && segment != 2) || (segment == 2 && o->max_depth < 2) || nrounds <= 0) return 2;
    hs.sc.literal_forms = (o->flags & PSDR_FLAG_LITERAL_FORMS) ? 1 : 0;
    const long long cells = (long long) reso[0] * reso[1] * reso[2], n = cells * reso[3], total = n * nrounds;
    nthreads = std::max(1, nthreads);
    ThreadImages acc(nthreads, (size_t) cells);
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
    acc.reduce(out_mass);
    return 0;
}
}

#ifdef PATH_GUIDE_MAIN
// Stand-alone run over a tables file (tests/test_path_guide_host.py writes it; host_common.h TablesFile), the program's own arrays:
//   int32 b_reso[3] | float b_sum | b_cmf, b_pmf [cells] | int32 mass_reso[4] | int32 nrounds | float d_sec_edge [num_sec_edges x 16] | float adj [W H 3]
// Prints: the sums of |derivative image| and |g_sec_edge|, the survivor counts, the sums of both masses.
int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: path_guide_san <tables file>\n"); return 2; }
    TablesFile tf;
    if (!tf.open("path_guide_san", argv[1])) return 2;
    const psdr_scene_desc &d = tf.d;
    const psdr_render_opts &o = tf.o;
    int32_t b_reso[3], mass_reso[4], nrounds = 0;
    float b_sum = 0.f;
    if (!tf.rd(b_reso, sizeof(b_reso)) || !tf.rd(&b_sum, 4)) { std::fprintf(stderr, "path_guide_san: short options\n"); return 2; }
    const long long cells_b = (long long) b_reso[0] * b_reso[1] * b_reso[2];
    if (cells_b <= 0 || cells_b > (1 << 20)) return 2;
    std::vector<float> b_cmf((size_t) cells_b), b_pmf((size_t) cells_b);
    if (!tf.rd(b_cmf) || !tf.rd(b_pmf) || !tf.rd(mass_reso, sizeof(mass_reso)) || !tf.rd(&nrounds, 4)) return 2;
    const long long cells_m = (long long) mass_reso[0] * mass_reso[1] * mass_reso[2];
    if (cells_m <= 0 || cells_m > (1 << 20) || d.num_sec_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    std::vector<float> d_se((size_t) d.num_sec_edges * PSDR_SEDGE_STRIDE), adj((size_t) d.width * d.height * 3), dimg(adj.size(), 0.f), g_se(d_se.size(), 0.f);
    if (!tf.rd(d_se) || !tf.rd(adj)) { std::fprintf(stderr, "path_guide_san: short tangents\n"); return 2; }
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
