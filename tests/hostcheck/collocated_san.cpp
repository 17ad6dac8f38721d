// collocated_san.cpp -- TEST-ONLY stand-alone program (its own main, no Python): the host harness of the CollocatedIntegrator (hostcheck_collocated.cpp, i.e. the
// product's csrc/psdr_collocated.h) over a tables file, built with the host sanitizers by tests/test_collocated_host.py.  Nothing of it is loaded into Python and
// nothing of it runs on a GPU.
// Tables file (the test writes it):
//   int64 sizeof(desc) | desc bytes | int64 m | m x (int64 offset of a pointer member in desc, int64 bytes, data) | opts bytes |
//   float d_tri_info [num_tris x 24] | float d_texels [num_texels] | float d_prim_edge [num_prim_edges x 8] | float adj [W H 3]
// Prints the sums of |image|, |derivative image|, |g_tri_info|, |g_texels|, |g_prim_edge|.
#include "hostcheck_collocated.cpp"

#include <cstdio>

namespace {
bool rd(std::FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }
double abs_sum(const std::vector<float> &v) { double s = 0; for (float x : v) s += std::fabs(x); return s; }
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: collocated_san <tables file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "collocated_san: cannot open %s\n", argv[1]); return 2; }
    long long sz = 0, m = 0;
    psdr_scene_desc d{};
    if (!rd(f, &sz, 8) || sz != (long long) sizeof(d) || !rd(f, &d, sizeof(d)) || !rd(f, &m, 8) || m < 0 || m > 64) { std::fprintf(stderr, "collocated_san: bad header\n"); return 2; }
    std::vector<std::vector<double>> blocks((size_t) m);          // (double: every table aligned for any element type)
    for (long long i = 0; i < m; ++i) {
        long long off = 0, bytes = 0;
        if (!rd(f, &off, 8) || !rd(f, &bytes, 8) || off < 0 || off + 8 > (long long) sizeof(d) || bytes < 0) { std::fprintf(stderr, "collocated_san: bad table record\n"); return 2; }
        blocks[(size_t) i].assign((size_t) bytes / 8 + 1, 0.0);
        if (!rd(f, blocks[(size_t) i].data(), (size_t) bytes)) { std::fprintf(stderr, "collocated_san: short table\n"); return 2; }
        const void *p = blocks[(size_t) i].data();
        std::memcpy(reinterpret_cast<char *>(&d) + off, &p, sizeof(p));
    }
    psdr_render_opts o{};
    if (!rd(f, &o, sizeof(o))) { std::fprintf(stderr, "collocated_san: short options\n"); return 2; }
    if (d.num_tris <= 0 || d.num_texels <= 0 || d.num_prim_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    std::vector<float> d_tri((size_t) d.num_tris * PSDR_TRI_STRIDE), d_tex((size_t) d.num_texels), d_pe((size_t) d.num_prim_edges * PSDR_PEDGE_STRIDE), adj((size_t) d.width * d.height * 3);
    if (!rd(f, d_tri.data(), 4 * d_tri.size()) || !rd(f, d_tex.data(), 4 * d_tex.size()) || !rd(f, d_pe.data(), 4 * d_pe.size()) || !rd(f, adj.data(), 4 * adj.size())) {
        std::fprintf(stderr, "collocated_san: short tangents\n"); return 2;
    }
    std::fclose(f);
    std::vector<float> img(adj.size(), 0.f), img1(adj.size(), 0.f), dimg(adj.size(), 0.f), g_tri(d_tri.size(), 0.f), g_tex(d_tex.size(), 0.f), g_pe(d_pe.size(), 0.f);
    psdr_tangents tan{}; tan.d_tri_info = d_tri.data(); tan.d_texels = d_tex.data(); tan.d_prim_edge = d_pe.data();
    psdr_grads g{}; g.g_tri_info = g_tri.data(); g.g_texels = g_tex.data(); g.g_prim_edge = g_pe.data();
    if (int rc = hostcheck_collocated_render(&d, &o, 0, nullptr, img.data(), nullptr, 2)) return 10 + rc;
    if (int rc = hostcheck_collocated_render(&d, &o, 1, &tan, img1.data(), dimg.data(), 2)) return 20 + rc;
    if (int rc = hostcheck_collocated_rev(&d, &o, adj.data(), img1.data(), &g)) return 30 + rc;
    std::printf("%.9g %.9g %.9g %.9g %.9g\n", abs_sum(img), abs_sum(dimg), abs_sum(g_tri), abs_sum(g_tex), abs_sum(g_pe));
    return 0;
}
