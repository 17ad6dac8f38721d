// colloc_san.cpp -- TEST-ONLY stand-alone program (its own main, no Python): the host harness of the CollocatedIntegrator (hostcheck_collocated.cpp, i.e. the
// product's csrc/psdr_collocated.h with csrc/psdr_colloc_microfacet.h) over a tables file, built with the host sanitizers by hostlibs.san_program for
// tests/test_collocated_host.py, tests/test_colloc_microfacet_host.py, tests/test_colloc_normal_host.py and tests/test_colloc_height_host.py.  Nothing of it is loaded into Python and nothing of it runs on a GPU.
//   colloc_san <tables file> [record type]
// Tables file (the test writes it; host_common.h TablesFile), the program's own arrays:
//   float d_tri_info [num_tris x 24] | float d_texels [num_texels] | float d_prim_edge [num_prim_edges x 8] | float adj [W H 3]
// With a record type (one of the three PSDR_BSDF_MICROFACET* values; -1 or absent: none) it refuses a file without such a record: exit status 2.  Any other
// second argument gets the usage line.
// Prints the sums of |image|, |derivative image|, |g_tri_info|, |g_texels|, |g_prim_edge|.
#include "hostcheck_collocated.cpp"

#include <cstdlib>

namespace {
double abs_sum(const std::vector<float> &v) { double s = 0; for (float x : v) s += std::fabs(x); return s; }

const char *record_name(int type) {
    switch (type) {
        case PSDR_BSDF_MICROFACET: return "MicrofacetBSDF";
        case PSDR_BSDF_MICROFACET_NORMAL: return "normal-mapped MicrofacetBSDF";
        case PSDR_BSDF_MICROFACET_HEIGHT: return "height-mapped MicrofacetBSDF";
        default: return nullptr;
    }
}
}  // namespace

int main(int argc, char **argv) {
    long need = -1;
    char *end = argc > 2 ? argv[2] : nullptr;
    if (argc > 2) need = std::strtol(argv[2], &end, 10);
    if (argc < 2 || (argc > 2 && (end == argv[2] || *end || (need != -1 && !record_name((int) need))))) {
        std::fprintf(stderr, "usage: colloc_san <tables file> [record type: %d, %d, %d or -1]\n", PSDR_BSDF_MICROFACET, PSDR_BSDF_MICROFACET_NORMAL, PSDR_BSDF_MICROFACET_HEIGHT);
        return 2;
    }
    TablesFile tf;
    if (!tf.open("colloc_san", argv[1])) return 2;
    const psdr_scene_desc &d = tf.d;
    const psdr_render_opts &o = tf.o;
    bool found = need < 0;
    for (int b = 0; b < d.num_bsdfs; ++b) found = found || d.bsdf_rec[(size_t) b * PSDR_BSDF_STRIDE] == need;
    if (!found) { std::fprintf(stderr, "colloc_san: no %s record (type %ld) in the tables\n", record_name((int) need), need); return 2; }
    if (d.num_tris <= 0 || d.num_texels <= 0 || d.num_prim_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    std::vector<float> d_tri((size_t) d.num_tris * PSDR_TRI_STRIDE), d_tex((size_t) d.num_texels), d_pe((size_t) d.num_prim_edges * PSDR_PEDGE_STRIDE), adj((size_t) d.width * d.height * 3);
    if (!tf.rd(d_tri) || !tf.rd(d_tex) || !tf.rd(d_pe) || !tf.rd(adj)) { std::fprintf(stderr, "colloc_san: short tangents\n"); return 2; }
    std::vector<float> img(adj.size(), 0.f), img1(adj.size(), 0.f), dimg(adj.size(), 0.f), g_tri(d_tri.size(), 0.f), g_tex(d_tex.size(), 0.f), g_pe(d_pe.size(), 0.f);
    psdr_tangents tan{}; tan.d_tri_info = d_tri.data(); tan.d_texels = d_tex.data(); tan.d_prim_edge = d_pe.data();
    psdr_grads g{}; g.g_tri_info = g_tri.data(); g.g_texels = g_tex.data(); g.g_prim_edge = g_pe.data();
    if (int rc = hostcheck_collocated_render(&d, &o, 0, nullptr, img.data(), nullptr, 2)) return 10 + rc;
    if (int rc = hostcheck_collocated_render(&d, &o, 1, &tan, img1.data(), dimg.data(), 2)) return 20 + rc;
    if (int rc = hostcheck_collocated_rev(&d, &o, adj.data(), img1.data(), &g)) return 30 + rc;
    std::printf("%.9g %.9g %.9g %.9g %.9g\n", abs_sum(img), abs_sum(dimg), abs_sum(g_tri), abs_sum(g_tex), abs_sum(g_pe));
    return 0;
}
