// colloc_height_san.cpp -- TEST-ONLY stand-alone program (its own main, no Python): the host harness of the CollocatedIntegrator (hostcheck_collocated.cpp, i.e.
// the product's csrc/psdr_collocated.h with csrc/psdr_colloc_microfacet.h) over the tables file of a scene that mixes a diffuse, a rough-conductor, a MicrofacetBSDF, a normal-mapped
// and a height-mapped MicrofacetBSDF mesh, built with the host sanitizers by tests/test_colloc_height_host.py.  Nothing of it is loaded into Python and nothing of it runs on a GPU.
// Tables file (the test writes it; host_common.h TablesFile), the program's own arrays:
//   float d_tri_info [num_tris x 24] | float d_texels [num_texels] | float d_prim_edge [num_prim_edges x 8] | float adj [W H 3]
// Refuses a file without a PSDR_BSDF_MICROFACET_HEIGHT record.  Prints the sums of |image|, |derivative image|, |g_tri_info|, |g_texels|, |g_prim_edge|.
#include "hostcheck_collocated.cpp"

namespace {
double abs_sum(const std::vector<float> &v) { double s = 0; for (float x : v) s += std::fabs(x); return s; }
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: colloc_height_san <tables file>\n"); return 2; }
    TablesFile tf;
    if (!tf.open("colloc_height_san", argv[1])) return 2;
    const psdr_scene_desc &d = tf.d;
    const psdr_render_opts &o = tf.o;
    bool has_height_map = false;
    for (int b = 0; b < d.num_bsdfs; ++b) has_height_map = has_height_map || d.bsdf_rec[(size_t) b * PSDR_BSDF_STRIDE] == PSDR_BSDF_MICROFACET_HEIGHT;
    if (!has_height_map) { std::fprintf(stderr, "colloc_height_san: no height-mapped MicrofacetBSDF record in the tables\n"); return 2; }
    if (d.num_tris <= 0 || d.num_texels <= 0 || d.num_prim_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    std::vector<float> d_tri((size_t) d.num_tris * PSDR_TRI_STRIDE), d_tex((size_t) d.num_texels), d_pe((size_t) d.num_prim_edges * PSDR_PEDGE_STRIDE), adj((size_t) d.width * d.height * 3);
    if (!tf.rd(d_tri) || !tf.rd(d_tex) || !tf.rd(d_pe) || !tf.rd(adj)) { std::fprintf(stderr, "colloc_height_san: short tangents\n"); return 2; }
    std::vector<float> img(adj.size(), 0.f), img1(adj.size(), 0.f), dimg(adj.size(), 0.f), g_tri(d_tri.size(), 0.f), g_tex(d_tex.size(), 0.f), g_pe(d_pe.size(), 0.f);
    psdr_tangents tan{}; tan.d_tri_info = d_tri.data(); tan.d_texels = d_tex.data(); tan.d_prim_edge = d_pe.data();
    psdr_grads g{}; g.g_tri_info = g_tri.data(); g.g_texels = g_tex.data(); g.g_prim_edge = g_pe.data();
    if (int rc = hostcheck_collocated_render(&d, &o, 0, nullptr, img.data(), nullptr, 2)) return 10 + rc;
    if (int rc = hostcheck_collocated_render(&d, &o, 1, &tan, img1.data(), dimg.data(), 2)) return 20 + rc;
    if (int rc = hostcheck_collocated_rev(&d, &o, adj.data(), img1.data(), &g)) return 30 + rc;
    std::printf("%.9g %.9g %.9g %.9g %.9g\n", abs_sum(img), abs_sum(dimg), abs_sum(g_tri), abs_sum(g_tex), abs_sum(g_pe));
    return 0;
}
