// lightstage_san.cpp -- TEST-ONLY stand-alone program (its own main, no Python): the host harness of the LightStageIntegrator (hostcheck_lightstage.cpp, i.e. the
// product's csrc/psdr_lightstage.h) over a tables file, built with the host sanitizers by hostlibs.san_program for tests/test_lightstage_host.py.  Nothing of it
// is loaded into Python and nothing of it runs on a GPU.
//   lightstage_san <tables file> <L>
// Tables file (the test writes it; host_common.h TablesFile), the program's own arrays:
//   float d_tri_info [num_tris x 24] | float d_texels [num_texels] | float d_prim_edge [num_prim_edges x 8] | float d_sec_edge [num_sec_edges x 16] |
//   float adj [L][W H 3] | float pos [L][3] | float d_pos [L][3]
// Prints the sums of |images|, |derivative images|, |g_tri_info|, |g_texels|, |g_prim_edge|, |g_sec_edge|, |g_pos|.
#include "hostcheck_lightstage.cpp"

namespace {
double abs_sum(const std::vector<float> &v) { double s = 0; for (float x : v) s += std::fabs(x); return s; }
}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: lightstage_san <tables file> <L>\n"); return 2; }
    const int L = std::atoi(argv[2]);
    if (L < 1 || L > PSDR_POINT_LIGHTS_MAX) return 2;
    TablesFile tf;
    if (!tf.open("lightstage_san", argv[1])) return 2;
    const psdr_scene_desc &d = tf.d;
    const psdr_render_opts &o = tf.o;
    if (d.num_tris <= 0 || d.num_texels <= 0 || d.num_prim_edges <= 0 || d.num_sec_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    std::vector<float> d_tri((size_t) d.num_tris * PSDR_TRI_STRIDE), d_tex((size_t) d.num_texels), d_pe((size_t) d.num_prim_edges * PSDR_PEDGE_STRIDE),
        d_se((size_t) d.num_sec_edges * PSDR_SEDGE_STRIDE), adj((size_t) L * d.width * d.height * 3), pos((size_t) 3 * L), d_pos((size_t) 3 * L);
    if (!tf.rd(d_tri) || !tf.rd(d_tex) || !tf.rd(d_pe) || !tf.rd(d_se) || !tf.rd(adj) || !tf.rd(pos) || !tf.rd(d_pos)) { std::fprintf(stderr, "lightstage_san: short tangents\n"); return 2; }
    std::vector<float> img(adj.size(), 0.f), img1(adj.size(), 0.f), dimg(adj.size(), 0.f), g_tri(d_tri.size(), 0.f), g_tex(d_tex.size(), 0.f), g_pe(d_pe.size(), 0.f),
        g_se(d_se.size(), 0.f), g_pos((size_t) 3 * L, 0.f);
    psdr_tangents tan{}; tan.d_tri_info = d_tri.data(); tan.d_texels = d_tex.data(); tan.d_prim_edge = d_pe.data(); tan.d_sec_edge = d_se.data();
    psdr_grads g{}; g.g_tri_info = g_tri.data(); g.g_texels = g_tex.data(); g.g_prim_edge = g_pe.data(); g.g_sec_edge = g_se.data();
    if (int rc = hostcheck_lightstage_render(&d, &o, 0, 1, nullptr, L, pos.data(), nullptr, img.data(), nullptr, 2)) return 10 + rc;
    if (int rc = hostcheck_lightstage_render(&d, &o, 1, 1, &tan, L, pos.data(), d_pos.data(), img1.data(), dimg.data(), 2)) return 20 + rc;
    if (int rc = hostcheck_lightstage_rev(&d, &o, L, pos.data(), adj.data(), img1.data(), &g, g_pos.data())) return 30 + rc;
    std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", abs_sum(img), abs_sum(dimg), abs_sum(g_tri), abs_sum(g_tex), abs_sum(g_pe), abs_sum(g_se), abs_sum(g_pos));
    return 0;
}
