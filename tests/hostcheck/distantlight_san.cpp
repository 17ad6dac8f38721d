// distantlight_san.cpp -- TEST-ONLY stand-alone program (its own main, no Python): the host harness of the light models (hostcheck_distantlight.cpp, i.e. the
// product's csrc/psdr_pointlight.h and csrc/psdr_lightstage.h with a kind per light) over a tables file, built with the host sanitizers by
// hostlibs.san_program for tests/test_distantlight_host.py.  Nothing of it is loaded into Python and nothing of it runs on a GPU.
//   distantlight_san <tables file> <L>
// Runs the stack of L lights (render, forward and reverse, all three terms) and light 0 alone through the single-light functions.
// Tables file (the test writes it; host_common.h TablesFile), the program's own arrays:
//   float d_tri_info [num_tris x 24] | float d_texels [num_texels] | float d_prim_edge [num_prim_edges x 8] | float d_sec_edge [num_sec_edges x 16] |
//   float adj [L][W H 3] | float v [L][3] | float d_v [L][3] | int32 kinds [L]
// Prints the sums of |images|, |derivative images|, |g_tri_info|, |g_texels|, |g_prim_edge|, |g_sec_edge|, |g_v| of the stack, then of light 0 alone:
// |image|, |derivative image|, |g_v|.
#include "hostcheck_distantlight.cpp"

namespace {
double abs_sum(const std::vector<float> &v) { double s = 0; for (float x : v) s += std::fabs(x); return s; }
}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: distantlight_san <tables file> <L>\n"); return 2; }
    const int L = std::atoi(argv[2]);
    if (L < 1 || L > PSDR_POINT_LIGHTS_MAX) return 2;
    TablesFile tf;
    if (!tf.open("distantlight_san", argv[1])) return 2;
    const psdr_scene_desc &d = tf.d;
    const psdr_render_opts &o = tf.o;
    if (d.num_tris <= 0 || d.num_texels <= 0 || d.num_prim_edges <= 0 || d.num_sec_edges <= 0 || d.width <= 0 || d.height <= 0) return 2;
    const size_t n = (size_t) d.width * d.height * 3;
    std::vector<float> d_tri((size_t) d.num_tris * PSDR_TRI_STRIDE), d_tex((size_t) d.num_texels), d_pe((size_t) d.num_prim_edges * PSDR_PEDGE_STRIDE),
        d_se((size_t) d.num_sec_edges * PSDR_SEDGE_STRIDE), adj((size_t) L * n), v((size_t) 3 * L), d_v((size_t) 3 * L);
    std::vector<int32_t> kinds((size_t) L);
    if (!tf.rd(d_tri) || !tf.rd(d_tex) || !tf.rd(d_pe) || !tf.rd(d_se) || !tf.rd(adj) || !tf.rd(v) || !tf.rd(d_v) || !tf.rd(kinds)) { std::fprintf(stderr, "distantlight_san: short tangents\n"); return 2; }
    std::vector<float> img(adj.size(), 0.f), img1(adj.size(), 0.f), dimg(adj.size(), 0.f), g_tri(d_tri.size(), 0.f), g_tex(d_tex.size(), 0.f), g_pe(d_pe.size(), 0.f),
        g_se(d_se.size(), 0.f), g_v((size_t) 3 * L, 0.f);
    psdr_tangents tan{}; tan.d_tri_info = d_tri.data(); tan.d_texels = d_tex.data(); tan.d_prim_edge = d_pe.data(); tan.d_sec_edge = d_se.data();
    psdr_grads g{}; g.g_tri_info = g_tri.data(); g.g_texels = g_tex.data(); g.g_prim_edge = g_pe.data(); g.g_sec_edge = g_se.data();
    if (int rc = hostcheck_distantstack_render(&d, &o, 0, 1, nullptr, L, kinds.data(), v.data(), nullptr, img.data(), nullptr, 2)) return 10 + rc;
    if (int rc = hostcheck_distantstack_render(&d, &o, 1, 1, &tan, L, kinds.data(), v.data(), d_v.data(), img1.data(), dimg.data(), 2)) return 20 + rc;
    if (int rc = hostcheck_distantstack_rev(&d, &o, L, kinds.data(), v.data(), adj.data(), img1.data(), &g, g_v.data())) return 30 + rc;
    std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", abs_sum(img), abs_sum(dimg), abs_sum(g_tri), abs_sum(g_tex), abs_sum(g_pe), abs_sum(g_se), abs_sum(g_v));
    // light 0 alone
    std::vector<float> one(n, 0.f), one1(n, 0.f), done(n, 0.f), g_tri1(d_tri.size(), 0.f), g_tex1(d_tex.size(), 0.f), g_pe1(d_pe.size(), 0.f), g_se1(d_se.size(), 0.f), g_v1(3, 0.f);
    psdr_grads g1{}; g1.g_tri_info = g_tri1.data(); g1.g_texels = g_tex1.data(); g1.g_prim_edge = g_pe1.data(); g1.g_sec_edge = g_se1.data();
    if (int rc = hostcheck_distantlight_render(&d, &o, 0, 1, nullptr, kinds[0], v.data(), nullptr, one.data(), nullptr, 2)) return 40 + rc;
    if (int rc = hostcheck_distantlight_render(&d, &o, 1, 1, &tan, kinds[0], v.data(), d_v.data(), one1.data(), done.data(), 2)) return 50 + rc;
    if (int rc = hostcheck_distantlight_rev(&d, &o, kinds[0], v.data(), adj.data(), one1.data(), &g1, g_v1.data())) return 60 + rc;
    std::printf("%.9g %.9g %.9g\n", abs_sum(one), abs_sum(done), abs_sum(g_v1));
    return 0;
}
