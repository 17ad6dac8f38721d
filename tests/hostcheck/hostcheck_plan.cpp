// hostcheck_plan.cpp -- TEST-ONLY harness: the launch planning of csrc/psdr_plan.h (pure host functions: grids, LDS plans, launch forms) run over hand-filled
// scene handles, so that tests/test_launch_plan_host.py can check every rule where no GPU exists; and the tree build and trace planning of csrc/psdr_tree_plan.h
// (hostcheck_tree at the end, for tests/test_tree_plan_host.py).  No HIP call is made and no device is opened; psdr_host::fail,
// which the product defines in psdr_hip.hip, is this file's own and keeps the message.  Never imported by the psdr_cuda package.
#include "../../psdr-cuda_amd/csrc/psdr_host.h"

namespace {
std::string g_error;
float g_table[1];          // stands for any caller-owned table that only has to be there

// what a test says of a handle; everything else keeps psdr_scene_s's defaults
struct PlanHandle {
    int32_t n_tiny, n_blas, num_nodes, num_btris, bvh_depth, num_nodes4, num_tris, num_meshes, num_bsdfs, num_emitters, emitter_tri0, emitter_tris, num_texels,
        has_rough, env_emitter, lds_budget, lds_limit, hot_rows, hot_identity, sink_rep, sink_private, rev_split, rev_sorted, own_pixels, chunk_log2, width, height;
};
void fill(psdr_scene_s &h, const PlanHandle &p) {
    h.n_tiny = p.n_tiny; h.n_blas = p.n_blas; h.num_nodes = p.num_nodes; h.num_btris = p.num_btris; h.bvh_depth = p.bvh_depth;
    h.num_nodes4 = p.num_nodes4; h.d_nodes4 = p.num_nodes4 > 0 ? reinterpret_cast<Bvh4Node *>(g_table) : nullptr;          // (never dereferenced: traced_wavefront asks whether it is there)
    h.desc.num_tris = p.num_tris; h.desc.num_meshes = p.num_meshes; h.desc.num_bsdfs = p.num_bsdfs; h.desc.num_emitters = p.num_emitters; h.desc.num_texels = p.num_texels;
    h.desc.face_cmf = h.desc.face_pmf = g_table;
    h.emitter_i.assign((size_t) std::max(p.num_emitters, 0) * PSDR_EMITTER_I_STRIDE, 0);
    if (p.num_emitters > 0) { h.emitter_i[1] = p.emitter_tri0; h.emitter_i[2] = p.emitter_tris; }
    h.has_rough = p.has_rough != 0; h.desc.env_emitter = p.env_emitter; h.opt.lds_budget = p.lds_budget; h.lds_limit = p.lds_limit;
    h.hot_rows = p.hot_rows; h.hot_identity = p.hot_identity != 0; h.opt.sink_rep = p.sink_rep; h.opt.sink_private = p.sink_private;
    h.opt.rev_split = p.rev_split; h.opt.rev_sorted = p.rev_sorted; h.opt.own_pixels = p.own_pixels; h.opt.chunk_log2 = p.chunk_log2;
    h.desc.width = p.width; h.desc.height = p.height;
    h.have_tables = h.have_bvh = true;
}
// grads_mask: bit 0 texels, 1 emitter radiances, 2 triangle rows, 3 camera matrix, 4 environment map
psdr_grads grads_of(int mask) {
    psdr_grads g{};
    if (mask & 1) g.g_texels = g_table;
    if (mask & 2) g.g_emitter_rad = g_table;
    if (mask & 4) g.g_tri_info = g_table;
    if (mask & 8) g.g_cam_to_world = g_table;
    if (mask & 16) g.g_env_f = g_table;
    return g;
}
int put_layout(const SinkLayout &L, int32_t *out) {
    const int32_t v[] = {L.cam_off, L.env_off, L.env_n, L.tex_off, L.tex_n, L.rad_off, L.rad_n, L.hot_off, L.hot_rows, L.total, L.rep, L.stride, L.priv_off, L.priv_rows,
                         L.priv_regs, L.pend_off, L.pend_rows, psdr_host::sink_bytes(L)};
    std::copy(std::begin(v), std::end(v), out);
    return (int) (sizeof(v) / sizeof(v[0]));
}
int put_ctx(const LaunchCtx &cx, int32_t *out) { out[0] = cx.off_stack; out[1] = cx.off_pathrec; out[2] = cx.off_sink; return 3; }
}  // namespace

namespace psdr_host {
int fail(const std::string &m) { g_error = m; return 1; }
}  // namespace psdr_host
using namespace psdr_host;

extern "C" {
const char *hostcheck_plan_error() { return g_error.c_str(); }

// out: return value, lds_bytes, then the blocks in their declared order as (offset, bytes) pairs -- nodes, leaf triangles, triangle rows, hit rows --, then
// n_lnodes, n_lbtris, n_ltri, lt_end, off_stack, lt_nfaces, then the 13 lt_* offsets
int hostcheck_plan_lds(const PlanHandle *p, int reserved, int32_t *out) {
    psdr_scene_s h; fill(h, *p);
    LaunchCtx cx{};
    const int ret = plan_lds(&h, cx, reserved);
    const SceneView &sc = cx.sc;
    const int32_t v[] = {ret, lds_bytes(cx, &h), sc.off_lnodes, sc.n_lnodes * kLdsNodeStride, sc.off_lbtris, sc.n_lbtris * 48, sc.off_ltri, sc.n_ltri * 96, sc.off_lprim, h.n_tiny * kTinyHitWords * 4,
                         sc.n_lnodes, sc.n_lbtris, sc.n_ltri, sc.lt_end, cx.off_stack, sc.lt_nfaces,
                         sc.lt_trimesh, sc.lt_meshbsdf, sc.lt_meshemitter, sc.lt_bsdf, sc.lt_emf, sc.lt_emi, sc.lt_fcmf, sc.lt_fpmf, sc.lt_ecmf, sc.lt_epmf, sc.lt_uv, sc.lt_tex, sc.lt_occ};
    std::copy(std::begin(v), std::end(v), out);
    return 0;
}
int hostcheck_plan_owns(const PlanHandle *p, int nsp, long long chunk) { psdr_scene_s h; fill(h, *p); return wave_owns_pixels(&h, nsp, chunk) ? 1 : 0; }
int hostcheck_plan_flag_set(const PlanHandle *p) { psdr_scene_s h; fill(h, *p); return scene_flag_set(&h); }
int hostcheck_plan_replicas(long long pe_words, long long n) { return primary_edge_replicas(pe_words, n); }
long long hostcheck_plan_filter_grid(long long n, int divisor) { return filter_grid_slots(n, divisor); }
int hostcheck_plan_record_words(int depth, int wavefront) { return rev_record_words(depth, wavefront != 0); }
// out[0]: rev_launch_splits, out[1]: rev_value_sweep_is_wavefront
int hostcheck_plan_split(const PlanHandle *p, const psdr_render_opts *o, long long n, int32_t *out) {
    psdr_scene_s h; fill(h, *p);
    out[0] = rev_launch_splits(&h, o, n) ? 1 : 0;
    out[1] = rev_value_sweep_is_wavefront(&h, o, n) ? 1 : 0;
    return 0;
}
int hostcheck_plan_sink_layout(const PlanHandle *p, int grads_mask, int32_t *out) {
    psdr_scene_s h; fill(h, *p);
    const psdr_grads g = grads_of(grads_mask);
    put_layout(make_sink_layout(&h, &g), out);
    return 0;
}
// out: dyn_bytes, the context's offsets (3), the layout (put_layout); returns plan_rev_one_vertex's value
int hostcheck_plan_one_vertex(const PlanHandle *p, int grads_mask, int32_t *out) {
    psdr_scene_s h; fill(h, *p);
    const psdr_grads g = grads_of(grads_mask);
    SinkLayout L = make_sink_layout(&h, &g);
    LaunchCtx cx{};
    plan_lds(&h, cx);
    int dyn = 0;
    const int rc = plan_rev_one_vertex(&h, cx, L, &dyn);
    out[0] = dyn; out += 1;
    out += put_ctx(cx, out);
    put_layout(L, out);
    return rc;
}
// out: form, depth, rec_bytes, cache_bytes, dyn1, dyn_bytes, geo, deep_rec, split, kept_fused, no_tree, rev_layout[0..15], cx's offsets, cx2's offsets, the layout;
// returns plan_rev_camera's value
int hostcheck_plan_rev_camera(const PlanHandle *p, const psdr_render_opts *o, int grads_mask, int fl, int reg_priv, int value_only, int32_t *out) {
    psdr_scene_s h; fill(h, *p);
    const psdr_grads g = grads_of(grads_mask);
    SinkLayout L = make_sink_layout(&h, &g);
    LaunchCtx cx{}, cx2{};
    plan_lds(&h, cx);
    RevCameraPlan pl{};
    const long long n = (long long) h.desc.width * h.desc.height * (o->spp_end - o->spp_begin);
    const int rc = plan_rev_camera(&h, o, &g, n, fl, reg_priv != 0, value_only != 0, false, L, cx, cx2, pl);
    const int32_t v[] = {pl.form, pl.depth, pl.rec_bytes, pl.cache_bytes, pl.dyn1, pl.dyn_bytes, pl.geo, pl.deep_rec, pl.split, pl.kept_fused, pl.no_tree};
    out = std::copy(std::begin(v), std::end(v), out);
    out = std::copy(std::begin(h.rev_layout), std::end(h.rev_layout), out);
    out += put_ctx(cx, out);
    out += put_ctx(cx2, out);
    put_layout(L, out);
    return rc;
}

// ---- tree build and trace planning (csrc/psdr_tree_plan.h), for tests/test_tree_plan_host.py and for tests/hostcheck/tree_plan_san.cpp, which runs the same entry
// under the host sanitizers: ONE entry, numbers in, numbers out (every integer and every float32 the rules see is exact in a double).  Rules that read the handle
// take TreeHandle's fields first.  Returns the count of numbers written to `out`, -1 for an unknown rule or too few numbers.
struct TreeHandle {
    double refit_enabled, tiny_enabled, two_level_enabled, refit_ok, tree_tris, num_nodes, refits_since_build, lbvh, built_area, bvh_device_mode, num_meshes, env_emitter,
        forest_min_inline, num_nodes4, stack_need4, lds_limit, trace_wg2, num_cus, blocks_per_cu;
};
int hostcheck_tree(const char *what, const double *in, int n, double *out) {
    const std::string w(what);
    const double *end = in + n;
    bool short_of = false;
    auto next = [&]() { if (in >= end) { short_of = true; return 0.0; } return *in++; };
    auto next_ints = [&](size_t count) { std::vector<int32_t> v; for (size_t i = 0; i < count && !short_of; ++i) v.push_back((int32_t) next()); return v; };
    psdr_scene_s h;
    if (w == "refit" || w == "kind" || w == "trace" || w == "probe") {
        TreeHandle t;
        if (n < (int) (sizeof(t) / sizeof(double))) return -1;
        std::memcpy(&t, in, sizeof(t)); in += sizeof(t) / sizeof(double);
        h.refit_enabled = t.refit_enabled != 0; h.tiny_enabled = t.tiny_enabled != 0; h.two_level_enabled = t.two_level_enabled != 0; h.refit_ok = t.refit_ok != 0;
        h.tree_tris = (int) t.tree_tris; h.num_nodes = (int) t.num_nodes; h.refits_since_build = (int) t.refits_since_build; h.lbvh = t.lbvh != 0;
        h.built_area = (float) t.built_area; h.bvh_device_mode = (int) t.bvh_device_mode; h.desc.num_meshes = (int) t.num_meshes; h.desc.env_emitter = (int) t.env_emitter;
        h.forest_min_inline = (int) t.forest_min_inline; h.num_nodes4 = (int) t.num_nodes4; h.stack_need4 = (int) t.stack_need4; h.lds_limit = (int) t.lds_limit;
        h.opt.trace_wg2 = (int) t.trace_wg2; h.num_cus = (int) t.num_cus; h.opt.blocks_per_cu = (int) t.blocks_per_cu;
    }
    int m = 0;
    if (w == "mask") {          // num_emitters, env_emitter, T, words of emitter_i, emitter_i -> emit_rows wanted, the mask
        h.desc.num_emitters = (int) next(); h.desc.env_emitter = (int) next();
        const int T = (int) next();
        h.emitter_i = next_ints((size_t) next());
        out[m++] = emit_rows_wanted(&h) ? 1 : 0;
        for (char c : emitter_triangle_mask(h.emitter_i, h.desc.num_emitters, T)) out[m++] = c;
    } else if (w == "hot") {          // T, tiny, num_emitters, words of emitter_i, emitter_i, entries of by_area, by_area -> slot -> triangle
        const int T = (int) next(), tiny = (int) next(), num_emitters = (int) next();
        const std::vector<int32_t> emitter_i = next_ints((size_t) next()), by_area = next_ints((size_t) next());
        for (int32_t t : hot_row_list(T, tiny != 0, emitter_i, num_emitters, by_area.data(), (int) by_area.size())) out[m++] = t;
    } else if (w == "occ") {          // T, n_tiny, is_em [T], occ [T * T] -> occ_max_rows
        const int T = (int) next(), n_tiny = (int) next();
        const std::vector<int32_t> em = next_ints((size_t) T);
        std::vector<uint32_t> occ;
        for (int i = 0; i < T * T; ++i) occ.push_back((uint32_t) next());
        if (!short_of) out[m++] = occluder_max_rows(occ, std::vector<char>(em.begin(), em.end()), T, n_tiny);
    } else if (w == "levels") {          // root, nodes, per node lo0 hi0 lo1 hi1 (12 floats) c0 c1 -> area, level_start
        const int32_t root = (int32_t) next();
        std::vector<BvhNode> nodes((size_t) next());
        for (BvhNode &nd : nodes) {
            for (float *f : {nd.lo0, nd.hi0, nd.lo1, nd.hi1}) for (int k = 0; k < 3; ++k) f[k] = (float) next();
            nd.c0 = (int32_t) next(); nd.c1 = (int32_t) next();
        }
        std::vector<int> levels{-7};          // (cleared by the rule)
        out[m++] = short_of ? 0.0 : tree_levels_and_area(nodes, root, levels);
        for (int l : levels) out[m++] = l;
    } else if (w == "refit") {          // T, tiny, emitters_same, forest_stands, prev_area -> refit_candidate, refit_choice
        const int T = (int) next(), tiny = (int) next(), same = (int) next(), stands = (int) next();
        const float prev_area = (float) next();
        out[m++] = refit_candidate(&h, T, tiny != 0) ? 1 : 0;
        out[m++] = refit_choice(&h, same != 0, stands != 0, prev_area);
    } else if (w == "inline_fits") {
        out[m++] = refit_inline_fits((int) next()) ? 1 : 0;
    } else if (w == "kind") {          // T, packed top primitives, inline triangles -> tiny_scene, device_build_wanted, forest_candidate, forest_kept
        const int T = (int) next(), n_top = (int) next(), n_inline = (int) next();
        const bool tiny = tiny_scene(&h, T);
        out[m++] = tiny; out[m++] = device_build_wanted(&h, T, tiny); out[m++] = forest_candidate(&h, T); out[m++] = forest_kept(&h, n_top, n_inline);
    } else if (w == "forest_stands") {          // n_blas, num_meshes, num_emitters, faces of emitter 0 -> forest_stands
        h.n_blas = (int) next(); h.desc.num_meshes = (int) next(); h.desc.num_emitters = (int) next(); h.desc.env_emitter = -1;
        h.desc.face_cmf = h.desc.face_pmf = g_table;
        h.emitter_i.assign((size_t) std::max(h.desc.num_emitters, 0) * PSDR_EMITTER_I_STRIDE, 0);
        const int faces = (int) next();
        if (!h.emitter_i.empty()) h.emitter_i[2] = faces;
        out[m++] = forest_stands(&h) ? 1 : 0;
    } else if (w == "trace") {          // sub_cap -> the plan
        const TracePlan p = plan_wf_trace(&h, (long long) next());
        for (double v : {(double) p.wg2, (double) p.ovf, (double) p.S, (double) p.n_lnodes, (double) p.off_stack, (double) p.stack_entries, (double) p.grid, (double) p.dyn,
                         (double) p.ovf_stride, (double) p.ovf_bytes}) out[m++] = v;
    } else if (w == "probe") {          // slots, rays_per_slot, per_cu -> the plan
        const long long slots = (long long) next();
        const int rays = (int) next(), per_cu = (int) next();
        const ProbePlan p = plan_probe_buffers(&h, slots, rays, per_cu);
        for (double v : {(double) p.sub_cap, (double) p.cnt_bytes, (double) p.hit_bytes, (double) p.mask_bytes, (double) p.req_bytes, (double) p.total}) out[m++] = v;
    } else if (w == "boxes") {          // n_blas, blas_root4 [kMaxBlas] -> lo.w and hi.w of every box as integers (lo.w = 100 + k, hi.w = -1 going in)
        h.n_blas = (int) next();
        for (int k = 0; k < kMaxBlas; ++k) {
            h.blas_root4[k] = (int32_t) next();
            const int32_t root = 100 + k, none = -1;
            h.blas_lo[k] = float4{(float) k, 0.f, 0.f, 0.f}; h.blas_hi[k] = float4{(float) k + 1.f, 1.f, 1.f, 0.f};
            std::memcpy(&h.blas_lo[k].w, &root, 4); std::memcpy(&h.blas_hi[k].w, &none, 4);
        }
        float4 lo[kMaxBlas], hi[kMaxBlas];
        pack_blas_boxes(&h, lo, hi);
        for (int k = 0; k < kMaxBlas; ++k) {
            int32_t a, b;
            std::memcpy(&a, &lo[k].w, 4); std::memcpy(&b, &hi[k].w, 4);
            out[m++] = a; out[m++] = b; out[m++] = lo[k].x; out[m++] = hi[k].x;
        }
    } else return -1;
    return short_of ? -1 : m;
}
}
