// psdr_plan.h -- launch planning: every rule that turns (scene handle, options, gradient request) into grids, LDS offsets, byte counts and launch forms,
// stated once.  Pure host code: inline functions that make no HIP call and launch nothing, so that tests/hostcheck/hostcheck_plan.cpp runs them on hand-filled
// handles where no GPU exists.  Included at the end of psdr_host.h; the launch drivers of every translation unit (psdr_kernels.h, psdr_collocated.hip,
// psdr_path_sedge.hip, psdr_logd_lean.hip, psdr_hip.hip) plan here and launch there.
#pragma once

namespace psdr_host {
// Grid of the grid-stride kernels: at most per_cu workgroups per CU (16 by default; the forward camera kernels
// choose theirs, camera_blocks_per_cu; the reverse kernels zero and flush a gradient cache per
// workgroup and are flat between 8 and 24).
inline int launch_blocks(const psdr_scene_s *h, long long n, int per_cu = 16) {
    const int forced = h->opt.blocks_per_cu;
    const long long need = (n + kBlock - 1) / kBlock;
    const long long cap = (long long) h->num_cus * (forced ? forced : per_cu);
    return (int) std::max(1LL, std::min(need, cap));
}

// LDS plan of one launch: stacks sized by the tree depth, the rest of a 40 KB budget (4 workgroups
// per CU) filled with the top of the BVH, then the leaf triangles, then the TriangleInfo rows.
constexpr int kLdsBudget = 40 * 1024;
inline bool tiny_only(const psdr_scene_s *h) { return h->n_tiny > 0 && h->n_blas == 0; }
// entries of face_cmf / face_pmf the emitters reference (host copy of emitter_i, psdr_bvh_build)
inline int emitter_faces(const psdr_scene_s *h) {
    int n = 0;
    for (int e = 0; e < h->desc.num_emitters && (size_t) (e + 1) * PSDR_EMITTER_I_STRIDE <= h->emitter_i.size(); ++e)
        n = std::max(n, h->emitter_i[(size_t) e * PSDR_EMITTER_I_STRIDE + 3] + h->emitter_i[(size_t) e * PSDR_EMITTER_I_STRIDE + 2]);
    return n;
}
// A scene without a tree whose small tables fit the LDS block of the kSceneTiny kernel instances (a few KB): every launch on it stages
// them (plan_lds) and variant_of picks those instances.  PSDR_TINY_VARIANTS=0: the general instances (A/B, tools).
constexpr int kLdsTexels = 256, kLdsTexelTangents = 3;
// the mesh-level tables (mesh -> bsdf / emitter, BSDF and emitter records, the emitters' face distributions) fit the LDS block of the kernels
inline bool small_tables_fit(const psdr_scene_s *h) {
    const psdr_scene_desc &d = h->desc;
    return d.env_emitter < 0 && d.num_meshes <= 64 && d.num_bsdfs <= 32 && d.num_emitters >= 0 && d.num_emitters <= 8 &&
           (d.num_emitters == 0 || (d.face_cmf && d.face_pmf)) && emitter_faces(h) <= 64;
}
inline bool tiny_tables_ok(const psdr_scene_s *h) {
    return h->opt.tiny_variants != 0 && tiny_only(h) && small_tables_fit(h);
}
// flag set of the scene's kernels (psdr_device.h TangentView FLAGS): bit 0 = environment map present, bit 1 = a rough conductor may be present, ...
inline int scene_flag_set(const psdr_scene_s *h) {
    return (h->desc.env_emitter >= 0 ? kSceneEnv : 0) | (h->has_rough ? kSceneRough : 0) | (h->n_blas > 0 ? kSceneForest : 0) | (tiny_tables_ok(h) ? kSceneTiny : 0);
}
// The kernels of a two-level scene read the mesh-level tables from LDS and have no other path (psdr_device.h Tab<FL>::lds_small): such a tree
// is only built, and only kept, while they fit (psdr_bvh_build, ensure_tree_kind).
inline bool forest_tables(const psdr_scene_s *h) { return PSDR_FOREST_LDS_TABLES && h->n_blas > 0; }

// traversal-stack entries per lane: none when no launch on this scene ever walks a tree
inline int stack_entries_of(const psdr_scene_s *h) { return tiny_only(h) ? 0 : (h->wide ? h->stack_need4 + 1 : std::min(kBvhStack, h->bvh_depth + 2)); }
inline int staged_nodes_of(const psdr_scene_s *h) { return h->wide ? h->num_nodes4 : h->num_nodes; }
inline int plan_lds(const psdr_scene_s *h, LaunchCtx &cx, int reserved = 0) {
    // the plain diffuse variant runs renderC at 5 workgroups per CU: 28 KB each (C4 PathTracer(3) 40.0 -> 37.6 ms,
    // C3 3.26 -> 3.15 ms; 32 KB is already one workgroup less)
    const int forced = h->opt.lds_budget;
    const bool lean = !h->has_rough && h->desc.env_emitter < 0;
    const int budget = forced ? forced : (lean ? 28 * 1024 : kLdsBudget);
    const int stack_bytes = stack_entries_of(h) * kBlock * 4;
    int room = std::max(0, budget - reserved - stack_bytes);
    // a scene without a tree (all primitives in the kernel arguments) ALWAYS stages its <= 16 TriangleInfo rows (1.5 KB): the kSceneTiny
    // kernel instances have no global-memory fallback for them (psdr_device.h load_tri_f)
    if (tiny_only(h)) room = std::max(room, staged_nodes_of(h) * kLdsNodeStride + h->num_btris * 48 + h->desc.num_tris * 96);
    SceneView &sc = cx.sc;
    int off = 0;
    sc.n_lnodes = std::min(staged_nodes_of(h), room / kLdsNodeStride); sc.off_lnodes = off; off += sc.n_lnodes * kLdsNodeStride; room -= sc.n_lnodes * kLdsNodeStride;
    sc.n_lbtris = (sc.n_lnodes == staged_nodes_of(h)) ? std::min(h->num_btris, room / 48) : 0;
    sc.off_lbtris = off; off += sc.n_lbtris * 48; room -= sc.n_lbtris * 48;
    sc.n_ltri = (sc.n_lbtris == h->num_btris) ? std::min(h->desc.num_tris, room / 96) : 0;
    sc.off_ltri = off; off += sc.n_ltri * 96;
    sc.off_lprim = off; off += h->n_tiny * kTinyHitWords * 4;          // hit rows of the kernel-argument primitives (resolve_tiny_hit)
    // the small tables of a scene without a tree (psdr_device.h Tab<FL>, staged by setup_lds): 16-byte aligned blocks
    sc.lt_trimesh = sc.lt_meshbsdf = sc.lt_meshemitter = sc.lt_bsdf = sc.lt_emf = sc.lt_emi = sc.lt_fcmf = sc.lt_fpmf = sc.lt_uv = sc.lt_tex = sc.lt_ecmf = sc.lt_epmf = -1;
    sc.lt_nfaces = 0; sc.lt_occ = -1; sc.occ = nullptr;
    const bool all_tables = tiny_tables_ok(h);
    if (all_tables || forest_tables(h)) {
        auto take = [&](int words) { const int o = off; off += (words * 4 + 15) / 16 * 16; return o; };
        const psdr_scene_desc &d = h->desc;
        sc.lt_nfaces = emitter_faces(h);
        if (all_tables) sc.lt_trimesh = take(d.num_tris);          // per-triangle tables: only where every triangle is a kernel-argument primitive
        sc.lt_meshbsdf = take(d.num_meshes); sc.lt_meshemitter = take(d.num_meshes);
        sc.lt_bsdf = take(std::max(d.num_bsdfs, 1) * PSDR_BSDF_STRIDE);
        sc.lt_emf = take(d.num_emitters * PSDR_EMITTER_F_STRIDE); sc.lt_emi = take(d.num_emitters * PSDR_EMITTER_I_STRIDE);
        sc.lt_fcmf = take(sc.lt_nfaces); sc.lt_fpmf = take(sc.lt_nfaces);
        if (d.num_emitters > 1 && d.emitter_cmf && d.emitter_pmf) { sc.lt_ecmf = take(d.num_emitters); sc.lt_epmf = take(d.num_emitters); }
        if (all_tables && d.tri_uv) sc.lt_uv = take(d.num_tris * PSDR_TRIUV_STRIDE);
        if (d.num_texels > 0 && d.num_texels <= kLdsTexels) sc.lt_tex = take(d.num_texels * (1 + kLdsTexelTangents));      // value pool + up to 3 tangent pools (forward mode)
        if (all_tables && h->have_occ && h->d_occ != nullptr) { sc.occ = h->d_occ; sc.lt_occ = take(d.num_tris * d.num_tris); }   // occluder rows of the light rays (<= 32 x 32 words)
    }
    sc.lt_end = off;
    cx.off_stack = off;
    return off + stack_bytes;
}
inline int lds_bytes(const LaunchCtx &cx, const psdr_scene_s *h) { return cx.off_stack + stack_entries_of(h) * kBlock * 4; }
// The context of a kernel that walks no tree (final passes behind the dense trace kernel, bounce stages of the traced wavefront, the adjoint kernel of a
// split reverse launch): nothing of the tree staged, no stacks -- only what plan_lds places without any room (the hit rows of the kernel-argument
// primitives and the small tables of the two-level / tiny instances, Tab<FL>::lds_small).  Its dynamic LDS ends at cx.off_stack.  Returns what the same
// block with the stacks behind it would take.
inline int plan_lds_no_walk(const psdr_scene_s *h, LaunchCtx &cx) {
    const int with_stacks = plan_lds(h, cx, 1 << 30);
    cx.sc.n_lnodes = cx.sc.n_lbtris = cx.sc.n_ltri = 0;
    return with_stacks;
}

// Strategy choice: a PURE FUNCTION of the scene and the options (round 3; it used to follow the survival ratio the previous PathTracer
// call on the handle had measured, so the same call could run either strategy depending on the call history -- and the two agree only
// to the rounding of separately compiled fp32 kernels, up to 1e-3 on a low-spp GGX scene where one firefly sample flips).
// Measured on MI355X (tools/perf_cases.py): in a closed room almost every path survives every bounce, compaction buys nothing and the
// fused kernel is 1.1-1.9x ahead; in an open scene (bunny_light: 2.5 of 7 possible rays per path) the wavefront is 1.35-1.5x ahead.
// "Room" = what psdr_bvh_build recognised as one: all primitives in the kernel arguments (the Cornell box) or a two-level tree (>= 6 inline
// wall triangles around the meshes); everything else (objects under a light, height fields, environment-lit scenes) counts as open.
inline bool open_scene(const psdr_scene_s *h) { return !(h->n_blas > 0 || (h->n_tiny > 0 && h->n_blas == 0)); }
// traced wavefront (psdr_hip.hip k_wf_trace): the scene has a two-level tree whose 4-wide forest is on the device
inline bool traced_wavefront(const psdr_scene_s *h) { return h->traced_enabled && h->n_blas > 0 && h->num_nodes4 > 0 && h->d_nodes4 != nullptr; }
inline bool use_wavefront(const psdr_scene_s *h, const psdr_render_opts *o) {
    if (o->integrator != PSDR_INTEGRATOR_PATH || o->max_depth > 250) return false;
    if (h->desc.num_tris >= (1 << 29)) return false;                // a stream record keeps its triangle in 29 bits (psdr_kernels.h kWfTriMask)
    if (o->flags & PSDR_FLAG_FUSED) return false;
    if (o->flags & PSDR_FLAG_WAVEFRONT) return true;
    if (o->max_depth < 2) return false;
    if (open_scene(h)) return true;                                 // most paths die early, compaction pays
    const long long n = (long long) h->desc.width * h->desc.height * (o->spp_end - o->spp_begin);
    // two-level scene (a room with objects): the TRACED wavefront -- in the fused kernel a wave pays the slowest lane's tree walk at every
    // closest_hit although only a fifth of the rays enter a tree; with the walks in the dense trace kernel between the stages C4's shard takes
    // 18.2 ms against 25.8 fused (21.8 class-binned), the 50 k-triangle interior 2.8 against 4.6, cbox_bunny at 4 M slots 1.6 against 2.1
    // (profiles/r04_traced_first.txt); below 2^16 slots the seven launches cost more than the walks
    if (traced_wavefront(h)) return n >= (1ll << 16);
    // without the trace kernel (PSDR_WF_TRACED=0): the class-binned streams (psdr_kernels.h) are ahead of the fused kernel on large launches only --
    // C4 shard (67 M slots) 27.5 against 29.6 ms; at 4 M slots their extra launches and stream traffic cost more than they save (3.7 against 2.9 ms)
    return h->n_blas > 0 && h->wf_binned && n >= (1ll << 25);
}

inline SinkLayout make_sink_layout(const psdr_scene_s *h, const psdr_grads *g) {
    SinkLayout L{};
    int off = 0;
    L.cam_off = off; off += 16;
    if (g->g_env_f && h->desc.env_emitter >= 0) { L.env_off = off; L.env_n = PSDR_ENV_WORDS; off += PSDR_ENV_WORDS; }
    const int nt = h->desc.num_texels, nr = h->desc.num_emitters * 3;
    if (g->g_texels && nt > 0 && nt <= 2048) { L.tex_off = off; L.tex_n = nt; off += nt; }
    if (g->g_emitter_rad && nr > 0 && nr <= 256) { L.rad_off = off; L.rad_n = nr; off += nr; }
    if (g->g_tri_info && h->hot_rows > 0) {
        const int rows = std::min(h->hot_rows, (kSinkCacheWords - off) / PSDR_TRI_STRIDE);
        // slots >= rows (cache too small for all of them) fall back to global atomics in add_tri
        if (rows > 0) { L.hot_off = off; L.hot_rows = rows; L.hot_map = h->d_hot_map; L.hot_tris = h->d_hot_tris; off += rows * PSDR_TRI_STRIDE; }
    }
    L.total = off;
    L.stride = off | 1;
    L.rep = 1;
    // 2 copies bought 6 % on C2, more nothing: 4 at most, so that a small scene's cache stays a few KB of LDS
    const int max_rep = h->opt.sink_rep;
    while (L.rep * 2 <= max_rep && L.rep * 2 * L.stride <= kSinkCacheWords) L.rep *= 2;
    // lane-private rows: the leading hot slots are emitter 0's triangles (build_bvh)
    const bool priv_on = h->opt.sink_private != 0;
    L.priv_tri[0] = L.priv_tri[1] = -1; L.priv_slot[0] = L.priv_slot[1] = 0; L.priv_emitter = -1;
    if (priv_on && L.hot_rows > 0 && h->desc.num_emitters > 0 && h->desc.env_emitter != 0) {
        const int32_t *ei = h->emitter_i.data();
        const int n = std::min(std::min(ei[2], 2), L.hot_rows);
        for (int r = 0; r < n; ++r) { L.priv_tri[r] = ei[1] + r; L.priv_slot[r] = h->hot_identity ? ei[1] + r : r; }
        L.priv_rows = n;
        if (n > 0) { L.priv_off = (L.rep * L.stride + 3) / 4 * 4; if (L.rad_n) L.priv_emitter = 0; }
    }
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- grids and chunks
// Grid of the forward camera kernels: finer workgroups balance image regions of different cost better (C2 +4.5 %,
// C4 PathTracer(3) shard 37.4 -> 34.2 ms at 40 per CU instead of 16), but every workgroup stages its share of the
// scene in LDS first: on a 4 M-slot launch of an open scene (bunny_light) 40 per CU is 9-15 % SLOWER.  So: 40 when
// nothing is staged (tiny scene) or when a workgroup still makes >= 8 trips of its grid-stride loop, else 16.
inline int camera_blocks_per_cu(const psdr_scene_s *h, long long n) {
    if (h->opt.camera_blocks > 0) return h->opt.camera_blocks;          // experiments (psdr_scene_set_option)
    if (h->has_rough) return 16;
    if (h->n_tiny > 0 && h->n_blas == 0) return 40;
    // tree scenes (lean variants): pixels on a mesh cost several times a wall pixel and neighbouring pixels share a workgroup, so the hardware's
    // workgroup scheduler balances the launch better the finer the grid -- two slots per thread, 16..64 workgroups per CU (cbox_bunny 256^2 spp 64:
    // PathTracer(3) 2.51 -> 2.37 ms, (6) 4.17 -> 3.90 against 16; the C4 shard's fused launch 25.8 -> 24.8 against 40)
    const long long fit = n / ((long long) kBlock * h->num_cus * 2);
    return (int) std::max(16LL, std::min(64LL, fit));
}
// workgroups per CU of the large launches that measured faster on a finer grid (traced wavefront stages, primary-edge reverse kernel, secondary-edge filter of a
// two-level scene): 16, up to 40 where a workgroup still makes >= 8 trips of its grid-stride loop (profiles/r04_wf_grid_abk.txt)
inline int big_launch_per_cu(const psdr_scene_s *h, long long n) { return (int) std::max(16LL, std::min(40LL, n / ((long long) kBlock * h->num_cus * 8))); }
// slots per chunk of the launches that keep per-slot state between kernels (wavefront streams, reverse-mode records, probe buffers): 2^log2_default,
// or what psdr_scene_set_option("chunk_log2", ...) says (tests: chunk boundaries on small scenes)
inline long long launch_chunk(const psdr_scene_s *h, int log2_default) { return 1ll << (h->opt.chunk_log2 > 0 ? h->opt.chunk_log2 : log2_default); }
// DirectIntegrator(1, 1) camera launches on a two-level scene run as probe pass + dense trace kernel + final pass (from 2^16 slots)
inline bool probe_direct(const psdr_scene_s *h, const psdr_render_opts *o, long long n) {
    return traced_wavefront(h) && h->opt.probe != 0 && o->bsdf_samples == 1 && o->light_samples == 1 && !(o->flags & PSDR_FLAG_FUSED) && n >= (1ll << 16);
}
// A camera kernel STORES a pixel instead of adding to it with atomics (the kernels' `own`) when every sample of the pixel sits in one wave of one launch:
// the pixel's samples are nsp consecutive slots, a wave holds 64, and a chunked launch starts each chunk at a multiple of `chunk` -- which must fall on a
// pixel boundary, or a chunk stores its partial sums over the previous chunk's (option chunk_log2 below log2(nsp)).  Callers whose launch is
// not chunked pass its slot count n.  The caller has zeroed img and dimg in the same call: a stored pixel and an added one start from the same image.
inline bool wave_owns_pixels(const psdr_scene_s *h, int nsp, long long chunk) {
    return h->opt.own_pixels != 0 && nsp <= 64 && 64 % nsp == 0 && chunk % nsp == 0;
}
// ---- the lean PathTracer twins of flag set 8 (psdr_path_lean.h): which kernel a fused PathTracer camera launch on a scene without a tree runs.
// kPathLeanNone: the kernels of before the twins -- k_camera / k_camera_seeded (K = 0), k_camera_logd_lean or k_camera_logd (K >= 1, logd_lean_launch_8).
// kPathLeanOwnSlab: k_camera_path_lean (K = 0) / k_camera_logd_path_lean<K>.  The twins exist in ONE form, "every wave on one pixel, every row a slab-form rectangle": a general form of them beside
// the kernels that already serve every other launch would only add four kernels to the library.
enum PathLeanForm { kPathLeanNone = 0, kPathLeanOwnSlab = 1 };
// parking columns of the twin per K (psdr_path_lean.h LeanLayout<K>::cols; 0: the twin holds everything in registers).  K = 0 has none: without columns the
// renderC twin takes 77 / 79 VGPRs and spills nothing (profiles/path_lean_ab.txt, the compile-only table); PSDR_PATH_LEAN_PARK_K0=1 builds it with columns (A/B)
#ifndef PSDR_PATH_LEAN_PARK_K0
#define PSDR_PATH_LEAN_PARK_K0 0
#endif
constexpr int path_lean_cols(int K) { return (K == 0 && !PSDR_PATH_LEAN_PARK_K0) ? 0 : 16 + 6 * K; }
constexpr int kPathLeanWaves = 6;          // the twins' waves per SIMD = workgroups per CU that keep their LDS blocks side by side
// what the rule reads: of the launch, of the scene, of the options
struct PathLeanCase {
    int flags, K, integrator, texels_only;          // flag set of the scene's kernels; tangent sets; PSDR_INTEGRATOR_*; K >= 1: every tangent set moves albedo texels only (the log-derivative launch)
    int nsp; long long chunk;                       // samples per pixel of the launch; its slots (or the slots per chunk of a chunked one)
    int n_tiny, aa_cnt, n_blas;                     // rows of kernel-argument primitives, slab-form slots per axis, trees
    int lds_scene, lds_budget;                      // staged scene in bytes (16-byte aligned); forced budget (0: none)
    int own_pixels, path_lean, logd_park;           // options
};
// every wave of the launch sits on ONE pixel and no wave is partial: wave_owns_pixels with exactly a wave's samples per pixel (fewer: a wave holds several
// pixels; more: a pixel's samples sit in several waves and the launch adds with atomics)
inline bool wave_is_pixel(int own_pixels, int nsp, long long chunk) { return own_pixels != 0 && nsp == 64 && chunk % nsp == 0; }
// every kernel-argument primitive is a slab-form rectangle: the plane-form rows, which start at kAaSlots, are none
inline bool slab_only(int n_tiny, int aa_cnt, int n_blas) { return n_blas == 0 && aa_cnt != 0 && n_tiny > 0 && n_tiny <= kAaSlots; }
inline int path_lean_form(const PathLeanCase &c) {
    if (c.path_lean == 0 || c.flags != kSceneTiny || c.integrator != PSDR_INTEGRATOR_PATH) return kPathLeanNone;
    if (!(c.K == 0 || (c.K == 1 && c.texels_only != 0 && c.logd_park != 0))) return kPathLeanNone;          // K = 3 keeps k_camera_logd
    if (!wave_is_pixel(c.own_pixels, c.nsp, c.chunk) || !slab_only(c.n_tiny, c.aa_cnt, c.n_blas)) return kPathLeanNone;
    constexpr int kCuLds = 160 * 1024;
    const int limit = c.lds_budget > 0 ? std::min(c.lds_budget, kCuLds / kPathLeanWaves) : kCuLds / kPathLeanWaves;
    const int park = path_lean_cols(c.K) * kBlock * 4;
    if (park > 0 && c.lds_scene + park > limit) return kPathLeanNone;
    return kPathLeanOwnSlab;
}
inline int path_lean_form(const psdr_scene_s *h, int flags, int K, int integrator, bool texels_only, int nsp, long long chunk, int lds_scene) {
    const PathLeanCase c{flags, K, integrator, texels_only ? 1 : 0, nsp, chunk, h->n_tiny, h->aa_cnt, h->n_blas, lds_scene, h->opt.lds_budget, h->opt.own_pixels, h->opt.path_lean, h->opt.logd_park};
    return path_lean_form(c);
}
// The secondary-edge term as filter + survivor kernel (option sedge_split: 1 / 0 force, -1 from 2^18 slots); a survivor list holds 32-bit slots
inline bool path_sedge_split(const psdr_scene_s *h, long long n) {
    const int split_env = h->opt.sedge_split;
    return !(split_env == 0 || (split_env < 0 && n < (1ll << 18))) && n <= 0x7fffffffLL;
}
// Grid of a kernel that walks the survivor list of a filter pass over n slots: sized for n / divisor survivors (16 behind the filter of segment A, 4 behind
// segment B's), 2^16 at least
inline long long filter_grid_slots(long long n, int divisor) { return std::max(n / divisor, 1ll << 16); }
// Copies of the primary-edge gradient table (psdr_kernels.h PrimaryEdgeSink): up to 64 within 64 MB, from 2^18 slots
inline int primary_edge_replicas(long long pe_words, long long n) {
    int reps = 1;
    while (reps < 64 && (long long) (reps * 2) * pe_words * 4 <= (64ll << 20)) reps *= 2;
    return n < (1ll << 18) ? 1 : reps;
}

// ---------------------------------------------------------------------------------------------------------------- reverse launches
inline bool same_camera_samples(const psdr_render_opts &a, const psdr_render_opts &b) {
    return a.integrator == b.integrator && a.max_depth == b.max_depth && a.hide_emitters == b.hide_emitters && a.spp == b.spp && a.spp_begin == b.spp_begin &&
           a.spp_end == b.spp_end && a.rng_offset[0] == b.rng_offset[0] && ((a.flags ^ b.flags) & (PSDR_FLAG_FUSED | PSDR_FLAG_WAVEFRONT)) == 0;
}
// words per record of a split reverse launch (2 + 5 depth; 2 + 8 depth from the wavefront's value sweep)
inline int rev_record_words(int depth, bool wavefront) { return kRevDiskHead + (wavefront ? kRevDiskPerVertexCf : kRevDiskPerVertex) * depth; }
// Does a reverse camera launch with geometry gradients over n slots run as value kernel + adjoint kernel?  A scene with a tree to walk, hits replayable.
inline bool rev_launch_splits(const psdr_scene_s *h, const psdr_render_opts *o, long long n) {
    const int split_env = h->opt.rev_split;
    const bool replayable = o->integrator == PSDR_INTEGRATOR_PATH || (o->integrator == PSDR_INTEGRATOR_DIRECT && o->bsdf_samples <= 1 && o->light_samples <= 1);
    const bool has_tree = h->num_nodes > 0 && (h->n_tiny == 0 || h->n_blas > 0);
    // measured (tools/rev_split_probe.py, 4 M slots): PathTracer(3) cbox_bunny 6.8 -> 4.8 ms, bunny_light 5.6 -> 3.9, 50 k-triangle interior
    // 11.4 -> 9.4, PathTracer(6) 21 -> 12 / 13 -> 7.3 / 36 -> 20; the DirectIntegrator (three rays per slot) only gains on the
    // large tree (3.8 -> 3.3 ms; bunny scenes 2.0 -> 2.4); the 12-triangle box neither way
    const bool worth = o->integrator == PSDR_INTEGRATOR_PATH ? o->max_depth >= 2 : h->num_nodes >= 16384;
    return replayable && split_env != 0 && (split_env == 1 || (has_tree && worth && n >= (1ll << 20)));
}
// the value sweep of a split PathTracer launch on a two-level scene runs as the TRACED WAVEFRONT (dense trace kernel between the stages):
// in the fused value kernel a wave pays its slowest lane's tree walk at every closest_hit (C4 shard: 29 ms of the 57; renderC by the
// wavefront: 16 ms)
inline bool rev_wavefront_sweep(const psdr_scene_s *h, const psdr_render_opts *o) {
    return o->integrator == PSDR_INTEGRATOR_PATH && std::min(o->max_depth, kMaxRevDepthDeep) <= kMaxRevDepth && traced_wavefront(h) && use_wavefront(h, o);
}
// Does the reverse launch of these camera slots with geometry gradients run its value sweep as the traced wavefront with recording stages
// (plan_rev_camera: wf_value)?  Then psdr_render_c(PSDR_FLAG_KEEP_RECORDS) can BE that value sweep.  (`geo` and the option rev_split == 1 on a
// scene without a tree are the caller's side of it.)
inline bool rev_value_sweep_is_wavefront(const psdr_scene_s *h, const psdr_render_opts *o, long long n) { return rev_launch_splits(h, o, n) && rev_wavefront_sweep(h, o); }

// psdr_scene_rev_layout: the words that describe the gradient cache of a reverse launch ([8]: the camera launch form, [9] and [15]: the primary-edge launch)
inline void rev_layout_of_sink(psdr_scene_s *h, const SinkLayout &L, bool deep_rec) {
    int32_t *r = h->rev_layout;
    r[0] = L.tex_n; r[1] = L.rad_n; r[2] = L.env_n; r[3] = L.hot_rows; r[4] = L.rep;
    r[5] = L.priv_rows; r[6] = L.priv_regs; r[7] = L.pend_rows;
    r[10] = h->hot_identity ? 1 : 0; r[11] = deep_rec ? 1 : 0; r[12] = L.priv_slot[0]; r[13] = L.priv_slot[1]; r[14] = h->hot_rows;
}

// LDS plan of a reverse kernel that meets ONE vertex per slot (the secondary-edge kernels of both integrators, the CollocatedIntegrator's camera kernel):
// [ staged scene | stacks | gradient cache ].  No private emitter rows (a slot lands on the emitter once at most), nothing deferred.  cx: the launch's
// context (make_ctx), replanned with the cache's bytes reserved; *dyn_bytes: the kernel's dynamic LDS.
inline int plan_rev_one_vertex(const psdr_scene_s *h, LaunchCtx &cx, SinkLayout &L, int *dyn_bytes) {
    L.priv_rows = 0; L.priv_emitter = -1; L.priv_regs = 0;
    L.pend_rows = 0; L.pend_off = 0;
    const int cache_bytes = sink_bytes(L);
    plan_lds(h, cx, cache_bytes);
    cx.off_sink = lds_bytes(cx, h);
    *dyn_bytes = cx.off_sink + cache_bytes;
    if (*dyn_bytes > h->lds_limit) return fail("psdr_render_d_rev: the launch needs " + std::to_string(*dyn_bytes) + " bytes of LDS per workgroup (traversal stacks + gradient cache), the device offers " +
                                               std::to_string(h->lds_limit));
    return 0;
}

// LDS plan of the reverse CAMERA launch (psdr_kernels.h render_rev_impl).  In: what the call asks for; out: the launch form, the final gradient-cache
// layout L, the two contexts and their byte counts:
//   cx   [ staged scene | stacks | path record | cache ]   the fused kernel (dyn_bytes), the value kernel of a split launch (dyn1: up to the record's end)
//   cx2  [ hit rows, small tables | path record | cache ]  the kernels that walk no tree (plan_lds_no_walk): the adjoint kernel of a split launch and the
//                                                           final pass of a probe launch (dyn_bytes)
// fl: the flag set of the kernels; reg_priv: its PathTracer geometry-adjoint kernels keep the lane-private emitter accumulators in registers (psdr_kernels.h
// reg_priv_kernel); value_only: psdr_render_c as the value kernel of a split launch
enum RevCameraForm { kRevFused = 0, kRevSplit = 1, kRevSplitWavefront = 2, kRevKeptRecords = 3, kRevProbe = 4 };          // rev_layout[8]
struct RevCameraPlan {
    int form, depth, rec_bytes, cache_bytes, dyn1, dyn_bytes;
    bool geo, deep_rec, split, kept_fused, no_tree;
};
inline int plan_rev_camera(psdr_scene_s *h, const psdr_render_opts *o, const psdr_grads *grads, long long n, int fl, bool reg_priv, bool value_only, bool has_out_img,
                           SinkLayout &L, LaunchCtx &cx, LaunchCtx &cx2, RevCameraPlan &p) {
    p.depth = o->integrator == PSDR_INTEGRATOR_PATH ? std::min(o->max_depth, kMaxRevDepthDeep) : 1;
    // up to kMaxRevDepth vertices the per-lane path record lives in LDS; deeper paths keep it in HBM, one column per thread of the grid
    p.deep_rec = p.depth > kMaxRevDepth;
    p.rec_bytes = p.deep_rec ? 0 : p.depth * kPathRecWords * kBlock * 4;
    p.geo = value_only || grads->g_tri_info != nullptr || grads->g_cam_to_world != nullptr;
    const int wg_per_cu = (o->integrator == PSDR_INTEGRATOR_DIRECT && !(fl & kSceneRough)) ? 3 : 2;       // rev_waves<FL, true, INTEG>
    // the records a recording psdr_render_c (value_only) left of exactly these samples on exactly these tables: this call is their adjoint kernel
    p.kept_fused = !value_only && p.geo && o->integrator == PSDR_INTEGRATOR_PATH && !p.deep_rec && h->opt.rev_split != 0 && h->kept.valid && h->kept.kind == 0 &&
                   h->kept.gen == h->tables_gen && h->kept.n == n && !has_out_img && same_camera_samples(h->kept.o, *o) && n <= launch_chunk(h, 26);
    p.split = value_only || p.kept_fused || (p.geo && rev_launch_splits(h, o, n));
    // the PathTracer's geometry-adjoint kernels keep the lane-private emitter accumulators in registers (RegPrivSink): no LDS block, never switched off
    L.priv_regs = (p.geo && o->integrator == PSDR_INTEGRATOR_PATH && reg_priv) ? 1 : 0;
    cx2 = cx;
    const int stacks_only = plan_lds_no_walk(h, cx2);
    const int base2 = cx2.off_stack;                           // bytes in front of where the stacks would start
    const int floor_bytes = (p.split ? base2 : stacks_only) + p.rec_bytes;                  // (tables +) stacks only + record
    // lane-private emitter rows (30 KB) only where they do not cost a resident workgroup (C5 PathTracer(3) fused: stacks 22 KB +
    // record 24 KB + cache 19 KB + 30 KB = one workgroup per CU instead of two, 11.5 -> 19.4 ms)
    if (!L.priv_regs && L.priv_rows > 0 && floor_bytes + sink_bytes(L) > h->lds_limit / wg_per_cu) { L.priv_rows = 0; L.priv_emitter = -1; }
    // deferred row adjoints (DeviceSink::defer_row -> sorted adds at the slot's end): one column per path vertex behind the primary one, where the
    // block does not cost a resident workgroup
    L.pend_rows = 0; L.pend_off = 0;
    // (rows: measured on the PathTracer only -- C2 all gradients 5.28 -> 4.99 ms, the C4 shard's adjoint kernel 19.5 -> 18.7; the DirectIntegrator's
    // single deferred row is level to 3 % slower: profiles/r05_rev_sorted_abk.txt)
    if (p.geo && h->opt.rev_sorted != 0 && grads->g_tri_info != nullptr && o->integrator == PSDR_INTEGRATOR_PATH) {
        for (int rows = std::min(p.depth, 4); rows >= 1; --rows) {
            SinkLayout t = L;
            sink_reserve_pending(t, rows);
            if (floor_bytes + sink_bytes(t) <= h->lds_limit / wg_per_cu) { L = t; break; }
        }
    }
    p.cache_bytes = sink_bytes(L);
    rev_layout_of_sink(h, L, p.deep_rec);
    plan_lds(h, cx, p.split ? p.rec_bytes : p.rec_bytes + p.cache_bytes);   // stage less of the scene: the record (+ cache) live in LDS too
    cx.off_pathrec = lds_bytes(cx, h);
    cx.off_sink = cx.off_pathrec + p.rec_bytes;
    cx2.off_pathrec = base2; cx2.off_sink = base2 + p.rec_bytes;
    // a scene without a tree runs both kernels of a (forced) split launch on the layout of the fused one
    p.no_tree = lds_bytes(cx, h) == cx.off_stack;
    if (p.split && p.no_tree) cx2 = cx;
    p.dyn1 = cx.off_pathrec + p.rec_bytes;
    p.dyn_bytes = (p.split ? cx2.off_sink : cx.off_sink) + p.cache_bytes;
    if (std::max(p.dyn_bytes, p.split ? p.dyn1 : 0) > h->lds_limit) return fail("psdr_render_d_rev: the launch needs " + std::to_string(p.dyn_bytes) + " bytes of LDS per workgroup (path record of " +
                                              std::to_string(p.depth) + " levels + traversal stacks + gradient cache), the device offers " + std::to_string(h->lds_limit));
    const bool forest = (fl & kSceneForest) != 0;
    const bool wf_value = forest && p.split && !value_only && !p.kept_fused && !p.no_tree && rev_wavefront_sweep(h, o);
    // DirectIntegrator(1, 1), one kernel, on a two-level scene: probe pass -> dense trace kernel -> the reverse kernel on primitives + hit rows
    const bool direct_probe = forest && !p.split && !p.no_tree && o->integrator == PSDR_INTEGRATOR_DIRECT && probe_direct(h, o, n);
    p.form = p.split ? (wf_value ? kRevSplitWavefront : kRevSplit) : direct_probe ? kRevProbe : kRevFused;
    if (direct_probe) p.dyn_bytes = cx2.off_sink + p.cache_bytes;
    h->rev_layout[8] = p.form;
    return 0;
}
}  // namespace psdr_host
