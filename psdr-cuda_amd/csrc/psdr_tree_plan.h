// psdr_tree_plan.h -- tree build and trace planning: every decision psdr_bvh_build takes (refit or build, where, which tree, the hot rows of the gradient cache,
// what the refit path keeps) and the two launch rules of the dense trace kernel and its request buffers, stated once.  Pure host code like psdr_plan.h, included
// behind it at the end of psdr_host.h: inline functions that make no HIP call, so that tests/hostcheck/hostcheck_plan.cpp runs them on hand-filled handles where
// no GPU exists.  psdr_hip.hip decides here and acts there.
#pragma once

namespace psdr_host {
// ---------------------------------------------------------------------------------------------------------------- emitter triangles, hot rows, occluder rows
// emitters whose record the handle's host copy of emitter_i holds (psdr_bvh_build refreshes it at every build)
inline int emitters_on_host(const std::vector<int32_t> &emitter_i, int num_emitters) {
    return (int) std::min<size_t>((size_t) std::max(num_emitters, 0), emitter_i.size() / PSDR_EMITTER_I_STRIDE);
}
// [T] 1 = the triangle belongs to an emitter mesh (faces outside the table are dropped)
inline std::vector<char> emitter_triangle_mask(const std::vector<int32_t> &emitter_i, int num_emitters, int T) {
    std::vector<char> is_em((size_t) std::max(T, 0), 0);
    for (int e = 0; e < emitters_on_host(emitter_i, num_emitters); ++e) {
        const int32_t *ei = emitter_i.data() + (size_t) e * PSDR_EMITTER_I_STRIDE;
        for (int f = 0; f < ei[2]; ++f) if (ei[1] + f >= 0 && ei[1] + f < T) is_em[(size_t) (ei[1] + f)] = 1;
    }
    return is_em;
}
// under an environment map every direction meets an emitter: no emitter rows to pre-test (SceneView::emit_rows = 0)
inline bool emit_rows_wanted(const psdr_scene_s *h) {
    return !(h->desc.env_emitter >= 0 && h->desc.env_emitter < emitters_on_host(h->emitter_i, h->desc.num_emitters));
}

// Hot rows of the reverse-mode gradient cache, slot -> triangle: emitter triangles first (the first 64 faces of each emitter: every light sample lands on
// them), then `by_area`, the triangles by decreasing area (walls, floors: the rows most path vertices land on) -- no triangle twice, none outside the table,
// kMaxHotRows at most.  A scene whose triangles travel in the kernel arguments (`tiny`) caches EVERY row, slot = triangle: its kernels (flag kSceneTiny) address
// the row without the map, the range test and the global-atomic arm (DeviceSink::add_tri).  Each build path brings its own by_area (std::partial_sort on the
// host, the radix sort of the area keys on the device: they break ties differently).
constexpr int kMaxHotRows = 200;
inline std::vector<int32_t> hot_row_list(int T, bool tiny, const std::vector<int32_t> &emitter_i, int num_emitters, const int32_t *by_area, int n_by_area) {
    std::vector<int32_t> tris;
    std::vector<char> taken((size_t) std::max(T, 0), 0);
    auto add = [&](int t) { if (t >= 0 && t < T && !taken[(size_t) t] && (int) tris.size() < kMaxHotRows) { taken[(size_t) t] = 1; tris.push_back(t); } };
    if (tiny) for (int t = 0; t < T; ++t) add(t);
    for (int e = 0; e < emitters_on_host(emitter_i, num_emitters); ++e) {
        const int32_t *ei = emitter_i.data() + (size_t) e * PSDR_EMITTER_I_STRIDE;
        for (int f = 0; f < ei[2] && f < 64; ++f) add(ei[1] + f);
    }
    for (int i = 0; i < n_by_area; ++i) add(by_area[i]);
    return tris;
}

// the most rows any (triangle, emitter triangle) entry of the occluder rows names (psdr_scene_info); occ: [T x T] row masks, n_tiny <= kTinyRows rows in use
inline int occluder_max_rows(const std::vector<uint32_t> &occ, const std::vector<char> &is_em, int T, int n_tiny) {
    int most = 0;
    for (int r = 0; r < T; ++r) for (int e = 0; e < T; ++e) if (is_em[(size_t) e]) most = std::max(most, (int) __builtin_popcount(occ[(size_t) r * T + e] & ((1u << n_tiny) - 1u)));
    return most;
}

// ---------------------------------------------------------------------------------------------------------------- what the refit path needs
// summed surface measure of a node's box (the union of its two child boxes): the reference the refits compare against (kRefitAreaGrowth)
inline double node_area(const BvhNode &n) {
    const float dx = std::max(n.hi0[0], n.hi1[0]) - std::min(n.lo0[0], n.lo1[0]), dy = std::max(n.hi0[1], n.hi1[1]) - std::min(n.lo0[1], n.lo1[1]),
                dz = std::max(n.hi0[2], n.hi1[2]) - std::min(n.lo0[2], n.lo1[2]);
    return (double) (dx * dy + dy * dz + dz * dx);
}
// The levels of the breadth-first node order of ONE tree (first node of every level + the end: k_refit_level runs level by level, bottom up) and the summed box
// area.  root < 0: the tree is a single leaf -- no nodes, no levels, area 0.
inline double tree_levels_and_area(const std::vector<BvhNode> &nodes, int32_t root, std::vector<int> &level_start) {
    level_start.clear();
    double area = 0.0;
    if (root < 0) return area;
    std::vector<int> depth(nodes.size(), 0);
    for (size_t i = 0; i < nodes.size(); ++i) {
        const BvhNode &n = nodes[i];
        if (n.c0 >= 0) depth[(size_t) n.c0] = depth[i] + 1;
        if (n.c1 >= 0) depth[(size_t) n.c1] = depth[i] + 1;
        if (i == 0 || depth[i] != depth[i - 1]) level_start.push_back((int) i);
        area += node_area(n);
    }
    level_start.push_back((int) nodes.size());
    return area;
}

// ---------------------------------------------------------------------------------------------------------------- refit or build
// the triangles travel in the kernel arguments (no tree is walked): host copy needed, never refitted, never built on the device
inline bool tiny_scene(const psdr_scene_s *h, int T) { return h->tiny_enabled && T <= kTinyTris; }
// Refit: same triangle count as the tree on the device ...
inline bool refit_candidate(const psdr_scene_s *h, int T, bool tiny) { return h->refit_enabled && !tiny && h->refit_ok && h->tree_tris == T && h->num_nodes > 0; }
// ... and the tree has not degraded: the emitter layout is the one the tree was built under (the host copy of emitter_i -- LDS table sizes, two-level
// eligibility, hot gradient rows -- is refreshed by the build paths only: with a changed layout the kernels would stage too few entries of face_cmf /
// face_pmf), a two-level tree's kernels can still stage the tables (else: rebuild as one tree), a full rebuild at least every kMaxRefits refits or when the
// summed inner-box area grew by kRefitAreaGrowth.  prev_area: what the previous refit summed (h->built_area before the first).
enum RefitKind { kRefitNone = 0, kRefitDeviceTree = 1, kRefitHostTree = 2 };          // device-built tree: lbvh_refit; host-built tree: k_refit_level, level by level
inline RefitKind refit_choice(const psdr_scene_s *h, bool emitters_same, bool forest_stands, float prev_area) {
    if (!emitters_same || !forest_stands || h->refits_since_build >= kMaxRefits) return kRefitNone;
    if (!(prev_area <= kRefitAreaGrowth * h->built_area)) return kRefitNone;
    return h->lbvh ? kRefitDeviceTree : kRefitHostTree;
}
inline bool forest_stands(const psdr_scene_s *h) { return !(forest_tables(h) && !small_tables_fit(h)); }
// moved wall vertices may no longer pair into parallelograms: more than kTinyTris inline primitives after a refit -> full rebuild (which then picks a single tree)
inline bool refit_inline_fits(int n_prims) { return n_prims <= kTinyTris; }

// build on the device: large tables (the host build is a D2H of the table + a single-threaded SAH build), or on request (option bvh_build 1 / 0 / -1)
inline bool device_build_wanted(const psdr_scene_s *h, int T, bool tiny) { return !tiny && (h->bvh_device_mode == 1 || (h->bvh_device_mode < 0 && T >= kLbvhAutoTris)); }
// which tree: two-level (a few small meshes + a few large ones, ForestBuilder::eligible) or one tree over everything; never under an environment map
inline bool forest_candidate(const psdr_scene_s *h, int T) {
    return h->two_level_enabled && h->tiny_enabled && T > kTinyTris && h->desc.num_meshes > 0 && h->desc.env_emitter < 0;
}
// too many inline primitives (after pairing): one tree.  Fewer inline triangles than forest_min_inline: nothing room-like to keep out of the trees (default 0
// since round 6; 6 = only rooms, walls around objects)
inline bool forest_kept(const psdr_scene_s *h, int n_top_prims, int n_inline_tris) { return n_top_prims <= kTinyTris && n_inline_tris >= h->forest_min_inline; }

// ---------------------------------------------------------------------------------------------------------------- dense trace kernel
// the tree boxes as they travel in the kernel arguments (SceneView, TraceArgs): lo.w = root of the tree, hi.w = its root in the 4-wide node array
inline void pack_blas_boxes(const psdr_scene_s *h, float4 *lo, float4 *hi) {
    std::memcpy(lo, h->blas_lo, sizeof(h->blas_lo));
    std::memcpy(hi, h->blas_hi, sizeof(h->blas_hi));
    for (int k = 0; k < h->n_blas; ++k) std::memcpy(&hi[k].w, &h->blas_root4[k], 4);
}
// LDS of k_wf_trace: stacks first in the budget (S + 1 columns: the unconditional stores of a node step may touch the entry above the top), the tree in the rest.
// TWO workgroups per CU (8 waves per SIMD, <= 64 VGPRs), each with half of the LDS -- stack columns of 8 entries (deeper ones, rare, in the
// overflow columns), fewer staged nodes -- where the walk gains more from the second set of waves than it loses to the smaller staging:
// a forest that does not fit the LDS anyway (C5: trace stage 326 -> 307 us) or a large launch (C4 shard: 754 -> 690 us); the 4 M-slot launch on
// the bunny, whose whole tree fits one workgroup's LDS, is 2.5 % faster with one (profiles/r04_trace_wg2_abk.txt).  Option trace_wg2: -1 this
// rule, 0 never, n > 0 always with columns of n entries.
struct TracePlan {
    bool wg2, ovf;                          // two workgroups per CU; stack entries beyond the LDS columns live in per-lane global columns
    int S, n_lnodes, off_stack, stack_entries, grid, dyn, ovf_stride;
    size_t ovf_bytes;
};
inline TracePlan plan_wf_trace(const psdr_scene_s *h, long long sub_cap) {
    TracePlan p{};
    const int full_S = std::min(h->stack_need4, kTraceStackMax);
    const bool tree_fits = (long long) h->num_nodes4 * kTraceNodeStride + (long long) (full_S + 1) * kTraceBlock * 4 + 1024 <= (long long) h->lds_limit;
    p.wg2 = h->lds_limit >= 160 * 1024 && (h->opt.trace_wg2 > 0 || (h->opt.trace_wg2 < 0 && (!tree_fits || sub_cap * kWfSub >= (1ll << 25))));
    const int budget = (p.wg2 ? h->lds_limit / 2 : h->lds_limit) - 1024;                             // 1 KB: the kernel's static LDS
    p.S = std::min(h->stack_need4, p.wg2 ? std::min(h->opt.trace_wg2 > 0 ? h->opt.trace_wg2 : 8, kTraceStackMax) : kTraceStackMax);
    p.S = std::min(p.S, std::max(0, budget / (kTraceBlock * 4) - 1));          // the columns fit the budget (a device with 64 KB of LDS: 14 entries, the rest overflows)
    p.ovf = h->stack_need4 > p.S;
    const int stack_bytes = (p.S + 1) * kTraceBlock * 4;
    const int room = budget - stack_bytes;
    p.n_lnodes = std::max(0, std::min(h->num_nodes4, room / kTraceNodeStride));
    p.off_stack = p.n_lnodes * kTraceNodeStride;
    p.stack_entries = p.S;
    p.grid = p.wg2 ? 2 * h->num_cus : h->num_cus;
    if (p.ovf) {
        p.ovf_stride = p.grid * kTraceBlock;
        p.ovf_bytes = (size_t) p.ovf_stride * (size_t) (h->stack_need4 - p.S) * sizeof(int32_t);
    }
    p.dyn = p.off_stack + stack_bytes;
    return p;
}

// Probe buffers: the request-queue counters, hit rows [slots * rays_per_slot], one mask word per slot (padded to 256 bytes), the request queue (kWfSub sub-queues,
// every ray can be a request: two rows each); per_cu: workgroups per CU of the probe launch, whose block b appends to queue b % kWfSub
struct ProbePlan { long long sub_cap; size_t cnt_bytes, hit_bytes, mask_bytes, req_bytes, total; };
inline ProbePlan plan_probe_buffers(const psdr_scene_s *h, long long slots, int rays_per_slot, int per_cu) {
    ProbePlan p{};
    const long long blocks = ((long long) launch_blocks(h, slots, per_cu) + kWfSub - 1) / kWfSub * kWfSub;
    const long long trips = (slots + blocks * kBlock - 1) / (blocks * kBlock);
    p.sub_cap = (blocks / kWfSub) * trips * kBlock * rays_per_slot;
    p.cnt_bytes = (size_t) kWfSub * kWfCountStride * sizeof(int32_t);
    p.hit_bytes = (size_t) (slots * rays_per_slot) * sizeof(float4);
    p.mask_bytes = ((size_t) slots * 4 + 255) & ~(size_t) 255;
    p.req_bytes = (size_t) 2 * p.sub_cap * kWfSub * sizeof(float4);
    p.total = p.cnt_bytes + p.hit_bytes + p.mask_bytes + p.req_bytes;
    return p;
}
}  // namespace psdr_host
