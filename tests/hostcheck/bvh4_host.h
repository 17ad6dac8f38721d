// bvh4_host.h -- TEST-ONLY: the product's host tree builders and 4-wide collapse / quantisation behind one call, shared by libhostcheck.so
// (hostcheck_bvh4) and the stand-alone sanitizer program (bvh4_san.cpp).
#pragma once
#include "../../psdr-cuda_amd/csrc/psdr_bvh_build.h"

#include <cstring>
#include <vector>

namespace psdr {
// The host side of the 4-wide tree as psdr_bvh_build runs it (tests/test_bvh4_host.py): Builder (forest = 0) or ForestBuilder (forest = 1; a table
// ForestBuilder::eligible refuses, or one whose inline triangles pair into more than kTinyTris primitives, gets the single tree, as in the library), then
// collapse_bvh4, then quantise_bvh4 per node.  Every output array holds T entries (child / src: 4 T; roots / boxes: num_meshes + 1).
//   sizes = { BVH2 nodes, leaf triangles, roots, 4-wide nodes, stack_need, inline triangles, 1 if a forest was built, BVH2 depth }
// btris: 12 floats per leaf triangle (p0 | id, e1 | -, e2 | -); boxes: tree_box of every root of a forest, (lo, hi) = 6 floats
inline int bvh4_host(const float *rows, const int32_t *tri_mesh, int T, int num_meshes, int max_leaf, int forest, int32_t *sizes, BvhNode *nodes_out,
                     float *btris_out, int32_t *roots2_out, int32_t *roots4_out, int32_t *child_out, int32_t *src_out, Bvh4Node *nodes4_out,
                     int32_t *inline_out, float *boxes_out) {
    Builder b;
    ForestBuilder fb;
    b.kMaxLeaf = fb.max_leaf = max_leaf;
    bool is_forest = forest != 0 && T > kTinyTris && num_meshes > 0 && ForestBuilder::eligible(tri_mesh, T, num_meshes);
    if (is_forest) {
        if (fb.run(rows, tri_mesh, T, num_meshes)) return 1;
        std::vector<float4> top_prims;
        pack_tiny_prims(fb.inline_tris, top_prims);
        if ((int) top_prims.size() / 3 > kTinyTris) { is_forest = false; fb = ForestBuilder(); }
    }
    int32_t root = 0;
    if (!is_forest && b.run(rows, T, root)) return 1;
    const std::vector<BvhNode> &nodes = is_forest ? fb.nodes : b.nodes;
    const std::vector<float4> &btris = is_forest ? fb.btris : b.btris;
    const std::vector<int32_t> roots2 = is_forest ? fb.roots : std::vector<int32_t>{root};
    Bvh4Topology tp;
    collapse_bvh4(nodes, roots2, tp);
    if ((int) nodes.size() > T || (int) btris.size() / 3 > T || tp.n4 > T || (int) roots2.size() > num_meshes + 1) return 2;
    sizes[0] = (int32_t) nodes.size(); sizes[1] = (int32_t) btris.size() / 3; sizes[2] = (int32_t) roots2.size(); sizes[3] = tp.n4; sizes[4] = tp.stack_need;
    sizes[5] = (int32_t) fb.inline_ids.size(); sizes[6] = is_forest ? 1 : 0; sizes[7] = is_forest ? fb.max_depth : b.max_depth;
    if (!nodes.empty()) std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(BvhNode));
    if (!btris.empty()) std::memcpy(btris_out, btris.data(), btris.size() * sizeof(float4));
    for (size_t k = 0; k < roots2.size(); ++k) {
        roots2_out[k] = roots2[k]; roots4_out[k] = tp.roots[k];
        if (is_forest) fb.tree_box((int) k, boxes_out + 6 * k, boxes_out + 6 * k + 3);
    }
    if (tp.n4 > 0) {
        std::memcpy(child_out, tp.child.data(), (size_t) tp.n4 * 4 * sizeof(int32_t));
        std::memcpy(src_out, tp.src.data(), (size_t) tp.n4 * 4 * sizeof(int32_t));
    }
    for (int i = 0; i < tp.n4; ++i) nodes4_out[i] = bvh4_node_of(nodes.data(), &tp.child[(size_t) i * 4], &tp.src[(size_t) i * 4]);
    for (size_t i = 0; i < fb.inline_ids.size(); ++i) inline_out[i] = fb.inline_ids[i];
    return 0;
}
}  // namespace psdr
