// bvh4_san.cpp -- TEST-ONLY stand-alone program (no Python): the host builders, collapse_bvh4 and quantise_bvh4 (bvh4_host.h) over triangle tables read
// from a file, meant to be compiled with -fsanitize=address,undefined (tests/test_bvh4_host.py builds and runs it as a child process).
//   file   = int32 count, then per table: int32 T, num_meshes, max_leaf, forest; float rows[T * PSDR_TRI_STRIDE]; int32 tri_mesh[T]
//   stdout = one line per table: the eight `sizes` of bvh4_host and a checksum of the quantised nodes
#include "bvh4_host.h"

#include <cstdio>

using namespace psdr;

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: bvh4_san <tables file>\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "bvh4_san: cannot open %s\n", argv[1]); return 2; }
    int32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    for (int k = 0; k < count; ++k) {
        int32_t hd[4];
        if (std::fread(hd, 4, 4, f) != 4 || hd[0] <= 0 || hd[1] <= 0) return 2;
        const size_t T = (size_t) hd[0];
        std::vector<float> rows(T * PSDR_TRI_STRIDE);
        std::vector<int32_t> tri_mesh(T);
        if (std::fread(rows.data(), sizeof(float), rows.size(), f) != rows.size() || std::fread(tri_mesh.data(), 4, T, f) != T) return 2;
        // exactly the sizes the interface promises, so that a write past them is the sanitizer's to find
        std::vector<BvhNode> nodes(T);
        std::vector<Bvh4Node> nodes4(T);
        std::vector<float> btris(T * 12), boxes((size_t) (hd[1] + 1) * 6);
        std::vector<int32_t> roots2((size_t) hd[1] + 1), roots4((size_t) hd[1] + 1), child(T * 4), src(T * 4), inl(T);
        int32_t sizes[8] = {};
        const int rc = bvh4_host(rows.data(), tri_mesh.data(), hd[0], hd[1], hd[2], hd[3], sizes, nodes.data(), btris.data(), roots2.data(), roots4.data(),
                                 child.data(), src.data(), nodes4.data(), inl.data(), boxes.data());
        if (rc) { std::fprintf(stderr, "bvh4_san: table %d failed (%d)\n", k, rc); return 1; }
        uint32_t sum = 0;
        for (int i = 0; i < sizes[3]; ++i) {
            uint32_t w[16];
            std::memcpy(w, &nodes4[(size_t) i], sizeof(w));
            for (int j = 0; j < 14; ++j) sum = sum * 31u + w[j];          // (the two pad words are zero)
        }
        std::printf("%d %d %d %d %d %d %d %d %u\n", sizes[0], sizes[1], sizes[2], sizes[3], sizes[4], sizes[5], sizes[6], sizes[7], sum);
    }
    std::fclose(f);
    return 0;
}
