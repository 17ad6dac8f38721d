// smooth_san.cpp -- TEST-ONLY stand-alone program (its own main, no Python): the host harness of the LargeSteps solve (hostcheck_smooth.cpp, i.e. the product's
// csrc/psdr_smooth.h) over meshes it makes itself, built with the host sanitizers by tests/test_smooth_host.py.  Nothing of it is loaded into Python and nothing
// of it runs on a GPU.  A planar grid (one all-zero column), a fan with a long row, a face list with a duplicated, a degenerate and a three-face edge, an
// out-of-range index; adjacency, operator, cold and warm solves, a solve cut at three iterations.  Prints one checksum per mesh; exits 0 when every result is
// finite, the zero column is exact and the bad index is refused.
#include "hostcheck_smooth.cpp"

#include <cstdio>
#include <vector>

namespace {
int fail(const char *what) { std::fprintf(stderr, "smooth_san: %s\n", what); return 1; }

int run(const char *name, int32_t V, const std::vector<int32_t> &faces, float lambda, bool planar) {
    const int32_t F = (int32_t) faces.size() / 3;
    std::vector<int32_t> rowptr((size_t) V + 1);
    int32_t nnz = 0;
    char err[256];
    if (hostcheck_smooth_csr(V, F, faces.data(), rowptr.data(), nullptr, 0, &nnz, err, 256)) return fail(err);
    std::vector<int32_t> cols((size_t) nnz + 1);
    if (hostcheck_smooth_csr(V, F, faces.data(), rowptr.data(), cols.data(), nnz, &nnz, err, 256)) return fail(err);
    std::vector<float> x((size_t) V * 3), u(x.size()), y(x.size()), z(x.size());
    uint32_t s = 12345u;
    for (size_t e = 0; e < x.size(); ++e) { s = s * 1664525u + 1013904223u; x[e] = (planar && e % 3 == 2) ? 0.f : (float) (s >> 8) / 16777216.f - 0.5f; }
    if (hostcheck_smooth_apply(V, F, faces.data(), lambda, x.data(), u.data())) return fail("apply");
    int32_t info[3];
    float res[3];
    if (hostcheck_smooth_solve(V, F, faces.data(), lambda, u.data(), nullptr, y.data(), 1e-6f, 1000, info, res)) return fail("solve");
    if (!info[1]) return fail("cold solve did not converge");
    if (hostcheck_smooth_solve(V, F, faces.data(), lambda, u.data(), y.data(), z.data(), 1e-6f, 1000, info, res)) return fail("warm solve");
    if (!info[1] || info[0] > 1) return fail("warm solve from the solution took more than one step");
    if (hostcheck_smooth_solve(V, F, faces.data(), lambda, u.data(), nullptr, z.data(), 1e-6f, 3, info, res)) return fail("cut solve");
    double sum = 0, worst = 0;
    for (size_t e = 0; e < x.size(); ++e) {
        if (!std::isfinite(y[e]) || !std::isfinite(z[e])) return fail("non-finite result");
        if (planar && e % 3 == 2 && (y[e] != 0.f || z[e] != 0.f)) return fail("the zero column is not exact");
        sum += std::fabs(y[e]);
        worst = std::fmax(worst, std::fabs((double) y[e] - x[e]));
    }
    if (worst > 1e-3) return fail("solve(apply(x)) is not x");
    std::printf("%s %d %d %.9g\n", name, V, nnz, sum);
    return 0;
}
}  // namespace

int main() {
    {   // planar grid, z = 0
        const int n = 12;
        std::vector<int32_t> f;
        for (int y = 0; y + 1 < n; ++y)
            for (int x = 0; x + 1 < n; ++x) {
                const int a = y * n + x;
                const int32_t t[6] = {a, a + 1, a + n, a + 1, a + n + 1, a + n};
                f.insert(f.end(), t, t + 6);
            }
        if (run("grid", n * n, f, 100.f, true)) return 1;
    }
    {   // fan: hub 0 with 200 spokes (a long row), and two unused vertices behind it
        const int m = 200;
        std::vector<int32_t> f;
        for (int k = 0; k < m; ++k) { const int32_t t[3] = {0, 1 + k, 1 + (k + 1) % m}; f.insert(f.end(), t, t + 3); }
        if (run("fan", m + 3, f, 10.f, false)) return 1;
    }
    {   // a duplicated face, an edge of three faces, a degenerate face
        const std::vector<int32_t> f = {0, 1, 2, 0, 1, 2, 0, 1, 3, 1, 0, 4, 2, 2, 3, 5, 5, 5};
        if (run("odd", 7, f, 1.f, false)) return 1;
    }
    {   // V = 1, F = 0
        if (run("single", 1, {}, 19.f, false)) return 1;
    }
    {   // an out-of-range index is refused with a message
        const std::vector<int32_t> f = {0, 1, 7};
        std::vector<int32_t> rowptr(8);
        int32_t nnz = 0;
        char err[256] = {0};
        if (hostcheck_smooth_csr(7, 1, f.data(), rowptr.data(), nullptr, 0, &nnz, err, 256) != 1 || !err[0]) return fail("an out-of-range index was accepted");
        const std::vector<int32_t> g = {0, -1, 2};
        if (hostcheck_smooth_csr(7, 1, g.data(), rowptr.data(), nullptr, 0, &nnz, err, 256) != 1) return fail("a negative index was accepted");
    }
    return 0;
}
