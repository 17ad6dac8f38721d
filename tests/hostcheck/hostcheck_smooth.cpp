// hostcheck_smooth.cpp -- TEST-ONLY harness: the LargeSteps operator and CG step (csrc/psdr_smooth.h) run on the host, so that `-m "not gpu"` tests can check
// the adjacency build, the row operator and the guarded CG loop where no GPU exists, and the GPU tests have a second reference beside the float64 direct
// solve.  A library of its own (libhostcheck_smooth.so), as hostcheck_collocated.cpp is for its header.  Never imported by the psdr_cuda package and not a
// fallback: the package only ever runs these functions inside HIP kernels.  tests/hostcheck/smooth_san.cpp includes this file into a stand-alone program for
// the host sanitizers.
#include "../../psdr-cuda_amd/csrc/psdr_smooth.h"

#include <cmath>
#include <cstring>

using namespace psdr_smooth;

namespace {
void put_error(const std::string &m, char *err, int32_t err_cap) {
    if (err && err_cap > 0) { std::strncpy(err, m.c_str(), (size_t) err_cap - 1); err[err_cap - 1] = 0; }
}
}  // namespace

extern "C" {

// rowptr [V + 1]; cols [cols_cap] (may be null: only the count); *nnz = the number of directed entries.  Returns 0, 1 (error, message in err) or 2 (cols_cap too small).
int hostcheck_smooth_csr(int32_t V, int32_t F, const int32_t *faces, int32_t *rowptr, int32_t *cols, int32_t cols_cap, int32_t *nnz, char *err, int32_t err_cap) {
    Adjacency adj;
    std::string m;
    if (!build_adjacency(V, F, faces, adj, m)) { put_error(m, err, err_cap); return 1; }
    if (nnz) *nnz = (int32_t) adj.cols.size();
    if (rowptr) std::memcpy(rowptr, adj.rowptr.data(), sizeof(int32_t) * adj.rowptr.size());
    if (cols) {
        if ((size_t) cols_cap < adj.cols.size()) return 2;
        if (!adj.cols.empty()) std::memcpy(cols, adj.cols.data(), sizeof(int32_t) * adj.cols.size());
    }
    return 0;
}

int hostcheck_smooth_apply(int32_t V, int32_t F, const int32_t *faces, float lambda, const float *x, float *u) {
    Adjacency adj;
    std::string m;
    if (!build_adjacency(V, F, faces, adj, m)) return 1;
    apply_host(V, adj.rowptr.data(), adj.cols.data(), lambda, x, u);
    return 0;
}

// info = {iterations, converged, zero columns (bit c)}; rel_res [3] = ||r|| / ||b|| of the recurrence (0 for a zero column)
int hostcheck_smooth_solve(int32_t V, int32_t F, const int32_t *faces, float lambda, const float *b, const float *x0, float *x, float tol, int32_t max_iter,
                           int32_t info[3], float rel_res[3]) {
    Adjacency adj;
    std::string m;
    if (!build_adjacency(V, F, faces, adj, m)) return 1;
    const CgState s = solve_host(V, adj.rowptr.data(), adj.cols.data(), lambda, b, x0, x, tol, max_iter);
    info[0] = s.iters; info[1] = cg_converged(s) ? 1 : 0; info[2] = s.zero[0] | (s.zero[1] << 1) | (s.zero[2] << 2);
    for (int c = 0; c < 3; ++c) rel_res[c] = s.zero[c] ? 0.f : std::sqrt(s.rr[c] / s.bb[c]);
    return 0;
}
}
