// psdr_smooth.h -- the "Large Steps" operator M = I + lambda L (L: the combinatorial Laplacian of a mesh's unique undirected edges) and the conjugate-gradient
// step that solves M x = b, on the [V][3] float layout of the vertex tables (Nicolet, Jacobson, Jakob 2021: optimise u = M x, recover x = M^-1 u every step,
// the vertex gradient becomes M^-1 g).  Plain C++: ONE copy of the adjacency build, the row operator and the scalar part of the CG step.  The kernels
// (psdr_smooth.hip, both launch forms) and the host harness (tests/hostcheck/hostcheck_smooth.cpp) compile from it; they differ only in the order in which
// they sum a dot product.
//
// CG runs on the three columns in lockstep with per-column alpha, beta and residuals, unpreconditioned (the degrees of a mesh are nearly uniform: Jacobi
// scaling changed the iteration count by one at most).  The guards below are what keeps a floor mesh (an all-zero z column) from returning NaN: a naive
// float CG divides 0 by 0 in alpha and beta there.
//   - a column is ACTIVE while ||r|| > tol ||b||; a column that is not active has alpha = beta = 0 (it is frozen: x and r keep their bits);
//   - a column with ||b|| = 0 is never active and its x is EXACT zeros, whatever x0 was;
//   - p^T A p <= 0 (p has vanished) gives alpha = 0 instead of a division;
//   - every comparison is written so that a NaN keeps the column active and reaches x: non-finite input gives non-finite output after max_iter iterations.
// The norms are float sums of squares, so the tests see overflow and underflow of ||b||^2 as they see infinity and zero: a finite column with |b| around 1e19
// or more (||b||^2 = inf) is treated as non-finite input -- it runs to max_iter and reports "not converged" -- and a column whose ||b||^2 underflows (flushed
// to zero below about 1e-19 per entry) comes back as exact zeros.  Both are far from the magnitudes of vertex and gradient tables; scale such a table first.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PSDR_SMOOTH_HD __host__ __device__ inline
#else
#define PSDR_SMOOTH_HD inline
#endif

#include <algorithm>
#include <string>
#include <vector>

namespace psdr_smooth {

// rows with more neighbours than this are not one lane's work: a wave gathers them (a hub of a fan with a thousand spokes must not serialise a launch)
constexpr int kLongRow = 64;

// ---- the row operator -----------------------------------------------------------------------------------------------------------------------------------
// (M x)_i = (1 + lambda deg_i) x_i - lambda sum_{j in N(i)} x_j, evaluated as x_i + lambda sum_j (x_i - x_j): the two large terms of the first form cancel
// (a hub of a thousand neighbours at lambda = 100 has a diagonal of 1e5), and in float that cancellation, not the stopping test, would bound the accuracy of
// the solve.  get(j, v) fetches row j of x into v[3]; the neighbours are summed in column order.
PSDR_SMOOTH_HD void row_finish(float lambda, const float xi[3], const float diff[3], float out[3]) {
    for (int c = 0; c < 3; ++c) out[c] = xi[c] + lambda * diff[c];
}
template <class Get> PSDR_SMOOTH_HD void apply_row(float lambda, int i, const int32_t *rowptr, const int32_t *cols, Get get, float xi[3], float out[3]) {
    const int a = rowptr[i], b = rowptr[i + 1];
    float diff[3] = {0.f, 0.f, 0.f};
    get(i, xi);
    for (int k = a; k < b; ++k) {
        float v[3];
        get(cols[k], v);
        diff[0] += xi[0] - v[0]; diff[1] += xi[1] - v[1]; diff[2] += xi[2] - v[2];
    }
    row_finish(lambda, xi, diff, out);
}

// ---- the scalar part of the CG step ---------------------------------------------------------------------------------------------------------------------
struct CgState {
    float rr[3];          // ||r||^2 of the iterate the state describes
    float bb[3];          // ||b||^2
    float thr[3];         // tol^2 ||b||^2
    int32_t active[3];    // the column still iterates
    int32_t zero[3];      // ||b|| = 0: the column's x is exact zeros
    int32_t iters;        // CG steps taken
    int32_t done;         // no column active, or max_iter reached
};

PSDR_SMOOTH_HD bool column_active(float rr, float thr, float bb) { return !(rr <= thr) || !(fabsf(bb) <= 3.402823466e38f); }

// before the first step: bb, rr = the norms of b and of r0 = b - M x0
PSDR_SMOOTH_HD void cg_begin(CgState &s, const float bb[3], const float rr[3], float tol, int max_iter) {
    bool any = false;
    for (int c = 0; c < 3; ++c) {
        s.bb[c] = bb[c]; s.rr[c] = rr[c]; s.thr[c] = tol * tol * bb[c];
        s.zero[c] = bb[c] == 0.f;
        s.active[c] = !s.zero[c] && column_active(rr[c], s.thr[c], bb[c]);
        any = any || s.active[c];
    }
    s.iters = 0;
    s.done = !any || max_iter < 1;
}
// after a step: rr_new = ||r||^2 of the updated residual.  Returns beta of every column for the next direction p = r + beta p.
PSDR_SMOOTH_HD void cg_advance(CgState &s, const float rr_new[3], int max_iter, float beta[3]) {
    bool any = false;
    for (int c = 0; c < 3; ++c) {
        const bool was = s.active[c] != 0;
        const bool now = was && column_active(rr_new[c], s.thr[c], s.bb[c]);
        beta[c] = now ? rr_new[c] / s.rr[c] : 0.f;
        if (was) s.rr[c] = rr_new[c];
        s.active[c] = now;
        any = any || now;
    }
    s.iters += 1;
    s.done = !any || s.iters >= max_iter;
}
// alpha of every column from pAp = p^T M p
PSDR_SMOOTH_HD void cg_alpha(const CgState &s, const float pAp[3], float alpha[3]) {
    for (int c = 0; c < 3; ++c) alpha[c] = (s.active[c] && !(pAp[c] <= 0.f)) ? s.rr[c] / pAp[c] : 0.f;
}
PSDR_SMOOTH_HD bool cg_converged(const CgState &s) { return !(s.active[0] || s.active[1] || s.active[2]); }

// ---- adjacency (host) -----------------------------------------------------------------------------------------------------------------------------------
// CSR of the unique undirected edges of a face table [F][3]: an edge shared by any number of faces or repeated by a duplicated face counts once, an edge
// (a, a) of a degenerate face is dropped, a vertex no face uses has an empty row (its row of M is the identity), rows are sorted by column -- one fixed byte
// string per face table.  An index outside [0, V) is an error (never clamped): returns false with a message.  long_rows = the rows with more than kLongRow
// neighbours, ascending.
struct Adjacency {
    std::vector<int32_t> rowptr, cols, long_rows;
};
inline bool build_adjacency(int32_t V, int32_t F, const int32_t *faces, Adjacency &adj, std::string &err) {
    if (V <= 0) { err = "V must be positive"; return false; }
    if (F < 0 || (F > 0 && !faces)) { err = "invalid face table"; return false; }
    std::vector<uint64_t> keys;
    keys.reserve((size_t) F * 6);
    for (int32_t f = 0; f < F; ++f) {
        const int32_t *t = faces + (size_t) f * 3;
        for (int k = 0; k < 3; ++k)
            if (t[k] < 0 || t[k] >= V) {
                err = "face " + std::to_string(f) + " names vertex " + std::to_string(t[k]) + " outside [0, " + std::to_string(V) + ")";
                return false;
            }
        for (int k = 0; k < 3; ++k) {
            const uint32_t a = (uint32_t) t[k], b = (uint32_t) t[(k + 1) % 3];
            if (a == b) continue;
            keys.push_back(((uint64_t) a << 32) | b);
            keys.push_back(((uint64_t) b << 32) | a);
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (keys.size() > (size_t) 0x7fffffff) { err = "too many edges for int32 offsets"; return false; }
    adj.rowptr.assign((size_t) V + 1, 0);
    adj.cols.resize(keys.size());
    for (size_t k = 0; k < keys.size(); ++k) {
        adj.rowptr[(size_t) (keys[k] >> 32) + 1] += 1;
        adj.cols[k] = (int32_t) (keys[k] & 0xffffffffu);
    }
    for (int32_t i = 0; i < V; ++i) adj.rowptr[(size_t) i + 1] += adj.rowptr[i];
    adj.long_rows.clear();
    for (int32_t i = 0; i < V; ++i)
        if (adj.rowptr[(size_t) i + 1] - adj.rowptr[i] > kLongRow) adj.long_rows.push_back(i);
    return true;
}

// ---- the whole solve on the host (the harness; the kernels run the same steps) --------------------------------------------------------------------------
inline void apply_host(int32_t V, const int32_t *rowptr, const int32_t *cols, float lambda, const float *x, float *u) {
    auto get = [x](int j, float v[3]) { v[0] = x[3 * (size_t) j]; v[1] = x[3 * (size_t) j + 1]; v[2] = x[3 * (size_t) j + 2]; };
    for (int32_t i = 0; i < V; ++i) {
        float xi[3], o[3];
        apply_row(lambda, i, rowptr, cols, get, xi, o);
        u[3 * (size_t) i] = o[0]; u[3 * (size_t) i + 1] = o[1]; u[3 * (size_t) i + 2] = o[2];
    }
}
// dot products are summed in double and rounded once: the harness is the more exact of the two sides
inline void dot3_host(int32_t V, const float *a, const float *b, float out[3]) {
    double s[3] = {0, 0, 0};
    for (size_t i = 0; i < (size_t) V; ++i)
        for (int c = 0; c < 3; ++c) s[c] += (double) a[3 * i + c] * (double) b[3 * i + c];
    for (int c = 0; c < 3; ++c) out[c] = (float) s[c];
}
inline CgState solve_host(int32_t V, const int32_t *rowptr, const int32_t *cols, float lambda, const float *b, const float *x0, float *x, float tol, int32_t max_iter) {
    const size_t n = (size_t) V * 3;
    std::vector<float> r(n), p(n), Ap(n);
    if (x0) {
        apply_host(V, rowptr, cols, lambda, x0, Ap.data());
        for (size_t e = 0; e < n; ++e) { x[e] = x0[e]; r[e] = b[e] - Ap[e]; }
    } else {
        for (size_t e = 0; e < n; ++e) { x[e] = 0.f; r[e] = b[e]; }
    }
    float bb[3], rr[3], beta[3] = {0.f, 0.f, 0.f}, alpha[3], pAp[3];
    dot3_host(V, b, b, bb);
    dot3_host(V, r.data(), r.data(), rr);
    CgState s;
    cg_begin(s, bb, rr, tol, max_iter);
    bool first = true;
    while (!s.done) {
        for (size_t e = 0; e < n; ++e) p[e] = first ? r[e] : r[e] + beta[e % 3] * p[e];
        first = false;
        apply_host(V, rowptr, cols, lambda, p.data(), Ap.data());
        dot3_host(V, p.data(), Ap.data(), pAp);
        cg_alpha(s, pAp, alpha);
        for (size_t e = 0; e < n; ++e) { x[e] += alpha[e % 3] * p[e]; r[e] -= alpha[e % 3] * Ap[e]; }
        dot3_host(V, r.data(), r.data(), rr);
        cg_advance(s, rr, max_iter, beta);
    }
    for (size_t e = 0; e < n; ++e)
        if (s.zero[e % 3]) x[e] = 0.f;
    return s;
}

}  // namespace psdr_smooth
