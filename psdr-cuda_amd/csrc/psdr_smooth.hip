// psdr_smooth.hip -- the LargeSteps solves x = (I + lambda L)^-1 b as HIP kernels (include/psdr_hip.h psdr_smooth_*; the operator and the CG step are
// csrc/psdr_smooth.h, shared with the host harness).  Two launch forms of the SAME iteration:
//   one workgroup   the whole solve is ONE launch of ONE workgroup of 1024 threads: p, r and A p live in LDS (p is the vector neighbours read), x in registers,
//                   every dot product is a DPP wave total plus one LDS stage, and the loop ends by a workgroup-uniform test.  Up to kOneWgMax vertices.
//   multi launch    two launches per iteration, every scalar on the device: k_direction forms p = r + beta p for the row AND for the neighbours it gathers
//                   (p is kept in two buffers), writes A p and the partial sums of p^T A p; k_update forms alpha, x += alpha p, r -= alpha A p and the
//                   partial sums of ||r||^2.  The iterations are enqueued on the caller's stream, sixteen at a time, until max_iter or until the host sees
//                   the solve's `done` word raised in pinned memory (a look, never a wait).  A launch that finds
//                   the `done` flag of the state raised returns at once.  No grid-wide barrier, no cooperative launch, no spin on another workgroup's flag.
// Reductions are per-workgroup partial sums in an array, summed by every consumer in one fixed order (lane l takes partials l, l + 64, ... in index order,
// then one DPP wave total): no float atomics, so two solves of one input return the same bits and the same iteration count.
// A row with more than kLongRow neighbours is gathered by a whole wave (the hub of a fan), in both forms.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <string>

#include "../../include/psdr_hip.h"
#include "psdr_smooth.h"

namespace psdr_host { int fail(const std::string &m); }

using namespace psdr_smooth;

namespace {
constexpr int kB = 256;                       // multi-launch workgroup
constexpr int kChunk = 16;                    // multi-launch form: iterations enqueued between two looks at the `done` word
constexpr int kOneWgThreads = 1024;           // one-workgroup form: 16 waves
constexpr int kOneWgRows = 4;                 // rows per thread there (x in registers: 12 VGPRs)
constexpr int kOneWgMax = kOneWgThreads * kOneWgRows;          // 4096 vertices: 3 LDS vectors x 48 KB = 144 KB of the 160 KB
constexpr int kOneWgWaves = kOneWgThreads / 64;
constexpr int kOneWgDefault = kOneWgMax;      // option one_workgroup = -1: meshes up to this many vertices take the one-workgroup form (the crossover)

// sum over the 64 lanes of a wave on the DPP path: an inclusive scan inside every row of 16 (row_shr 1, 2, 4, 8), the row totals carried into the following
// rows (row_bcast:15, row_bcast:31); lane 63 holds the total.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true));
}
__device__ __forceinline__ float wave_total(float v) {
    v = dpp_add<0x111, 0xf>(v); v = dpp_add<0x112, 0xf>(v); v = dpp_add<0x114, 0xf>(v); v = dpp_add<0x118, 0xf>(v);
    v = dpp_add<0x142, 0xa>(v); v = dpp_add<0x143, 0xc>(v);
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// sum of v[3] over a workgroup of NW waves, returned to every thread: wave totals, one LDS stage, the waves' totals added in wave order.  scratch: NW * 3 floats.
template <int NW> __device__ __forceinline__ void block_sum3(float v[3], float *scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < 3; ++c) {
        const float t = wave_total(v[c]);
        if (lane == 0) scratch[wave * 3 + c] = t;
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
        float t = 0.f;
        for (int w = 0; w < NW; ++w) t += scratch[w * 3 + c];
        v[c] = t;
    }
    __syncthreads();
}

// sum of n per-workgroup partials [n][3], returned to every thread of the workgroup: wave 0 reads them (lane l: l, l + 64, ... in index order) and totals them
template <int NW> __device__ __forceinline__ void sum_partials(const float *part, int n, float out[3], float *scratch) {
    if (threadIdx.x < 64) {
        float a[3] = {0.f, 0.f, 0.f};
        for (int k = threadIdx.x; k < n; k += 64) { a[0] += part[3 * k]; a[1] += part[3 * k + 1]; a[2] += part[3 * k + 2]; }
        for (int c = 0; c < 3; ++c) {
            const float t = wave_total(a[c]);
            if (threadIdx.x == 0) scratch[c] = t;
        }
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) out[c] = scratch[c];
    __syncthreads();
}

// Every row of M x, each finished by exactly ONE lane which calls put(i, x_i, (M x)_i): rows up to kLongRow neighbours by the thread that owns them (thread t
// of `threads`: rows t, t + threads, ...), longer rows by whole waves (wave w of `waves`: long rows w, w + waves, ...; the lanes share the neighbours, one DPP
// total per column).  The long-row loop is wave-uniform: all 64 lanes reach every wave_total.
template <class Get, class Put>
__device__ __forceinline__ void for_each_row(int V, const int32_t *rowptr, const int32_t *cols, const int32_t *long_rows, int nlong, float lambda, int t, int threads,
                                             Get get, Put put) {
    const int lane = threadIdx.x & 63, wave = t >> 6, waves = threads >> 6;
    for (int l = wave; l < nlong; l += waves) {
        const int i = long_rows[l];
        const int a = rowptr[i], b = rowptr[i + 1];
        float xi[3], diff[3] = {0.f, 0.f, 0.f}, out[3];
        get(i, xi);
        for (int k = a + lane; k < b; k += 64) {
            float v[3];
            get(cols[k], v);
            diff[0] += xi[0] - v[0]; diff[1] += xi[1] - v[1]; diff[2] += xi[2] - v[2];
        }
        for (int c = 0; c < 3; ++c) diff[c] = wave_total(diff[c]);
        if (lane == 0) {
            row_finish(lambda, xi, diff, out);
            put(i, xi, out);
        }
    }
    for (int i = t; i < V; i += threads) {
        if (rowptr[i + 1] - rowptr[i] > kLongRow) continue;
        float xi[3], out[3];
        apply_row(lambda, i, rowptr, cols, get, xi, out);
        put(i, xi, out);
    }
}

__device__ __forceinline__ void ld3(const float *p, int i, float v[3]) { v[0] = p[3 * (size_t) i]; v[1] = p[3 * (size_t) i + 1]; v[2] = p[3 * (size_t) i + 2]; }
__device__ __forceinline__ void st3(float *p, int i, const float v[3]) { p[3 * (size_t) i] = v[0]; p[3 * (size_t) i + 1] = v[1]; p[3 * (size_t) i + 2] = v[2]; }

struct Csr { const int32_t *rowptr, *cols, *long_rows; int32_t nlong; };

// ---- u = M x -------------------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kB) k_apply(int V, Csr m, float lambda, const float *x, float *u) {
    const int t = blockIdx.x * kB + threadIdx.x;
    for_each_row(V, m.rowptr, m.cols, m.long_rows, m.nlong, lambda, t, (int) gridDim.x * kB,
                 [x](int j, float v[3]) { ld3(x, j, v); }, [u](int i, const float *, const float o[3]) { st3(u, i, o); });
}

// ---- multi-launch form ---------------------------------------------------------------------------------------------------------------------------------------
// x = x0 or 0, r = b - M x0 or b; per-workgroup partial sums of ||b||^2 and ||r||^2
__global__ void __launch_bounds__(kB) k_init(int V, Csr m, float lambda, const float *b, const float *x0, float *x, float *r, float *part_bb, float *part_rr) {
    __shared__ float scratch[(kB / 64) * 3];
    const int t = blockIdx.x * kB + threadIdx.x;
    float abb[3] = {0.f, 0.f, 0.f}, arr[3] = {0.f, 0.f, 0.f};
    if (x0) {
        for_each_row(V, m.rowptr, m.cols, m.long_rows, m.nlong, lambda, t, (int) gridDim.x * kB, [x0](int j, float v[3]) { ld3(x0, j, v); },
                     [&](int i, const float xi[3], const float o[3]) {
                         float bi[3], ri[3];
                         ld3(b, i, bi);
                         for (int c = 0; c < 3; ++c) { ri[c] = bi[c] - o[c]; abb[c] += bi[c] * bi[c]; arr[c] += ri[c] * ri[c]; }
                         st3(x, i, xi); st3(r, i, ri);
                     });
    } else if (t < V) {
        float bi[3];
        const float z[3] = {0.f, 0.f, 0.f};
        ld3(b, t, bi);
        for (int c = 0; c < 3; ++c) { abb[c] = bi[c] * bi[c]; arr[c] = abb[c]; }
        st3(x, t, z); st3(r, t, bi);
    }
    block_sum3<kB / 64>(abb, scratch);
    block_sum3<kB / 64>(arr, scratch);
    if (threadIdx.x == 0) { st3(part_bb, blockIdx.x, abb); st3(part_rr, blockIdx.x, arr); }
}

// The id of the solve whose `done` flag is up, in a word of pinned host memory: the host PEEKS at it between chunks of iterations and stops enqueuing when it
// sees the id of the solve it is enqueuing (psdr_smooth_solve).  It never waits for it: a word that arrives late only costs idle launches.
__device__ __forceinline__ void publish_done(uint32_t *done_word, uint32_t solve_id) { __hip_atomic_store(done_word, solve_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

// step k, first half: the scalars of the step (every workgroup computes them from the same partials in the same order), then p = r + beta p_old for the row and
// its neighbours, A p, the partial sums of p^T A p.  Reads the state of step k - 1, writes the state of step k (two slots: nobody reads the slot being written).
__global__ void __launch_bounds__(kB) k_direction(int k, int V, Csr m, float lambda, float tol, int max_iter, const float *r, const float *p_old, float *p_new, float *Ap,
                                                  const float *part_bb, const float *part_rr, int nparts, float *part_pAp, const CgState *st_prev, CgState *st_cur, uint32_t *done_word, uint32_t solve_id) {
    __shared__ float scratch[(kB / 64) * 3];
    CgState s;
    float beta[3] = {0.f, 0.f, 0.f}, rr[3];
    if (k == 0) {
        float bb[3];
        sum_partials<kB / 64>(part_bb, nparts, bb, scratch);
        sum_partials<kB / 64>(part_rr, nparts, rr, scratch);
        cg_begin(s, bb, rr, tol, max_iter);
    } else {
        s = *st_prev;
        if (s.done) {
            if (blockIdx.x == 0 && threadIdx.x == 0) { *st_cur = s; publish_done(done_word, solve_id); }
            return;
        }
        sum_partials<kB / 64>(part_rr, nparts, rr, scratch);
        cg_advance(s, rr, max_iter, beta);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *st_cur = s;
        if (s.done) publish_done(done_word, solve_id);
    }
    if (s.done) return;
    const int t = blockIdx.x * kB + threadIdx.x;
    const bool first = k == 0;
    const float b0 = beta[0], b1 = beta[1], b2 = beta[2];
    float acc[3] = {0.f, 0.f, 0.f};
    for_each_row(V, m.rowptr, m.cols, m.long_rows, m.nlong, lambda, t, (int) gridDim.x * kB,
                 [=](int j, float v[3]) {
                     ld3(r, j, v);
                     if (!first) { float q[3]; ld3(p_old, j, q); v[0] += b0 * q[0]; v[1] += b1 * q[1]; v[2] += b2 * q[2]; }
                 },
                 [&](int i, const float pi[3], const float o[3]) {
                     st3(p_new, i, pi); st3(Ap, i, o);
                     for (int c = 0; c < 3; ++c) acc[c] += pi[c] * o[c];
                 });
    block_sum3<kB / 64>(acc, scratch);
    if (threadIdx.x == 0) st3(part_pAp, blockIdx.x, acc);
}

// step k, second half: alpha from the partial sums, x += alpha p, r -= alpha A p, the partial sums of the new ||r||^2
__global__ void __launch_bounds__(kB) k_update(int V, const float *p, const float *Ap, float *x, float *r, const float *part_pAp, int nparts, const CgState *st_cur,
                                               float *part_rr_next) {
    __shared__ float scratch[(kB / 64) * 3];
    const CgState s = *st_cur;
    if (s.done) return;
    float pAp[3], alpha[3], acc[3] = {0.f, 0.f, 0.f};
    sum_partials<kB / 64>(part_pAp, nparts, pAp, scratch);
    cg_alpha(s, pAp, alpha);
    const int t = blockIdx.x * kB + threadIdx.x;
    if (t < V) {
        float pi[3], ai[3], xi[3], ri[3];
        ld3(p, t, pi); ld3(Ap, t, ai); ld3(x, t, xi); ld3(r, t, ri);
        for (int c = 0; c < 3; ++c) { xi[c] += alpha[c] * pi[c]; ri[c] -= alpha[c] * ai[c]; acc[c] = ri[c] * ri[c]; }
        st3(x, t, xi); st3(r, t, ri);
    }
    block_sum3<kB / 64>(acc, scratch);
    if (threadIdx.x == 0) st3(part_rr_next, blockIdx.x, acc);
}

// after the last enqueued step: close the state if the steps ran out before the test did, write exact zeros into the columns whose b is zero, publish the state
__global__ void __launch_bounds__(kB) k_finish(int V, float *x, const float *part_rr, int nparts, int max_iter, const CgState *st_prev, CgState *result) {
    __shared__ float scratch[(kB / 64) * 3];
    CgState s = *st_prev;
    if (!s.done) {
        float rr[3], beta[3];
        sum_partials<kB / 64>(part_rr, nparts, rr, scratch);
        cg_advance(s, rr, max_iter, beta);
        s.done = 1;
    }
    const int t = blockIdx.x * kB + threadIdx.x;
    if (t < V)
        for (int c = 0; c < 3; ++c)
            if (s.zero[c]) x[3 * (size_t) t + c] = 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) *result = s;
}

// ---- one-workgroup form ----------------------------------------------------------------------------------------------------------------------------------------
// Thread t owns rows t, t + 1024, ... (at most kOneWgRows).  LDS rows are 12 bytes: lane l of a wave touches bank (3 l + c) mod 32, conflict-free in the
// element-wise passes.  The CSR is read from global memory (L2) every iteration; nothing else leaves the CU until x is stored.
__global__ void __launch_bounds__(kOneWgThreads) k_solve_one(int V, Csr m, float lambda, float tol, int max_iter, const float *b, const float *x0, float *x, CgState *result) {
    __shared__ float lds[3 * 3 * kOneWgMax + kOneWgWaves * 3];
    float *p = lds, *r = lds + 3 * kOneWgMax, *Ap = lds + 6 * kOneWgMax, *scratch = lds + 9 * kOneWgMax;
    const int t = threadIdx.x;
    float xr[kOneWgRows][3];
    float abb[3] = {0.f, 0.f, 0.f}, arr[3] = {0.f, 0.f, 0.f};
    if (x0) {
        for_each_row(V, m.rowptr, m.cols, m.long_rows, m.nlong, lambda, t, kOneWgThreads, [x0](int j, float v[3]) { ld3(x0, j, v); },
                     [Ap](int i, const float *, const float o[3]) { st3(Ap, i, o); });
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kOneWgRows; ++q) {
        const int i = t + q * kOneWgThreads;
        xr[q][0] = xr[q][1] = xr[q][2] = 0.f;
        if (i < V) {
            float bi[3], ri[3];
            ld3(b, i, bi);
            if (x0) {
                float mx[3];
                ld3(x0, i, xr[q]); ld3(Ap, i, mx);
                for (int c = 0; c < 3; ++c) ri[c] = bi[c] - mx[c];
            } else {
                for (int c = 0; c < 3; ++c) ri[c] = bi[c];
            }
            for (int c = 0; c < 3; ++c) { abb[c] += bi[c] * bi[c]; arr[c] += ri[c] * ri[c]; }
            st3(r, i, ri);
        }
    }
    block_sum3<kOneWgWaves>(abb, scratch);
    block_sum3<kOneWgWaves>(arr, scratch);
    CgState s;
    cg_begin(s, abb, arr, tol, max_iter);
    float beta[3] = {0.f, 0.f, 0.f};
    bool first = true;
    while (!s.done) {          // (workgroup-uniform: every thread holds the same sums)
#pragma unroll
        for (int q = 0; q < kOneWgRows; ++q) {
            const int i = t + q * kOneWgThreads;
            if (i < V) {
                float ri[3], pi[3];
                ld3(r, i, ri);
                if (first) { pi[0] = ri[0]; pi[1] = ri[1]; pi[2] = ri[2]; }
                else { ld3(p, i, pi); for (int c = 0; c < 3; ++c) pi[c] = ri[c] + beta[c] * pi[c]; }
                st3(p, i, pi);
            }
        }
        first = false;
        __syncthreads();
        float acc[3] = {0.f, 0.f, 0.f};
        for_each_row(V, m.rowptr, m.cols, m.long_rows, m.nlong, lambda, t, kOneWgThreads, [p](int j, float v[3]) { ld3(p, j, v); },
                     [&](int i, const float pi[3], const float o[3]) {
                         st3(Ap, i, o);
                         for (int c = 0; c < 3; ++c) acc[c] += pi[c] * o[c];
                     });
        block_sum3<kOneWgWaves>(acc, scratch);
        float alpha[3];
        cg_alpha(s, acc, alpha);
        float rr[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < kOneWgRows; ++q) {
            const int i = t + q * kOneWgThreads;
            if (i < V) {
                float pi[3], ai[3], ri[3];
                ld3(p, i, pi); ld3(Ap, i, ai); ld3(r, i, ri);
                for (int c = 0; c < 3; ++c) { xr[q][c] += alpha[c] * pi[c]; ri[c] -= alpha[c] * ai[c]; rr[c] += ri[c] * ri[c]; }
                st3(r, i, ri);
            }
        }
        block_sum3<kOneWgWaves>(rr, scratch);
        cg_advance(s, rr, max_iter, beta);
    }
#pragma unroll
    for (int q = 0; q < kOneWgRows; ++q) {
        const int i = t + q * kOneWgThreads;
        if (i < V) {
            for (int c = 0; c < 3; ++c) if (s.zero[c]) xr[q][c] = 0.f;
            st3(x, i, xr[q]);
        }
    }
    if (t == 0) *result = s;
}

inline dim3 grid(int n) { return dim3((unsigned) ((n + kB - 1) / kB)); }
}  // namespace

struct psdr_smooth_s {
    int32_t V = 0, nnz = 0, nlong = 0, nparts = 0;
    int32_t *d_rowptr = nullptr, *d_cols = nullptr, *d_long = nullptr;
    float *d_work = nullptr;          // r | p (two buffers) | A p | partial sums: bb, p^T A p, rr (two buffers)
    CgState *d_state = nullptr;       // two step slots + the published result
    hipEvent_t ev = nullptr;
    uint32_t *done_word = nullptr;    // pinned host memory: the id of the last multi-launch solve that raised its `done` flag (k_direction writes, the host peeks)
    uint32_t solve_id = 0;
    int32_t opt_one_workgroup = -1;
    int32_t last_form = -1, last_launches = 0;
    bool pending = false;
    Csr csr() const { return Csr{d_rowptr, d_cols, d_long, nlong}; }
};

#define SMOOTH_TRY(expr)                                                                           \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) return psdr_host::fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

extern "C" {

void psdr_smooth_destroy(psdr_smooth_t h) {
    if (!h) return;
    if (h->ev) { (void) hipEventSynchronize(h->ev); (void) hipEventDestroy(h->ev); }
    (void) hipFree(h->d_rowptr); (void) hipFree(h->d_cols); (void) hipFree(h->d_long); (void) hipFree(h->d_work); (void) hipFree(h->d_state);
    if (h->done_word) (void) hipHostFree(h->done_word);
    delete h;
}

int psdr_smooth_create(int32_t V, int32_t F, const int32_t *faces, psdr_smooth_t *out) {
    if (!out) return psdr_host::fail("psdr_smooth_create: null output handle");
    *out = nullptr;
    if (V <= 0) return psdr_host::fail("psdr_smooth_create: V must be positive");
    if (F < 0 || (F > 0 && !faces)) return psdr_host::fail("psdr_smooth_create: invalid face table");
    Adjacency adj;
    std::string err;
    if (!build_adjacency(V, F, faces, adj, err)) return psdr_host::fail("psdr_smooth_create: " + err);
    psdr_smooth_s *h = new (std::nothrow) psdr_smooth_s();
    if (!h) return psdr_host::fail("psdr_smooth_create: out of host memory");
    h->V = V; h->nnz = (int32_t) adj.cols.size(); h->nlong = (int32_t) adj.long_rows.size(); h->nparts = (V + kB - 1) / kB;
    const size_t n3 = (size_t) V * 3, np3 = (size_t) h->nparts * 3;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&h->d_rowptr), sizeof(int32_t) * ((size_t) V + 1));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->d_cols), sizeof(int32_t) * (adj.cols.size() + 1));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->d_long), sizeof(int32_t) * (adj.long_rows.size() + 1));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->d_work), sizeof(float) * (4 * n3 + 4 * np3));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->d_state), sizeof(CgState) * 3);
    if (e == hipSuccess) e = hipMemcpy(h->d_rowptr, adj.rowptr.data(), sizeof(int32_t) * ((size_t) V + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && !adj.cols.empty()) e = hipMemcpy(h->d_cols, adj.cols.data(), sizeof(int32_t) * adj.cols.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !adj.long_rows.empty()) e = hipMemcpy(h->d_long, adj.long_rows.data(), sizeof(int32_t) * adj.long_rows.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(h->d_state, 0, sizeof(CgState) * 3);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&h->done_word), sizeof(uint32_t), hipHostMallocDefault);
    if (e == hipSuccess) *h->done_word = 0;
    if (e != hipSuccess) {
        psdr_smooth_destroy(h);
        return psdr_host::fail(std::string("psdr_smooth_create: ") + hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

int psdr_smooth_set_option(psdr_smooth_t h, const char *name, int value) {
    if (!h || !name) return psdr_host::fail("psdr_smooth_set_option: null handle or name");
    if (std::string(name) == "one_workgroup") {
        if (value < -1 || value > 1) return psdr_host::fail("psdr_smooth_set_option: one_workgroup takes 1 (always), 0 (never) or -1 (by the vertex count)");
        if (value == 1 && h->V > kOneWgMax)
            return psdr_host::fail("psdr_smooth_set_option: the one-workgroup form holds at most " + std::to_string(kOneWgMax) + " vertices, this mesh has " + std::to_string(h->V));
        h->opt_one_workgroup = value;
        return 0;
    }
    return psdr_host::fail(std::string("psdr_smooth_set_option: unknown option ") + name);
}

int psdr_smooth_apply(psdr_smooth_t h, float lambda, const float *x, float *u, void *stream) {
    if (!h) return psdr_host::fail("psdr_smooth_apply: null handle");
    if (!x || !u || x == u) return psdr_host::fail("psdr_smooth_apply: x and u must be two device tables");
    if (!(lambda >= 0.f)) return psdr_host::fail("psdr_smooth_apply: lambda must not be negative");
    hipLaunchKernelGGL(k_apply, grid(h->V), dim3(kB), 0, (hipStream_t) stream, h->V, h->csr(), lambda, x, u);
    SMOOTH_TRY(hipGetLastError());
    return 0;
}

int psdr_smooth_solve(psdr_smooth_t h, float lambda, const float *b, const float *x0, float *x, float tol, int32_t max_iter, void *stream) {
    if (!h) return psdr_host::fail("psdr_smooth_solve: null handle");
    if (!b || !x || x == b) return psdr_host::fail("psdr_smooth_solve: b and x must be two device tables");
    if (!(lambda >= 0.f)) return psdr_host::fail("psdr_smooth_solve: lambda must not be negative");
    if (!(tol > 0.f)) return psdr_host::fail("psdr_smooth_solve: tol must be positive");
    if (max_iter < 1) return psdr_host::fail("psdr_smooth_solve: max_iter must be at least 1");
    hipStream_t s = (hipStream_t) stream;
    const int V = h->V, np = h->nparts;
    const bool one = h->opt_one_workgroup == 1 || (h->opt_one_workgroup == -1 && V <= kOneWgDefault);
    CgState *result = h->d_state + 2;
    if (h->pending) SMOOTH_TRY(hipStreamWaitEvent(s, h->ev, 0));          // the work vectors are the handle's: a solve on another stream runs behind the last one
    if (one) {
        hipLaunchKernelGGL(k_solve_one, dim3(1), dim3(kOneWgThreads), 0, s, V, h->csr(), lambda, tol, (int) max_iter, b, x0, x, result);
        // (x0 == x is fine here: x is stored once, at the end, after every read of x0)
        h->last_launches = 1;
    } else {
        const size_t n3 = (size_t) V * 3, np3 = (size_t) np * 3;
        float *r = h->d_work, *p[2] = {h->d_work + n3, h->d_work + 2 * n3}, *Ap = h->d_work + 3 * n3;
        float *part_bb = h->d_work + 4 * n3, *part_pAp = part_bb + np3, *part_rr[2] = {part_pAp + np3, part_pAp + 2 * np3};
        CgState *st[2] = {h->d_state, h->d_state + 1};
        const float *x0_in = x0;
        if (x0 == x) {          // k_init gathers x0 while it stores x: stage the warm start in a buffer no launch before step 0 reads
            SMOOTH_TRY(hipMemcpyAsync(p[1], x0, sizeof(float) * n3, hipMemcpyDeviceToDevice, s));
            x0_in = p[1];
        }
        hipLaunchKernelGGL(k_init, grid(V), dim3(kB), 0, s, V, h->csr(), lambda, b, x0_in, x, r, part_bb, part_rr[0]);
        // The iterations are enqueued in chunks; between chunks the host looks (one load of pinned memory, no wait) whether the device has raised this solve's
        // `done` flag meanwhile, and stops enqueuing if so: the launches behind the flag are idle.  What the solve computes does not depend on where it stops.
        const uint32_t id = ++h->solve_id ? h->solve_id : ++h->solve_id;          // (never 0: the word's initial value)
        int K = 0;
        while (K < max_iter) {
            const int end = max_iter - K > kChunk ? K + kChunk : (int) max_iter;
            for (int k = K; k < end; ++k) {
                hipLaunchKernelGGL(k_direction, grid(V), dim3(kB), 0, s, k, V, h->csr(), lambda, tol, (int) max_iter, r, p[(k + 1) & 1], p[k & 1], Ap, part_bb, part_rr[k & 1], np,
                                   part_pAp, st[(k + 1) & 1], st[k & 1], h->done_word, id);
                hipLaunchKernelGGL(k_update, grid(V), dim3(kB), 0, s, V, p[k & 1], Ap, x, r, part_pAp, np, st[k & 1], part_rr[(k + 1) & 1]);
            }
            K = end;
            if (__atomic_load_n(h->done_word, __ATOMIC_RELAXED) == id) break;
        }
        hipLaunchKernelGGL(k_finish, grid(V), dim3(kB), 0, s, V, x, part_rr[K & 1], np, (int) max_iter, st[(K - 1) & 1], result);
        h->last_launches = 2 + 2 * K;
    }
    SMOOTH_TRY(hipGetLastError());
    SMOOTH_TRY(hipEventRecord(h->ev, s));
    h->pending = true;
    h->last_form = one ? 1 : 0;
    return 0;
}

int psdr_smooth_info(psdr_smooth_t h, psdr_smooth_info_t *out) {
    if (!h || !out) return psdr_host::fail("psdr_smooth_info: null handle or output");
    *out = psdr_smooth_info_t{};
    out->form = h->last_form;
    out->launches = h->last_launches;
    out->one_workgroup_limit = kOneWgMax;
    out->one_workgroup_default = kOneWgDefault;
    out->num_vertices = h->V;
    out->num_entries = h->nnz;
    out->long_rows = h->nlong;
    if (!h->pending) return 0;
    SMOOTH_TRY(hipEventSynchronize(h->ev));
    CgState s;
    SMOOTH_TRY(hipMemcpy(&s, h->d_state + 2, sizeof(s), hipMemcpyDeviceToHost));
    out->iterations = s.iters;
    out->converged = cg_converged(s) ? 1 : 0;
    for (int c = 0; c < 3; ++c) out->rel_residual[c] = s.zero[c] ? 0.f : sqrtf(s.rr[c] / s.bb[c]);
    return 0;
}
}
