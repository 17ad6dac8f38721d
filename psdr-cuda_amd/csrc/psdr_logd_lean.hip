// psdr_logd_lean.hip -- the lean twin of the log-derivative camera kernel (psdr_logd_lean.h) for flag set 8 (plain diffuse, no tree) and its launch.
// A translation unit of its own: the twin's register allocation does not depend on, and does not disturb, the other kernels of the flag set
// (tests/test_isa_guard.py pins those).  The K = 1 instances of the lean PathTracer twin (psdr_path_lean.h: k_camera_logd_path_lean<1, SEEDED>) live here too: the launch
// below tries that twin's form first.
#define PSDR_WIDE_TREE 0
#define PSDR_LEAF_PAIR 0
#include "psdr_kernels.h"
#include "psdr_logd_lean.h"
#include "psdr_path_lean.h"

namespace {

constexpr int kLeanFlags = kSceneTiny;

// k_camera_logd with the path's idle state in LDS columns (psdr_logd_lean.h).  SEEDED: the slot's stream comes from the handle's seed table.
template <int K, int FL, bool SEEDED>
__global__ __launch_bounds__(kBlock, PSDR_LOGD_WAVES_K1) void k_camera_logd_lean(LaunchCtx cx, TV<Dual<K>, FL> tv, int spp, int s_begin, SlotDiv nsp, long long n, float inv_spp,
                                                                                  float *__restrict__ img, float *__restrict__ dimg, long long plane, unsigned long long *counters, int own,
                                                                                  const ulonglong2 *__restrict__ seed) {
    constexpr int NV = 3 * (1 + K);
    if (counters[kLogdGateWord] != 1ull) return;
    TraversalStack st; setup_lds(cx, st, tv);
    Park pk{nullptr};
#if defined(__HIP_DEVICE_COMPILE__)
    pk.base = reinterpret_cast<float *>(psdr_dyn_lds + cx.off_park) + threadIdx.x;
#endif
    uint32_t nrays = 0;
    const long long nceil = (n + kBlock - 1) / kBlock * kBlock;
    for (long long jb = (long long) blockIdx.x * kBlock; jb < nceil; jb += (long long) gridDim.x * kBlock) {          // (a uniform counter: the slot index is not carried in VGPRs)
        const long long j = jb + threadIdx.x;
        const bool in = j < n;
        int pixel = 0x7fffffff, s_in = 0;
        if (in) slot_to_pixel(j, nsp, pixel, s_in);
        Rng rng;
        if constexpr (SEEDED) {
            const ulonglong2 sd = in ? seed[j] : ulonglong2{0ull, 0ull};
            rng.init_seeded(sd.x, sd.y, cx.jump);
        } else {
            rng.init((uint64_t) pixel * (uint64_t) spp + (uint64_t) (s_begin + s_in), cx.jump);
        }
        // camera_sample_logd, for every lane of the trip (in = false: an inactive path)
        const float j0 = rng.next(), j1 = rng.next();
        const int W = cx.sc.d.width;
        const float sx = ((float) (pixel % W) + j0) / (float) W, sy = ((float) (pixel / W) + j1) / (float) cx.sc.d.height;
        const TangentView<0, FL> tv0{};
        const RayT<float> ray = primary_ray<float>(cx.sc, tv0, sx, sy);
        const Vec3<Dual<K>> r = zero_nonfinite(li_path_logd_lean<K>(cx.sc, tv, st, cx.lp, rng, ray, in, nrays, pk));
        float v[NV];
        v[0] = in ? r.x.v * inv_spp : 0.f; v[1] = in ? r.y.v * inv_spp : 0.f; v[2] = in ? r.z.v * inv_spp : 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { v[3 + 3 * k] = in ? r.x.d[k] * inv_spp : 0.f; v[4 + 3 * k] = in ? r.y.d[k] * inv_spp : 0.f; v[5 + 3 * k] = in ? r.z.d[k] * inv_spp : 0.f; }
        const bool head = wave_segmented_sum<NV>(pixel, v);
        if (head && in) {
            float *p = img + (size_t) pixel * 3;
            if (own) {
                p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
#pragma unroll
                for (int k = 0; k < K; ++k) { float *q = dimg + (size_t) k * plane + (size_t) pixel * 3; q[0] = v[3 + 3 * k]; q[1] = v[4 + 3 * k]; q[2] = v[5 + 3 * k]; }
            } else {
                if (v[0] != 0.f) atomicAdd(p, v[0]);
                if (v[1] != 0.f) atomicAdd(p + 1, v[1]);
                if (v[2] != 0.f) atomicAdd(p + 2, v[2]);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    float *q = dimg + (size_t) k * plane + (size_t) pixel * 3;
                    if (v[3 + 3 * k] != 0.f) atomicAdd(q, v[3 + 3 * k]);
                    if (v[4 + 3 * k] != 0.f) atomicAdd(q + 1, v[4 + 3 * k]);
                    if (v[5 + 3 * k] != 0.f) atomicAdd(q + 2, v[5 + 3 * k]);
                }
            }
        }
    }
    count_rays(counters, nrays);
}

}  // namespace

namespace psdr_host {
// Six workgroups per CU (the kernel's six waves per SIMD) must keep their dynamic LDS blocks side by side: staged scene + parking columns within a sixth of
// the CU's 160 KiB, and within a forced lds_budget (tests).  The seeded form under the conditions of the seeded renderC kernel (seed_table).
int logd_lean_launch_8(psdr_scene_s *h, const psdr_render_opts *o, const LaunchCtx &cx0, const psdr::TangentView<1, psdr::kSceneTiny> &tv, float *img, float *dimg, hipStream_t s, bool *ran) {
    *ran = false;
    // the launch the headline makes (every wave on one pixel, slab-form rows only): the twin of psdr_path_lean.h
    if (int rc = path_lean_launch<1>(h, o, cx0, tv, img, dimg, s, ran)) return rc;
    if (*ran) return 0;
    if (h->opt.logd_park == 0) return 0;
    constexpr int kCuLds = 160 * 1024, park = ParkLayout<1>::cols * kBlock * 4;
    const int lds = (lds_bytes(cx0, h) + 15) / 16 * 16;
    const int limit = h->opt.lds_budget > 0 ? std::min(h->opt.lds_budget, kCuLds / PSDR_LOGD_WAVES_K1) : kCuLds / PSDR_LOGD_WAVES_K1;
    if (lds + park > limit) return 0;
    LaunchCtx cx = cx0;
    cx.off_park = lds;
    const long long WH = (long long) h->desc.width * h->desc.height;
    const int nsp = o->spp_end - o->spp_begin;
    const long long n = WH * nsp;
    const int own = wave_owns_pixels(h, nsp, n);
    const dim3 grid(launch_blocks(h, n, camera_blocks_per_cu(h, n)));
    const ulonglong2 *seed = seed_table(h, o, WH, nsp, n, s);
    if (seed != nullptr)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_camera_logd_lean<1, kLeanFlags, true>), grid, dim3(kBlock), lds + park, s, cx, tv, o->spp, o->spp_begin, SlotDiv(nsp), n, 1.f / (float) o->spp, img, dimg,
                           WH * 3, h->d_counters, own, seed);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_camera_logd_lean<1, kLeanFlags, false>), grid, dim3(kBlock), lds + park, s, cx, tv, o->spp, o->spp_begin, SlotDiv(nsp), n, 1.f / (float) o->spp, img, dimg,
                           WH * 3, h->d_counters, own, seed);
    h->logd_lean_launches++;
    if (seed != nullptr) { h->logd_lean_seeded++; h->seed_launches++; }
    h->logd_lean_lds = lds; h->logd_lean_park = park;
    *ran = true;
    return 0;
}
}  // namespace psdr_host
