// psdr_path_lean.hip -- the lean renderC twin of flag set 8 (psdr_path_lean.h, K = 0) and its launch.  A translation unit of its own like psdr_logd_lean.hip, which
// holds the K = 1 instances: the twins' register allocation does not depend on, and does not disturb, the kernels tests/test_isa_guard.py pins.
#define PSDR_WIDE_TREE 0
#define PSDR_LEAF_PAIR 0
#include "psdr_kernels.h"
#include "psdr_path_lean.h"

namespace psdr_host {
int path_lean_launch_8(psdr_scene_s *h, const psdr_render_opts *o, const LaunchCtx &cx, const psdr::TangentView<0, psdr::kSceneTiny> &tv, float *img, float *dimg, hipStream_t s, bool *ran) {
    return path_lean_launch<0>(h, o, cx, tv, img, dimg, s, ran);
}
}  // namespace psdr_host
