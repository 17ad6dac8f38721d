// hostcheck_path_lean.cpp -- TEST-ONLY harness: the selection rule of the lean PathTracer twins (csrc/psdr_plan.h path_lean_form, a pure host function) run on cases
// tests/test_path_lean_plan_host.py fills in, both as the plain case record and through a hand-filled scene handle.  No HIP call is made and no device is opened;
// psdr_host::fail, which the product defines in psdr_hip.hip, is this file's own.  Never imported by the psdr_cuda package.
#include "../../psdr-cuda_amd/csrc/psdr_host.h"

namespace psdr_host {
int fail(const std::string &) { return 1; }
}  // namespace psdr_host
using namespace psdr_host;

extern "C" {
int hostcheck_path_lean_form(const PathLeanCase *c) { return path_lean_form(*c); }
// the same case through a scene handle (what the launch drivers call): scene and options from the handle, the launch from the arguments
int hostcheck_path_lean_form_handle(const PathLeanCase *c) {
    psdr_scene_s h;
    h.n_tiny = c->n_tiny; h.aa_cnt = c->aa_cnt; h.n_blas = c->n_blas;
    h.opt.lds_budget = c->lds_budget; h.opt.own_pixels = c->own_pixels; h.opt.path_lean = c->path_lean; h.opt.logd_park = c->logd_park;
    return path_lean_form(&h, c->flags, c->K, c->integrator, c->texels_only != 0, c->nsp, c->chunk, c->lds_scene);
}
int hostcheck_path_lean_cols(int K) { return path_lean_cols(K); }
int hostcheck_path_lean_wave_is_pixel(int own_pixels, int nsp, long long chunk) { return wave_is_pixel(own_pixels, nsp, chunk) ? 1 : 0; }
int hostcheck_path_lean_owns(int own_pixels, int nsp, long long chunk) { psdr_scene_s h; h.opt.own_pixels = own_pixels; return wave_owns_pixels(&h, nsp, chunk) ? 1 : 0; }
int hostcheck_path_lean_slab_only(int n_tiny, int aa_cnt, int n_blas) { return slab_only(n_tiny, aa_cnt, n_blas) ? 1 : 0; }
}
