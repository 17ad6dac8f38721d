// hostcheck_path_sedge.cpp -- TEST-ONLY harness, a sibling of hostcheck.cpp: runs the PathTracer's secondary-edge estimator (csrc/psdr_path_sedge.h, PSDR_HD
// functions) on the host, slot by slot, so that `-m "not gpu"` tests can check the term (depth-1 anchor, forward = reverse, AD against finite
// differences) where no GPU exists.  Never imported by the psdr_cuda package and not a fallback.  The slot loops are host_common.h's; here the options are the
// caller's, raw, and any grid of the descriptor is dropped (PathTracer slots are not guided).
#include "host_common.h"

extern "C" {

// forward mode (K = 1): the derivative image of the PathTracer's secondary-edge term ALONE (slots [W H sppse_begin, W H sppse_end) of sampler 2);
// seg / walk: the scene options pt_sedge / pt_sedge_walk
int hostcheck_path_sedge_fwd(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const psdr_tangents *tan, float *dimg, int nthreads) {
    return path_sedge_fwd(d, o, Grid::drop, PathSedgeOpts{o->max_depth, seg, walk}, tan, dimg, nthreads);
}

// reverse mode: the same slots scattered into the caller's gradient tables (accumulated with +=, one thread: the summation order is fixed)
int hostcheck_path_sedge_rev(const psdr_scene_desc *d, const psdr_render_opts *o, int seg, int walk, const float *adj, const psdr_grads *grads) {
    return path_sedge_rev(d, o, Grid::drop, PathSedgeOpts{o->max_depth, seg, walk}, adj, grads);
}

// how many of the slots get past the first two rays of segment A / segment B (the survivor lists of a split launch): out[0], out[1]; returns the slot count in out[2]
int hostcheck_path_sedge_survivors(const psdr_scene_desc *d, const psdr_render_opts *o, long long *out) {
    return path_sedge_survivors(d, o, Grid::drop, nullptr, out);
}

int hostcheck_path_sedge_draws(int max_depth) { return path_sedge_draws(max_depth); }
}
