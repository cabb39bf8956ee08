// The grouped update of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_apply_groups, the guarded update with a
// learning-rate and a weight-decay scale per tensor and optional Nesterov momentum.  Shaped like launch 1 of
// x3dstep_measure: a wave per item of the flat buffer's item table, so that a lane knows its tensor.  The decision, tensor,
// element and per-item rules and the walk of a lane are step_core.h's, shared with the CPU twin.  No LDS, no atomics, no
// allocation, no synchronisation.
#include "step_priv.h"

using namespace x3ds;

// wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v.  With a state every thread reads the decision first
// (uniform loads); thread 0 of workgroup 0 writes the three counters, words no thread of the grid reads.
__global__ __launch_bounds__(kItemThreads) void x3dstep_apply_groups_kernel(float* w, const float* g, float* m, int64_t n,
                                                                              const X3DStepItem* __restrict__ items,
                                                                              int64_t nitems,
                                                                              const X3DStepHyper* __restrict__ hyper, int S,
                                                                              int64_t* state, const void* ring, int R,
                                                                              SgdArgs a) {
    float coef = 1.0f;
    if (state && !apply_begin(state, ring, R, S, blockIdx.x == 0 && threadIdx.x == 0, &coef)) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    const GroupItem c = group_resolve(items, i, hyper, S, n, a);
    if (c.len > 0) group_lane(w, g, m, c, threadIdx.x & (kLanes - 1), coef, a);
}

extern "C" int x3dstep_apply_groups(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                                    const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R, float lr,
                                    float momentum, float weight_decay, float grad_scale, int first, int nesterov,
                                    void* stream) {
    const int rc = x3dstep_check_groups("x3dstep_apply_groups", w, g, m, n, items, nitems, hyper, S, state, ring, R, momentum,
                                        first, nesterov);
    if (rc) return rc;
    const SgdArgs a = {lr, momentum, weight_decay, grad_scale, first, nesterov};
    x3dstep_apply_groups_kernel<<<item_grid(nitems), kItemThreads, 0, (hipStream_t)stream>>>(w, g, m, n, items, nitems,
                                                                                             hyper, S, state, ring, R, a);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}
