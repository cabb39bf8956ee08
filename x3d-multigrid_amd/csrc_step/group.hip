// The grouped update of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_apply_groups, the guarded update with a
// learning-rate and a weight-decay scale per tensor and optional Nesterov momentum.  Shaped like launch 1 of
// x3dstep_measure: a wave per item of the flat buffer's item table, so that a lane knows its tensor.  The decision, tensor,
// element and per-item rules and the walk of a lane are step_core.h's, shared with the CPU twin.  No LDS, no atomics, no
// allocation, no synchronisation.
#include "step_core.h"

void x3dstep_set_error(const char* fmt, ...);  // step_host.cpp
int x3dstep_check_groups(const char* who, const float* w, const float* g, const float* m, int64_t n, const X3DStepItem* items,
                         int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state, const void* ring, int R,
                         float momentum, int first, int nesterov);

using namespace x3ds;

constexpr int kGroupThreads = kLanes * X3DSTEP_ITEMS_PER_GROUP;

// wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v.  With a state every thread reads the decision first
// (uniform loads); thread 0 of workgroup 0 writes the three counters, words no thread of the grid reads.
__global__ __launch_bounds__(kGroupThreads) void x3dstep_apply_groups_kernel(float* w, const float* g, float* m, int64_t n,
                                                                              const X3DStepItem* __restrict__ items,
                                                                              int64_t nitems,
                                                                              const X3DStepHyper* __restrict__ hyper, int S,
                                                                              int64_t* state, const void* ring, int R,
                                                                              GroupArgs a) {
    float coef = 1.0f;
    if (state) {
        const Decision d = apply_decision(state, ring, R, S);
        if (!d.go) return;
        if (blockIdx.x == 0 && threadIdx.x == 0) apply_counters(state, d.skip);
        if (d.skip) return;
        coef = d.coef;
    }
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
    const GroupArgs a = {lr, momentum, weight_decay, grad_scale, first, nesterov};
    const unsigned grid = (unsigned)((nitems + X3DSTEP_ITEMS_PER_GROUP - 1) / X3DSTEP_ITEMS_PER_GROUP);
    x3dstep_apply_groups_kernel<<<grid, kGroupThreads, 0, (hipStream_t)stream>>>(w, g, m, n, items, nitems, hyper, S, state,
                                                                                 ring, R, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        x3dstep_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e));
        return X3DSTEP_ELAUNCH;
    }
    return X3DSTEP_OK;
}
