// Trust ratios of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_trust -- the fp64 sum of squares of every tensor of w
// (two launches shaped like launches 1 and 2 of x3dstep_measure) and the LARS ratio of every tensor from it and the latest
// record of the gradient -- and x3dstep_apply_lars, the grouped update with the ratio in its element rule.  The per-lane
// sums, the sum of a tensor's items, the trust rule, the per-item and per-tensor tests and the walk of a lane are
// step_core.h's, shared with the CPU twins.  No float atomics, no allocation, no synchronisation.
#include "step_priv.h"

using namespace x3ds;

// launch 1: wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v; lane 0 stores the item's sum of squares.  Every
// thread reads the counter first (a uniform load): nothing was measured, nothing is stored.
__global__ __launch_bounds__(kItemThreads) void x3dstep_trust_partials_kernel(const float* __restrict__ w, int64_t n,
                                                                               const X3DStepItem* __restrict__ items,
                                                                               int64_t nitems, int S,
                                                                               const int64_t* __restrict__ state,
                                                                               double* __restrict__ part, int vec) {
    if (state[X3DSTEP_S_STEP] == 0) return;
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;                       // the whole wave leaves: no shuffle below is left without its lanes
    const X3DStepItem it = items[i];
    const bool ok = trust_item_ok(it, S, n);       // the same in every lane of the wave
    double p = ok ? trust_lane(w, it, lane, vec != 0) : trust_nan();
    for (int off = kLanes / 2; off > 0; off >>= 1) p = p + __shfl_down(p, off, kLanes);
    if (lane == 0) part[i] = p;
}

// The partials of the first kTrustCached items copied into LDS, as the finalize step of x3dstep_measure does.
constexpr int kTrustCached = 2560;

// launch 2: one workgroup.  Thread t takes the tensors t, t + 1024, ..: the sum of the tensor's items and its ratio.
__global__ __launch_bounds__(kFinalThreads) void x3dstep_trust_finalize_kernel(const int32_t* __restrict__ seg_item, int S,
                                                                                int64_t nitems,
                                                                                const double* __restrict__ part,
                                                                                const X3DStepHyper* __restrict__ hyper,
                                                                                const float* __restrict__ eta,
                                                                                const int64_t* __restrict__ state,
                                                                                const void* ring, int R, TrustArgs a,
                                                                                double* __restrict__ wsumsq,
                                                                                float* __restrict__ trust) {
    __shared__ double c_part[kTrustCached];
    const int64_t step = state[X3DSTEP_S_STEP];
    if (step == 0) return;                         // uniform: before the barrier
    const int t = threadIdx.x;
    const int cached = nitems < kTrustCached ? (int)nitems : kTrustCached;
    for (int i = t; i < cached; i += kFinalThreads) c_part[i] = part[i];
    __syncthreads();
    const Record rec = record_at((void*)ring, R, S, step - 1);
    const float coef = state_coef(state);
    const SumsqSource src = {part, c_part, cached};
    for (int s = t; s < S; s += kFinalThreads) trust_tensor(src, s, seg_item, nitems, hyper, eta, rec, coef, a, wsumsq, trust);
}

extern "C" int x3dstep_trust(const float* w, int64_t n, const X3DStepItem* items, const int32_t* seg_item, int64_t nitems,
                             const X3DStepHyper* hyper, const float* eta, int S, const int64_t* state, const void* ring, int R,
                             void* workspace, double* wsumsq, float* trust, float lr, float weight_decay, float grad_scale,
                             float eps, int clip, void* stream) {
    const int rc = x3dstep_check_trust("x3dstep_trust", w, n, items, seg_item, nitems, hyper, eta, S, state, ring, R, workspace,
                                       wsumsq, trust, eps, clip);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TrustArgs a = {lr, weight_decay, grad_scale, eps, clip};
    const int vec = ((uintptr_t)w & 15) == 0;
    double* part = (double*)workspace;
    x3dstep_trust_partials_kernel<<<item_grid(nitems), kItemThreads, 0, st>>>(w, n, items, nitems, S, state, part, vec);
    X3DSTEP_LAUNCH_CHECK();
    x3dstep_trust_finalize_kernel<<<1, kFinalThreads, 0, st>>>(seg_item, S, nitems, part, hyper, eta, state, ring, R, a, wsumsq,
                                                               trust);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

// x3dstep_apply_groups_kernel (group.hip) with the tensor's trust: the same decision, the same grid, the same walk.
__global__ __launch_bounds__(kItemThreads) void x3dstep_apply_lars_kernel(float* w, const float* g, float* m, int64_t n,
                                                                           const X3DStepItem* __restrict__ items,
                                                                           int64_t nitems,
                                                                           const X3DStepHyper* __restrict__ hyper,
                                                                           const float* __restrict__ trust, int S,
                                                                           int64_t* state, const void* ring, int R,
                                                                           SgdArgs a) {
    float coef = 1.0f;
    if (state && !apply_begin(state, ring, R, S, blockIdx.x == 0 && threadIdx.x == 0, &coef)) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    float t = 1.0f;
    const GroupItem c = lars_resolve(items, i, hyper, trust, S, n, a, &t);
    if (c.len > 0) group_lane<true>(w, g, m, c, threadIdx.x & (kLanes - 1), coef, a, t);
}

extern "C" int x3dstep_apply_lars(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                                  const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring, int R,
                                  float lr, float momentum, float weight_decay, float grad_scale, int first, int nesterov,
                                  void* stream) {
    const int rc = x3dstep_check_lars("x3dstep_apply_lars", w, g, m, n, items, nitems, hyper, trust, S, state, ring, R, momentum,
                                      first, nesterov);
    if (rc) return rc;
    const SgdArgs a = {lr, momentum, weight_decay, grad_scale, first, nesterov};
    x3dstep_apply_lars_kernel<<<item_grid(nitems), kItemThreads, 0, (hipStream_t)stream>>>(w, g, m, n, items, nitems, hyper,
                                                                                           trust, S, state, ring, R, a);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}
