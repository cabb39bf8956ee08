// Second-moment updates of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_adam (Adam with L2 and AdamW, one launch) and
// LAMB in three launches -- x3dstep_lamb_moments (the moments and, per item, the fp64 sums of squares of the direction and
// of the weights), x3dstep_lamb_trust (one workgroup: the per-tensor sums and |w| / |r|) and x3dstep_lamb_apply (the step
// along the direction, recomputed from the stored moments).  The walk of a lane is group.hip's (rule_lane of step_core.h)
// with one more buffer; the decision, count, correction, tensor and element rules and the per-item and per-tensor tests
// are step_core.h's, shared with the CPU twins.  No float atomics, no allocation, no synchronisation.
#include "step_priv.h"

using namespace x3ds;

// wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v.  Every thread reads the decision and the count first
// (uniform loads); thread 0 of workgroup 0 writes the three counters, words no other thread of an applied update reads.
__global__ __launch_bounds__(kItemThreads) void x3dstep_adam_kernel(float* w, const float* g, float* m, float* v, int64_t n,
                                                                     const X3DStepItem* __restrict__ items, int64_t nitems,
                                                                     const X3DStepHyper* __restrict__ hyper, int S,
                                                                     int64_t* state, const void* ring, int R, int64_t count,
                                                                     AdamArgs a) {
    float coef;
    int64_t k;
    if (!adam_begin(state, ring, R, S, count, blockIdx.x == 0 && threadIdx.x == 0, &coef, &k)) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    const SgdArgs sa = {a.lr, 0.0f, a.wd, a.gs, 0, 0};
    const GroupItem c = group_resolve(items, i, hyper, S, n, sa);
    if (c.len < 1) return;
    const AdamCorr corr = adam_corr(k, a.b1, a.b2);
    const AdamRule rule = {a, corr, coef, c.wd_s, adam_step_size(c.lr_s, corr), c.lr_s * c.wd_s};
    float* const base[4] = {w, (float*)g, m, v};
    rule_lane(rule, base, c.start, c.len, threadIdx.x & (kLanes - 1));
}

extern "C" int x3dstep_adam(float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items, int64_t nitems,
                            const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R, int64_t count, float lr,
                            float b1, float b2, float eps, float weight_decay, float grad_scale, int decoupled, void* stream) {
    const int rc = x3dstep_check_adam("x3dstep_adam", w, g, m, v, true, n, items, nitems, hyper, S, state, ring, R, count, b1,
                                      b2, eps, decoupled);
    if (rc) return rc;
    const AdamArgs a = {lr, b1, b2, eps, weight_decay, grad_scale, decoupled};
    x3dstep_adam_kernel<<<item_grid(nitems), kItemThreads, 0, (hipStream_t)stream>>>(w, g, m, v, n, items, nitems, hyper, S,
                                                                                     state, ring, R, count, a);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

// LAMB, launch 1.  The wave first adds the squares of the direction and of the weights from what it loads (nothing is
// stored yet: the lanes of the sums are lane_part's, those of the walk rule_lane's), then walks the item and stores the
// moments.  It writes no state word.
__global__ __launch_bounds__(kItemThreads) void x3dstep_lamb_moments_kernel(const float* w, const float* g, float* m, float* v,
                                                                             int64_t n, const X3DStepItem* __restrict__ items,
                                                                             int64_t nitems,
                                                                             const X3DStepHyper* __restrict__ hyper, int S,
                                                                             const int64_t* state, const void* ring, int R,
                                                                             int64_t count, AdamArgs a,
                                                                             double* __restrict__ rpart,
                                                                             double* __restrict__ wpart, int vec) {
    float coef;
    int64_t k;
    if (!adam_begin((int64_t*)state, ring, R, S, count, false, &coef, &k)) return;
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;                       // the whole wave leaves: no shuffle below is left without its lanes
    const SgdArgs sa = {0.0f, 0.0f, a.wd, a.gs, 0, 0};
    const GroupItem c = group_resolve(items, i, hyper, S, n, sa);      // the same in every lane of the wave
    const LambMomentsRule rule = {a, adam_corr(k, a.b1, a.b2), coef};
    LambSums s = {trust_nan(), trust_nan()};
    if (c.len > 0) s = lamb_lane_sums(w, g, m, v, c, lane, vec != 0, rule);
    for (int off = kLanes / 2; off > 0; off >>= 1) {
        s.r = s.r + __shfl_down(s.r, off, kLanes);
        s.w = s.w + __shfl_down(s.w, off, kLanes);
    }
    if (lane == 0) {
        rpart[i] = s.r;
        wpart[i] = s.w;
    }
    if (c.len < 1) return;
    // every load of the sums has returned (the shuffles needed them); the fence keeps the walk's stores behind them
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    float* const base[3] = {(float*)g, m, v};
    rule_lane(rule, base, c.start, c.len, lane);
}

// The partials of the first kLambCached items copied into LDS, as the finalize step of x3dstep_trust does: two arrays.
constexpr int kLambCached = 2560;

// LAMB, launch 2: one workgroup.  Thread t takes the tensors t, t + 1024, ..: the sums of the tensor's items and its ratio.
__global__ __launch_bounds__(kFinalThreads) void x3dstep_lamb_trust_kernel(const int32_t* __restrict__ seg_item, int S,
                                                                            int64_t nitems, const double* __restrict__ rpart,
                                                                            const double* __restrict__ wpart,
                                                                            const X3DStepHyper* __restrict__ hyper,
                                                                            const uint8_t* __restrict__ adapt,
                                                                            const int64_t* __restrict__ state,
                                                                            const void* ring, int R, int64_t count,
                                                                            double* __restrict__ wsumsq,
                                                                            double* __restrict__ rsumsq,
                                                                            float* __restrict__ trust) {
    __shared__ double c_r[kLambCached];
    __shared__ double c_w[kLambCached];
    float coef;
    int64_t k;
    if (!adam_begin((int64_t*)state, ring, R, S, count, false, &coef, &k)) return;      // uniform: before the barrier
    const int32_t* nf = state ? record_at((void*)ring, R, S, state[X3DSTEP_S_STEP] - 1).nf : nullptr;
    const int t = threadIdx.x;
    const int cached = nitems < kLambCached ? (int)nitems : kLambCached;
    for (int i = t; i < cached; i += kFinalThreads) {
        c_r[i] = rpart[i];
        c_w[i] = wpart[i];
    }
    __syncthreads();
    const SumsqSource rsrc = {rpart, c_r, cached};
    const SumsqSource wsrc = {wpart, c_w, cached};
    for (int s = t; s < S; s += kFinalThreads)
        lamb_tensor(rsrc, wsrc, s, seg_item, nitems, hyper, adapt, nf, wsumsq, rsumsq, trust);
}

// LAMB, launch 3: x3dstep_adam_kernel's decision, grid and walk over w, m, v with the tensor's trust.
__global__ __launch_bounds__(kItemThreads) void x3dstep_lamb_apply_kernel(float* w, const float* m, const float* v, int64_t n,
                                                                           const X3DStepItem* __restrict__ items,
                                                                           int64_t nitems,
                                                                           const X3DStepHyper* __restrict__ hyper,
                                                                           const float* __restrict__ trust, int S,
                                                                           int64_t* state, const void* ring, int R,
                                                                           int64_t count, AdamArgs a) {
    float coef;
    int64_t k;
    if (!adam_begin(state, ring, R, S, count, blockIdx.x == 0 && threadIdx.x == 0, &coef, &k)) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    const SgdArgs sa = {a.lr, 0.0f, a.wd, a.gs, 0, 0};
    float t = 1.0f;
    const GroupItem c = lars_resolve(items, i, hyper, trust, S, n, sa, &t);
    if (c.len < 1) return;
    const LambApplyRule rule = {a, adam_corr(k, a.b1, a.b2), c.wd_s, c.lr_s * t};
    float* const base[3] = {w, (float*)m, (float*)v};
    rule_lane(rule, base, c.start, c.len, threadIdx.x & (kLanes - 1));
}

extern "C" int x3dstep_lamb_moments(const float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items,
                                    int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state, const void* ring,
                                    int R, int64_t count, float b1, float b2, float eps, float weight_decay, float grad_scale,
                                    void* workspace, void* stream) {
    const char* who = "x3dstep_lamb_moments";
    const int rc = x3dstep_check_lamb_moments(who, w, g, m, v, n, items, nitems, hyper, S, state, ring, R, count, b1, b2, eps,
                                              workspace);
    if (rc) return rc;
    const AdamArgs a = {0.0f, b1, b2, eps, weight_decay, grad_scale, 1};
    const int vec = (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    double* rpart = (double*)workspace;
    x3dstep_lamb_moments_kernel<<<item_grid(nitems), kItemThreads, 0, (hipStream_t)stream>>>(
        w, g, m, v, n, items, nitems, hyper, S, state, ring, R, count, a, rpart, rpart + nitems, vec);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

extern "C" int x3dstep_lamb_trust(const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper, const uint8_t* adapt,
                                  int S, const int64_t* state, const void* ring, int R, int64_t count, const void* workspace,
                                  double* wsumsq, double* rsumsq, float* trust, void* stream) {
    const char* who = "x3dstep_lamb_trust";
    const int rc = x3dstep_check_lamb_trust(who, seg_item, nitems, hyper, adapt, S, state, ring, R, count, workspace, wsumsq,
                                            rsumsq, trust);
    if (rc) return rc;
    const double* rpart = (const double*)workspace;
    x3dstep_lamb_trust_kernel<<<1, kFinalThreads, 0, (hipStream_t)stream>>>(seg_item, S, nitems, rpart, rpart + nitems, hyper,
                                                                            adapt, state, ring, R, count, wsumsq, rsumsq,
                                                                            trust);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

extern "C" int x3dstep_lamb_apply(float* w, const float* m, const float* v, int64_t n, const X3DStepItem* items,
                                  int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S, int64_t* state,
                                  const void* ring, int R, int64_t count, float lr, float b1, float b2, float eps,
                                  float weight_decay, void* stream) {
    const char* who = "x3dstep_lamb_apply";
    const int rc = x3dstep_check_lamb_apply(who, w, m, v, n, items, nitems, hyper, trust, S, state, ring, R, count, b1, b2, eps);
    if (rc) return rc;
    const AdamArgs a = {lr, b1, b2, eps, weight_decay, 1.0f, 1};
    x3dstep_lamb_apply_kernel<<<item_grid(nitems), kItemThreads, 0, (hipStream_t)stream>>>(w, m, v, n, items, nitems, hyper,
                                                                                           trust, S, state, ring, R, count, a);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}
