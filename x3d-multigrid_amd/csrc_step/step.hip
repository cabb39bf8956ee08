// The kernels of libx3dstep (include/x3dstep.h) for gfx950: the three launches of x3dstep_observe -- partials (a wave per
// item), finalize (one workgroup: the record and the state) and scale --, the guarded update of x3dstep_apply and the copy
// of x3dstep_keep.  The arithmetic and the per-thread rules are step_core.h's, shared with the CPU twin.
#include <stdarg.h>
#include <stdio.h>

#include "step_core.h"

void x3dstep_set_error(const char* fmt, ...);  // step_host.cpp
int x3dstep_check_observe(const char* who, const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                          const int32_t* seg_item, int64_t nitems, const void* workspace, const int64_t* state,
                          const void* ring, int R);

using namespace x3ds;

constexpr int kPartThreads = kLanes * X3DSTEP_ITEMS_PER_GROUP;
constexpr int kScaleThreads = 256;
constexpr int kScaleMaxGroups = 1024;

// launch 1: wave w of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + w; lane 0 stores its three partials
__global__ __launch_bounds__(kPartThreads) void x3dstep_partials_kernel(const float* __restrict__ g,
                                                                         const int64_t* __restrict__ seg_off,
                                                                         const X3DStepItem* __restrict__ items,
                                                                         int64_t nitems, Scratch w, int vec) {
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;                       // the whole wave leaves: no shuffle below is left without its lanes
    const X3DStepItem it = items[i];
    const uint64_t first = (uint64_t)(it.start - seg_off[it.seg]);
    Part p = lane_part(g, it.start, it.len, first, lane, vec != 0);
    for (int off = kLanes / 2; off > 0; off >>= 1) {
        Part q;
        q.sumsq = __shfl_down(p.sumsq, off, kLanes);
        q.hash = __shfl_down((unsigned long long)p.hash, off, kLanes);
        q.nf = __shfl_down(p.nf, off, kLanes);
        part_merge(p, q);                          // lanes >= off add what they do not hand on: lane 0 holds the tree's sum
    }
    if (lane == 0) {
        w.sumsq[i] = p.sumsq;
        w.hash[i] = p.hash;
        w.nf[i] = p.nf;
    }
}

// The partials of the first kFinalCached items copied into LDS (one coalesced pass of the whole workgroup instead of one
// load latency per item of a thread's tensor: X3D-M's 2092 items all fit); later items are read from the scratch.
constexpr int kFinalCached = 2560;

struct CachedSource {
    Scratch w;
    const double* sumsq;
    const unsigned long long* hash;
    const int32_t* nf;
    int cached;
    __device__ inline int near_end(int a, int b) const { return b < cached ? b : (a > cached ? a : cached); }
    __device__ inline Part near(int i) const {
        const Part p = {sumsq[i], hash[i], nf[i]};
        return p;
    }
    __device__ inline Part far(int i) const {
        const Part p = {w.sumsq[i], w.hash[i], w.nf[i]};
        return p;
    }
};

// launch 2: one workgroup.  Thread t takes the tensors t, t + 1024, ..; thread 0 adds each round's sums in tensor order.
__global__ __launch_bounds__(kFinalThreads) void x3dstep_finalize_kernel(const int32_t* __restrict__ seg_item, int S,
                                                                          int64_t nitems, Scratch w, int64_t* state,
                                                                          void* ring, int R, double max_norm,
                                                                          double inv_world) {
    __shared__ double s_sumsq[kFinalThreads];
    __shared__ int32_t s_nf[kFinalThreads];
    __shared__ double c_sumsq[kFinalCached];
    __shared__ unsigned long long c_hash[kFinalCached];
    __shared__ int32_t c_nf[kFinalCached];
    const int t = threadIdx.x;
    const int64_t step = state[X3DSTEP_S_STEP];    // read by every thread before the first barrier, written after the last
    const Record r = record_at(ring, R, S, step);
    const int cached = nitems < kFinalCached ? (int)nitems : kFinalCached;
    for (int i = t; i < cached; i += kFinalThreads) {
        c_sumsq[i] = w.sumsq[i];
        c_hash[i] = w.hash[i];
        c_nf[i] = w.nf[i];
    }
    __syncthreads();
    const CachedSource src = {w, c_sumsq, c_hash, c_nf, cached};
    Sum total = {0.0, 0.0};
    int32_t nf = 0, first_bad = -1;
    for (int base = 0; base < S; base += kFinalThreads) {
        const int s = base + t;
        if (s < S) {
            const Part p = tensor_part(src, seg_item[s], seg_item[s + 1]);
            r.sumsq[s] = p.sumsq;
            r.hash[s] = p.hash;
            r.nf[s] = p.nf;
            s_sumsq[t] = p.sumsq;
            s_nf[t] = p.nf;
        }
        __syncthreads();
        if (t == 0) {
            const int cnt = S - base < kFinalThreads ? S - base : kFinalThreads;
            for (int k = 0; k < cnt; ++k) {
                sum_add(total, s_sumsq[k]);
                nf += s_nf[k];
                if (first_bad < 0 && s_nf[k] > 0) first_bad = base + k;
            }
        }
        __syncthreads();
    }
    if (t == 0) finish_step(r, state, step, S, sum_value(total), nf, first_bad, max_norm, inv_world);
}

// launch 3: g[i] = g[i] * coef, 16-byte groups where the address allows, the head and the tail element by element
__global__ __launch_bounds__(kScaleThreads) void x3dstep_scale_kernel(float* __restrict__ g, int64_t n,
                                                                       const int64_t* __restrict__ state) {
    const float coef = state_coef(state);
    if (coef == 1.0f) return;                      // the same bits either way
    int64_t head = (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int64_t groups = (n - head) >> 2;
    const int64_t tail = head + 4 * groups;
    const int64_t tid = (int64_t)blockIdx.x * kScaleThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kScaleThreads;
    Vec4* body = (Vec4*)(g + head);
    for (int64_t q = tid; q < groups; q += nthreads) {
        Vec4 x = body[q];
        for (int e = 0; e < 4; ++e) x.v[e] = scale_one(x.v[e], coef);
        body[q] = x;
    }
    if (tid < head) g[tid] = scale_one(g[tid], coef);
    if (tid < n - tail) g[tail + tid] = scale_one(g[tail + tid], coef);
}

#define X3DSTEP_LAUNCH_CHECK()                                                                                  \
    do {                                                                                                        \
        hipError_t e_ = hipGetLastError();                                                                      \
        if (e_ != hipSuccess) {                                                                                 \
            x3dstep_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_));           \
            return X3DSTEP_ELAUNCH;                                                                             \
        }                                                                                                       \
    } while (0)

// launches 1 and 2, what x3dstep_measure and x3dstep_observe share
static int enqueue_measure(const char* who, const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                           const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                           double max_norm, double inv_world, hipStream_t st) {
    const int rc = x3dstep_check_observe(who, g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R);
    if (rc) return rc;
    const Scratch w = scratch_at(workspace, nitems);
    const int vec = ((uintptr_t)g & 15) == 0;
    const unsigned grid1 = (unsigned)((nitems + X3DSTEP_ITEMS_PER_GROUP - 1) / X3DSTEP_ITEMS_PER_GROUP);
    x3dstep_partials_kernel<<<grid1, kPartThreads, 0, st>>>(g, seg_off, items, nitems, w, vec);
    X3DSTEP_LAUNCH_CHECK();
    x3dstep_finalize_kernel<<<1, kFinalThreads, 0, st>>>(seg_item, S, nitems, w, state, ring, R, max_norm, inv_world);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

extern "C" int x3dstep_measure(const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                               const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                               double max_norm, double inv_world, void* stream) {
    return enqueue_measure("x3dstep_measure", g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R, max_norm,
                           inv_world, (hipStream_t)stream);
}

extern "C" int x3dstep_observe(float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                               const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                               double max_norm, double inv_world, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int rc = enqueue_measure("x3dstep_observe", g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R,
                                   max_norm, inv_world, st);
    if (rc) return rc;
    if (max_norm > 0.0) {
        int64_t blocks = ((n >> 2) + kScaleThreads) / kScaleThreads;
        if (blocks > kScaleMaxGroups) blocks = kScaleMaxGroups;
        x3dstep_scale_kernel<<<(unsigned)blocks, kScaleThreads, 0, st>>>(g, n, state);
        X3DSTEP_LAUNCH_CHECK();
    }
    return X3DSTEP_OK;
}

// The guarded update.  Unit: a 16-byte group (Vec4, the buffers moved past their head) or an element (float); a workgroup
// takes a run of kApplyThreads * kApplyPieces units and a lane its kApplyPieces units kApplyThreads apart, so that a wave
// reads whole 1 KB runs; its loads of w, g and m (3 * kApplyPieces independent ones) are issued before its first store.
// The decision is read by every thread: the loads are uniform over the grid, and a skipped step costs one wave's latency.
constexpr int kApplyThreads = 256;
constexpr int kApplyPieces = 4;
constexpr int64_t kApplyRun = (int64_t)kApplyThreads * kApplyPieces;

__device__ inline void apply_unit(Vec4& w, const Vec4& g, Vec4& m, float coef, const ApplyArgs& a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) apply_one(w.v[e], g.v[e], m.v[e], coef, a);
}
__device__ inline void apply_unit(float& w, const float& g, float& m, float coef, const ApplyArgs& a) {
    apply_one(w, g, m, coef, a);
}

template <class Unit>
__global__ __launch_bounds__(kApplyThreads) void x3dstep_apply_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                                       float* __restrict__ m, int64_t n, ApplyPlan plan,
                                                                       int64_t* state, const void* __restrict__ ring, int R,
                                                                       int S, ApplyArgs a) {
    const Decision d = apply_decision(state, ring, R, S);
    if (!d.go) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) apply_counters(state, d.skip);   // words no thread of the grid reads above
    if (d.skip) return;
    constexpr bool kVec = sizeof(Unit) == 16;
    const int64_t units = kVec ? plan.groups : n;
    const int64_t shift = kVec ? plan.head : 0;
    Unit* wu = (Unit*)(w + shift);
    const Unit* gu = (const Unit*)(g + shift);
    Unit* mu = (Unit*)(m + shift);
    const int64_t at0 = (int64_t)blockIdx.x * kApplyRun + threadIdx.x;
    Unit wv[kApplyPieces], gv[kApplyPieces], mv[kApplyPieces];
#pragma unroll
    for (int k = 0; k < kApplyPieces; ++k) {
        const int64_t at = at0 + (int64_t)k * kApplyThreads;
        if (at < units) {
            wv[k] = wu[at];
            gv[k] = gu[at];
            mv[k] = mu[at];
        }
    }
#pragma unroll
    for (int k = 0; k < kApplyPieces; ++k) {
        const int64_t at = at0 + (int64_t)k * kApplyThreads;
        if (at < units) {
            apply_unit(wv[k], gv[k], mv[k], d.coef, a);
            mu[at] = mv[k];
            wu[at] = wv[k];
        }
    }
    if (kVec && blockIdx.x == 0) {                 // at most three elements before the groups and three after
        const int64_t t = threadIdx.x;
        if (t < plan.head) apply_one(w[t], g[t], m[t], d.coef, a);
        if (t < n - plan.tail) apply_one(w[plan.tail + t], g[plan.tail + t], m[plan.tail + t], d.coef, a);
    }
}

int x3dstep_check_apply(const char* who, const float* w, const float* g, const float* m, int64_t n, const int64_t* state,
                        const void* ring, int R, int S);
int x3dstep_check_keep(const char* who, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                       const float* snap, int64_t snap_n, const int64_t* state, int mode);

extern "C" int x3dstep_apply(float* w, const float* g, float* m, int64_t n, int64_t* state, const void* ring, int R, int S,
                             float lr, float momentum, float weight_decay, float grad_scale, int first, void* stream) {
    const int rc = x3dstep_check_apply("x3dstep_apply", w, g, m, n, state, ring, R, S);
    if (rc) return rc;
    const ApplyPlan plan = apply_plan(w, g, m, n);
    const ApplyArgs a = {lr, momentum, weight_decay, grad_scale, first ? 1 : 0};
    hipStream_t st = (hipStream_t)stream;
    if (plan.vec) {
        const int64_t blocks = plan.groups > 0 ? (plan.groups + kApplyRun - 1) / kApplyRun : 1;
        x3dstep_apply_kernel<Vec4><<<(unsigned)blocks, kApplyThreads, 0, st>>>(w, g, m, n, plan, state, ring, R, S, a);
    } else {
        const int64_t blocks = (n + kApplyRun - 1) / kApplyRun;
        x3dstep_apply_kernel<float><<<(unsigned)blocks, kApplyThreads, 0, st>>>(w, g, m, n, plan, state, ring, R, S, a);
    }
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

// keep: wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v.  A restore reads the skip word first: uniform.
__global__ __launch_bounds__(kPartThreads) void x3dstep_keep_kernel(const X3DStepKeep* __restrict__ table, int nbuf,
                                                                     const X3DStepItem* __restrict__ items, int64_t nitems,
                                                                     float* snap, int64_t snap_n,
                                                                     const int64_t* __restrict__ state, int mode) {
    if (mode == X3DSTEP_KEEP_RESTORE && state[X3DSTEP_S_SKIP] != 1) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    bool bad;
    const KeepCopy c = keep_resolve(table, nbuf, items, i, snap, snap_n, mode, &bad);
    if (c.len > 0) keep_lane(c, threadIdx.x & (kLanes - 1));
}

extern "C" int x3dstep_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                            int64_t snap_n, const int64_t* state, int mode, void* stream) {
    const int rc = x3dstep_check_keep("x3dstep_keep", table, nbuf, items, nitems, snap, snap_n, state, mode);
    if (rc) return rc;
    const unsigned grid = (unsigned)((nitems + X3DSTEP_ITEMS_PER_GROUP - 1) / X3DSTEP_ITEMS_PER_GROUP);
    x3dstep_keep_kernel<<<grid, kPartThreads, 0, (hipStream_t)stream>>>(table, nbuf, items, nitems, snap, snap_n, state, mode);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}
