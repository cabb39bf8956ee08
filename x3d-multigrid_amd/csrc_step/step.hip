// The kernels of libx3dstep (include/x3dstep.h) for gfx950: the three launches of x3dstep_observe -- partials (a wave per
// item), finalize (one workgroup: the record and the state) and scale --, the guarded update of x3dstep_apply (the flat
// walk of step_priv.h) and the copy of x3dstep_keep (its item walk).  The arithmetic and the per-thread rules are
// step_core.h's, shared with the CPU twin.
#include "step_priv.h"

using namespace x3ds;

constexpr int kScaleThreads = 256;
constexpr int kScaleMaxGroups = 1024;

// launch 1: wave w of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + w; lane 0 stores its three partials
__global__ __launch_bounds__(kItemThreads) void x3dstep_partials_kernel(const float* __restrict__ g,
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
    const Plan p = walk_plan(mod16(g), true, n);
    const int64_t tid = (int64_t)blockIdx.x * kScaleThreads + threadIdx.x;
    const int64_t nthreads = (int64_t)gridDim.x * kScaleThreads;
    Vec4* body = (Vec4*)(g + p.head);
    for (int64_t q = tid; q < p.groups; q += nthreads) {
        Vec4 x = body[q];
        for (int e = 0; e < 4; ++e) x.v[e] = scale_one(x.v[e], coef);
        body[q] = x;
    }
    if (tid < p.head) g[tid] = scale_one(g[tid], coef);
    if (tid < n - p.tail) g[p.tail + tid] = scale_one(g[p.tail + tid], coef);
}

// launches 1 and 2, what x3dstep_measure and x3dstep_observe share
static int enqueue_measure(const char* who, const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                           const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                           double max_norm, double inv_world, hipStream_t st) {
    const int rc = x3dstep_check_observe(who, g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R);
    if (rc) return rc;
    const Scratch w = scratch_at(workspace, nitems);
    const int vec = ((uintptr_t)g & 15) == 0;
    x3dstep_partials_kernel<<<item_grid(nitems), kItemThreads, 0, st>>>(g, seg_off, items, nitems, w, vec);
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

// the guarded update: the flat walk over w, g, m
extern "C" int x3dstep_apply(float* w, const float* g, float* m, int64_t n, int64_t* state, const void* ring, int R, int S,
                             float lr, float momentum, float weight_decay, float grad_scale, int first, void* stream) {
    const int rc = x3dstep_check_apply("x3dstep_apply", w, g, m, n, state, ring, R, S);
    if (rc) return rc;
    const ApplyOp op = {state, ring, R, S, {lr, momentum, weight_decay, grad_scale, first ? 1 : 0, 0}, 1.0f};
    return launch_flat(op, Bufs<ApplyOp>{{w, (float*)g, m}}, n, stream);
}

// keep: the item walk, a copy; a restore reads the skip word first (uniform)
extern "C" int x3dstep_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                            int64_t snap_n, const int64_t* state, int mode, void* stream) {
    const int rc = x3dstep_check_table("x3dstep_keep", table, nbuf, items, nitems, snap, snap_n, state, true, mode, 0.0f);
    if (rc) return rc;
    return launch_items(CopyOp{state, mode}, table, nbuf, items, nitems, snap, snap_n, stream);
}
