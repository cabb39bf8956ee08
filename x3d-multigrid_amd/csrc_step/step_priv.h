// What the translation units of libx3dstep share beside the arithmetic of step_core.h: the error text and the argument
// checks of step_host.cpp, the grid of a wave-per-item launch and, for the .hip files, the launch check and the kernels of
// the two walks -- the flat walk (a run of units per workgroup) and the item walk (a wave per item of a keep table) --
// which the entry points instantiate with an element operation of step_core.h.
#pragma once
#include "step_core.h"

void x3dstep_set_error(const char* fmt, ...);

// the argument checks an entry point and its twin share (no pointer is followed: the tables may be device memory)
int x3dstep_check_observe(const char* who, const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                          const int32_t* seg_item, int64_t nitems, const void* workspace, const int64_t* state,
                          const void* ring, int R);
int x3dstep_check_apply(const char* who, const float* w, const float* g, const float* m, int64_t n, const int64_t* state,
                        const void* ring, int R, int S);
int x3dstep_check_groups(const char* who, const float* w, const float* g, const float* m, int64_t n, const X3DStepItem* items,
                         int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state, const void* ring, int R,
                         float momentum, int first, int nesterov);
// x3dstep_check_groups and the trust table
int x3dstep_check_lars(const char* who, const float* w, const float* g, const float* m, int64_t n, const X3DStepItem* items,
                       int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S, const int64_t* state,
                       const void* ring, int R, float momentum, int first, int nesterov);
int x3dstep_check_trust(const char* who, const float* w, int64_t n, const X3DStepItem* items, const int32_t* seg_item,
                        int64_t nitems, const X3DStepHyper* hyper, const float* eta, int S, const int64_t* state,
                        const void* ring, int R, const void* workspace, const double* wsumsq, const float* trust, float eps,
                        int clip);
// The second-moment updates: the pointer, size and table checks of x3dstep_check_groups over w, g (need_g: x3dstep_lamb_apply
// has none), m and v, then b1, b2, eps, decoupled and, without a state, the count
int x3dstep_check_adam(const char* who, const float* w, const float* g, const float* m, const float* v, bool need_g, int64_t n,
                       const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state,
                       const void* ring, int R, int64_t count, float b1, float b2, float eps, int decoupled);
int x3dstep_check_lamb_moments(const char* who, const float* w, const float* g, const float* m, const float* v, int64_t n,
                               const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper, int S,
                               const int64_t* state, const void* ring, int R, int64_t count, float b1, float b2, float eps,
                               const void* workspace);
int x3dstep_check_lamb_trust(const char* who, const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper,
                             const uint8_t* adapt, int S, const int64_t* state, const void* ring, int R, int64_t count,
                             const void* workspace, const double* wsumsq, const double* rsumsq, const float* trust);
int x3dstep_check_lamb_apply(const char* who, const float* w, const float* m, const float* v, int64_t n,
                             const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S,
                             const int64_t* state, const void* ring, int R, int64_t count, float b1, float b2, float eps);
int x3dstep_check_ema(const char* who, const float* e, const float* w, int64_t n, const int64_t* state, float decay);
int x3dstep_check_swap(const char* who, const float* a, const float* b, int64_t n);
// need_state: x3dstep_keep, which reads the state whatever the mode; the others pass X3DSTEP_KEEP_SAVE, x3dstep_swap_keep
// decay 0
int x3dstep_check_table(const char* who, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                        const float* snap, int64_t snap_n, const int64_t* state, bool need_state, int mode, float decay);
int x3dstep_check_pbn(const char* who, const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                      const double* acc, bool finish, int W, int64_t expect_n, const float* snap, int64_t snap_n);

namespace x3ds {

constexpr int kItemThreads = kLanes * X3DSTEP_ITEMS_PER_GROUP;

// workgroups of a launch in which wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v
static inline unsigned item_grid(int64_t nitems) {
    return (unsigned)((nitems + X3DSTEP_ITEMS_PER_GROUP - 1) / X3DSTEP_ITEMS_PER_GROUP);
}

}  // namespace x3ds

#if defined(__HIPCC__)
#define X3DSTEP_LAUNCH_CHECK()                                                                                  \
    do {                                                                                                        \
        hipError_t e_ = hipGetLastError();                                                                      \
        if (e_ != hipSuccess) {                                                                                 \
            x3dstep_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_));           \
            return X3DSTEP_ELAUNCH;                                                                             \
        }                                                                                                       \
    } while (0)

namespace x3ds {

// The flat walk.  Unit: a 16-byte group (the buffers moved past their head) or an element; a workgroup takes a run of
// kFlatThreads * kFlatPieces units and a lane its kFlatPieces units kFlatThreads apart, so that a wave reads whole 1 KB
// runs; a lane's loads of all buffers (kBufs * kFlatPieces independent ones) are issued before its first store.  What
// begin() reads is read by every thread: the loads are uniform over the grid, and a launch that does nothing costs one
// wave's latency.
constexpr int kFlatThreads = 256;
constexpr int kFlatPieces = 4;
constexpr int64_t kFlatRun = (int64_t)kFlatThreads * kFlatPieces;

template <class Op, class Unit>
__global__ __launch_bounds__(kFlatThreads) void x3dstep_flat_kernel(Bufs<Op> bufs, int64_t n, Plan plan, Op op) {
    if (!op.begin(blockIdx.x == 0 && threadIdx.x == 0)) return;
    constexpr bool kVec = sizeof(Unit) == 16;
    const int64_t units = kVec ? plan.groups : n;
    Unit* u[Op::kBufs];
#pragma unroll
    for (int b = 0; b < Op::kBufs; ++b) u[b] = (Unit*)(bufs.p[b] + (kVec ? plan.head : 0));
    const int64_t at0 = (int64_t)blockIdx.x * kFlatRun + threadIdx.x;
    Unit v[kFlatPieces][Op::kBufs];
#pragma unroll
    for (int k = 0; k < kFlatPieces; ++k) {
        const int64_t at = at0 + (int64_t)k * kFlatThreads;
        if (at < units) {
#pragma unroll
            for (int b = 0; b < Op::kBufs; ++b)
                if (Op::kLoads >> b & 1) v[k][b] = u[b][at];
        }
    }
#pragma unroll
    for (int k = 0; k < kFlatPieces; ++k) {
        const int64_t at = at0 + (int64_t)k * kFlatThreads;
        if (at < units) {
            walk_unit(op, v[k]);
#pragma unroll
            for (int b = 0; b < Op::kBufs; ++b)
                if (Op::kStores >> b & 1) u[b][at] = v[k][b];
        }
    }
    if (kVec && blockIdx.x == 0) {                 // at most three elements before the groups and three after
        const int64_t t = threadIdx.x;
        if (t < plan.head) walk_at(op, bufs.p, t);
        if (t < n - plan.tail) walk_at(op, bufs.p, plan.tail + t);
    }
}

template <class Op>
static int launch_flat(const Op& op, const Bufs<Op>& bufs, int64_t n, void* stream) {
    const Plan plan = flat_plan(bufs, n);
    const int64_t units = plan.vec ? plan.groups : n;
    const unsigned blocks = (unsigned)(units > 0 ? (units + kFlatRun - 1) / kFlatRun : 1);
    if (plan.vec)
        x3dstep_flat_kernel<Op, typename Op::Group><<<blocks, kFlatThreads, 0, (hipStream_t)stream>>>(bufs, n, plan, op);
    else
        x3dstep_flat_kernel<Op, typename Op::Elem><<<blocks, kFlatThreads, 0, (hipStream_t)stream>>>(bufs, n, plan, op);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

// The item walk: wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v of a keep table; op.mode says which end
// of the item is buffer 0 (keep_resolve).  The per-item tests are keep_resolve's.
template <class Op>
__global__ __launch_bounds__(kItemThreads) void x3dstep_item_kernel(const X3DStepKeep* __restrict__ table, int nbuf,
                                                                     const X3DStepItem* __restrict__ items, int64_t nitems,
                                                                     float* snap, int64_t snap_n, Op op) {
    if (!op.begin(false)) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    bool bad;
    const KeepCopy c = keep_resolve(table, nbuf, items, i, snap, snap_n, op.mode, &bad);
    if (c.len > 0) item_lane(op, c, threadIdx.x & (kLanes - 1));
}

template <class Op>
static int launch_items(const Op& op, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                        float* snap, int64_t snap_n, void* stream) {
    x3dstep_item_kernel<Op><<<item_grid(nitems), kItemThreads, 0, (hipStream_t)stream>>>(table, nbuf, items, nitems, snap,
                                                                                         snap_n, op);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

}  // namespace x3ds
#endif
