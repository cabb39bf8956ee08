// The weight average of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_ema and x3dstep_swap over flat buffers (shaped
// like x3dstep_apply), x3dstep_ema_keep and x3dstep_swap_keep over a keep table (shaped like x3dstep_keep: a wave per
// item).  The count, skip, decay and element rules are step_core.h's, shared with the CPU twins.  The EMA launches read the
// state and never write it; no LDS, no atomics, no allocation, no synchronisation.
#include "step_core.h"

void x3dstep_set_error(const char* fmt, ...);  // step_host.cpp
int x3dstep_check_ema(const char* who, const float* e, const float* w, int64_t n, const int64_t* state, float decay);
int x3dstep_check_swap(const char* who, const float* a, const float* b, int64_t n);
int x3dstep_check_table(const char* who, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                        const float* snap, int64_t snap_n, const int64_t* state, float decay);

using namespace x3ds;

#define X3DSTEP_LAUNCH_CHECK()                                                                                  \
    do {                                                                                                        \
        hipError_t e_ = hipGetLastError();                                                                      \
        if (e_ != hipSuccess) {                                                                                 \
            x3dstep_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_));           \
            return X3DSTEP_ELAUNCH;                                                                             \
        }                                                                                                       \
    } while (0)

// Unit: a 16-byte group (the buffers moved past their head) or an element; a workgroup takes a run of kPairThreads *
// kPairPieces units and a lane its kPairPieces units kPairThreads apart (a wave reads whole 1 KB runs); a lane's loads of
// both buffers are issued before its first store.
constexpr int kPairThreads = 256;
constexpr int kPairPieces = 4;
constexpr int64_t kPairRun = (int64_t)kPairThreads * kPairPieces;
constexpr int kItemThreads = kLanes * X3DSTEP_ITEMS_PER_GROUP;

__device__ inline void ema_unit(Vec4& e, const Vec4& w, const EmaCoef& c) {
#pragma unroll
    for (int x = 0; x < 4; ++x) ema_one(e.v[x], w.v[x], c);
}
__device__ inline void ema_unit(float& e, const float& w, const EmaCoef& c) { ema_one(e, w, c); }

// Every thread reads the three state words (uniform loads) and derives k and the two coefficients itself.
template <class Unit>
__global__ __launch_bounds__(kPairThreads) void x3dstep_ema_kernel(float* __restrict__ e, const float* __restrict__ w,
                                                                    int64_t n, ApplyPlan plan,
                                                                    const int64_t* __restrict__ state, int64_t count,
                                                                    float decay, int warmup) {
    if (ema_skips(state)) return;
    const int64_t k = ema_count(state, count);
    if (k <= 0) return;
    const EmaCoef c = ema_coef(k, decay, warmup);
    constexpr bool kVec = sizeof(Unit) == 16;
    const int64_t units = kVec ? plan.groups : n;
    const int64_t shift = kVec ? plan.head : 0;
    Unit* eu = (Unit*)(e + shift);
    const Unit* wu = (const Unit*)(w + shift);
    const int64_t at0 = (int64_t)blockIdx.x * kPairRun + threadIdx.x;
    Unit ev[kPairPieces], wv[kPairPieces];
#pragma unroll
    for (int i = 0; i < kPairPieces; ++i) {
        const int64_t at = at0 + (int64_t)i * kPairThreads;
        if (at < units) {
            ev[i] = eu[at];
            wv[i] = wu[at];
        }
    }
#pragma unroll
    for (int i = 0; i < kPairPieces; ++i) {
        const int64_t at = at0 + (int64_t)i * kPairThreads;
        if (at < units) {
            ema_unit(ev[i], wv[i], c);
            eu[at] = ev[i];
        }
    }
    if (kVec && blockIdx.x == 0) {                 // at most three elements before the groups and three after
        const int64_t t = threadIdx.x;
        if (t < plan.head) ema_one(e[t], w[t], c);
        if (t < n - plan.tail) ema_one(e[plan.tail + t], w[plan.tail + t], c);
    }
}

static unsigned pair_blocks(const ApplyPlan& plan, int64_t n) {
    const int64_t units = plan.vec ? plan.groups : n;
    return (unsigned)(units > 0 ? (units + kPairRun - 1) / kPairRun : 1);
}

extern "C" int x3dstep_ema(float* e, const float* w, int64_t n, const int64_t* state, int64_t count, float decay, int warmup,
                           void* stream) {
    const int rc = x3dstep_check_ema("x3dstep_ema", e, w, n, state, decay);
    if (rc) return rc;
    const ApplyPlan plan = pair_plan(e, w, n);
    hipStream_t st = (hipStream_t)stream;
    if (plan.vec)
        x3dstep_ema_kernel<Vec4><<<pair_blocks(plan, n), kPairThreads, 0, st>>>(e, w, n, plan, state, count, decay,
                                                                                 warmup ? 1 : 0);
    else
        x3dstep_ema_kernel<float><<<pair_blocks(plan, n), kPairThreads, 0, st>>>(e, w, n, plan, state, count, decay,
                                                                                  warmup ? 1 : 0);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

// wave v of workgroup b takes item b * X3DSTEP_ITEMS_PER_GROUP + v; the per-item tests are x3dstep_keep's
__global__ __launch_bounds__(kItemThreads) void x3dstep_ema_keep_kernel(const X3DStepKeep* __restrict__ table, int nbuf,
                                                                         const X3DStepItem* __restrict__ items,
                                                                         int64_t nitems, float* esnap, int64_t snap_n,
                                                                         const int64_t* __restrict__ state, int64_t count,
                                                                         float decay, int warmup) {
    if (ema_skips(state)) return;
    const int64_t k = ema_count(state, count);
    if (k <= 0) return;
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    bool bad;
    const KeepCopy c = keep_resolve(table, nbuf, items, i, esnap, snap_n, X3DSTEP_KEEP_SAVE, &bad);
    if (c.len > 0) ema_lane(c, threadIdx.x & (kLanes - 1), ema_coef(k, decay, warmup));
}

extern "C" int x3dstep_ema_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* esnap,
                                int64_t snap_n, const int64_t* state, int64_t count, float decay, int warmup, void* stream) {
    const int rc = x3dstep_check_table("x3dstep_ema_keep", table, nbuf, items, nitems, esnap, snap_n, state, decay);
    if (rc) return rc;
    const unsigned grid = (unsigned)((nitems + X3DSTEP_ITEMS_PER_GROUP - 1) / X3DSTEP_ITEMS_PER_GROUP);
    x3dstep_ema_keep_kernel<<<grid, kItemThreads, 0, (hipStream_t)stream>>>(table, nbuf, items, nitems, esnap, snap_n, state,
                                                                            count, decay, warmup ? 1 : 0);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

// the exchange of two flat buffers: the same walk on bits
template <class Unit>
__global__ __launch_bounds__(kPairThreads) void x3dstep_swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                                                     int64_t n, ApplyPlan plan) {
    constexpr bool kVec = sizeof(Unit) == 16;
    const int64_t units = kVec ? plan.groups : n;
    const int64_t shift = kVec ? plan.head : 0;
    Unit* au = (Unit*)(a + shift);
    Unit* bu = (Unit*)(b + shift);
    const int64_t at0 = (int64_t)blockIdx.x * kPairRun + threadIdx.x;
    Unit av[kPairPieces], bv[kPairPieces];
#pragma unroll
    for (int i = 0; i < kPairPieces; ++i) {
        const int64_t at = at0 + (int64_t)i * kPairThreads;
        if (at < units) {
            av[i] = au[at];
            bv[i] = bu[at];
        }
    }
#pragma unroll
    for (int i = 0; i < kPairPieces; ++i) {
        const int64_t at = at0 + (int64_t)i * kPairThreads;
        if (at < units) {
            au[at] = bv[i];
            bu[at] = av[i];
        }
    }
    if (kVec && blockIdx.x == 0) {
        const int64_t t = threadIdx.x;
        if (t < plan.head) swap_one(a[t], b[t]);
        if (t < n - plan.tail) swap_one(a[plan.tail + t], b[plan.tail + t]);
    }
}

extern "C" int x3dstep_swap(float* a, float* b, int64_t n, void* stream) {
    const int rc = x3dstep_check_swap("x3dstep_swap", a, b, n);
    if (rc) return rc;
    const ApplyPlan plan = pair_plan(a, b, n);
    hipStream_t st = (hipStream_t)stream;
    if (plan.vec)
        x3dstep_swap_kernel<Bits4><<<pair_blocks(plan, n), kPairThreads, 0, st>>>((uint32_t*)a, (uint32_t*)b, n, plan);
    else
        x3dstep_swap_kernel<uint32_t><<<pair_blocks(plan, n), kPairThreads, 0, st>>>((uint32_t*)a, (uint32_t*)b, n, plan);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

__global__ __launch_bounds__(kItemThreads) void x3dstep_swap_keep_kernel(const X3DStepKeep* __restrict__ table, int nbuf,
                                                                          const X3DStepItem* __restrict__ items,
                                                                          int64_t nitems, float* snap, int64_t snap_n) {
    const int64_t i = (int64_t)blockIdx.x * X3DSTEP_ITEMS_PER_GROUP + (threadIdx.x >> 6);
    if (i >= nitems) return;
    bool bad;
    const KeepCopy c = keep_resolve(table, nbuf, items, i, snap, snap_n, X3DSTEP_KEEP_SAVE, &bad);
    if (c.len > 0) swap_lane(c, threadIdx.x & (kLanes - 1));
}

extern "C" int x3dstep_swap_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                                 int64_t snap_n, void* stream) {
    const int rc = x3dstep_check_table("x3dstep_swap_keep", table, nbuf, items, nitems, snap, snap_n, nullptr, 0.0f);
    if (rc) return rc;
    const unsigned grid = (unsigned)((nitems + X3DSTEP_ITEMS_PER_GROUP - 1) / X3DSTEP_ITEMS_PER_GROUP);
    x3dstep_swap_keep_kernel<<<grid, kItemThreads, 0, (hipStream_t)stream>>>(table, nbuf, items, nitems, snap, snap_n);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}
