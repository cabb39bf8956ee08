// The weight average of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_ema and x3dstep_swap over flat buffers (the flat
// walk, as x3dstep_apply), x3dstep_ema_keep and x3dstep_swap_keep over a keep table (the item walk, as x3dstep_keep).  The
// walks are step_priv.h's; the count, skip, decay and element rules are step_core.h's, shared with the CPU twins.  The EMA
// launches read the state and never write it; no LDS, no atomics, no allocation, no synchronisation.
#include "step_priv.h"

using namespace x3ds;

extern "C" int x3dstep_ema(float* e, const float* w, int64_t n, const int64_t* state, int64_t count, float decay, int warmup,
                           void* stream) {
    const int rc = x3dstep_check_ema("x3dstep_ema", e, w, n, state, decay);
    if (rc) return rc;
    const EmaOp op = {state, count, decay, warmup ? 1 : 0, {0.0f, 0.0f}};
    return launch_flat(op, Bufs<EmaOp>{{e, (float*)w}}, n, stream);
}

extern "C" int x3dstep_ema_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* esnap,
                                int64_t snap_n, const int64_t* state, int64_t count, float decay, int warmup, void* stream) {
    const int rc = x3dstep_check_table("x3dstep_ema_keep", table, nbuf, items, nitems, esnap, snap_n, state, false,
                                       X3DSTEP_KEEP_SAVE, decay);
    if (rc) return rc;
    const EmaOp op = {state, count, decay, warmup ? 1 : 0, {0.0f, 0.0f}};
    return launch_items(op, table, nbuf, items, nitems, esnap, snap_n, stream);
}

// the exchange: the same walks on bits
extern "C" int x3dstep_swap(float* a, float* b, int64_t n, void* stream) {
    const int rc = x3dstep_check_swap("x3dstep_swap", a, b, n);
    if (rc) return rc;
    return launch_flat(SwapOp{}, Bufs<SwapOp>{{(uint32_t*)a, (uint32_t*)b}}, n, stream);
}

extern "C" int x3dstep_swap_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                                 int64_t snap_n, void* stream) {
    const int rc = x3dstep_check_table("x3dstep_swap_keep", table, nbuf, items, nitems, snap, snap_n, nullptr, false,
                                       X3DSTEP_KEEP_SAVE, 0.0f);
    if (rc) return rc;
    return launch_items(SwapOp{}, table, nbuf, items, nitems, snap, snap_n, stream);
}
