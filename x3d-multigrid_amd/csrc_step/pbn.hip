// Precise BN statistics of libx3dstep (include/x3dstep.h) for gfx950: x3dstep_pbn_accum (one cell update per split for every
// channel, from the live buffers into the accumulators) and x3dstep_pbn_finish (the rank merge and the pooled mean and
// variance into every split's slot of a keep table's snapshot).  The cell, merge and result rules and the per-item tests are
// step_core.h's, shared with the CPU twins.  One workgroup per run of at most X3DSTEP_PBN_RUN channels, one thread per
// channel, reads coalesced over the channel; no LDS, no atomics, no allocation, no synchronisation.
#include "step_priv.h"

using namespace x3ds;

__global__ __launch_bounds__(X3DSTEP_PBN_RUN) void x3dstep_pbn_accum_kernel(const X3DStepPbnLayer* __restrict__ layers,
                                                                             int nlayers,
                                                                             const X3DStepItem* __restrict__ work,
                                                                             double* acc) {
    const PbnRun r = pbn_resolve(layers, nlayers, work, blockIdx.x, -1);
    if ((int)threadIdx.x < r.len) pbn_accum_one(r, threadIdx.x, acc);
}

extern "C" int x3dstep_pbn_accum(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork, double* acc,
                                 void* stream) {
    const int rc = x3dstep_check_pbn("x3dstep_pbn_accum", layers, nlayers, work, nwork, acc, false, 1, 1, nullptr, 0);
    if (rc) return rc;
    x3dstep_pbn_accum_kernel<<<(unsigned)nwork, X3DSTEP_PBN_RUN, 0, (hipStream_t)stream>>>(layers, nlayers, work, acc);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}

__global__ __launch_bounds__(X3DSTEP_PBN_RUN) void x3dstep_pbn_finish_kernel(const X3DStepPbnLayer* __restrict__ layers,
                                                                              int nlayers,
                                                                              const X3DStepItem* __restrict__ work,
                                                                              const double* __restrict__ acc_all, int W,
                                                                              int64_t expect_n, float* snap, int64_t snap_n) {
    const PbnRun r = pbn_resolve(layers, nlayers, work, blockIdx.x, snap_n);
    if ((int)threadIdx.x < r.len)
        pbn_finish_one(r, threadIdx.x, acc_all, W, pbn_channels(layers, nlayers), expect_n, snap);
}

extern "C" int x3dstep_pbn_finish(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                                  const double* acc_all, int W, int64_t expect_n, float* snap, int64_t snap_n, void* stream) {
    const int rc = x3dstep_check_pbn("x3dstep_pbn_finish", layers, nlayers, work, nwork, acc_all, true, W, expect_n, snap,
                                     snap_n);
    if (rc) return rc;
    x3dstep_pbn_finish_kernel<<<(unsigned)nwork, X3DSTEP_PBN_RUN, 0, (hipStream_t)stream>>>(layers, nlayers, work, acc_all, W,
                                                                                            expect_n, snap, snap_n);
    X3DSTEP_LAUNCH_CHECK();
    return X3DSTEP_OK;
}
