// Device stage of the indexed Huffman decoder of libx3djpeg (include/x3djpeg.h), gfx950: one workgroup per frame walks
// the phases of index_core.h, a workgroup barrier between them.  One pass over the scan: the states the relaxation of
// entropy.hip converges to are read from the frame's sync index, and every hand-over is compared with it.  All state is in
// LDS (tables, the frame's context, the per-worker sums); there is no workspace, and a workgroup writes only its own
// frame's coefficients and status word, with plain vector stores, so there is nothing to wait for between workgroups.
//
// Every barrier is reached by the whole workgroup: what decides whether the workgroup leaves early is either in LDS and
// written before the previous barrier, or the result of __syncthreads_or.
#include "index_core.h"
#include "jpeg_common.h"

namespace {

using namespace x3dj;

__global__ __launch_bounds__(kMaxWorkers) void entropy_indexed_kernel(const X3DJpegScanJob* __restrict__ jobs,
                                                                      const int32_t* __restrict__ ids,
                                                                      const X3DJpegIndexRec* __restrict__ recs, int nrecs,
                                                                      const uint32_t* __restrict__ entries,
                                                                      long long entries_total, int index_bits,
                                                                      int32_t* __restrict__ status) {
    __shared__ HuffTable tables[8];
    __shared__ int32_t scratch[kScratchInts];
    __shared__ FrameCtx C;
    __shared__ IndexCtx X;
    __shared__ int s_err;
    const X3DJpegScanJob& J = jobs[blockIdx.x];
    const int tid = threadIdx.x, nt = kMaxWorkers;

    if (tid == 0) s_err = idx_setup(J, ids[blockIdx.x], recs, nrecs, entries, entries_total, index_bits, tables, &C, &X);
    __syncthreads();
    if (s_err) {
        if (tid == 0) status[blockIdx.x] = s_err;
        return;
    }
    const int bad_table = __syncthreads_or(build_tables(J, C, tables, tid, nt));
    const int bad_seg = __syncthreads_or(seg_count(C, tid, nt, scratch));
    if (bad_table || bad_seg) {
        if (tid == 0) status[blockIdx.x] = bad_seg ? X3DJPEG_EINVAL : X3DJPEG_ECORRUPT;
        return;
    }
    if (tid == 0) s_err = idx_total(&C, X, nt, scratch);
    __syncthreads();
    if (s_err) {
        if (tid == 0) status[blockIdx.x] = s_err;
        return;
    }
    zero(C, tid, nt);
    __syncthreads();
    const int bits = __syncthreads_or(idx_write(C, X, tid, nt, scratch));
    dc_sum(C, tid, nt, scratch);
    __syncthreads();
    if (tid < C.ncomp) carry_scan(scratch + 2 * tid * nt, nt);
    __syncthreads();
    dc_place(C, tid, nt, scratch);
    if (tid == 0) status[blockIdx.x] = idx_status(bits);
}

}  // namespace

extern "C" int x3djpeg_entropy_decode_indexed(const void* jobs, int njobs, const void* ids, const void* index_recs, int nrecs,
                                              const void* entries, size_t entries_total, int index_bits, void* status,
                                              void* stream) {
    X3DJPEG_CHECK_ARG(jobs != nullptr && ids != nullptr && index_recs != nullptr && entries != nullptr && status != nullptr);
    X3DJPEG_CHECK_ARG(njobs >= 1 && njobs <= 65535 && nrecs >= 1);
    X3DJPEG_CHECK_ARG(index_bits_ok(index_bits));
    X3DJPEG_CHECK_ARG(((uintptr_t)entries & 7) == 0 && ((uintptr_t)index_recs & 7) == 0 && entries_total <= ((size_t)1 << 59));
    hipLaunchKernelGGL(entropy_indexed_kernel, dim3(njobs), dim3(kMaxWorkers), 0, (hipStream_t)stream,
                       (const X3DJpegScanJob*)jobs, (const int32_t*)ids, (const X3DJpegIndexRec*)index_recs, nrecs,
                       (const uint32_t*)entries, (long long)entries_total, index_bits, (int32_t*)status);
    X3DJPEG_LAUNCH_CHECK();
    return X3DJPEG_OK;
}
