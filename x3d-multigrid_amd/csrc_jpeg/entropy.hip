// Device stage of the parallel Huffman decoder of libx3djpeg (include/x3djpeg.h), gfx950: one workgroup per frame walks
// the phases of entropy_core.h, a workgroup barrier between them.  All state is in LDS (tables, the frame's context, the
// per-worker sums) or in the caller's workspace; a workgroup touches only its own frame's part of it, so there is nothing
// to wait for between workgroups: no ticket, no flag, no device-scope fence.
//
// Every barrier is reached by the whole workgroup: what decides whether a phase is skipped or the relaxation goes on is
// either in LDS and written before the previous barrier, or the result of __syncthreads_or.
#include "entropy_core.h"
#include "jpeg_common.h"

namespace {

using namespace x3dj;

__global__ __launch_bounds__(kMaxWorkers) void entropy_kernel(const X3DJpegScanJob* __restrict__ jobs, int sub_bits,
                                                              uint8_t* workspace, long long workspace_bytes,
                                                              int32_t* __restrict__ status) {
    __shared__ HuffTable tables[8];
    __shared__ int32_t scratch[kScratchInts];
    __shared__ FrameCtx C;
    __shared__ int s_err;
    const X3DJpegScanJob& J = jobs[blockIdx.x];
    const int tid = threadIdx.x, nt = kMaxWorkers;

    if (tid == 0) s_err = setup(J, sub_bits, workspace, workspace_bytes, tables, &C);
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
    if (tid == 0) s_err = seg_total(&C, nt, scratch);
    __syncthreads();
    if (s_err) {
        if (tid == 0) status[blockIdx.x] = s_err;
        return;
    }
    seg_place(C, tid, nt, scratch);
    __syncthreads();
    init(C, tid, nt);
    __syncthreads();
    // Relaxation.  Each round makes at least one more subsequence of every segment exact, so nsub rounds always suffice;
    // whether the barriers order anything only decides how many rounds it takes.
    const int nsub = C.nsub;
    int rounds = 0;
    while (rounds < nsub) {
        ++rounds;
        if (!__syncthreads_or(relax_take(C, tid, nt))) break;
        relax_run(C, tid, nt);
        __syncthreads();
    }
    count_sum(C, tid, nt, scratch);
    zero(C, tid, nt);
    __syncthreads();
    if (tid == 0) carry_scan(scratch, nt);
    __syncthreads();
    count_place(C, tid, nt, scratch);
    __syncthreads();
    const int bad = __syncthreads_or(write_coef(C, tid, nt));
    dc_sum(C, tid, nt, scratch);
    __syncthreads();
    if (tid < C.ncomp) carry_scan(scratch + 2 * tid * nt, nt);
    __syncthreads();
    dc_place(C, tid, nt, scratch);
    if (tid == 0) {
        C.head[0] = rounds;
        status[blockIdx.x] = bad ? X3DJPEG_ECORRUPT : X3DJPEG_OK;
    }
}

}  // namespace

extern "C" int x3djpeg_entropy_decode_batch(const void* jobs, int njobs, int sub_bits, void* workspace,
                                            size_t workspace_bytes, void* status, void* stream) {
    X3DJPEG_CHECK_ARG(jobs != nullptr && workspace != nullptr && status != nullptr);
    X3DJPEG_CHECK_ARG(njobs >= 1 && njobs <= 65535);
    X3DJPEG_CHECK_ARG(sub_bits >= 32 && sub_bits % 32 == 0 && sub_bits <= (1 << 20));
    X3DJPEG_CHECK_ARG(((uintptr_t)workspace & 15) == 0 && workspace_bytes <= ((size_t)1 << 62));
    hipLaunchKernelGGL(entropy_kernel, dim3(njobs), dim3(kMaxWorkers), 0, (hipStream_t)stream, (const X3DJpegScanJob*)jobs,
                       sub_bits, (uint8_t*)workspace, (long long)workspace_bytes, (int32_t*)status);
    X3DJPEG_LAUNCH_CHECK();
    return X3DJPEG_OK;
}
