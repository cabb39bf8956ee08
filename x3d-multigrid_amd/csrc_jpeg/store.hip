// Device stage of libx3djpeg's frame store (include/x3djpeg.h), gfx950: the two kernels that build a batch's job tables
// from frame ids, through store_core.h.
//
// plan_kernel: one workgroup.  A pass takes X3DJPEG_STORE_PLAN_CHUNK requests, kPlanPerThread consecutive ones per thread:
// each thread sums its own, the workgroup runs an inclusive Hillis-Steele sum of the two needs over the threads in LDS,
// and a carry (the same in every thread: read from LDS after a barrier) joins the passes.  Every barrier is reached by the
// whole workgroup: the pass count depends on n alone.
//
// emit_kernel: one wave per request, kEmitWaves requests per workgroup; lane l writes pieces l, l + 64, ... of the
// request's two jobs, so consecutive lanes store consecutive 16-byte pieces.  No LDS, no barrier, no atomics.  (The plan
// kernel's only atomic is an OR into LDS of the refusal bits.)
#include "jpeg_common.h"
#include "store_core.h"

namespace {

using namespace x3dj;

constexpr int kWave = 64;
constexpr int kEmitWaves = 4;

__global__ __launch_bounds__(kPlanThreads) void plan_kernel(StoreArgs A, int32_t* __restrict__ build_status) {
    __shared__ int64_t s_coef[kPlanThreads], s_ws[kPlanThreads];
    __shared__ int s_seen;  // the OR of every request's flags
    const int tid = threadIdx.x;
    if (tid == 0) s_seen = 0;  // ordered before the atomics below by the barriers of the first pass (n >= 1)
    int64_t carry_coef = 0, carry_ws = 0;
    int seen = 0;
    for (int base = 0; base < A.n; base += X3DJPEG_STORE_PLAN_CHUNK) {
        int64_t cc[kPlanPerThread], ws[kPlanPerThread];
        int fl[kPlanPerThread];
        int64_t sum_coef = 0, sum_ws = 0;
        const int first = base + tid * kPlanPerThread;
#pragma unroll
        for (int k = 0; k < kPlanPerThread; ++k) {
            cc[k] = ws[k] = 0;
            fl[k] = 0;
            if (first + k < A.n) fl[k] = plan_request(A, first + k, &cc[k], &ws[k]);
            sum_coef += cc[k];
            sum_ws += ws[k];
        }
        s_coef[tid] = sum_coef;
        s_ws[tid] = sum_ws;
        __syncthreads();
        for (int d = 1; d < kPlanThreads; d <<= 1) {
            const int64_t a = tid >= d ? s_coef[tid - d] : 0, b = tid >= d ? s_ws[tid - d] : 0;
            __syncthreads();
            s_coef[tid] += a;
            s_ws[tid] += b;
            __syncthreads();
        }
        int64_t off_coef = carry_coef + s_coef[tid] - sum_coef, off_ws = carry_ws + s_ws[tid] - sum_ws;
#pragma unroll
        for (int k = 0; k < kPlanPerThread; ++k) {
            if (first + k < A.n) seen |= plan_place(A, first + k, fl[k], off_coef, cc[k], off_ws, ws[k]);
            off_coef += cc[k];
            off_ws += ws[k];
        }
        carry_coef += s_coef[kPlanThreads - 1];
        carry_ws += s_ws[kPlanThreads - 1];
        __syncthreads();  // the sums are read before the next pass overwrites them
    }
    if (seen) atomicOr(&s_seen, seen);  // __syncthreads_or would give a truth value, not the bits
    __syncthreads();
    if (tid == 0) {
        plan_totals(A)[0] = carry_coef;
        plan_totals(A)[1] = carry_ws;
        *build_status = s_seen;
    }
}

__global__ __launch_bounds__(kWave* kEmitWaves) void emit_kernel(StoreArgs A) {
    const int i = blockIdx.x * kEmitWaves + (int)(threadIdx.x / kWave);
    if (i >= A.n) return;
    emit_request(A, i, (int)(threadIdx.x % kWave), kWave);
}

}  // namespace

extern "C" int x3djpeg_store_build_jobs(const void* recs, int nrecs, const void* headers, int nheaders, const void* ids, int n,
                                        int sub_bits, void* coef, size_t coef_cap, void* planes, size_t planes_cap,
                                        size_t workspace_bytes, const void* dsts, void* plan, void* scan_jobs,
                                        void* frame_jobs, void* build_status, void* stream) {
    X3DJPEG_CHECK_ARG(recs && headers && ids && coef && planes && dsts && plan && scan_jobs && frame_jobs && build_status);
    X3DJPEG_CHECK_ARG(nrecs >= 1 && nheaders >= 1 && n >= 1 && n <= 65535);
    X3DJPEG_CHECK_ARG(sub_bits >= 32 && sub_bits % 32 == 0 && sub_bits <= (1 << 20));
    X3DJPEG_CHECK_ARG(coef_cap <= ((size_t)1 << 60) && planes_cap <= ((size_t)1 << 60) && workspace_bytes <= ((size_t)1 << 62));
    X3DJPEG_CHECK_ARG((((uintptr_t)recs | (uintptr_t)headers | (uintptr_t)coef) & 15) == 0);
    X3DJPEG_CHECK_ARG((((uintptr_t)scan_jobs | (uintptr_t)frame_jobs) & 15) == 0);
    X3DJPEG_CHECK_ARG((((uintptr_t)plan | (uintptr_t)dsts) & 7) == 0 && (((uintptr_t)ids | (uintptr_t)build_status) & 3) == 0);
    StoreArgs A;
    A.recs = (const X3DJpegStoreRec*)recs;
    A.headers = (const X3DJpegStoreHeader*)headers;
    A.ids = (const int32_t*)ids;
    A.dsts = (const X3DJpegStoreDst*)dsts;
    A.nrecs = nrecs;
    A.nheaders = nheaders;
    A.n = n;
    A.sub_bits = sub_bits;
    A.coef = (int16_t*)coef;
    A.planes = (uint8_t*)planes;
    A.coef_cap = (int64_t)coef_cap;
    A.planes_cap = (int64_t)planes_cap;
    A.ws_cap = (int64_t)workspace_bytes;
    A.plan = (int64_t*)plan;
    A.scan_jobs = (X3DJpegScanJob*)scan_jobs;
    A.frame_jobs = (X3DJpegFrameJob*)frame_jobs;
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(kPlanThreads), 0, (hipStream_t)stream, A, (int32_t*)build_status);
    X3DJPEG_LAUNCH_CHECK();
    hipLaunchKernelGGL(emit_kernel, dim3(jpeg_cdiv(n, kEmitWaves)), dim3(kWave * kEmitWaves), 0, (hipStream_t)stream, A);
    X3DJPEG_LAUNCH_CHECK();
    return X3DJPEG_OK;
}
