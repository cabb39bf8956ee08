// Device stage of the two-tier frame store (include/x3djpeg.h), gfx950: the two kernels that gather a batch's frames from
// an arena the device reads over the host link into a staging buffer in HBM, through stage_core.h, and the two entry
// points that allocate and free that arena's pinned memory.
//
// plan_kernel: one workgroup, passes of X3DJPEG_STORE_PLAN_CHUNK requests joined by a carry, as store.hip's: each thread
// sums kPlanPerThread consecutive requests, the workgroup runs an inclusive Hillis-Steele sum over the threads in LDS.
// The offset of the first request refused for lack of room is kept as a minimum in LDS (its only atomics, with the OR of
// the refusal bits); every barrier is reached by the whole workgroup, the pass count depends on n alone.
//
// copy_kernel: blockIdx.y is the request, blockIdx.x a run of kCopyThreads * kCopyPieces 16-byte pieces of it; the grid
// comes from n and max_frame_bytes, which the host knows, and a workgroup past its frame's end leaves at once.  A lane
// issues its kCopyPieces loads (kCopyThreads pieces apart, so a wave reads 1 KB runs) before its first store: with
// n * frame / 16 pieces in flight over the whole grid, the latency of the host link is hidden by breadth.  No LDS, no
// barrier, no atomics, nothing waits for another workgroup.
#include "jpeg_common.h"
#include "stage_core.h"

namespace {

using namespace x3dj;

constexpr int kCopyThreads = 256;
constexpr int kCopyPieces = 4;
constexpr int64_t kCopyBytes = 16 * (int64_t)kCopyThreads * kCopyPieces;  // per workgroup

__global__ __launch_bounds__(kPlanThreads) void stage_plan_kernel(StageArgs A, int32_t* __restrict__ stage_status) {
    __shared__ int64_t s_sum[kPlanThreads];
    __shared__ unsigned long long s_first;  // the smallest offset refused for lack of room
    __shared__ int s_seen;                  // the OR of every request's flags
    const int tid = threadIdx.x;
    if (tid == 0) {  // ordered before the atomics below by the barriers of the first pass (n >= 1)
        s_seen = 0;
        s_first = (unsigned long long)kStageNever;
    }
    int64_t carry = 0, first_refused = kStageNever;
    int seen = 0;
    for (int base = 0; base < A.n; base += X3DJPEG_STORE_PLAN_CHUNK) {
        int64_t b[kPlanPerThread], at[kPlanPerThread];
        int fl[kPlanPerThread];
        int64_t sum = 0;
        const int first = base + tid * kPlanPerThread;
#pragma unroll
        for (int k = 0; k < kPlanPerThread; ++k) {
            b[k] = 0;
            fl[k] = 0;
            if (first + k < A.n) fl[k] = stage_request(A, first + k, &b[k]);
            sum += b[k];
        }
        s_sum[tid] = sum;
        __syncthreads();
        for (int d = 1; d < kPlanThreads; d <<= 1) {
            const int64_t a = tid >= d ? s_sum[tid - d] : 0;
            __syncthreads();
            s_sum[tid] += a;
            __syncthreads();
        }
        int64_t off = carry + s_sum[tid] - sum, mine = kStageNever;
#pragma unroll
        for (int k = 0; k < kPlanPerThread; ++k) {
            at[k] = off;
            if (first + k < A.n) {
                fl[k] = stage_place(A, first + k, fl[k], off, b[k]);
                seen |= fl[k];
                const int64_t t = stage_total(fl[k], off, b[k]);
                mine = t < mine ? t : mine;
            }
            off += b[k];
        }
        if (mine != kStageNever) atomicMin(&s_first, (unsigned long long)mine);
        carry += s_sum[kPlanThreads - 1];
        __syncthreads();  // the minimum is complete, and the sums are read before the next pass overwrites them
        first_refused = (int64_t)s_first;  // the next pass's atomics come after its own barriers
#pragma unroll
        for (int k = 0; k < kPlanPerThread; ++k)
            if (first + k < A.n) stage_offset(A, first + k, at[k], first_refused);
    }
    if (seen) atomicOr(&s_seen, seen);
    __syncthreads();
    if (tid == 0) {
        stage_offset(A, A.n, carry, first_refused);
        *stage_status = s_seen;
    }
}

__global__ __launch_bounds__(kCopyThreads) void stage_copy_kernel(StageArgs A) {
    const int i = blockIdx.y;
    StageFrame F;
    if (!stage_frame(A, i, &F)) return;
    const int64_t at0 = (int64_t)blockIdx.x * kCopyBytes;
    if (at0 >= F.bytes) return;
    Piece v[kCopyPieces];
#pragma unroll
    for (int k = 0; k < kCopyPieces; ++k) {
        const int64_t at = at0 + 16 * ((int64_t)k * kCopyThreads + threadIdx.x);
        if (at < F.bytes) v[k] = stage_load(F, at);
    }
#pragma unroll
    for (int k = 0; k < kCopyPieces; ++k) {
        const int64_t at = at0 + 16 * ((int64_t)k * kCopyThreads + threadIdx.x);
        if (at < F.bytes) store_piece(F.dst + at, v[k]);
    }
}

}  // namespace

extern "C" int x3djpeg_stage(const void* recs, int nrecs, const void* ids, int n, size_t max_frame_bytes, void* staging,
                             size_t staging_cap, void* staged_recs, void* staged_ids, void* offsets, void* stage_status,
                             void* stream) {
    X3DJPEG_CHECK_ARG(recs && ids && staging && staged_recs && staged_ids && offsets && stage_status);
    X3DJPEG_CHECK_ARG(nrecs >= 1 && n >= 1 && n <= 65535);
    X3DJPEG_CHECK_ARG(max_frame_bytes >= 1 && staging_cap <= ((size_t)1 << 60));
    X3DJPEG_CHECK_ARG((uint64_t)n * (uint64_t)max_frame_bytes < ((uint64_t)1 << 44) && max_frame_bytes < ((size_t)1 << 40));
    X3DJPEG_CHECK_ARG((((uintptr_t)recs | (uintptr_t)staging | (uintptr_t)staged_recs) & 15) == 0);
    X3DJPEG_CHECK_ARG(((uintptr_t)offsets & 7) == 0 && (((uintptr_t)ids | (uintptr_t)staged_ids | (uintptr_t)stage_status) & 3) == 0);
    StageArgs A;
    A.recs = (const X3DJpegStoreRec*)recs;
    A.ids = (const int32_t*)ids;
    A.nrecs = nrecs;
    A.n = n;
    A.max_frame_bytes = (int64_t)max_frame_bytes;
    A.staging = (uint8_t*)staging;
    A.cap = (int64_t)staging_cap;
    A.staged_recs = (X3DJpegStoreRec*)staged_recs;
    A.staged_ids = (int32_t*)staged_ids;
    A.offsets = (int64_t*)offsets;
    hipLaunchKernelGGL(stage_plan_kernel, dim3(1), dim3(kPlanThreads), 0, (hipStream_t)stream, A, (int32_t*)stage_status);
    X3DJPEG_LAUNCH_CHECK();
    const unsigned runs = (unsigned)(((int64_t)max_frame_bytes + kCopyBytes - 1) / kCopyBytes);
    hipLaunchKernelGGL(stage_copy_kernel, dim3(runs, (unsigned)n), dim3(kCopyThreads), 0, (hipStream_t)stream, A);
    X3DJPEG_LAUNCH_CHECK();
    return X3DJPEG_OK;
}

extern "C" int x3djpeg_pinned_alloc(size_t bytes, void** host, void** dev) {
    X3DJPEG_CHECK_ARG(host && dev && bytes >= 1);
    *host = *dev = nullptr;
    void* h = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocPortable);
    if (e != hipSuccess || !h) {
        (void)hipGetLastError();
        x3djpeg_set_error("x3djpeg_pinned_alloc: %zu bytes of pinned host memory: %s", bytes, hipGetErrorString(e));
        return X3DJPEG_ELAUNCH;
    }
    void* d = nullptr;
    e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess || !d) {
        (void)hipGetLastError();
        (void)hipHostFree(h);
        x3djpeg_set_error("x3djpeg_pinned_alloc: no device address for %zu bytes of pinned host memory: %s", bytes,
                          hipGetErrorString(e));
        return X3DJPEG_ELAUNCH;
    }
    *host = h;
    *dev = d;
    return X3DJPEG_OK;
}

extern "C" int x3djpeg_pinned_free(void* host) {
    X3DJPEG_CHECK_ARG(host);
    const hipError_t e = hipHostFree(host);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        x3djpeg_set_error("x3djpeg_pinned_free: %s", hipGetErrorString(e));
        return X3DJPEG_ELAUNCH;
    }
    return X3DJPEG_OK;
}
