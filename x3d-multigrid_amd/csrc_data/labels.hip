// Charades per-frame labels on the device.  The reference keeps a dense float [157, n_frames] array per video on the host
// (make_dataset, charades.py:91-97; about 4.5 GB for the training split), slices a window out of it per sample (:140),
// reduces it for task='class' (:142-143), pads it and builds the mask in custom_collate_fn (:174-185), and ships the
// [B, 157, TL] result to the GPU every step.  Here the annotations stay on the device as frame ranges (under 1 MB for the
// whole file) and one launch writes labels, masks and clip-level labels of a batch.
//
// One 64-lane wave per (b, k) row: the row's video and class are wave-uniform, so the scan over the video's annotations
// (at most 28 in the Charades file; any number works) runs on uniform addresses and first narrows itself to the row's own
// class, and the lanes stream the row out in 16-byte groups.  Every element is written exactly once: float4 where a
// group lies inside the row (every group when TLmax is a multiple of 4), single floats for the at most 3 + 3 elements of
// a row's unaligned head and tail.
#include "data_common.h"

namespace {

constexpr int WAVES = 4;

struct LabelRow {
    const int32_t* cls;
    const int32_t* lo;
    const int32_t* hi;
    int a0, a1, k, start, n;
    __device__ __forceinline__ void eval(int t0, float v[4]) const {
        bool on[4] = {false, false, false, false};
        for (int i = a0; i < a1; ++i) {
            if (cls[i] != k) continue;
            const int l = lo[i] - start, h = hi[i] - start;
#pragma unroll
            for (int j = 0; j < 4; ++j) on[j] = on[j] || (t0 + j >= l && t0 + j < h);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (on[j] && t0 + j >= 0 && t0 + j < n) ? 1.0f : 0.0f;
    }
    __device__ __forceinline__ bool any() const {
        bool r = false;
        for (int i = a0; i < a1; ++i) {
            if (cls[i] != k) continue;
            const int l = lo[i] > start ? lo[i] : start;
            const int h = hi[i] - start < n ? hi[i] : start + n;
            r = r || l < h;
        }
        return r;
    }
};

struct MaskRow {
    int n;
    __device__ __forceinline__ void eval(int t0, float v[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (t0 + j >= 0 && t0 + j < n) ? 1.0f : 0.0f;
    }
};

// Elements [e0, e0 + TL) of `out` (4-byte aligned), in the 16-byte groups of the address space.
template <class F>
__device__ __forceinline__ void write_row(float* out, long long e0, int TL, int lane, const F& f) {
    const int mis = (int)(((uintptr_t)out >> 2) & 3);
    const long long g_first = (e0 + mis) >> 2, g_last = (e0 + mis + TL - 1) >> 2;
    for (long long g = g_first + lane; g <= g_last; g += 64) {
        const int t0 = (int)((g << 2) - mis - e0);      // -3 .. TL - 1
        float v[4];
        f.eval(t0, v);
        float* p = out + e0 + t0;
        if (t0 >= 0 && t0 + 4 <= TL) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + j >= 0 && t0 + j < TL) p[j] = v[j];
        }
    }
}

__global__ __launch_bounds__(64 * WAVES) void charades_labels_kernel(
    const int32_t* __restrict__ ann_off, const int32_t* __restrict__ ann_cls, const int32_t* __restrict__ ann_lo,
    const int32_t* __restrict__ ann_hi, int V, const X3DDataLabelJob* __restrict__ jobs, int B, int K, int TLmax,
    int nlab, int rows, float* labels, float* masks, float* cls) {
    const int lane = threadIdx.x & 63;
    const long long row_ll = (long long)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row_ll >= rows) return;
    const int row = (int)row_ll;
    if (row >= nlab) {                                  // a mask row
        const int b = row - nlab;
        int n = jobs[b].n;
        n = n < 0 ? 0 : (n > TLmax ? TLmax : n);
        write_row(masks, (long long)b * TLmax, TLmax, lane, MaskRow{n});
        return;
    }
    const int b = row / K, k = row - b * K;
    const X3DDataLabelJob J = jobs[b];
    LabelRow R;
    R.cls = ann_cls; R.lo = ann_lo; R.hi = ann_hi;
    R.a0 = R.a1 = 0;
    if (J.video >= 0 && J.video < V) {
        R.a0 = ann_off[J.video];
        R.a1 = ann_off[J.video + 1];
    }
    R.k = k;
    R.start = J.start;
    R.n = J.n < 0 ? 0 : (J.n > TLmax ? TLmax : J.n);
    // one pass over the video's annotations per wave: the scan of eval() is narrowed to [first, last] annotation of class
    // k, so a row with no annotation of its class (almost all of the 157 rows of a sample) streams zeros without a load
    int m0 = R.a1, m1 = R.a0;
    for (int i = R.a0; i < R.a1; ++i)
        if (ann_cls[i] == k) {
            m0 = i < m0 ? i : m0;
            m1 = i + 1;
        }
    R.a0 = m0 < m1 ? m0 : m1;
    R.a1 = m1;
    if (labels) write_row(labels, (long long)row * TLmax, TLmax, lane, R);
    if (cls && lane == 0) cls[row] = R.any() ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int x3ddata_charades_labels(const int32_t* ann_off, const int32_t* ann_cls, const int32_t* ann_lo,
                                       const int32_t* ann_hi, int V, const void* jobs, int B, int K, int TLmax,
                                       float* labels, float* masks, float* cls, void* stream) {
    X3DDATA_CHECK_ARG(ann_off && ann_cls && ann_lo && ann_hi && jobs);
    X3DDATA_CHECK_ARG(labels || masks || cls);
    X3DDATA_CHECK_ARG(V >= 0 && B > 0 && K > 0 && TLmax > 0);
    X3DDATA_CHECK_ARG((long long)B * K + B < (1LL << 31) - 64 * WAVES);
    X3DDATA_CHECK_ARG((long long)K * TLmax < (1LL << 31));
    X3DDATA_CHECK_ARG(((uintptr_t)labels & 3) == 0 && ((uintptr_t)masks & 3) == 0 && ((uintptr_t)cls & 3) == 0);
    const int nlab = (labels || cls) ? B * K : 0;
    const int rows = nlab + (masks ? B : 0);
    hipLaunchKernelGGL(charades_labels_kernel, dim3(data_cdiv(rows, WAVES)), dim3(64 * WAVES), 0, (hipStream_t)stream,
                       ann_off, ann_cls, ann_lo, ann_hi, V, (const X3DDataLabelJob*)jobs, B, K, TLmax, nlab, rows, labels,
                       masks, cls);
    X3DDATA_LAUNCH_CHECK();
    return X3DDATA_OK;
}
