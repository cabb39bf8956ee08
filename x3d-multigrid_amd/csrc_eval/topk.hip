// Device-resident top-k classification meter (include/x3deval.h; the validation arithmetic of the reference's
// train_x3d_kinetics_multigrid.py:253-265, 293-295).
//
// Append: the one-workgroup reserve kernel of the AP meter's appends (it also counts the append as one batch), then one
// workgroup per video.  A video's row is computed in fp64 from the fp32 logits and rounded once, the rule of the finalize
// kernels of csrc/bn.hip: per crop the softmax (one wave per crop: maximum, then the sum of exponentials), then per class
// the crop means s[k] (kept in LDS) and m[k] (recomputed where needed: a sum of n_crops logits), the log-sum-exp of m,
// the rank of the label among s and the argmax of s.  Every sum has a fixed order, so a row is the same bits run to run,
// and two classes with identical logits get identical s (the same instructions on the same values): ties are exact.
// The append is sized for simplicity, not for occupancy: a crop's softmax belongs to one wave (with one crop three of the
// four waves idle in that pass) and m[k] is recomputed in three passes rather than kept.  A call is launch-bound at the
// validation shapes and sits behind a forward pass of milliseconds (profiles/kinetics_val/).
//
// value(): ONE workgroup strides over the rows (a validation set is some 10^4 rows of 20 bytes; thread t owns rows t,
// t + 1024, ... and the partial sums meet in a fixed order), so the fp64 sums are the same bits run to run.  The per-class
// histograms are integer atomics, where order cannot matter.
#include "eval_common.h"

namespace {

constexpr int CLS_NT = 256;                // threads of the append workgroup
constexpr int CLS_W = CLS_NT / 64;
constexpr int VAL_NT = 1024;               // threads of the value workgroup
constexpr int VAL_W = VAL_NT / 64;

__global__ void cls_reserve_kernel(int* state, int n) {
    if (threadIdx.x != 0) return;
    reserve_rows(state, n);
    if (state[X3DEVAL_S_GO]) state[X3DEVAL_S_BATCHES] += 1;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);     // a + b == b + a: every lane ends with the same bits
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// Workgroup reductions through W slots of LDS, combined in slot order by every thread.  Every thread must call them.
template <int W>
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    __syncthreads();                       // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < W; ++i) t += red[i];
    return t;
}

template <int W>
__device__ __forceinline__ double block_max(double v, double* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
    for (int i = 1; i < W; ++i) t = fmax(t, red[i]);
    return t;
}

template <int W>
__device__ __forceinline__ long long block_sum_i(long long v, long long* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = 0;
    for (int i = 0; i < W; ++i) t += red[i];
    return t;
}

// m[k]: the mean over the crops of the logits, summed in crop order
__device__ __forceinline__ double mean_logit(const float* __restrict__ z, int K, int nc, int k) {
    double a = 0.0;
    for (int j = 0; j < nc; ++j) a += (double)z[(size_t)j * K + k];
    return a / (double)nc;
}

__global__ __launch_bounds__(CLS_NT) void cls_append_kernel(int* state, float* loss, int* rank, int* pred, int* label_out,
                                                            int* batch_rows, int K, const float* __restrict__ logits,
                                                            const long long* __restrict__ labels, int b, int nc) {
    if (state[X3DEVAL_S_GO] == 0) return;              // the append did not fit: nothing is written
    __shared__ double s[X3DEVAL_CLS_MAX_K];
    __shared__ double cmax[X3DEVAL_CLS_MAX_CROPS];
    __shared__ double csum[X3DEVAL_CLS_MAX_CROPS];
    __shared__ double redd[CLS_W];
    __shared__ long long redi[CLS_W];
    __shared__ int redk[CLS_W];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int v = blockIdx.x;
    const float* z = logits + (size_t)v * nc * K;
    const double ninf = -__builtin_inf();

    // per crop (one wave each): the maximum and the sum of exponentials of its softmax.  fmax skips a NaN, the sum keeps it.
    for (int j = w; j < nc; j += CLS_W) {
        const float* zj = z + (size_t)j * K;
        double mx = ninf;
        for (int k = lane; k < K; k += 64) mx = fmax(mx, (double)zj[k]);
        mx = wave_max(mx);
        double se = 0.0;
        for (int k = lane; k < K; k += 64) se += exp((double)zj[k] - mx);
        se = wave_sum(se);
        if (lane == 0) {
            cmax[j] = mx;
            csum[j] = se;
        }
    }
    __syncthreads();

    // s[k] and the maximum of m
    double mmax = ninf;
    for (int k = tid; k < K; k += CLS_NT) {
        double a = 0.0;
        for (int j = 0; j < nc; ++j) a += exp((double)z[(size_t)j * K + k] - cmax[j]) / csum[j];
        s[k] = a / (double)nc;
        mmax = fmax(mmax, mean_logit(z, K, nc, k));
    }
    mmax = block_max<CLS_W>(mmax, redd);               // its barriers also publish s
    double se = 0.0;
    for (int k = tid; k < K; k += CLS_NT) se += exp(mean_logit(z, K, nc, k) - mmax);
    se = block_sum<CLS_W>(se, redd);

    const long long lab = labels[v];
    const bool ok = lab >= 0 && lab < (long long)K;
    const double sl = s[ok ? (int)lab : 0];            // s is NaN in every class or in none (a crop's sum is shared)
    const bool isnan_ = sl != sl;

    // the label's rank and the argmax (lowest index among equals; s >= 0, so -1 loses to every class)
    long long above = 0;
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int k = tid; k < K; k += CLS_NT) {
        const double x = s[k];
        above += (x > sl) || (x == sl && k < (int)lab);
        if (x > bv) {
            bv = x;
            bi = k;
        }
    }
    above = block_sum_i<CLS_W>(above, redi);
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        redd[w] = bv;                                  // block_sum_i's last barrier is behind every read of redd
        redk[w] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < CLS_W; ++i)
            if (redd[i] > bv || (redd[i] == bv && redk[i] < bi)) {
                bv = redd[i];
                bi = redk[i];
            }
        const size_t o = (size_t)state[X3DEVAL_S_BASE] + v;
        const double nan_ = __builtin_nan("");
        loss[o] = ok ? (float)((mmax + log(se)) - mean_logit(z, K, nc, (int)lab)) : (float)nan_;
        rank[o] = (ok && !isnan_) ? (int)above : K;
        pred[o] = isnan_ ? -1 : bi;
        label_out[o] = (int)(lab < -1 ? -1 : (lab > 0x7fffffffLL ? 0x7fffffffLL : lab));
        batch_rows[o] = b;
        if (!ok) state[X3DEVAL_S_BAD] = 1;
    }
}

__global__ __launch_bounds__(VAL_NT) void cls_value_kernel(const int* __restrict__ state, const float* __restrict__ loss,
                                                           const int* __restrict__ rank, const int* __restrict__ label,
                                                           const int* __restrict__ batch_rows, int K, int capacity, int kmax,
                                                           long long* __restrict__ totals, double* __restrict__ loss_sums,
                                                           int* class_correct, int* class_count) {
    __shared__ double redd[VAL_W];
    __shared__ long long redi[VAL_W];
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += VAL_NT) {
        class_correct[k] = 0;
        class_count[k] = 0;
    }
    const int N = state[X3DEVAL_S_COUNT];
    if (state[X3DEVAL_S_OVERFLOW] != 0 || state[X3DEVAL_S_BAD] != 0 || N < 0 || N > capacity) {
        if (tid == 0) {
            for (int i = 0; i < 4; ++i) totals[i] = -1;
            loss_sums[0] = loss_sums[1] = __builtin_nan("");
        }
        return;
    }
    __syncthreads();                                   // the zeroed histograms, before this workgroup's atomics
    const int kk = kmax < K ? kmax : K;                // a NaN row has rank K: never among the top
    long long c1 = 0, ck = 0;
    double ls = 0.0, lb = 0.0;
    for (int i = tid; i < N; i += VAL_NT) {
        const int r = rank[i], y = label[i];
        const double l = (double)loss[i];
        c1 += r == 0;
        ck += r < kk;
        ls += l;
        lb += l / (double)batch_rows[i];
        if (y >= 0 && y < K) {                         // always, while the BAD flag is clear
            atomicAdd(&class_count[y], 1);
            if (r == 0) atomicAdd(&class_correct[y], 1);
        }
    }
    c1 = block_sum_i<VAL_W>(c1, redi);
    ck = block_sum_i<VAL_W>(ck, redi);
    ls = block_sum<VAL_W>(ls, redd);
    lb = block_sum<VAL_W>(lb, redd);
    if (tid == 0) {
        totals[0] = N;
        totals[1] = c1;
        totals[2] = ck;
        totals[3] = state[X3DEVAL_S_BATCHES];
        loss_sums[0] = ls;
        loss_sums[1] = lb;
    }
}

}  // namespace

extern "C" int x3deval_cls_append_crops(int* state, float* loss, int* rank, int* pred, int* label, int* batch_rows, int K,
                                        const float* logits, const int64_t* labels, int b, int n_crops, void* stream) {
    X3DEVAL_CHECK_ARG(state && loss && rank && pred && label && batch_rows && logits && labels);
    X3DEVAL_CHECK_ARG(K > 0 && K <= X3DEVAL_CLS_MAX_K && b > 0 && n_crops > 0 && n_crops <= X3DEVAL_CLS_MAX_CROPS);
    X3DEVAL_CHECK_ARG((long long)b * n_crops * K <= 0x7fffffffLL);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cls_reserve_kernel, dim3(1), dim3(64), 0, s, state, b);
    hipLaunchKernelGGL(cls_append_kernel, dim3(b), dim3(CLS_NT), 0, s, state, loss, rank, pred, label, batch_rows, K, logits,
                       (const long long*)labels, b, n_crops);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" int x3deval_cls_value(const int* state, const float* loss, const int* rank, const int* pred, const int* label,
                                 const int* batch_rows, int K, int capacity, int kmax, int64_t* totals, double* loss_sums,
                                 int* class_correct, int* class_count, void* stream) {
    (void)pred;                                        // part of a row, not of any total
    X3DEVAL_CHECK_ARG(state && loss && rank && label && batch_rows && totals && loss_sums && class_correct && class_count);
    X3DEVAL_CHECK_ARG(K > 0 && kmax > 0 && capacity >= 0 && capacity <= X3DEVAL_MAX_CAPACITY);
    hipLaunchKernelGGL(cls_value_kernel, dim3(1), dim3(VAL_NT), 0, (hipStream_t)stream, state, loss, rank, label, batch_rows, K,
                       capacity, kmax, (long long*)totals, loss_sums, class_correct, class_count);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}
