// Device-resident average-precision meter (include/x3deval.h; the reference's apmeter.APMeter, apmeter.py:30-136).
//
// Appends: a one-workgroup reserve kernel reads the device row count, checks the device capacity and publishes the base row
// of the append (or sets the overflow flag); the writer kernel that follows on the stream stores the rows class-major.
// Nothing is read back to the host, so an append can be captured into a graph and replayed.
//
// value(): one workgroup per class sorts its contiguous segment with a stable LSD radix sort (four 8-bit digits of a 32-bit
// order-preserving key, the row index and target bit as payload), then computes the class's AP from the sorted payload with
// workgroup scans.  A workgroup never waits on another one; classes beyond the workspace's slots loop over the grid.
#include "eval_common.h"

namespace {

constexpr int AP_NT = 512;                 // threads of the sort / AP workgroup
constexpr int AP_W = AP_NT / 64;           // its waves
constexpr int AP_IT = 4;                   // elements per thread per chunk
constexpr int AP_CH = AP_NT * AP_IT;       // rows per chunk
constexpr int AP_SLOTS = AP_IT * AP_W;     // (item, wave) sub-chunks of a chunk, in segment order
constexpr size_t WS_CAP_BYTES = (size_t)2 << 30;   // sort workspace cap: classes beyond it take turns on the slots
constexpr unsigned TRUTH = 0x80000000u;    // payload: row index | target << 31

__host__ __device__ inline size_t ws_rows(int capacity) { return ((size_t)capacity + 63) & ~(size_t)63; }
__host__ inline size_t ws_slot_bytes(int capacity) { return 4 * sizeof(unsigned) * ws_rows(capacity); }

__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }

// Ascending-sortable key of a DESCENDING order: every NaN becomes one positive quiet NaN (above +inf, where torch.sort puts
// it), -0.0 becomes +0.0 (they tie), then the usual sign flip, then the complement.
__device__ __forceinline__ unsigned desc_key(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u;
    else if (u == 0x80000000u) u = 0u;
    const unsigned asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~asc;
}

__global__ void ap_state_kernel(int* state, int capacity, int reset) {
    if (threadIdx.x != 0) return;
    if (reset)
        for (int i = 0; i < X3DEVAL_STATE_INTS; ++i) state[i] = 0;
    state[X3DEVAL_S_CAPACITY] = capacity;
}

__global__ void ap_reserve_kernel(int* state, int n) {
    if (threadIdx.x == 0) reserve_rows(state, n);
}

// rows [n, K] -> class-major [K, capacity] at the reserved base: 64 x 64 tiles through LDS (coalesced on both sides)
__global__ __launch_bounds__(256) void ap_append_kernel(int* state, float* scores, uint8_t* targets, float* wstore, int K,
                                                        const float* __restrict__ in_s, const float* __restrict__ in_t,
                                                        const float* __restrict__ in_w, int n) {
    if (state[X3DEVAL_S_GO] == 0) return;
    const int base = state[X3DEVAL_S_BASE];
    const size_t cap = (size_t)state[X3DEVAL_S_CAPACITY];
    __shared__ float ts[64][65];
    __shared__ float tt[64][65];
    const int r0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    int bad = 0;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, k = k0 + tx;
        if (r < n && k < K) {
            const size_t o = (size_t)r * K + k;
            const float t = in_t[o];
            bad |= !(t == 0.f || t == 1.f);
            ts[i][tx] = in_s[o];
            tt[i][tx] = t;
        }
    }
    if (in_w && blockIdx.y == 0 && threadIdx.x < 64) {
        const int r = r0 + threadIdx.x;
        if (r < n) {
            const float w = in_w[r];
            bad |= !(w >= 0.f);
            wstore[(size_t)base + r] = w;
        }
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int k = k0 + i, r = r0 + tx;
        if (r < n && k < K) {
            const size_t o = (size_t)k * cap + base + r;
            scores[o] = ts[tx][i];
            targets[o] = tt[tx][i] != 0.f;
        }
    }
    if (bad) state[X3DEVAL_S_BAD] = 1;
}

// crop-max rows: one thread per (sample, class); the max logit is written whether or not the rows fit
__global__ __launch_bounds__(256) void ap_crops_kernel(int* state, float* scores, uint8_t* targets, int K,
                                                       const float* __restrict__ logits, const float* __restrict__ in_t,
                                                       float* __restrict__ maxlogit, int b, int nc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= b * K) return;
    const int s = i / K, k = i - s * K;
    float zm = logits[(size_t)s * nc * K + k];
    float pm = sigmoid_f(zm);
    for (int j = 1; j < nc; ++j) {
        const float z = logits[((size_t)s * nc + j) * K + k];
        const float p = sigmoid_f(z);
        if (zm == zm && (z > zm || z != z)) zm = z;       // NaN propagates, as torch.amax
        if (pm == pm && (p > pm || p != p)) pm = p;
    }
    maxlogit[i] = zm;
    const float t = in_t[i];
    if (!(t == 0.f || t == 1.f)) state[X3DEVAL_S_BAD] = 1;
    if (state[X3DEVAL_S_GO] == 0) return;
    const size_t o = (size_t)k * (size_t)state[X3DEVAL_S_CAPACITY] + state[X3DEVAL_S_BASE] + s;
    scores[o] = pm;
    targets[o] = t != 0.f;
}

// valid_t[b] = (int) sum_t masks[b, t] clamped to [0, TL] (torch.sum(masks, 1).int()), one wave per sample; then the
// b-major row offsets and the reservation of their total
__global__ __launch_bounds__(256) void ap_frames_reserve_kernel(int* state, int* rowoff, const float* __restrict__ masks, int B,
                                                                int TL) {
    __shared__ int vt[X3DEVAL_MAX_FRAMES_B];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int b = w; b < B; b += 4) {
        float s = 0.f;
        for (int t = lane; t < TL; t += 64) s += masks[(size_t)b * TL + t];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) vt[b] = s >= (float)TL ? TL : (s > 0.f ? (int)s : 0);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long tot = 0;
        for (int b = 0; b < B; ++b) {
            rowoff[b] = (int)tot;
            tot += vt[b];
        }
        rowoff[B] = (int)tot;
        reserve_rows(state, tot);
    }
}

// per-frame rows: thread = (sample b = blockIdx.y, class k, frame t).  The interpolation is loc_loss_kernel's (csrc/head.hip:301:
// F.interpolate(mode='linear', align_corners=False)) with torch's two roundings fused -- the source index
// fma(scale, t + 0.5, -0.5) and the value fma(l0, z0, l1 * z1) -- so that a row equals F.interpolate's bit for bit (the
// loss kernel's unfused form differs from it by an ulp of the weights, which matters for ranks, not for a loss)
__global__ __launch_bounds__(256) void ap_frames_kernel(int* state, const int* __restrict__ rowoff, float* scores,
                                                        uint8_t* targets, int K, const float* __restrict__ logits,
                                                        const float* __restrict__ labels, const float* __restrict__ masks,
                                                        int T, int TL) {
    if (state[X3DEVAL_S_GO] == 0) return;
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * TL) return;
    const int k = e / TL, t = e - k * TL;
    const int r0 = rowoff[b];
    if (t >= rowoff[b + 1] - r0) return;
    const float* z = logits + ((size_t)b * K + k) * T;
    const float scale = (float)T / (float)TL;
    float src = fmaf(scale, (float)t + 0.5f, -0.5f);
    src = src < 0.f ? 0.f : src;
    const int i0 = min((int)src, T - 1), i1 = i0 + (i0 < T - 1 ? 1 : 0);
    const float l1 = src - (float)i0, l0 = 1.f - l1;
    const float zi = fmaf(l0, z[i0], l1 * z[i1]);
    const float p = sigmoid_f(zi) * masks[(size_t)b * TL + t];
    const float y = labels[((size_t)b * K + k) * TL + t];
    if (!(y == 0.f || y == 1.f)) state[X3DEVAL_S_BAD] = 1;
    const size_t o = (size_t)k * (size_t)state[X3DEVAL_S_CAPACITY] + state[X3DEVAL_S_BASE] + r0 + t;
    scores[o] = p;
    targets[o] = y != 0.f;
}

template <typename V>
__device__ __forceinline__ V wave_incl_scan(V v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const V u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// exclusive scan over the workgroup in a fixed order (bitwise reproducible for fp64); *total = the workgroup's sum.
// red: AP_W slots of LDS.  Every thread must call it.
template <typename V>
__device__ __forceinline__ V block_excl_scan(V v, V* red, V* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const V inc = wave_incl_scan(v);
    V ex = __shfl_up(inc, 1);
    if (lane == 0) ex = (V)0;
    if (lane == 63) red[w] = inc;
    __syncthreads();
    V before = (V)0, tot = (V)0;
    for (int i = 0; i < AP_W; ++i) {
        const V x = red[i];
        if (i < w) before += x;
        tot += x;
    }
    *total = tot;
    __syncthreads();
    return before + ex;
}

// One workgroup per class (classes beyond the grid loop over it; workspace slot = blockIdx.x).
//   1. the four digit histograms in one read of the scores (per-wave LDS histograms, integer atomics);
//   2. per digit whose histogram is not a single bin: a stable scatter, chunk by chunk in segment order.  Inside a chunk an
//      element's rank among equal digits is (earlier (item, wave) sub-chunks) + (lower lanes of its wave: ballot match);
//   3. AP from the sorted payload: tp and rank are exact integers (the fp32 division tp / rank as apmeter.py:128-131), or
//      fp64 weighted sums; the sum of precisions is fp64, rounded once.
__global__ __launch_bounds__(AP_NT) void ap_value_kernel(const int* __restrict__ state, const float* __restrict__ scores,
                                                         const uint8_t* __restrict__ targets,
                                                         const float* __restrict__ weights, int K, int capacity,
                                                         unsigned* __restrict__ ws, float* __restrict__ ap) {
    __shared__ int cnt[AP_SLOTS * 256];    // first the per-wave histograms [AP_W][4][256], then the chunk ranks
    __shared__ int hist[4 * 256];
    __shared__ int run[256];
    __shared__ int skip[4];
    __shared__ int redi[AP_W];
    __shared__ double redd[AP_W];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const size_t wsr = ws_rows(capacity);
    unsigned* const KA = ws + (size_t)blockIdx.x * 4 * wsr;
    unsigned* const PA = KA + wsr;
    unsigned* const KB = PA + wsr;
    unsigned* const PB = KB + wsr;
    const int N = state[X3DEVAL_S_COUNT];
    const bool bad = state[X3DEVAL_S_OVERFLOW] != 0 || state[X3DEVAL_S_BAD] != 0 || N < 0 || N > capacity;

    for (int k = blockIdx.x; k < K; k += gridDim.x) {
        if (bad || N == 0) {
            if (tid == 0) ap[k] = bad ? __builtin_nanf("") : 0.f;
            continue;
        }
        const float* sc = scores + (size_t)k * capacity;
        const uint8_t* tg = targets + (size_t)k * capacity;
        __syncthreads();                   // LDS of the previous class

        // 1. histograms
        for (int i = tid; i < AP_SLOTS * 256; i += AP_NT) cnt[i] = 0;
        if (tid < 4) skip[tid] = 0;
        __syncthreads();
        int* wh = cnt + w * 1024;
        for (int i0 = 0; i0 < N; i0 += 4 * AP_NT) {
            unsigned key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j * AP_NT + tid;
                key[j] = i < N ? desc_key(sc[i]) : 0u;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i0 + j * AP_NT + tid < N) {
                    atomicAdd(&wh[key[j] & 255], 1);
                    atomicAdd(&wh[256 + ((key[j] >> 8) & 255)], 1);
                    atomicAdd(&wh[512 + ((key[j] >> 16) & 255)], 1);
                    atomicAdd(&wh[768 + (key[j] >> 24)], 1);
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < 1024; i += AP_NT) {
            int s = 0;
            for (int v = 0; v < AP_W; ++v) s += cnt[v * 1024 + i];
            hist[i] = s;
            if (s == N) skip[i >> 8] = 1;           // one bin holds the whole segment: the digit cannot reorder it
        }
        __syncthreads();

        // 2. the passes
        bool ident = true;
        const unsigned* ks = nullptr;
        const unsigned* ps = nullptr;
        unsigned* kd = KA;
        unsigned* pd = PA;
        for (int p = 0; p < 4; ++p) {
            if (skip[p]) continue;
            int hv = 0, inc = 0;
            if (tid < 256) {
                hv = hist[p * 256 + tid];
                inc = wave_incl_scan(hv);
                if (lane == 63) redi[w] = inc;
            }
            __syncthreads();
            if (tid < 256) {
                int before = 0;
                for (int v = 0; v < w; ++v) before += redi[v];
                run[tid] = before + inc - hv;
            }
            __syncthreads();
            const int sh = 8 * p;
            for (int c = 0; c < N; c += AP_CH) {
                unsigned key[AP_IT], pay[AP_IT];
                unsigned long long peers[AP_IT];
                int dig[AP_IT];
#pragma unroll
                for (int j = 0; j < AP_IT; ++j) {
                    const int e = c + j * AP_NT + tid;
                    key[j] = 0u;
                    pay[j] = 0u;
                    if (e < N) {
                        if (ident) {
                            key[j] = desc_key(sc[e]);
                            pay[j] = (unsigned)e | (tg[e] ? TRUTH : 0u);
                        } else {
                            key[j] = ks[e];
                            pay[j] = ps[e];
                        }
                    }
                }
                for (int i = tid; i < AP_SLOTS * 256; i += AP_NT) cnt[i] = 0;
                __syncthreads();
#pragma unroll
                for (int j = 0; j < AP_IT; ++j) {
                    const bool valid = c + j * AP_NT + tid < N;
                    const int d = (int)((key[j] >> sh) & 255u);
                    unsigned long long m = __ballot(valid);
#pragma unroll
                    for (int bit = 0; bit < 8; ++bit) {
                        const unsigned long long bb = __ballot(valid && ((d >> bit) & 1));
                        m &= ((d >> bit) & 1) ? bb : ~bb;
                    }
                    peers[j] = m;
                    dig[j] = d;
                    if (valid && __ffsll((long long)m) - 1 == lane) cnt[(j * AP_W + w) * 256 + d] = __popcll(m);
                }
                __syncthreads();
                if (tid < 256) {
                    int r = run[tid];
                    for (int s = 0; s < AP_SLOTS; ++s) {
                        const int v = cnt[s * 256 + tid];
                        cnt[s * 256 + tid] = r;
                        r += v;
                    }
                    run[tid] = r;
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < AP_IT; ++j) {
                    if (c + j * AP_NT + tid < N) {
                        const int dst = cnt[(j * AP_W + w) * 256 + dig[j]] + __popcll(peers[j] & below);
                        kd[dst] = key[j];
                        pd[dst] = pay[j];
                    }
                }
                __syncthreads();
            }
            ident = false;
            ks = kd;
            ps = pd;
            kd = kd == KA ? KB : KA;
            pd = pd == PA ? PB : PA;
        }

        // 3. AP over the sorted rows; thread tid takes AP_IT consecutive rows of each chunk
        int tp_run = 0;
        double wr_run = 0.0, wt_run = 0.0, psum = 0.0;
        for (int c = 0; c < N; c += AP_CH) {
            const int e0 = c + tid * AP_IT;
            unsigned pay[AP_IT];
            int npos = 0;
#pragma unroll
            for (int j = 0; j < AP_IT; ++j) {
                const int e = e0 + j;
                pay[j] = 0u;
                if (e < N) pay[j] = ident ? ((unsigned)e | (tg[e] ? TRUTH : 0u)) : ps[e];
                npos += (int)(pay[j] >> 31);
            }
            int ctot;
            const int cex = block_excl_scan(npos, redi, &ctot);
            if (weights == nullptr) {
                int tp = tp_run + cex;
#pragma unroll
                for (int j = 0; j < AP_IT; ++j) {
                    if (pay[j] >> 31) {
                        ++tp;
                        psum += (double)((float)tp / (float)(e0 + j + 1));
                    }
                }
            } else {
                double wv[AP_IT], ws_ = 0.0, wts = 0.0;
#pragma unroll
                for (int j = 0; j < AP_IT; ++j) {
                    wv[j] = e0 + j < N ? (double)weights[pay[j] & ~TRUTH] : 0.0;
                    ws_ += wv[j];
                    if (pay[j] >> 31) wts += wv[j];
                }
                double wtot, ttot;
                double rk = wr_run + block_excl_scan(ws_, redd, &wtot);
                double tp = wt_run + block_excl_scan(wts, redd, &ttot);
#pragma unroll
                for (int j = 0; j < AP_IT; ++j) {
                    rk += wv[j];
                    if (pay[j] >> 31) {
                        tp += wv[j];
                        psum += tp / rk;
                    }
                }
                wr_run += wtot;
                wt_run += ttot;
            }
            tp_run += ctot;
        }
        double ptot;
        block_excl_scan(psum, redd, &ptot);
        if (tid == 0) ap[k] = (float)(ptot / (double)(tp_run > 1 ? tp_run : 1));
    }
}

}  // namespace

extern "C" int x3deval_ap_reset(int* state, int capacity, void* stream) {
    X3DEVAL_CHECK_ARG(state && capacity >= 0 && capacity <= X3DEVAL_MAX_CAPACITY);
    hipLaunchKernelGGL(ap_state_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, capacity, 1);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" int x3deval_ap_set_capacity(int* state, int capacity, void* stream) {
    X3DEVAL_CHECK_ARG(state && capacity >= 0 && capacity <= X3DEVAL_MAX_CAPACITY);
    hipLaunchKernelGGL(ap_state_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, capacity, 0);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" int x3deval_ap_append(int* state, float* scores, uint8_t* targets, float* weights_out, int K,
                                 const float* in_scores, const float* in_targets, const float* in_weights, int n,
                                 void* stream) {
    X3DEVAL_CHECK_ARG(state && scores && targets && in_scores && in_targets && K > 0 && n >= 0);
    X3DEVAL_CHECK_ARG((weights_out == nullptr) == (in_weights == nullptr));
    X3DEVAL_CHECK_ARG((long long)n * K <= 0x7fffffffLL);
    if (n == 0) return X3DEVAL_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ap_reserve_kernel, dim3(1), dim3(64), 0, s, state, n);
    hipLaunchKernelGGL(ap_append_kernel, dim3(eval_cdiv(n, 64), eval_cdiv(K, 64)), dim3(256), 0, s, state, scores, targets,
                       weights_out, K, in_scores, in_targets, in_weights, n);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" int x3deval_ap_append_crops(int* state, float* scores, uint8_t* targets, int K, const float* logits,
                                       const float* in_targets, float* maxlogit, int b, int n_crops, void* stream) {
    X3DEVAL_CHECK_ARG(state && scores && targets && logits && in_targets && maxlogit && K > 0 && b > 0 && n_crops > 0);
    X3DEVAL_CHECK_ARG((long long)b * n_crops * K <= 0x7fffffffLL);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ap_reserve_kernel, dim3(1), dim3(64), 0, s, state, b);
    hipLaunchKernelGGL(ap_crops_kernel, dim3(eval_cdiv(b * K, 256)), dim3(256), 0, s, state, scores, targets, K, logits,
                       in_targets, maxlogit, b, n_crops);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" int x3deval_ap_append_frames(int* state, int* rowoff, float* scores, uint8_t* targets, int K, const float* logits,
                                        const float* labels, const float* masks, int B, int T, int TL, void* stream) {
    X3DEVAL_CHECK_ARG(state && rowoff && scores && targets && logits && labels && masks);
    X3DEVAL_CHECK_ARG(K > 0 && B > 0 && B <= X3DEVAL_MAX_FRAMES_B && T > 0 && TL > 0);
    X3DEVAL_CHECK_ARG((long long)B * K * (T > TL ? T : TL) <= 0x7fffffffLL);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ap_frames_reserve_kernel, dim3(1), dim3(256), 0, s, state, rowoff, masks, B, TL);
    hipLaunchKernelGGL(ap_frames_kernel, dim3(eval_cdiv(K * TL, 256), B), dim3(256), 0, s, state, rowoff, scores, targets, K,
                       logits, labels, masks, T, TL);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}

extern "C" size_t x3deval_ap_workspace_bytes(int K, int capacity) {
    if (K <= 0 || capacity <= 0 || capacity > X3DEVAL_MAX_CAPACITY) return 0;
    const size_t per = ws_slot_bytes(capacity);
    size_t slots = WS_CAP_BYTES / per;
    if (slots < 1) slots = 1;
    if (slots > (size_t)K) slots = (size_t)K;
    return slots * per;
}

extern "C" int x3deval_ap_value(const int* state, const float* scores, const uint8_t* targets, const float* weights, int K,
                                int capacity, void* workspace, size_t workspace_bytes, float* ap, void* stream) {
    X3DEVAL_CHECK_ARG(state && scores && targets && workspace && ap && K > 0);
    X3DEVAL_CHECK_ARG(capacity > 0 && capacity <= X3DEVAL_MAX_CAPACITY);
    const size_t per = ws_slot_bytes(capacity);
    X3DEVAL_CHECK_ARG(workspace_bytes >= per);
    size_t slots = workspace_bytes / per;
    const int grid = slots < (size_t)K ? (int)slots : K;
    hipLaunchKernelGGL(ap_value_kernel, dim3(grid), dim3(AP_NT), 0, (hipStream_t)stream, state, scores, targets, weights, K,
                       capacity, (unsigned*)workspace, ap);
    X3DEVAL_LAUNCH_CHECK();
    return X3DEVAL_OK;
}
