// The kernels of libx3dmix (include/x3dmix.h) for gfx950.  The element rules, the meaning of a plan entry and the terms of the
// cross entropy are mix_core.h's, shared with the CPU twins of mix_host.cpp.  No atomics, no allocation, no synchronisation.
#include "mix_priv.h"

using namespace x3dm;

#define X3DMIX_LAUNCH_CHECK()                                                                                  \
    do {                                                                                                       \
        hipError_t e_ = hipGetLastError();                                                                     \
        if (e_ != hipSuccess) {                                                                                \
            x3dmix_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e_));           \
            return X3DMIX_ELAUNCH;                                                                             \
        }                                                                                                      \
    } while (0)

// -- x3dmix_clips ------------------------------------------------------------------------------------------------------------
// A clip of n floats is cut at the 16-byte grid of its OUTPUT: `head` elements (0..3) before the first aligned address, then
// groups of four, then up to three elements.  A run is kClipThreads * kClipPieces groups of one sample (16 KB of output); a
// workgroup takes the runs blockIdx.x, blockIdx.x + gridDim.x, ..: sample and plan entry are the same for the whole
// workgroup, so the entry is read once per wave through uniform loads and the mode is one uniform branch.  A lane's groups
// are kClipThreads apart, so that a wave moves whole 1 KB runs, and all of a lane's loads are issued before its first
// store.  Stores are always 16 bytes; the loads of the sample and of the partner are 16 bytes each where their own address
// at `head` falls on the grid (always, when the base is aligned and n is a multiple of 4), and four 4-byte loads otherwise
// (a clip of 3 T 79 79 floats, a view that starts one float into a buffer).  The first run of a sample also takes the head
// and the tail, one element per thread.
constexpr int kClipThreads = 256;
constexpr int kClipPieces = 4;
constexpr int kClipRun = kClipThreads * kClipPieces;      // groups per run
constexpr int kClipMaxBlocks = 1024;                      // four workgroups for each of the 256 CUs

struct ClipGeom {
    int64_t n;            // elements of a clip
    int B, H, W;
    int runs_per_clip;
};

static __device__ __forceinline__ float4 load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const float4*>(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

// is any / which of the four elements from i on lie in the box: bit e for element i + e
static __device__ __forceinline__ unsigned box_mask(const Sample& s, uint32_t i, int H, int W) {
    int y, x;
    plane_pos(i, H, W, &y, &x);
    unsigned m = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        m |= in_box(s, y, x) ? 1u << e : 0u;
        plane_next(H, W, &y, &x);
    }
    return m;
}

__global__ __launch_bounds__(kClipThreads) void x3dmix_clips_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                                    const X3DMixSample* __restrict__ plan, ClipGeom g) {
    const int tid = threadIdx.x;
    const int64_t total = (int64_t)g.B * g.runs_per_clip;
    for (int64_t run = blockIdx.x; run < total; run += gridDim.x) {
        const int b = (int)(run / g.runs_per_clip), r = (int)(run - (int64_t)b * g.runs_per_clip);
        const Sample s = resolve(plan[b], b, g.B, g.H, g.W);              // uniform: one look per wave
        const float* a = src + (int64_t)b * g.n;
        const float* q = src + (int64_t)s.p * g.n;
        float* o = dst + (int64_t)b * g.n;
        int64_t head = (int64_t)((16 - ((uintptr_t)o & 15)) & 15) >> 2;
        if (head > g.n) head = g.n;
        const int64_t groups = (g.n - head) >> 2, tail = head + 4 * groups;
        const bool avec = ((uintptr_t)(a + head) & 15) == 0, qvec = ((uintptr_t)(q + head) & 15) == 0;
        const int64_t g0 = (int64_t)r * kClipRun + tid;

        float4 va[kClipPieces], vq[kClipPieces];
        unsigned in[kClipPieces];
#pragma unroll
        for (int k = 0; k < kClipPieces; ++k) {
            const int64_t gi = g0 + (int64_t)k * kClipThreads;
            in[k] = 0;
            if (gi < groups) {
                const int64_t i = head + 4 * gi;
                va[k] = load4(a + i, avec);
                if (s.mode == kMixup) {
                    vq[k] = load4(q + i, qvec);
                } else if (s.mode == kCutmix) {
                    in[k] = box_mask(s, (uint32_t)i, g.H, g.W);
                    if (in[k]) vq[k] = load4(q + i, qvec);                // the partner only where the box is
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kClipPieces; ++k) {
            const int64_t gi = g0 + (int64_t)k * kClipThreads;
            if (gi < groups) {
                float4 v = va[k];
                if (s.mode == kMixup) {
                    v.x = mixup_elem(s, va[k].x, vq[k].x);
                    v.y = mixup_elem(s, va[k].y, vq[k].y);
                    v.z = mixup_elem(s, va[k].z, vq[k].z);
                    v.w = mixup_elem(s, va[k].w, vq[k].w);
                } else if (in[k]) {                                       // a select, never arithmetic
                    v.x = in[k] & 1u ? vq[k].x : v.x;
                    v.y = in[k] & 2u ? vq[k].y : v.y;
                    v.z = in[k] & 4u ? vq[k].z : v.z;
                    v.w = in[k] & 8u ? vq[k].w : v.w;
                }
                *reinterpret_cast<float4*>(o + head + 4 * gi) = v;
            }
        }
        if (r == 0) {                                  // at most three elements before the groups and three after
            const int64_t i = tid < head ? tid : tail + (tid - head);
            if (tid < head + (g.n - tail)) {
                float v = a[i];
                if (s.mode == kMixup) {
                    v = mixup_elem(s, v, q[i]);
                } else if (s.mode == kCutmix) {
                    int y, x;
                    plane_pos((uint32_t)i, g.H, g.W, &y, &x);
                    if (in_box(s, y, x)) v = q[i];
                }
                o[i] = v;
            }
        }
    }
}

extern "C" int x3dmix_clips(const float* src, float* dst, const X3DMixSample* plan, int B, int planes, int H, int W,
                            void* stream) {
    const int rc = x3dmix_check_clips("x3dmix_clips", src, dst, plan, B, planes, H, W);
    if (rc) return rc;
    ClipGeom g;
    g.n = (int64_t)planes * H * W;
    g.B = B;
    g.H = H;
    g.W = W;
    // the groups of a clip are at most n / 4 wherever its head falls; a clip of fewer than four elements still has a run
    const int64_t rpc = (g.n / 4 + kClipRun - 1) / kClipRun;
    g.runs_per_clip = (int)(rpc > 0 ? rpc : 1);
    const int64_t total = (int64_t)B * g.runs_per_clip;
    const unsigned blocks = (unsigned)(total < kClipMaxBlocks ? total : kClipMaxBlocks);
    x3dmix_clips_kernel<<<blocks, kClipThreads, 0, (hipStream_t)stream>>>(src, dst, plan, g);
    X3DMIX_LAUNCH_CHECK();
    return X3DMIX_OK;
}

// -- x3dmix_targets ----------------------------------------------------------------------------------------------------------
// A workgroup takes 256 classes of one sample: the plan entry and the two labels are uniform loads.
constexpr int kTargetThreads = 256;

__global__ __launch_bounds__(kTargetThreads) void x3dmix_targets_kernel(const int64_t* __restrict__ labels,
                                                                        const X3DMixSample* __restrict__ plan, int B, int C,
                                                                        int chunks, Smooth sm, float* __restrict__ targets) {
    const int b = blockIdx.x / chunks, c = (blockIdx.x - b * chunks) * kTargetThreads + threadIdx.x;
    const Sample s = resolve(plan[b], b, B, 1, 1);
    const int64_t yo = labels[b], yp = labels[s.p];
    if (c < C) targets[(int64_t)b * C + c] = target_elem(sm, s.lam, s.om, c, yo, yp);
}

extern "C" int x3dmix_targets(const int64_t* labels, const X3DMixSample* plan, int B, int C, float smoothing, float* targets,
                              void* stream) {
    const int rc = x3dmix_check_targets("x3dmix_targets", labels, plan, B, C, smoothing, targets);
    if (rc) return rc;
    const int chunks = (C + kTargetThreads - 1) / kTargetThreads;
    if ((int64_t)B * chunks > 0x7fffffff) {
        x3dmix_set_error("x3dmix_targets: B * ceil(C / 256) = %lld workgroups", (long long)B * chunks);
        return X3DMIX_EINVAL;
    }
    x3dmix_targets_kernel<<<(unsigned)(B * chunks), kTargetThreads, 0, (hipStream_t)stream>>>(labels, plan, B, C, chunks,
                                                                                               smooth_rule(smoothing, C),
                                                                                               targets);
    X3DMIX_LAUNCH_CHECK();
    return X3DMIX_OK;
}

// -- x3dmix_soft_ce ----------------------------------------------------------------------------------------------------------
template <class T>
static __device__ __forceinline__ T wave_sum(T v) {
    for (int o = kLanes / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, kLanes);
    return v;
}

// the sum over the workgroup's 256 threads, the same in every thread: (wave 0 + wave 1) + (wave 2 + wave 3)
template <class T>
static __device__ __forceinline__ T block_sum(T v, T* red) {
    v = wave_sum(v);
    __syncthreads();                                   // the readers of the sum before are done with red
    if ((threadIdx.x & (kLanes - 1)) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// launch 1: a workgroup per row.  Thread t takes the classes t, t + 256, ..
__global__ __launch_bounds__(kRowThreads) void x3dmix_soft_ce_rows_kernel(const float* __restrict__ logits,
                                                                          const float* __restrict__ targets,
                                                                          float* __restrict__ loss_rows,
                                                                          float* __restrict__ dlogits, int C, float scale) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const float* z = logits + (int64_t)blockIdx.x * C;
    const float* t = targets + (int64_t)blockIdx.x * C;
    float m = -INFINITY;
    for (int c = tid; c < C; c += kRowThreads) m = fmaxf(m, z[c]);
    for (int o = kLanes / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, kLanes));
    if ((tid & (kLanes - 1)) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float s = 0.f, St = 0.f;
    for (int c = tid; c < C; c += kRowThreads) {
        s += ce_exp(z[c], m);
        St += t[c];
    }
    s = block_sum(s, red);
    St = block_sum(St, red);
    const float lse = ce_lse(m, s);
    float l = 0.f;
    for (int c = tid; c < C; c += kRowThreads) l += ce_term(t[c], lse, z[c]);
    l = block_sum(l, red);
    if (tid == 0) loss_rows[blockIdx.x] = l;
    float* d = dlogits + (int64_t)blockIdx.x * C;
    for (int c = tid; c < C; c += kRowThreads) d[c] = ce_grad(z[c], m, s, St, t[c], scale);
}

// launch 2: one workgroup; the mean of the rows in fp64, rounded once, and the head's draw counter
__global__ __launch_bounds__(kRowThreads) void x3dmix_soft_ce_mean_kernel(const float* __restrict__ loss_rows, int R,
                                                                          float* __restrict__ loss,
                                                                          unsigned long long* __restrict__ rng) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < R; i += kRowThreads) s += (double)loss_rows[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        loss[0] = (float)(s / (double)R);
        if (rng != nullptr) rng[1] += 1ull;
    }
}

extern "C" int x3dmix_soft_ce(const float* logits, const float* targets, float* loss, float* dlogits, float* scratch, int R,
                              int C, float grad_scale, unsigned long long* rng, void* stream) {
    const int rc = x3dmix_check_soft_ce("x3dmix_soft_ce", logits, targets, loss, dlogits, scratch, R, C, grad_scale);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    x3dmix_soft_ce_rows_kernel<<<(unsigned)R, kRowThreads, 0, st>>>(logits, targets, scratch, dlogits, C,
                                                                    ce_scale(grad_scale, R));
    X3DMIX_LAUNCH_CHECK();
    x3dmix_soft_ce_mean_kernel<<<1, kRowThreads, 0, st>>>(scratch, R, loss, rng);
    X3DMIX_LAUNCH_CHECK();
    return X3DMIX_OK;
}
