// The host side of libx3dmix (include/x3dmix.h), plain C++: the error text, the argument checks of every entry point and
// the serial twins, which run the element rules of mix_core.h one element after the other and, for the soft-target cross
// entropy, add up in the order the kernel's 256 threads and 4 waves do.
#include <stdarg.h>
#include <stdio.h>

#include "mix_priv.h"

using namespace x3dm;

static thread_local char g_error[512] = "";

void x3dmix_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

extern "C" int x3dmix_abi_version(void) { return X3DMIX_ABI_VERSION; }
extern "C" const char* x3dmix_last_error(void) { return g_error; }
extern "C" size_t x3dmix_sample_bytes(void) { return sizeof(X3DMixSample); }

static_assert(sizeof(X3DMixSample) == 32, "the plan entry is 32 bytes");

// -- the argument checks ---------------------------------------------------------------------------------------------------
int x3dmix_check_clips(const char* who, const float* src, const float* dst, const X3DMixSample* plan, int B, int planes,
                       int H, int W) {
    if (!src || !dst || !plan) {
        x3dmix_set_error("%s: null pointer", who);
        return X3DMIX_EINVAL;
    }
    if (B < 1 || planes < 1 || H < 1 || W < 1) {
        x3dmix_set_error("%s: B, planes, H, W = %d, %d, %d, %d must be positive", who, B, planes, H, W);
        return X3DMIX_EINVAL;
    }
    const int64_t n = (int64_t)planes * H * W;
    if (n >= ((int64_t)1 << 31)) {
        x3dmix_set_error("%s: a clip of %lld elements (2^31 or more)", who, (long long)n);
        return X3DMIX_EINVAL;
    }
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 3) || ((uintptr_t)plan & 3)) {
        x3dmix_set_error("%s: a pointer is not 4-byte aligned", who);
        return X3DMIX_EINVAL;
    }
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)B * sizeof(float);
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    if (s0 < d0 + bytes && d0 < s0 + bytes) {
        x3dmix_set_error("%s: src and dst overlap (the mix is out of place)", who);
        return X3DMIX_EINVAL;
    }
    return X3DMIX_OK;
}

int x3dmix_check_targets(const char* who, const int64_t* labels, const X3DMixSample* plan, int B, int C, float smoothing,
                         const float* targets) {
    if (!labels || !plan || !targets) {
        x3dmix_set_error("%s: null pointer", who);
        return X3DMIX_EINVAL;
    }
    if (B < 1 || C < 1) {
        x3dmix_set_error("%s: B, C = %d, %d must be positive", who, B, C);
        return X3DMIX_EINVAL;
    }
    if (!(smoothing >= 0.0f && smoothing < 1.0f)) {
        x3dmix_set_error("%s: smoothing %g outside [0, 1)", who, (double)smoothing);
        return X3DMIX_EINVAL;
    }
    if (((uintptr_t)labels & 7) || ((uintptr_t)targets & 3) || ((uintptr_t)plan & 3)) {
        x3dmix_set_error("%s: a pointer is not aligned to its element", who);
        return X3DMIX_EINVAL;
    }
    return X3DMIX_OK;
}

int x3dmix_check_soft_ce(const char* who, const float* logits, const float* targets, const float* loss,
                         const float* dlogits, const float* scratch, int R, int C, float grad_scale) {
    if (!logits || !targets || !loss || !dlogits || !scratch) {
        x3dmix_set_error("%s: null pointer", who);
        return X3DMIX_EINVAL;
    }
    if (R < 1 || C < 1) {
        x3dmix_set_error("%s: R, C = %d, %d must be positive", who, R, C);
        return X3DMIX_EINVAL;
    }
    if (!(grad_scale == grad_scale) || grad_scale - grad_scale != 0.0f) {
        x3dmix_set_error("%s: grad_scale is not finite", who);
        return X3DMIX_EINVAL;
    }
    if (((uintptr_t)logits | (uintptr_t)targets | (uintptr_t)loss | (uintptr_t)dlogits | (uintptr_t)scratch) & 3) {
        x3dmix_set_error("%s: a pointer is not 4-byte aligned", who);
        return X3DMIX_EINVAL;
    }
    return X3DMIX_OK;
}

// -- the twins -------------------------------------------------------------------------------------------------------------
extern "C" int x3dmix_clips_host(const float* src, float* dst, const X3DMixSample* plan, int B, int planes, int H, int W) {
    const int rc = x3dmix_check_clips("x3dmix_clips_host", src, dst, plan, B, planes, H, W);
    if (rc) return rc;
    const size_t n = (size_t)planes * H * W;
    for (int b = 0; b < B; ++b) {
        const Sample s = resolve(plan[b], b, B, H, W);
        const float* a = src + (size_t)b * n;
        const float* q = src + (size_t)s.p * n;
        float* o = dst + (size_t)b * n;
        if (s.mode == kCopy) {
            for (size_t i = 0; i < n; ++i) o[i] = a[i];
        } else if (s.mode == kMixup) {
            for (size_t i = 0; i < n; ++i) o[i] = mixup_elem(s, a[i], q[i]);
        } else {
            int y = 0, x = 0;
            for (size_t i = 0; i < n; ++i) {
                o[i] = in_box(s, y, x) ? q[i] : a[i];
                plane_next(H, W, &y, &x);
            }
        }
    }
    return X3DMIX_OK;
}

extern "C" int x3dmix_targets_host(const int64_t* labels, const X3DMixSample* plan, int B, int C, float smoothing,
                                   float* targets) {
    const int rc = x3dmix_check_targets("x3dmix_targets_host", labels, plan, B, C, smoothing, targets);
    if (rc) return rc;
    const Smooth sm = smooth_rule(smoothing, C);
    for (int b = 0; b < B; ++b) {
        const Sample s = resolve(plan[b], b, B, 1, 1);
        const int64_t yo = labels[b], yp = labels[s.p];
        for (int c = 0; c < C; ++c) targets[(size_t)b * C + c] = target_elem(sm, s.lam, s.om, c, yo, yp);
    }
    return X3DMIX_OK;
}

// The sum of the kernel's 256 per-thread values: a wave's 64 by the exchange with lane ^ 32, ^ 16, .. ^ 1 (after which every
// lane holds the wave's sum), then (wave 0 + wave 1) + (wave 2 + wave 3).
template <class T>
static T block_sum(T* v) {
    T w[4];
    for (int wave = 0; wave < 4; ++wave) {
        T* l = v + wave * kLanes;
        for (int o = kLanes / 2; o > 0; o >>= 1) {
            T next[kLanes];
            for (int i = 0; i < kLanes; ++i) next[i] = l[i] + l[i ^ o];
            for (int i = 0; i < kLanes; ++i) l[i] = next[i];
        }
        w[wave] = l[0];
    }
    return (w[0] + w[1]) + (w[2] + w[3]);
}

extern "C" int x3dmix_soft_ce_host(const float* logits, const float* targets, float* loss, float* dlogits, float* scratch,
                                   int R, int C, float grad_scale, unsigned long long* rng) {
    const int rc = x3dmix_check_soft_ce("x3dmix_soft_ce_host", logits, targets, loss, dlogits, scratch, R, C, grad_scale);
    if (rc) return rc;
    const float scale = ce_scale(grad_scale, R);
    for (int r = 0; r < R; ++r) {
        const float* z = logits + (size_t)r * C;
        const float* t = targets + (size_t)r * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
        float ps[kRowThreads], pt[kRowThreads], pl[kRowThreads];
        for (int tid = 0; tid < kRowThreads; ++tid) {
            float s = 0.f, st = 0.f;
            for (int c = tid; c < C; c += kRowThreads) {
                s += ce_exp(z[c], m);
                st += t[c];
            }
            ps[tid] = s;
            pt[tid] = st;
        }
        const float s = block_sum(ps), St = block_sum(pt);
        const float lse = ce_lse(m, s);
        for (int tid = 0; tid < kRowThreads; ++tid) {
            float l = 0.f;
            for (int c = tid; c < C; c += kRowThreads) l += ce_term(t[c], lse, z[c]);
            pl[tid] = l;
        }
        scratch[r] = block_sum(pl);
        for (int c = 0; c < C; ++c) dlogits[(size_t)r * C + c] = ce_grad(z[c], m, s, St, t[c], scale);
    }
    double pd[kRowThreads];
    for (int tid = 0; tid < kRowThreads; ++tid) {
        double s = 0.0;
        for (int i = tid; i < R; i += kRowThreads) s += (double)scratch[i];
        pd[tid] = s;
    }
    loss[0] = (float)(block_sum(pd) / (double)R);
    if (rng) rng[1] += 1ull;
    return X3DMIX_OK;
}
