// The arithmetic of libx3dmix (include/x3dmix.h), compiled into the kernels (mix.hip) and into the serial twins
// (mix_host.cpp): what a plan entry means for a sample, the element rules of mixup, CutMix and the soft targets, and the
// terms of the soft-target cross entropy.  Built with -ffp-contract=off on both sides: every fused multiply-add below is
// written as one, and nothing else is contracted.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/x3dmix.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MIX_HD __host__ __device__ static inline
#else
#define MIX_HD static inline
#endif

namespace x3dm {

constexpr int kLanes = 64;        // lanes of a wave
constexpr int kRowThreads = 256;  // threads of a soft_ce row: the partition of its sums (the twin walks the same one)

enum Mode { kCopy = 0, kMixup = 1, kCutmix = 2 };

// A plan entry as the sample uses it: the partner an index that can be followed, the box clipped to the plane.
struct Sample {
    int p;
    int mode;
    float lam, om;                // om = 1.0f - lam
    int y0, y1, x0, x1;
};

MIX_HD Sample resolve(const X3DMixSample& e, int b, int B, int H, int W) {
    Sample s;
    s.p = (e.partner >= 0 && e.partner < B) ? e.partner : b;
    s.lam = e.lam;
    s.om = 1.0f - e.lam;
    s.y0 = e.y0 > 0 ? e.y0 : 0;
    s.x0 = e.x0 > 0 ? e.x0 : 0;
    s.y1 = e.y1 < H ? e.y1 : H;
    s.x1 = e.x1 < W ? e.x1 : W;
    const bool empty = e.y0 >= e.y1 || e.x0 >= e.x1;          // the plan's own box decides the mode ...
    const bool clipped_empty = s.y0 >= s.y1 || s.x0 >= s.x1;  // ... and one that lies outside the plane selects nothing
    if (!empty) {
        s.mode = kCutmix;
        if (clipped_empty) s.y0 = s.y1 = s.x0 = s.x1 = 0;
    } else {
        s.mode = e.lam == 1.0f ? kCopy : kMixup;
    }
    return s;
}

// mixup of one element: a the sample's own, q the partner's
MIX_HD float mixup_elem(const Sample& s, float a, float q) { return fmaf(s.lam, a, s.om * q); }

// CutMix: is (y, x) of a plane inside the box
MIX_HD bool in_box(const Sample& s, int y, int x) { return y >= s.y0 && y < s.y1 && x >= s.x0 && x < s.x1; }

// (y, x) of element i of a clip [planes][H][W]
MIX_HD void plane_pos(uint32_t i, int H, int W, int* y, int* x) {
    const uint32_t row = i / (uint32_t)W;
    *x = (int)(i - row * (uint32_t)W);
    *y = (int)(row % (uint32_t)H);
}

// the position one element further
MIX_HD void plane_next(int H, int W, int* y, int* x) {
    if (++*x == W) {
        *x = 0;
        if (++*y == H) *y = 0;
    }
}

// timm's smoothed one-hot and the mixed target
struct Smooth {
    float on, off;
};

MIX_HD Smooth smooth_rule(float smoothing, int C) {
    Smooth s;
    s.off = smoothing / (float)C;
    s.on = (1.0f - smoothing) + s.off;
    return s;
}

MIX_HD float target_elem(const Smooth& sm, float lam, float om, int64_t c, int64_t y_own, int64_t y_partner) {
    const float so = c == y_own ? sm.on : sm.off;
    const float sp = c == y_partner ? sm.on : sm.off;
    return fmaf(lam, so, om * sp);
}

// soft-target cross entropy: the terms of a row
MIX_HD float ce_exp(float z, float m) { return expf(z - m); }
MIX_HD float ce_lse(float m, float s) { return m + logf(s); }
MIX_HD float ce_term(float t, float lse, float z) { return t * (lse - z); }
MIX_HD float ce_scale(float grad_scale, int R) { return grad_scale / (float)R; }
MIX_HD float ce_grad(float z, float m, float s, float St, float t, float scale) {
    return (ce_exp(z, m) / s * St - t) * scale;
}

}  // namespace x3dm
