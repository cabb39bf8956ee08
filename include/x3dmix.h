/*
 * x3dmix.h -- C ABI of libx3dmix.so: HIP kernels (gfx950 / MI355X) for the batch-mixing half of a video recipe: mixup and
 * CutMix of a batch of clips in one pass, the soft targets that go with them (label smoothing included), and the mean
 * softmax cross entropy against soft targets with its gradient (F.cross_entropy(logits, probabilities)).
 *
 * A separate library from libx3dhip.so on purpose: tools/stamp.py and the gradient-hash record hash the training library's
 * sources, and nothing here changes them.
 *
 * Conventions (as include/x3ddata.h and include/x3dstep.h)
 *   - plain pointers and sizes; the caller (torch) owns every buffer; every kernel is enqueued on the hipStream_t passed
 *     as `stream`; no entry point allocates or synchronises (each may be captured into a graph)
 *   - return 0 on success, negative X3DMIX_E* on failure; x3dmix_last_error() gives the message (thread-local)
 *   - deterministic bit for bit: no atomics, every sum in a fixed order, every output element written exactly once
 *   - the *_host entry points take host pointers only and run the same arithmetic (csrc_mix/mix_core.h)
 *
 * The plan: one X3DMixSample per sample of the batch, device-resident for the kernels.  Nothing in it is trusted with an
 * address: a partner outside [0, B) is taken as the sample itself, and a box is clipped to the plane before it is used.
 */
#ifndef X3DMIX_H
#define X3DMIX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X3DMIX_ABI_VERSION 1

#define X3DMIX_OK 0
#define X3DMIX_EINVAL (-1)   /* bad size / null pointer / overlapping buffers */
#define X3DMIX_ELAUNCH (-2)  /* hipLaunch error */

typedef struct X3DMixSample {
    int32_t partner;          /* index in [0, B) of the sample mixed in */
    float   lam;              /* weight of the sample's own label (and, for mixup, pixels) */
    int32_t y0, y1, x0, x1;   /* CutMix box, half open; empty (y0 >= y1 or x0 >= x1) means mixup */
    int32_t pad[2];
} X3DMixSample;

int x3dmix_abi_version(void);
const char* x3dmix_last_error(void);
size_t x3dmix_sample_bytes(void);   /* sizeof(X3DMixSample) = 32 */

/*
 * dst[b] = the mix of src[b] and src[p], p = plan[b].partner, for fp32 clips [B][planes][H][W] (planes = 3 T); out of place:
 * the ranges of src and dst must not overlap (X3DMIX_EINVAL).  planes * H * W < 2^31.  Per sample, uniformly:
 *   lam == 1.0f and an empty box   dst[b] = src[b] bit for bit; src[p] is not read
 *   an empty box otherwise         dst[b][i] = fmaf(lam, src[b][i], (1.0f - lam) * src[p][i])            (mixup)
 *   a non-empty box                dst[b][i] = src[p][i] inside the box on every plane, src[b][i] outside    (CutMix)
 * CutMix is a select, never arithmetic; the partner is read only where the box is; lam is not used.
 */
int x3dmix_clips(const float* src, float* dst, const X3DMixSample* plan, int B, int planes, int H, int W, void* stream);
int x3dmix_clips_host(const float* src, float* dst, const X3DMixSample* plan, int B, int planes, int H, int W);

/*
 * targets[b][c] = fmaf(lam_b, s(c, y_b), (1.0f - lam_b) * s(c, y_p)) with timm's smoothing in fp32:
 * off = smoothing / (float)C, on = (1.0f - smoothing) + off, s(c, y) = c == y ? on : off.  A label outside [0, C) matches no
 * class.  0 <= smoothing < 1.
 */
int x3dmix_targets(const int64_t* labels, const X3DMixSample* plan, int B, int C, float smoothing, float* targets,
                   void* stream);
int x3dmix_targets_host(const int64_t* labels, const X3DMixSample* plan, int B, int C, float smoothing, float* targets);

/*
 * loss[0] = mean over the R rows of sum_c t_c (lse - z_c), dlogits = (expf(z - m) / s * St - t) * (grad_scale / R), with
 * m = max_c z_c, s = sum_c expf(z_c - m), lse = m + logf(s), St = sum_c t_c (rows need not sum to 1).  scratch: R floats (the
 * rows' losses, summed in fp64 in a fixed order and rounded once).  rng: the head's dropout state {seed, draw counter} or
 * NULL; the last kernel adds one to rng[1].  Two launches.  Non-finite logits are out of scope.  The twin has the same
 * structure on the host's libm: it is not expected to give the device's expf / logf bits.
 */
int x3dmix_soft_ce(const float* logits, const float* targets, float* loss, float* dlogits, float* scratch, int R, int C,
                   float grad_scale, unsigned long long* rng, void* stream);
int x3dmix_soft_ce_host(const float* logits, const float* targets, float* loss, float* dlogits, float* scratch, int R, int C,
                        float grad_scale, unsigned long long* rng);

#ifdef __cplusplus
}
#endif

#endif /* X3DMIX_H */
