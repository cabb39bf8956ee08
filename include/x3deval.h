/*
 * x3deval.h -- C ABI of libx3deval.so: HIP kernels (gfx950 / MI355X) of the evaluation path, a device-resident
 * average-precision meter (the reference's apmeter.APMeter, apmeter.py:98-136) and the appends of the two Charades scripts
 * (train_x3d_charades.py:150-183, train_x3d_charades_loc.py:152-186).
 *
 * A separate library from libx3dhip.so on purpose: tools/stamp.py and the gradient-hash record hash the training library's
 * sources, and the meter never runs inside a training step.
 *
 * Conventions (as include/x3dhip.h)
 *   - plain pointers and sizes; the caller (torch) owns every buffer; every kernel is enqueued on the hipStream_t passed
 *     as `stream`; the append entry points never allocate and never synchronise (they may be captured into a graph)
 *   - return 0 on success, negative X3DEVAL_E* on failure; x3deval_last_error() gives the message (thread-local)
 *   - deterministic bit for bit: integer counters only where order cannot change a result, no float atomics
 *
 * The meter
 *   state    int32 [X3DEVAL_STATE_INTS] on the device: the row count, the capacity and two sticky flags (layout below)
 *   scores   fp32  [K, capacity]   class-major, so that each class is one contiguous segment
 *   targets  uint8 [K, capacity]   0 / 1
 *   weights  fp32  [capacity]      optional (NULL: an unweighted meter)
 * Rows are appended at the device-resident count.  An append that would pass the device capacity writes nothing and
 * sets X3DEVAL_S_OVERFLOW; a target other than 0 / 1 or a weight that is negative or NaN sets X3DEVAL_S_BAD.
 * x3deval_ap_value writes NaN for every class while either flag is set.
 */
#ifndef X3DEVAL_H
#define X3DEVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X3DEVAL_ABI_VERSION 1

#define X3DEVAL_OK 0
#define X3DEVAL_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define X3DEVAL_ELAUNCH (-2)  /* hipLaunch error */

/* state words */
#define X3DEVAL_S_COUNT 0     /* rows appended so far */
#define X3DEVAL_S_CAPACITY 1  /* rows the buffers hold */
#define X3DEVAL_S_OVERFLOW 2  /* sticky: an append did not fit */
#define X3DEVAL_S_BAD 3       /* sticky: a non-binary target or a negative / NaN weight */
#define X3DEVAL_S_BASE 4      /* first row of the append in flight */
#define X3DEVAL_S_GO 5        /* 1 when the append in flight fits */
#define X3DEVAL_STATE_INTS 8

#define X3DEVAL_MAX_CAPACITY 0x7fffffc0   /* row indices are 31-bit in the sort payload */
#define X3DEVAL_MAX_FRAMES_B 1024         /* samples per x3deval_ap_append_frames call */

int x3deval_abi_version(void);
const char* x3deval_last_error(void);

/* count := 0, flags := 0, capacity := capacity */
int x3deval_ap_reset(int* state, int capacity, void* stream);
/* capacity := capacity (after the caller has grown the buffers to [K, capacity]; the count and flags are kept) */
int x3deval_ap_set_capacity(int* state, int capacity, void* stream);

/* apmeter.py:30-96 add(): n rows of scores [n, K] and targets [n, K] (fp32, 0 / 1), weights [n] or NULL.
 * weights_out must be non-NULL exactly when in_weights is. */
int x3deval_ap_append(int* state, float* scores, uint8_t* targets, float* weights_out, int K, const float* in_scores,
                      const float* in_targets, const float* in_weights, int n, void* stream);

/* Crop-max rows (train_x3d_charades.py:150-183): logits [b * n_crops, K] (crops of a sample adjacent), targets [b, K];
 * appends probs[i, k] = max_j sigmoid(logits[i * n_crops + j, k]) and writes maxlogit[i, k] = max_j logits[.., k]. */
int x3deval_ap_append_crops(int* state, float* scores, uint8_t* targets, int K, const float* logits,
                            const float* in_targets, float* maxlogit, int b, int n_crops, void* stream);

/* Per-frame rows (train_x3d_charades_loc.py:165-186): logits [B, K, T] (before interpolation), labels [B, K, TL] (0 / 1),
 * masks [B, TL].  valid_t[b] = (int) sum_t masks[b, t] clamped to [0, TL]; rows (b, t < valid_t[b]) are appended in b-major
 * order with scores sigmoid(interp(logits)[b, k, t]) * masks[b, t] (F.interpolate(mode='linear'), align_corners False).
 * rowoff: int32 [B + 1] scratch (the per-sample row offsets, computed on the device).  B <= X3DEVAL_MAX_FRAMES_B. */
int x3deval_ap_append_frames(int* state, int* rowoff, float* scores, uint8_t* targets, int K, const float* logits,
                             const float* labels, const float* masks, int B, int T, int TL, void* stream);

/* Bytes of the sort workspace x3deval_ap_value needs for K classes at this capacity (host only).  Classes are sorted in
 * batches when K * capacity would pass a fixed cap. */
size_t x3deval_ap_workspace_bytes(int K, int capacity);

/* apmeter.py:98-136 value(): ap [K] fp32.  Per class a stable descending LSD radix sort of the scores (-0.0 ties +0.0,
 * NaN above +inf), then AP = sum over the positives of tp_i / rank_i, divided by max(positives, 1); rank_i = i and
 * tp_i = positives up to i, or their weighted sums.  workspace: x3deval_ap_workspace_bytes(K, capacity) bytes. */
int x3deval_ap_value(const int* state, const float* scores, const uint8_t* targets, const float* weights, int K,
                     int capacity, void* workspace, size_t workspace_bytes, float* ap, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X3DEVAL_H */
