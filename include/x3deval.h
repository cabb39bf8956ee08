/*
 * x3deval.h -- C ABI of libx3deval.so: HIP kernels (gfx950 / MI355X) of the evaluation path, a device-resident
 * average-precision meter (the reference's apmeter.APMeter, apmeter.py:98-136), the appends of the two Charades scripts
 * (train_x3d_charades.py:150-183, train_x3d_charades_loc.py:152-186) and a top-k classification meter (the Kinetics
 * validation, train_x3d_kinetics_multigrid.py:253-265).
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

#define X3DEVAL_ABI_VERSION 3

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
#define X3DEVAL_S_BATCHES 6   /* classification meter: append calls that fitted */
#define X3DEVAL_STATE_INTS 8

#define X3DEVAL_MAX_CAPACITY 0x7fffffc0   /* row indices are 31-bit in the sort payload */
#define X3DEVAL_MAX_FRAMES_B 1024         /* samples per x3deval_ap_append_frames call */
#define X3DEVAL_CLS_MAX_K 4096            /* classes of the classification meter */
#define X3DEVAL_CLS_MAX_CROPS 32          /* crops per video of x3deval_cls_append_crops */
#define X3DEVAL_MERGE_MAX_SHARDS 64       /* meters per x3deval_ap_merge call (one lane of a wave each) */
#define X3DEVAL_MERGE_MAX_MARKS (1 << 20) /* segment marks per meter */

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

/*
 * Segment marks and the merge of several meters (data-parallel evaluation: one meter per rank, one AP over all rows).
 *
 * AP is not a sum over ranks: the rows of every rank go through one stable sort, so the merged rows need a defined ORDER.
 * A meter that is to be merged records where each add ended:
 *   marks    int32 [1 + max_marks] on the device: marks[0] = segments so far, marks[1 + j] = X3DEVAL_S_COUNT after
 *            segment j (the ends are non-decreasing; an add that was dropped for capacity ends a segment of length 0)
 *
 * x3deval_ap_mark: call it after every append (same stream; capturable, one thread).  A mark that does not fit
 * (marks[0] >= max_marks) sets X3DEVAL_S_OVERFLOW in `state` and writes nothing else.  marks[0] = 0 starts over.
 * max_marks <= X3DEVAL_MERGE_MAX_MARKS.
 */
int x3deval_ap_mark(int* state, int* marks, int max_marks, void* stream);

/* Bytes of the workspace x3deval_ap_merge needs (host only): the destination offset of every segment and a header.
 * 0 beyond the limits (nshards <= X3DEVAL_MERGE_MAX_SHARDS, max_marks <= X3DEVAL_MERGE_MAX_MARKS). */
size_t x3deval_ap_merge_workspace_bytes(int nshards, int max_marks);

/* Merges W = nshards meters, stacked as an all-gather leaves them, into one:
 *   states int32 [W, X3DEVAL_STATE_INTS], marks int32 [W, 1 + max_marks], scores fp32 [W, K, capacity],
 *   targets uint8 [W, K, capacity], weights fp32 [W, capacity] or NULL (dst_weights is NULL exactly when weights is)
 *   -> dst_state, dst_scores [K, dst_capacity], dst_targets [K, dst_capacity], dst_weights [dst_capacity]
 * With n_r the count of shard r, s_r = marks[r][0], e_{r,j} = marks[r][1 + j] and e_{r,-1} = 0, row i of segment j of
 * shard r lands at destination row off(r, j) + (i - e_{r,j-1}); off(r, j) is the total length of the segments that
 * precede (j, r) in the order SEGMENT INDEX FIRST, SHARD SECOND: (0,0), (0,1), .., (0,W-1), (1,0), ..  A shard with fewer
 * segments is absent from the later rounds.  That is the row order of one process that visits global batch j * W + r, and
 * of DataParallel's per-step chunks.  Destination count = sum of the n_r, capacity word = dst_capacity; the shards'
 * sticky flags are OR-ed into the destination's.
 * A shard whose marks are inconsistent (s_r outside [0, max_marks], ends that are not non-decreasing, a last end != n_r,
 * n_r > capacity) sets X3DEVAL_S_BAD; a total above dst_capacity sets X3DEVAL_S_OVERFLOW; in either case no row is
 * written and the count is 0.
 * Two launches whatever the counts are (a one-workgroup plan, a copy whose grid is sized by `capacity`), no allocation,
 * no synchronisation (capturable); every destination element is stored once, so the result is the same bits run to run.
 * workspace: x3deval_ap_merge_workspace_bytes(nshards, max_marks) bytes.  X3DEVAL_EINVAL beyond the limits above. */
int x3deval_ap_merge(const int* states, const int* marks, const float* scores, const uint8_t* targets,
                     const float* weights, int nshards, int max_marks, int K, int capacity, int* dst_state,
                     float* dst_scores, uint8_t* dst_targets, float* dst_weights, int dst_capacity, void* workspace,
                     size_t workspace_bytes, void* stream);

/*
 * The classification (top-k) meter: the validation arithmetic of train_x3d_kinetics_multigrid.py:253-265, 293-295.
 * The state is the AP meter's (x3deval_ap_reset / x3deval_ap_set_capacity operate on it; X3DEVAL_S_BATCHES counts the
 * append calls that fitted).  One row per video, in five caller-owned arrays of `capacity` elements:
 *   loss fp32, rank int32, pred int32, label int32, batch_rows int32
 *
 * x3deval_cls_append_crops: logits fp32 [b * n_crops, K] (crops of a video adjacent), labels int64 [b].  Per video, in
 * fp64 from the fp32 logits:
 *   s[k] = mean over crops of softmax_k(logits[crop]);  m[k] = mean over crops of logits[crop][k]
 *   loss = logsumexp(m) - m[label], rounded to fp32 once
 *   pred = index of the largest s, the lowest index among equals
 *   rank = #{k : s[k] > s[label]} + #{k < label : s[k] == s[label]}      (top-k correct iff rank < k)
 *   s[label] NaN (s is then NaN in every class): rank = K, pred = -1; loss is what the arithmetic gives
 *   label outside [0, K): rank = K, loss = NaN, X3DEVAL_S_BAD is set
 *   batch_rows = b for every row of the call
 * An append that would pass the device capacity writes nothing and sets X3DEVAL_S_OVERFLOW.
 * K <= X3DEVAL_CLS_MAX_K and n_crops <= X3DEVAL_CLS_MAX_CROPS, X3DEVAL_EINVAL beyond.
 */
int x3deval_cls_append_crops(int* state, float* loss, int* rank, int* pred, int* label, int* batch_rows, int K,
                             const float* logits, const int64_t* labels, int b, int n_crops, void* stream);

/* Totals over the rows, the same bits run to run (one workgroup, sums in a fixed order; integer atomics for the
 * histograms only).  capacity: elements of the row arrays.
 *   totals         int64 [4]  rows, top-1 correct (rank == 0), top-kmax correct (rank < kmax), batches
 *   loss_sums      fp64  [2]  sum_i loss_i, sum_i loss_i / batch_rows_i   (the latter / batches = the mean of batch means)
 *   class_correct  int32 [K]  top-1 correct rows per label;  class_count int32 [K] rows per label
 * While a sticky flag is set: totals = -1, loss_sums = NaN, histograms 0.  pred is not read (it may be NULL). */
int x3deval_cls_value(const int* state, const float* loss, const int* rank, const int* pred, const int* label,
                      const int* batch_rows, int K, int capacity, int kmax, int64_t* totals, double* loss_sums,
                      int* class_correct, int* class_count, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X3DEVAL_H */
