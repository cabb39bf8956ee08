/*
 * x3dstep.h -- C ABI of libx3dstep.so: HIP kernels (gfx950 / MI355X) that look at the flat gradient between the
 * all-reduce and the fused SGD kernel: per-tensor statistics (fp64 sum of squares, count of non-finite elements, a 64-bit
 * hash of the bits), a record of them in a device-resident ring, and clipping by the global norm (the rule of
 * torch.nn.utils.clip_grad_norm_).
 *
 * A separate library from libx3dhip.so on purpose: tools/stamp.py and the gradient-hash record hash the training library's
 * sources, and nothing here changes them.
 *
 * Conventions (as include/x3deval.h)
 *   - plain pointers and sizes; the caller (torch) owns every buffer; every kernel is enqueued on the hipStream_t passed
 *     as `stream`; x3dstep_observe never allocates and never synchronises (it may be captured into a graph)
 *   - return 0 on success, negative X3DSTEP_E* on failure; x3dstep_last_error() gives the message (thread-local)
 *   - deterministic bit for bit: no float atomics, every sum in a fixed order, every output element written once
 *   - the *_host entry points take host pointers only and run the same per-item and per-tensor code (step_core.h)
 *
 * Tables (built once per flat buffer)
 *   seg_off   int64 [S + 1]        tensor s is g[seg_off[s] .. seg_off[s + 1]); seg_off[0] = 0, every tensor has between 1
 *                                  and 2^31 - 1 elements, seg_off[S] = n
 *   items     X3DStepItem [nitems] a tensor cut into pieces of at most X3DSTEP_ITEM elements, the pieces of one tensor
 *                                  consecutive and in order; one wave of launch 1 takes one item
 *   seg_item  int32 [S + 1]        the items of tensor s are items[seg_item[s] .. seg_item[s + 1])
 *
 * The statistics of tensor s with elements x_0 .. x_{k-1}
 *   sumsq      fp64: per item, lane l = ((start mod 4 + j) / 4) mod 64 adds (double) x_j * (double) x_j (an exact product) of
 *              its elements in rising j (start: the item's first element in g, j: the index within the item); the 64 lanes
 *              are summed by halving (l += l + 32, l += l + 16, ..); the items of the tensor are added in item order by one
 *              thread, as the tensors are for the total: both with a compensated (Neumaier) sum, which a step that leaves
 *              the finite numbers drops out of, so that Inf and NaN stay what plain addition gives
 *   nonfinite  int32: elements whose exponent bits are all ones (NaN, +Inf, -Inf)
 *   hash       uint64: sum mod 2^64 over j of splitmix64((j << 32) | bits(x_j)), j the index within the TENSOR;
 *              splitmix64(z): z += 0x9e3779b97f4a7c15; z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;
 *              z = (z ^ z >> 27) * 0x94d049bb133111eb; z ^ z >> 31
 *
 * The record of one step (x3dstep_record_bytes(S) bytes, 8-byte aligned, little-endian)
 *   offset 0                     X3DStepHeader (40 bytes)
 *   offset 40                    fp64   sumsq[S]
 *   offset 40 + 8 S              uint64 hash[S]
 *   offset 40 + 16 S             int32  nonfinite[S]
 *   padded to a multiple of 8
 * The ring holds R records; the step with counter c is written to slot c mod R.
 *
 * The state (int64 [X3DSTEP_STATE_WORDS] on the device; the caller sets it to {0, -1, -1, 0, ..} before the first step)
 *   [X3DSTEP_S_STEP]      steps observed so far (the counter the next record carries)
 *   [X3DSTEP_S_BAD_STEP]  sticky: the first step that had a non-finite element, -1 while there was none
 *   [X3DSTEP_S_BAD_SEG]   sticky: the lowest tensor with a non-finite element at that step, -1 likewise
 *   [X3DSTEP_S_NORM]      the bits of the fp64 norm of the latest step
 *   [X3DSTEP_S_COEF]      low 32 bits: the bits of the fp32 coefficient of the latest step (launch 3 reads it here)
 *   [X3DSTEP_S_SKIP]      1 if the latest x3dstep_apply left the parameters alone, else 0 (x3dstep_keep reads it)
 *   [X3DSTEP_S_SKIPPED]   updates x3dstep_apply skipped so far
 *   [X3DSTEP_S_RUN]       updates skipped in a row; an applied update sets it to 0
 * x3dstep_observe / x3dstep_measure never touch the last three words; only x3dstep_apply writes them.
 *
 * The weight average (x3dstep_ema, x3dstep_ema_keep; the exchange x3dstep_swap, x3dstep_swap_keep)
 *   An exponential moving average of the parameters and of the kept buffers, updated after every applied update by
 *   launches that read the state and never write it: S_STEP - S_SKIPPED is the number of updates applied so far, so the
 *   average needs no counter of its own, skips what x3dstep_apply skipped, and warms its decay up by the count of updates
 *   that were really averaged.  Scoring with the average exchanges it with the live buffers in place, bit for bit, so
 *   that no address a captured graph holds moves.
 */
#ifndef X3DSTEP_H
#define X3DSTEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X3DSTEP_ABI_VERSION 1

#define X3DSTEP_OK 0
#define X3DSTEP_EINVAL (-1)   /* bad size / null or unaligned pointer / inconsistent table */
#define X3DSTEP_ELAUNCH (-2)  /* hipLaunch error */

/* Elements per item.  X3D-M (316 tensors, 3.79 M elements) gives about 2000 items, X3DSTEP_ITEMS_PER_GROUP to a
 * workgroup: about 500 workgroups for the 256 CUs of the card. */
#define X3DSTEP_ITEM 2048
#define X3DSTEP_ITEMS_PER_GROUP 4

#define X3DSTEP_S_STEP 0
#define X3DSTEP_S_BAD_STEP 1
#define X3DSTEP_S_BAD_SEG 2
#define X3DSTEP_S_NORM 3
#define X3DSTEP_S_COEF 4
#define X3DSTEP_S_SKIP 5
#define X3DSTEP_S_SKIPPED 6
#define X3DSTEP_S_RUN 7
#define X3DSTEP_STATE_WORDS 8

#define X3DSTEP_KEEP_SAVE 0
#define X3DSTEP_KEEP_RESTORE 1

#define X3DSTEP_MAX_SEGMENTS (1 << 20)
#define X3DSTEP_MAX_ITEMS 0x7fffff00

typedef struct {
    int64_t start;  /* first element in g */
    int32_t seg;    /* tensor */
    int32_t len;    /* 1 .. X3DSTEP_ITEM */
} X3DStepItem;

typedef struct {
    int64_t step;       /* the counter of this step */
    double total;       /* sum over the tensors, in tensor order, of sumsq[s] */
    double norm;        /* sqrt(total) * inv_world */
    float coef;         /* (float) min(1, max_norm / (norm + 1e-6)) computed in fp64; 1 when max_norm <= 0 */
    int32_t nonfinite;  /* sum of nonfinite[s] */
    int32_t first_bad;  /* the lowest s with nonfinite[s] > 0, or -1 */
    int32_t nseg;       /* S */
} X3DStepHeader;

/* One small buffer x3dstep_keep saves and restores (24 bytes). */
typedef struct {
    int64_t addr;    /* the live buffer: the address of fp32 [len], 4-byte aligned, not null */
    int64_t offset;  /* its first element in snap */
    int32_t len;     /* elements, >= 1 */
    int32_t pad;
} X3DStepKeep;

int x3dstep_abi_version(void);
const char* x3dstep_last_error(void);
size_t x3dstep_item_bytes(void);
size_t x3dstep_keep_bytes(void);
size_t x3dstep_header_bytes(void);
size_t x3dstep_record_bytes(int S);

/* Items the table of this segment table has (host only); negative X3DSTEP_E* when the table is refused. */
int64_t x3dstep_item_count(const int64_t* seg_off, int S);
/* Writes the item table and seg_item [S + 1] (host only, host pointers); `cap`: items the caller allocated.  Returns the
 * count, or negative X3DSTEP_E*. */
int64_t x3dstep_build_items(const int64_t* seg_off, int S, X3DStepItem* items, int64_t cap, int32_t* seg_item);

/* Bytes of the scratch the partials of `nitems` items take (host only): fp64 [nitems], uint64 [nitems], int32 [nitems]. */
size_t x3dstep_workspace_bytes(int64_t nitems);

/*
 * One step: launch 1 (partials: a wave per item), launch 2 (finalize: one workgroup; the record, the state) and, when
 * max_norm > 0, launch 3 (g[i] = g[i] * coef, one fp32 multiply; it leaves at once when coef == 1.0f).
 *   g fp32 [n], 4-byte aligned (16-byte aligned for the vector loads of launch 1; launch 3 vectorises by address);
 *   workspace: x3dstep_workspace_bytes(nitems) bytes, 8-byte aligned; ring: R * x3dstep_record_bytes(S) bytes, 8-byte aligned
 *   inv_world: 1 / world, what the SGD kernel multiplies the summed gradient by
 * coef: NaN and Inf are left as the arithmetic gives them (a NaN norm gives a NaN coefficient, an infinite one 0).
 */
int x3dstep_observe(float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items, const int32_t* seg_item,
                    int64_t nitems, void* workspace, int64_t* state, void* ring, int R, double max_norm, double inv_world,
                    void* stream);

/* The CPU twin: host pointers, the same code item by item and tensor by tensor, the same bytes. */
int x3dstep_observe_host(float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                         const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                         double max_norm, double inv_world);

/*
 * Launches 1 and 2 of x3dstep_observe with the same arguments: the record, the norm and the coefficient for max_norm are
 * written as x3dstep_observe writes them, and launch 3 is never issued: g is only read.  x3dstep_observe is x3dstep_measure
 * followed by the scale launch.
 */
int x3dstep_measure(const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                    const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                    double max_norm, double inv_world, void* stream);
int x3dstep_measure_host(const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                         const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                         double max_norm, double inv_world);

/*
 * The guarded update: one launch in place of launch 3 and the SGD kernel of libx3dhip.so, after x3dstep_measure on the
 * same state and ring (R records of S tensors).  Every thread reads state[X3DSTEP_S_STEP] = c, the `nonfinite` field of the
 * header in slot (c - 1) mod R and the coefficient word.  When nonfinite > 0 the whole grid leaves without a store to w, g
 * or m.  Otherwise, per element, in fp32 with every operation rounded once (no contraction):
 *     gi = coef == 1.0f ? g[i] : g[i] * coef          (the multiply of launch 3)
 *     t  = gi * grad_scale;  gi' = fmaf(weight_decay, w[i], t)
 *     m' = first ? gi' : fmaf(momentum, m[i], gi');   w' = w[i] - lr * m'
 * which is the SGD kernel's arithmetic on the gradient launch 3 would have left.  g is NOT written: the scaled gradient
 * exists in registers only, and g holds the unscaled gradient afterwards.
 * Thread 0 of workgroup 0 then writes state[X3DSTEP_S_SKIP], [X3DSTEP_S_SKIPPED] and [X3DSTEP_S_RUN]; no other thread reads them.
 *   w, g, m fp32 [n], distinct, 4-byte aligned; 16-byte accesses when the three addresses are congruent mod 16 (head and
 *   tail element by element), element accesses otherwise.  No atomics, no allocation, no synchronisation: capturable.
 * A state whose counter is 0 (nothing measured): x3dstep_apply_host refuses it; the kernel, which alone can read the device's
 * counter, leaves without any store, the three words included.
 */
int x3dstep_apply(float* w, const float* g, float* m, int64_t n, int64_t* state, const void* ring, int R, int S, float lr,
                  float momentum, float weight_decay, float grad_scale, int first, void* stream);
int x3dstep_apply_host(float* w, const float* g, float* m, int64_t n, int64_t* state, const void* ring, int R, int S, float lr,
                       float momentum, float weight_decay, float grad_scale, int first);

/*
 * The grouped update: x3dstep_apply with a learning-rate scale and a weight-decay scale per tensor, and optional Nesterov
 * momentum.  One launch, one wave per item of the item table of the flat buffer (X3DSTEP_ITEMS_PER_GROUP items to a
 * workgroup, the grid from nitems alone), so that every lane knows which tensor its elements belong to.
 *   hyper  X3DStepHyper [S] on the device: the scales of tensor s
 *   decision rule  state non-null: x3dstep_apply's, word for word (every thread reads the counter, the `nonfinite` field of
 *                  the latest record and the coefficient word; nonfinite > 0: no store to w, g or m; a counter of 0: the
 *                  kernel stores nothing and the twin refuses; thread 0 of workgroup 0 writes state[X3DSTEP_S_SKIP],
 *                  [X3DSTEP_S_SKIPPED] and [X3DSTEP_S_RUN], which no other thread reads).  state null: the unguarded form:
 *                  nothing is read from a state or a ring (ring and R are ignored), the coefficient is 1, the update is
 *                  always applied and no state word is written.
 *   tensor rule    lr_s = lr * hyper[seg].lr_scale; wd_s = weight_decay * hyper[seg].wd_scale: fp32, each rounded once,
 *                  once per item, the same in every lane.  A scale of exactly 1.0f gives the bits of lr and weight_decay.
 *   element rule   fp32, every operation rounded once (no contraction):
 *     gi = coef == 1.0f ? g[i] : g[i] * coef
 *     t  = gi * grad_scale;  gg = fmaf(wd_s, w[i], t)         (always the fma, also when wd_s == 0)
 *     m' = first ? gg : fmaf(momentum, m[i], gg)
 *     u  = nesterov ? fmaf(momentum, m', gg) : m';            w' = w[i] - lr_s * u           (g is never written)
 *                  With nesterov == 0 and every scale 1.0f this is x3dstep_apply's rule: the same bits.  wd_s == 0 gives
 *                  gg = t up to the sign of a zero for finite w (fmaf(0, w, -0) is +0 when w > 0).  lr_scale == 0 is plain
 *                  arithmetic, not a freeze: the momentum still moves, and w stays put for a finite u.
 *   walk           inside an item, 16-byte groups when w + start, g + start and m + start are congruent mod 16 (the elements
 *                  before the 16-byte grid and after the last whole group one by one), element by element otherwise; a
 *                  lane's loads for a batch of four groups are issued before that batch's first store; every element of w
 *                  and m is stored at most once.  No LDS, no atomics, no allocation, no synchronisation: capturable.
 *   per-item tests seg in [0, S), len in 1 .. X3DSTEP_ITEM, start in [0, n - len], both scales of the tensor finite and >= 0:
 *                  an item that fails one is left untouched by the kernel (the tables are device memory nobody checked).
 * x3dstep_apply_groups_host refuses the same with X3DSTEP_EINVAL and writes nothing; both refuse null or 4-byte-unaligned
 * pointers, n < 1, overlapping w / g / m, nesterov or first outside {0, 1} and nesterov with momentum <= 0; the twin also an
 * item table that is not exactly the in-order tiling of [0, n), and a counter of 0 when state is given.
 */
typedef struct {
    float lr_scale;  /* the tensor's learning rate is lr * lr_scale */
    float wd_scale;  /* ... and its weight decay weight_decay * wd_scale */
} X3DStepHyper;

size_t x3dstep_hyper_bytes(void);
int x3dstep_apply_groups(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                         const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R, float lr, float momentum,
                         float weight_decay, float grad_scale, int first, int nesterov, void* stream);
int x3dstep_apply_groups_host(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                              const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R, float lr,
                              float momentum, float weight_decay, float grad_scale, int first, int nesterov);

/*
 * Layer-wise adaptive rate scaling (LARS, You et al. 2017): a trust ratio per tensor, from the norm of the tensor's weights
 * and the norm of its gradient, multiplied into the grouped update.  x3dstep_trust computes the ratios on the device after
 * x3dstep_measure / x3dstep_observe on the same state and ring; x3dstep_apply_lars is x3dstep_apply_groups with the ratio in
 * its element rule.
 *
 * x3dstep_trust: two launches, shaped like launches 1 and 2 of x3dstep_measure.
 *   launch 1   a wave per item of the flat buffer's item table (X3DSTEP_ITEMS_PER_GROUP items to a workgroup): the fp64 sum
 *              of squares of the item's elements of w, no hash, no count: the lane assignment, the order within a lane and
 *              the halving reduction of `sumsq` above, 16-byte loads when w is 16-byte aligned.  workspace: fp64 [nitems]
 *              (x3dstep_trust_workspace_bytes(nitems) bytes, 8-byte aligned).  An item that fails the per-item tests of
 *              x3dstep_apply_groups (seg, len, start) gets a NaN partial, which gives its tensor a trust of 1.
 *   launch 2   one workgroup, thread t takes the tensors t, t + 1024, ..: the items of tensor s added in item order with
 *              the compensated sum, so that wsumsq[s] is, bit for bit, the sumsq[s] x3dstep_measure would record on w.
 *   trust rule fp64, every operation rounded once.  c = state[X3DSTEP_S_STEP], rec the record in slot (c - 1) mod R, coef the
 *              coefficient word of the state:
 *     a    = sqrt(wsumsq[s]);   b = sqrt(rec.sumsq[s]) * (double) grad_scale * (double) coef
 *     wd_s = weight_decay * hyper[s].wd_scale;   lr_s = lr * hyper[s].lr_scale       (fp32: the tensor rule's products)
 *     den  = (b + (double) wd_s * a) + (double) eps;   r = ((double) eta[s] * a) / den
 *     clip : r = lr_s > 0 ? min(r / (double) lr_s, 1.0) : 1.0
 *     trust[s] = (float) r when eta[s] > 0, a > 0, b > 0, rec.nonfinite[s] == 0 and (float) r is finite, else 1.0f
 *              Without clip: trust_coefficient * |w| / (|g| + wd |w| + eps), the LARS of torchlars and Lightning-Bolts; with
 *              clip: apex's LARC in clipping mode.  eta[s] == 0 is the exemption: a trust of exactly 1.0f.  b is the norm of
 *              the gradient the update applies: the recorded one times grad_scale and the clipping coefficient.
 *   per-tensor tests  eta[s], hyper[s].lr_scale and hyper[s].wd_scale finite and >= 0, 0 <= seg_item[s] < seg_item[s + 1] <=
 *              nitems: a tensor that fails one gets no store to wsumsq[s] or trust[s].  A counter of 0 (nothing measured):
 *              neither launch stores anything.
 * x3dstep_trust_host refuses the same with X3DSTEP_EINVAL and writes nothing, and also an item table that is not the in-order
 * tiling of [0, n) or a seg_item that does not index it; both refuse null or misaligned pointers (w, eta, trust, hyper: 4
 * bytes; the others 8), n < 1, eps < 0 or NaN and clip outside {0, 1}.  w, the state and the ring are only read.  No float
 * atomics, no allocation, no synchronisation: capturable.
 *
 * x3dstep_apply_lars: x3dstep_apply_groups with `trust` (fp32 [S] on the device) after hyper.  The decision rule, the tensor
 * rule, the walk, the per-item tests and the refusals are x3dstep_apply_groups', word for word; the element rule is
 *     gi = coef == 1.0f ? g[i] : g[i] * coef;   t = gi * grad_scale;   gg = fmaf(wd_s, w[i], t)
 *     gl = trust_s == 1.0f ? gg : gg * trust_s
 *     m' = first ? gl : fmaf(momentum, m[i], gl)
 *     u  = nesterov ? fmaf(momentum, m', gl) : m';            w' = w[i] - lr_s * u
 * With every trust 1.0f: the bits of x3dstep_apply_groups.  One more per-item test: trust[seg] finite and >= 0; an item that
 * fails it is left untouched by the kernel, and the twin refuses the call.  Both refuse a null or unaligned trust.
 */
size_t x3dstep_trust_workspace_bytes(int64_t nitems);
int x3dstep_trust(const float* w, int64_t n, const X3DStepItem* items, const int32_t* seg_item, int64_t nitems,
                  const X3DStepHyper* hyper, const float* eta, int S, const int64_t* state, const void* ring, int R,
                  void* workspace, double* wsumsq, float* trust, float lr, float weight_decay, float grad_scale, float eps,
                  int clip, void* stream);
int x3dstep_trust_host(const float* w, int64_t n, const X3DStepItem* items, const int32_t* seg_item, int64_t nitems,
                       const X3DStepHyper* hyper, const float* eta, int S, const int64_t* state, const void* ring, int R,
                       void* workspace, double* wsumsq, float* trust, float lr, float weight_decay, float grad_scale,
                       float eps, int clip);
int x3dstep_apply_lars(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                       const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring, int R, float lr,
                       float momentum, float weight_decay, float grad_scale, int first, int nesterov, void* stream);
int x3dstep_apply_lars_host(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                            const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring, int R,
                            float lr, float momentum, float weight_decay, float grad_scale, int first, int nesterov);

/*
 * Second-moment updates: Adam with L2, AdamW (Loshchilov & Hutter 2019) and LAMB (You et al. 2020) on the flat buffers, with
 * a second flat state buffer v (exp_avg_sq) next to m (exp_avg).  The walk is x3dstep_apply_groups': one wave per item,
 * X3DSTEP_ITEMS_PER_GROUP items to a workgroup, the grid from nitems alone; inside an item 16-byte groups when the item's
 * addresses in all the buffers of the launch are congruent mod 16, element by element otherwise; a lane's loads for a batch of
 * four groups are issued before that batch's first store; every element of an output is stored at most once.  No LDS in the
 * item launches, no float atomics, no allocation, no synchronisation: capturable.
 *   decision rule   x3dstep_apply_groups', word for word.  state non-null: every thread reads the counter, the `nonfinite`
 *                   field of the latest record and the coefficient word; nonfinite > 0: no store to w, m or v; a counter of
 *                   0: no store at all, and the twin refuses; thread 0 of workgroup 0 of x3dstep_adam and of
 *                   x3dstep_lamb_apply writes state[X3DSTEP_S_SKIP], [X3DSTEP_S_SKIPPED] and [X3DSTEP_S_RUN].  state null:
 *                   the unguarded form, coefficient 1, nothing read from or written to a state (ring and R are ignored).
 *   tensor rule     lr_s = lr * hyper[seg].lr_scale; wd_s = weight_decay * hyper[seg].wd_scale: fp32, each rounded once,
 *                   once per item.
 *   count rule      x3dstep_ema's: k = count + (state ? state[X3DSTEP_S_STEP] - state[X3DSTEP_S_SKIPPED] : 0), formed by every
 *                   thread of an applied update (a skipping launch's counting thread alone reads S_SKIPPED, before it writes
 *                   it).  At the update's launches S_SKIPPED does not yet count this step, so k is the 1-based index of this
 *                   update among the applied ones: a skipped update does not advance the bias correction.  k < 1: the twin
 *                   refuses, the kernel stores nothing (the state words included).
 *   correction rule fp64, once per wave: p1 = b1^k, p2 = b2^k by binary exponentiation in which every product is carried as
 *                   an unevaluated sum of two doubles (Veltkamp's split: fp64 multiplies and adds only, each rounded once;
 *                   pow_count of step_core.h, shared by kernel and twin), the leading part taken: within one ulp of the
 *                   power, where plain repeated squaring doubles its rounding error at every step (about k ulp; 9e4 ulp at
 *                   k = 10^6, b = 0.9999) and a libm pow would not give the same bits on both sides.
 *                   bc1 = 1 - p1; bc2 = 1 - p2; step_s = (float)((double) lr_s / bc1); rbc2 = (float) sqrt(bc2);
 *                   omb1 = (float)(1 - (double) b1); omb2 = (float)(1 - (double) b2); bc1f = (float) bc1; bc2f = (float) bc2
 *   per-item tests  x3dstep_apply_groups': seg, len, start and both scales; x3dstep_lamb_apply also trust[seg] finite and
 *                   >= 0.  An item that fails one is left untouched (x3dstep_lamb_moments: and gets NaN partials).
 *
 * x3dstep_adam: one launch.  Element rule, fp32, every operation rounded once (no contraction; sqrtf and / correctly rounded):
 *     gi = coef == 1.0f ? g[i] : g[i] * coef;      t = gi * grad_scale
 *     decoupled == 0:  t = fmaf(wd_s, w[i], t)                                  (Adam with L2)
 *     m' = fmaf(b1, m[i], omb1 * t);               v' = fmaf(b2, v[i], omb2 * (t * t))
 *     den = sqrtf(v') / rbc2 + eps
 *     w1  = decoupled ? fmaf(-(lr_s * wd_s), w[i], w[i]) : w[i]                 (AdamW: w * (1 - lr wd))
 *     w'  = w1 - step_s * (m' / den)
 * torch.optim.AdamW / Adam (amsgrad off) in the order of torch's single-tensor path.  g is never written.
 *
 * LAMB: three launches, always the decoupled form, without a gradient pre-clipping of its own (the coefficient of
 * x3dstep_measure is the clipping).  The direction of an element, fp32: t, m', v' as above;
 *     mh = m' / bc1f;  vh = v' / bc2f;  r = fmaf(wd_s, w[i], mh / (sqrtf(vh) + eps))
 *   x3dstep_lamb_moments  stores m' and v' (or nothing under the decision rule) and writes no state word.  Per item it writes
 *              two fp64 partials, the sum of (double) r * (double) r and of (double) w * (double) w, with the lane assignment,
 *              the order within a lane and the halving reduction of `sumsq` above (16-byte loads when w, g, m and v are all
 *              16-byte aligned); a wave adds its item's partials from what it loads before it stores anything.  workspace:
 *              fp64 [2 * nitems] (x3dstep_lamb_workspace_bytes(nitems), 8-byte aligned): the partials of r, then those of w.
 *   x3dstep_lamb_trust    one workgroup, shaped like launch 2 of x3dstep_trust: per tensor the items are added in item order
 *              with the compensated sum, so that wsumsq[s] and rsumsq[s] are, bit for bit, the sumsq[s] x3dstep_measure
 *              would record on w and on r.  a = sqrt(wsumsq[s]); b = sqrt(rsumsq[s]); trust[s] = (float)(a / b) when
 *              adapt[s] != 0, a > 0, b > 0, the record's nonfinite[s] == 0 (with a state) and the quotient is finite, else
 *              1.0f.  adapt: uint8 [S] on the device, 0: exempt.  Per-tensor tests: both scales finite and >= 0,
 *              0 <= seg_item[s] < seg_item[s + 1] <= nitems: a tensor that fails one gets no store.  Under the decision
 *              rule a skipped step stores nothing here: the three outputs keep the latest applied update's values.
 *   x3dstep_lamb_apply    recomputes r from the stored m', v' and from w (the same expression: the same bits) and stores
 *              w' = w[i] - (lr_s * trust_s) * r; writes the three skip words under the decision rule.  m and v are only read.
 *
 * The twins refuse what x3dstep_apply_groups_host and x3dstep_trust_host refuse, and also a null or misaligned v, v
 * overlapping w, g or m, b1 or b2 outside [0, 1) or NaN, eps < 0 or not finite, decoupled outside {0, 1} and k < 1 (the entry
 * points too, except what only device memory tells).  A refused call writes nothing.
 */
size_t x3dstep_lamb_workspace_bytes(int64_t nitems);
int x3dstep_adam(float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items, int64_t nitems,
                 const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R, int64_t count, float lr, float b1,
                 float b2, float eps, float weight_decay, float grad_scale, int decoupled, void* stream);
int x3dstep_adam_host(float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items, int64_t nitems,
                      const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R, int64_t count, float lr,
                      float b1, float b2, float eps, float weight_decay, float grad_scale, int decoupled);
int x3dstep_lamb_moments(const float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items,
                         int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state, const void* ring, int R,
                         int64_t count, float b1, float b2, float eps, float weight_decay, float grad_scale, void* workspace,
                         void* stream);
int x3dstep_lamb_moments_host(const float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items,
                              int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state, const void* ring, int R,
                              int64_t count, float b1, float b2, float eps, float weight_decay, float grad_scale,
                              void* workspace);
int x3dstep_lamb_trust(const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper, const uint8_t* adapt, int S,
                       const int64_t* state, const void* ring, int R, int64_t count, const void* workspace, double* wsumsq,
                       double* rsumsq, float* trust, void* stream);
int x3dstep_lamb_trust_host(const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper, const uint8_t* adapt, int S,
                            const int64_t* state, const void* ring, int R, int64_t count, const void* workspace,
                            double* wsumsq, double* rsumsq, float* trust);
int x3dstep_lamb_apply(float* w, const float* m, const float* v, int64_t n, const X3DStepItem* items, int64_t nitems,
                       const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring, int R,
                       int64_t count, float lr, float b1, float b2, float eps, float weight_decay, void* stream);
int x3dstep_lamb_apply_host(float* w, const float* m, const float* v, int64_t n, const X3DStepItem* items, int64_t nitems,
                            const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring, int R,
                            int64_t count, float lr, float b1, float b2, float eps, float weight_decay);

/*
 * Saves and restores small buffers that a forward pass overwrites (the running statistics of batch normalisation).
 *   table  X3DStepKeep [nbuf]: the live buffers and where each lies in snap (fp32 [snap_n]); the ranges do not overlap
 *   items  the item table x3dstep_build_items gives for a segment table of snap (tensor s is buffer s; a tensor may be
 *          longer than table[s].len, e.g. padded to a multiple of four elements: what lies past len is left alone)
 *   mode   X3DSTEP_KEEP_SAVE: snap <- live, always.  X3DSTEP_KEEP_RESTORE: live <- snap when state[X3DSTEP_S_SKIP] == 1,
 *          and otherwise every workgroup leaves at once.
 * One launch, one wave per item, every element stored once; 16-byte accesses where both addresses of an item allow.
 * x3dstep_keep_host refuses a table with a null or unaligned address, a range outside snap or an item outside its buffer's
 * range; the kernel cannot be refused for the contents of device memory and makes the same tests per item: an item that
 * fails them is not copied.
 */
int x3dstep_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap, int64_t snap_n,
                 const int64_t* state, int mode, void* stream);
int x3dstep_keep_host(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                      int64_t snap_n, const int64_t* state, int mode);

/*
 * The weight average: e <- d * e + (1 - d) * w after an update of w.
 *   count rule   k = count + (state ? state[X3DSTEP_S_STEP] - state[X3DSTEP_S_SKIPPED] : 0), computed by every thread.  With a
 *                state, S_STEP - S_SKIPPED is the number of updates applied so far, this one included (x3dstep_measure /
 *                x3dstep_observe and x3dstep_apply wrote both words in earlier launches), and count is an offset that may be
 *                negative.  state may be null: count is then the host's own count of updates, this one included.
 *   skip rule    state non-null and state[X3DSTEP_S_SKIP] == 1 (the latest x3dstep_apply skipped): the whole grid leaves
 *                without a store.  k <= 0: the twin refuses with X3DSTEP_EINVAL; the kernel, which alone can read the
 *                device's words, leaves without a store.
 *   decay rule   fp64, rounded once per value: d = (float)(warmup ? min((double)decay, (1 + k) / (10.0 + k)) : (double)decay),
 *                omd = (float)(1.0 - (double)d)
 *   element rule fp32, each operation rounded once: p = omd * w[i]; e'[i] = fmaf(d, e[i], p)
 * No thread of these launches writes a word another thread of the same launch reads; w is only read.  Refused: null or
 * 4-byte-unaligned pointers, n < 1, decay outside [0, 1) or NaN, e overlapping w.
 *   x3dstep_ema: e, w fp32 [n]; one launch shaped like x3dstep_apply: 16-byte groups when e and w are congruent mod 16 (at
 *   most three head and three tail elements one by one in workgroup 0), an element kernel otherwise; a lane's loads are
 *   issued before its first store; every element of e stored once.  No LDS, no atomics, no allocation, no
 *   synchronisation: capturable (count is then part of the captured launch).
 */
int x3dstep_ema(float* e, const float* w, int64_t n, const int64_t* state, int64_t count, float decay, int warmup, void* stream);
int x3dstep_ema_host(float* e, const float* w, int64_t n, const int64_t* state, int64_t count, float decay, int warmup);

/*
 * The same rules over a keep table (x3dstep_keep's table and items), esnap in the place of snap: one wave per item,
 * esnap[offset + j] <- fmaf(d, esnap[offset + j], omd * live[j]).  The per-item tests are x3dstep_keep's: an item that fails
 * them is not touched, and what lies past len in a padded tensor is left alone.  The live buffers are only read.
 */
int x3dstep_ema_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* esnap, int64_t snap_n,
                     const int64_t* state, int64_t count, float decay, int warmup, void* stream);
int x3dstep_ema_keep_host(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* esnap,
                          int64_t snap_n, const int64_t* state, int64_t count, float decay, int warmup);

/*
 * The exchange: a <-> b (fp32 [n], 4-byte aligned, not overlapping), or the live buffers of a table <-> their snapshot, in
 * place and bit for bit (the values are moved as 32-bit words: NaN payloads and the sign of zero are kept).  One launch
 * each, both sides of a lane loaded before its first store, every element of both sides stored once, the vectorisation
 * rules of x3dstep_ema / x3dstep_keep.  Two exchanges are the identity.
 */
int x3dstep_swap(float* a, float* b, int64_t n, void* stream);
int x3dstep_swap_host(float* a, float* b, int64_t n);
int x3dstep_swap_keep(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap, int64_t snap_n,
                      void* stream);
int x3dstep_swap_keep_host(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                           int64_t snap_n);

/*
 * Precise BN statistics: the running statistics of batch normalisation recomputed over K batches, S splits and W ranks.
 * A cell is one split of one batch on one rank: for a channel it has a mean mu and an unbiased variance v, which a forward
 * pass in training mode with BN momentum 1 leaves in the live buffers (split j of channel c at [j * C + c]).  Over n cells
 *     mean = sum mu / n,   var = sum v / n + sum (mu - mean)^2 / n
 * computed in fp64, streaming, in a fixed order, every operation rounded once.  One accumulator per channel: four doubles
 * {n, mean, m2, vsum} (X3DSTEP_PBN_ACC_DOUBLES; all zero before the first cell).
 *   cell    n' = n + 1; d = mu - mean; mean' = mean + d / n'; m2' = m2 + d * (mu - mean'); vsum' = vsum + v
 *   merge   of A then B (rank order): nB == 0 keeps A, nA == 0 takes B, otherwise n = nA + nB; d = meanB - meanA;
 *           mean = meanA + d * (nB / n); m2 = (m2A + m2B) + (d * d) * (nA * nB / n); vsum = vsumA + vsumB
 *   result  mean32 = (float) mean; var32 = (float) ((vsum + m2) / n); both a NaN when n != expect_n
 * Tables (host builders below; the kernels read them from device memory)
 *   layers  X3DStepPbnLayer [nlayers]: `first` of layer l is the sum of C over the layers before it, so the accumulator
 *           array has x3dstep_pbn_build_layers' return value T channels: fp64 [4 * T], 8-byte aligned
 *   work    X3DStepItem [nwork]: a layer cut into runs of at most X3DSTEP_PBN_RUN channels; seg: the layer, start: the run's
 *           first channel in the accumulator array, len: its channels.  One workgroup per run, one thread per channel.
 * Both launches: the grid comes from the tables alone, every output element is stored once, no atomics, no LDS, no
 * allocation, no synchronisation: capturable.  A work item that fails the per-item tests (a null or unaligned address,
 * C < 1, S < 1, a run outside its layer, a range outside snap) is not touched.  The twins refuse with X3DSTEP_EINVAL what
 * the kernels leave out, and also ranges of snap that overlap a neighbour's and work items that overlap or are out of order.
 */
#define X3DSTEP_PBN_RUN 256
#define X3DSTEP_PBN_ACC_DOUBLES 4
#define X3DSTEP_PBN_MAX_CHANNELS (1 << 28)

typedef struct {
    int64_t mean_addr;  /* the live buffer of the means: the address of fp32 [S * C], 4-byte aligned, not null */
    int64_t var_addr;   /* the live buffer of the variances, likewise */
    int64_t mean_off;   /* the first element of the means' buffer in a keep table's snapshot */
    int64_t var_off;    /* ... and of the variances' */
    int64_t first;      /* the layer's first channel in the accumulator array */
    int32_t C;          /* channels, >= 1 */
    int32_t S;          /* splits, >= 1 */
} X3DStepPbnLayer;

size_t x3dstep_pbn_layer_bytes(void);

/* Writes the layer table of a keep table whose buffers come in pairs (means, variances) of splits[l] * C_l elements each
 * (host only, host pointers; nbuf == 2 * nlayers).  Returns the total number of channels T, or negative X3DSTEP_E*. */
int64_t x3dstep_pbn_build_layers(const X3DStepKeep* table, int nbuf, const int32_t* splits, int nlayers,
                                 X3DStepPbnLayer* layers);
/* Runs the work table of these layers has; then the table itself (`cap`: items the caller allocated).  Host only. */
int64_t x3dstep_pbn_work_count(const X3DStepPbnLayer* layers, int nlayers);
int64_t x3dstep_pbn_build_work(const X3DStepPbnLayer* layers, int nlayers, X3DStepItem* work, int64_t cap);

/* One cell update per split, splits in order j = 0 .. S - 1, for every channel: reads the live buffers, updates acc. */
int x3dstep_pbn_accum(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork, double* acc,
                      void* stream);
int x3dstep_pbn_accum_host(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork, double* acc);

/*
 * Merges the W accumulators of every channel in rank order (acc_all: fp64 [W][4 * T], only read) and writes mean32 into
 * all S slots of the layer's means in snap (fp32 [snap_n]) and var32 into all S slots of its variances.  What lies between
 * the buffers in snap (padding) is not touched; the live buffers are neither read nor written.  expect_n >= 1.
 */
int x3dstep_pbn_finish(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                       const double* acc_all, int W, int64_t expect_n, float* snap, int64_t snap_n, void* stream);
int x3dstep_pbn_finish_host(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                            const double* acc_all, int W, int64_t expect_n, float* snap, int64_t snap_n);

#ifdef __cplusplus
}
#endif

#endif /* X3DSTEP_H */
