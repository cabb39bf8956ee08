// The arithmetic of libx3dstep (include/x3dstep.h) item by item and tensor by tensor, compiled into the .hip files (the
// kernels) and step_host.cpp (the CPU twins): what a lane adds and in which order, the sum of a tensor's items, the
// coefficient rule, the record's layout and what the one finishing thread writes; the plan of a walk, the element operations
// of the two walks of step_priv.h and the item walk of one lane.  No HIP call, no global state.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/x3dstep.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define STEP_HD __host__ __device__ static inline
#define STEP_HD_MEMBER __host__ __device__ inline
#else
#define STEP_HD static inline
#define STEP_HD_MEMBER inline
#endif

namespace x3ds {

constexpr int kLanes = 64;                 // lanes of a wave: the partial sums of an item
constexpr int kFinalThreads = 1024;        // tensors per round of the finalize step

struct Part {
    double sumsq;
    uint64_t hash;
    int32_t nf;
};

struct alignas(16) Vec4 {
    float v[4];
};

// A 16-byte group of the two walks: one aligned load or store, held in registers.  Vector types, not structs of four: an
// array of structs that a lane holds between its loads and its stores is left in private memory by the compiler.
typedef float Float4 __attribute__((vector_size(16)));
typedef uint32_t Bits4 __attribute__((vector_size(16)));

STEP_HD uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

STEP_HD uint32_t float_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// one element: idx is its index within the tensor
STEP_HD void part_add(Part& p, uint64_t idx, float x) {
    const uint32_t u = float_bits(x);
    const double d = (double)x;
    p.sumsq = p.sumsq + d * d;     // the product of two widened fp32 values is exact
    p.nf += (u & 0x7f800000u) == 0x7f800000u ? 1 : 0;
    p.hash += splitmix64((idx << 32) | (uint64_t)u);
}

// What lane `lane` of the wave that owns an item accumulates: the groups of four elements q = lane, lane + 64, ..; group q
// holds the elements j of the item with (start mod 4 + j) / 4 == q, so that a whole group is one aligned 16-byte load when
// g itself is 16-byte aligned (`vec`).  `first`: the index within the tensor of the item's first element.
STEP_HD Part lane_part(const float* g, int64_t start, int len, uint64_t first, int lane, bool vec) {
    Part p = {0.0, 0, 0};
    const int m = (int)(start & 3);
    const int groups = (m + len + 3) >> 2;
    for (int q = lane; q < groups; q += kLanes) {
        const int j0 = 4 * q - m;
        if (vec && j0 >= 0 && j0 + 4 <= len) {
            const Vec4 x = *(const Vec4*)(g + start + j0);
            for (int e = 0; e < 4; ++e) part_add(p, first + (uint64_t)(j0 + e), x.v[e]);
        } else {
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                if (j >= 0 && j < len) part_add(p, first + (uint64_t)j, g[start + j]);
            }
        }
    }
    return p;
}

STEP_HD void part_merge(Part& a, const Part& b) {
    a.sumsq = a.sumsq + b.sumsq;
    a.hash += b.hash;
    a.nf += b.nf;
}

// the scratch of the partials: fp64 [nitems], uint64 [nitems], int32 [nitems]
struct Scratch {
    double* sumsq;
    uint64_t* hash;
    int32_t* nf;
};

STEP_HD size_t scratch_bytes(int64_t nitems) { return (((size_t)nitems * 20) + 7) & ~(size_t)7; }

STEP_HD Scratch scratch_at(void* ws, int64_t nitems) {
    Scratch s;
    s.sumsq = (double*)ws;
    s.hash = (uint64_t*)((char*)ws + 8 * (size_t)nitems);
    s.nf = (int32_t*)((char*)ws + 16 * (size_t)nitems);
    return s;
}

// The two sums one thread adds term after term (a tensor's items, the tensors of the buffer) are compensated (Neumaier):
// some hundred terms in a row would otherwise cost several ulp of the norm.  A step that leaves the finite numbers is not
// compensated, so that an infinite or NaN sum stays what plain addition gives (no Inf - Inf).
struct Sum {
    double s, c;
};

STEP_HD void sum_add(Sum& a, double x) {
    const double t = a.s + x;
    if (fabs(t) <= 1.7976931348623157e308) a.c = a.c + (fabs(a.s) >= fabs(x) ? (a.s - t) + x : (x - t) + a.s);
    a.s = t;
}

STEP_HD double sum_value(const Sum& a) { return a.s + a.c; }

// a tensor: its items in item order.  Src gives the partials of item i: the scratch itself (ScratchSource), or the kernel's
// copy of its head in LDS.
struct ScratchSource {
    Scratch w;
    STEP_HD_MEMBER int near_end(int a, int) const { return a; }      // nothing nearer than the scratch
    STEP_HD_MEMBER Part near(int i) const { return far(i); }
    STEP_HD_MEMBER Part far(int i) const {
        const Part p = {w.sumsq[i], w.hash[i], w.nf[i]};
        return p;
    }
};

// Items [a, near_end) come from the source's near copy and the rest from the scratch: two plain loops, in item order, so
// that the loads of the near loop (LDS in the kernel) can be issued several iterations ahead of the sum that needs them.
template <class Src>
STEP_HD Part tensor_part(const Src& src, int a, int b) {
    Sum sq = {0.0, 0.0};
    Part p = {0.0, 0, 0};
    const int mid = src.near_end(a, b);
#pragma unroll 8
    for (int i = a; i < mid; ++i) {
        const Part q = src.near(i);
        sum_add(sq, q.sumsq);
        p.hash += q.hash;
        p.nf += q.nf;
    }
    for (int i = mid; i < b; ++i) {
        const Part q = src.far(i);
        sum_add(sq, q.sumsq);
        p.hash += q.hash;
        p.nf += q.nf;
    }
    p.sumsq = sum_value(sq);
    return p;
}

struct Record {
    X3DStepHeader* head;
    double* sumsq;
    uint64_t* hash;
    int32_t* nf;
};

STEP_HD size_t record_bytes(int S) { return ((sizeof(X3DStepHeader) + (size_t)S * 20) + 7) & ~(size_t)7; }

STEP_HD Record record_at(void* ring, int R, int S, int64_t step) {
    const int64_t slot = ((step % (int64_t)R) + R) % R;      // inside the ring whatever the counter holds
    char* base = (char*)ring + (size_t)slot * record_bytes(S);
    Record r;
    r.head = (X3DStepHeader*)base;
    r.sumsq = (double*)(base + sizeof(X3DStepHeader));
    r.hash = (uint64_t*)(base + sizeof(X3DStepHeader) + 8 * (size_t)S);
    r.nf = (int32_t*)(base + sizeof(X3DStepHeader) + 16 * (size_t)S);
    return r;
}

// torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped from above at 1 (a NaN stays a NaN)
STEP_HD float coef_rule(double total, double inv_world, double max_norm, double* norm_out) {
    const double norm = sqrt(total) * inv_world;
    *norm_out = norm;
    if (!(max_norm > 0.0)) return 1.0f;
    double c = max_norm / (norm + 1e-6);
    if (c > 1.0) c = 1.0;
    return (float)c;
}

// what the one finishing thread writes after the per-tensor part of the record: the header and the state
STEP_HD void finish_step(const Record& r, int64_t* state, int64_t step, int S, double total, int32_t nf, int32_t first_bad,
                         double max_norm, double inv_world) {
    double norm;
    const float coef = coef_rule(total, inv_world, max_norm, &norm);
    X3DStepHeader h;
    h.step = step;
    h.total = total;
    h.norm = norm;
    h.coef = coef;
    h.nonfinite = nf;
    h.first_bad = first_bad;
    h.nseg = S;
    *r.head = h;
    if (nf > 0 && state[X3DSTEP_S_BAD_STEP] < 0) {
        state[X3DSTEP_S_BAD_STEP] = step;
        state[X3DSTEP_S_BAD_SEG] = first_bad;
    }
    int64_t nb;
    memcpy(&nb, &norm, 8);
    state[X3DSTEP_S_NORM] = nb;
    state[X3DSTEP_S_COEF] = (int64_t)float_bits(coef);
    state[X3DSTEP_S_STEP] = step + 1;
}

STEP_HD float state_coef(const int64_t* state) {
    const uint32_t u = (uint32_t)state[X3DSTEP_S_COEF];
    float c;
    memcpy(&c, &u, 4);
    return c;
}

STEP_HD float scale_one(float x, float coef) { return x * coef; }

// -- the plan and the element operations of the walks ----------------------------------------------------------------------
// How a run of n elements in one or more buffers is cut: `head` elements one by one, `groups` 16-byte groups, then the
// tail, when all the addresses are congruent mod 16 (`same`; r: the residue of any of them); otherwise n elements one by
// one (vec says which: head, groups and tail are then never used).
struct Plan {
    bool vec;
    int64_t head, groups, tail;      // tail: the index of the first element after the groups
};

STEP_HD Plan walk_plan(uintptr_t r, bool same, int64_t n) {
    Plan p;
    p.vec = same;
    p.head = (int64_t)(((16 - r) & 15) >> 2);
    if (p.head > n) p.head = n;
    p.groups = (n - p.head) >> 2;
    p.tail = p.head + 4 * p.groups;
    return p;
}

STEP_HD uintptr_t mod16(const void* p) { return (uintptr_t)p & 15; }

// An element operation Op of the flat walk (step_priv.h; flat_host of step_host.cpp) and of the item walk (item_lane) says:
//   Elem, Group       what it works on, float or bits, and sixteen bytes of it;
//   kBufs             how many buffers it takes; kLoads, kStores: the masks of those a walk loads and of those it stores
//                     (a buffer the operation only reads is never stored, one it only writes never loaded);
//   begin(counting)   what every thread reads before anything else (uniform loads); false: the launch does nothing.
//                     `counting` is true in the one thread that writes the state's counters;
//   one(x)            the rule on one element of each buffer, x[kBufs];
//   mode              (item walk only) which end of an item is buffer 0: X3DSTEP_KEEP_SAVE, the snapshot's.
// A unit of a walk is an element or a group; on a group the rule runs on its four elements in order.
template <class Op, class Unit>
STEP_HD void walk_unit(const Op& op, Unit (&v)[Op::kBufs]) {
    if constexpr (sizeof(Unit) == sizeof(typename Op::Elem)) {
        op.one(v);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            typename Op::Elem x[Op::kBufs];
#pragma unroll
            for (int b = 0; b < Op::kBufs; ++b)
                if (Op::kLoads >> b & 1) x[b] = v[b][e];
            op.one(x);
#pragma unroll
            for (int b = 0; b < Op::kBufs; ++b)
                if (Op::kStores >> b & 1) v[b][e] = x[b];
        }
    }
}

// unit `at` of the buffers p: load, rule, store
template <class Op, class Unit>
STEP_HD void walk_at(const Op& op, Unit* const* p, int64_t at) {
    Unit v[Op::kBufs];
#pragma unroll
    for (int b = 0; b < Op::kBufs; ++b)
        if (Op::kLoads >> b & 1) v[b] = p[b][at];
    walk_unit(op, v);
#pragma unroll
    for (int b = 0; b < Op::kBufs; ++b)
        if (Op::kStores >> b & 1) p[b][at] = v[b];
}

// the flat buffers of an operation and their plan
template <class Op>
struct Bufs {
    typename Op::Elem* p[Op::kBufs];
};

template <class Op>
STEP_HD Plan flat_plan(const Bufs<Op>& bufs, int64_t n) {
    bool same = true;
    for (int b = 1; b < Op::kBufs; ++b) same = same && mod16(bufs.p[b]) == mod16(bufs.p[0]);
    return walk_plan(mod16(bufs.p[0]), same, n);
}

// -- the guarded update (x3dstep_apply, x3dstep_apply_groups) --------------------------------------------------------------
struct SgdArgs {
    float lr, mu, wd, gs;
    int first, nesterov;
};

// What every thread of an update kernel reads before anything else: the decision and the coefficient of the step measured
// last.  go: the counter is not 0 (something was measured); skip: that step's gradient had a non-finite element.
struct Decision {
    bool go, skip;
    float coef;
};

STEP_HD Decision apply_decision(const int64_t* state, const void* ring, int R, int S) {
    Decision d;
    const int64_t step = state[X3DSTEP_S_STEP];
    d.go = step != 0;
    d.skip = record_at((void*)ring, R, S, step - 1).head->nonfinite > 0;
    d.coef = state_coef(state);
    return d;
}

// what the one counting thread writes
STEP_HD void apply_counters(int64_t* state, bool skip) {
    state[X3DSTEP_S_SKIP] = skip ? 1 : 0;
    if (skip) {
        state[X3DSTEP_S_SKIPPED] = state[X3DSTEP_S_SKIPPED] + 1;
        state[X3DSTEP_S_RUN] = state[X3DSTEP_S_RUN] + 1;
    } else {
        state[X3DSTEP_S_RUN] = 0;
    }
}

// The start of an update launch: false when nothing was measured or the step is skipped, else the coefficient.  The
// counters are words no thread of the grid reads here.
STEP_HD bool apply_begin(int64_t* state, const void* ring, int R, int S, bool counting, float* coef) {
    const Decision d = apply_decision(state, ring, R, S);
    if (!d.go) return false;
    if (counting) apply_counters(state, d.skip);
    *coef = d.coef;
    return !d.skip;
}

// One element: the multiply of the scale launch, then the arithmetic of the SGD kernel of libx3dhip.so (csrc/bn.hip
// sgd_kernel) with the tensor's own rate and decay and the Nesterov look-ahead, each operation rounded once (both libraries
// compile with -ffp-contract=off).  kPlain: no Nesterov term, whatever a.nesterov says.  kTrust: the decayed gradient times
// `trust` before the momentum (a trust of exactly 1.0f: no multiply, the same bits as without).
template <bool kPlain = false, bool kTrust = false>
STEP_HD void sgd_one(float& w, float g, float& m, float coef, const SgdArgs& a, float lr_s, float wd_s, float trust = 1.0f) {
    const float gi = coef == 1.0f ? g : scale_one(g, coef);
    const float t = gi * a.gs;
    const float gd = fmaf(wd_s, w, t);
    const float gg = kTrust && trust != 1.0f ? gd * trust : gd;      // x3dstep_apply_lars: the tensor's trust ratio
    const float mi = a.first ? gg : fmaf(a.mu, m, gg);
    const float u = !kPlain && a.nesterov ? fmaf(a.mu, mi, gg) : mi;
    const float step = lr_s * u;
    m = mi;
    w = w - step;
}

// x3dstep_apply over w, g, m: every tensor at the rate lr and the decay wd, no Nesterov term
struct ApplyOp {
    typedef float Elem;
    typedef Float4 Group;
    static constexpr int kBufs = 3;
    static constexpr unsigned kLoads = 7, kStores = 5;
    int64_t* state;
    const void* ring;
    int R, S;
    SgdArgs a;
    float coef;
    STEP_HD_MEMBER bool begin(bool counting) { return apply_begin(state, ring, R, S, counting, &coef); }
    STEP_HD_MEMBER void one(float (&x)[3]) const { sgd_one<true>(x[0], x[1], x[2], coef, a, a.lr, a.wd); }
};

// -- the grouped update (x3dstep_apply_groups) -----------------------------------------------------------------------------
// a scale the tensor rule takes: finite and not negative (a NaN fails both comparisons)
STEP_HD bool group_scale_ok(float s) { return s >= 0.0f && s <= 3.402823466e38f; }

struct GroupItem {
    int64_t start;
    int len;                         // 0: the item is refused, nothing is touched
    float lr_s, wd_s;                // the tensor rule: two fp32 multiplies, the same in every lane
};

// Item i resolved against the hyper table.  The tests are those x3dstep_apply_groups_host refuses a call for; the kernel
// makes them per item, since the tables it reads are device memory nobody has checked.
STEP_HD GroupItem group_resolve(const X3DStepItem* items, int64_t i, const X3DStepHyper* hyper, int S, int64_t n,
                                const SgdArgs& a) {
    GroupItem r = {0, 0, 0.0f, 0.0f};
    const X3DStepItem it = items[i];
    if (it.seg < 0 || it.seg >= S || it.len < 1 || it.len > X3DSTEP_ITEM || it.start < 0 || it.start > n - it.len) return r;
    const X3DStepHyper h = hyper[it.seg];
    if (!group_scale_ok(h.lr_scale) || !group_scale_ok(h.wd_scale)) return r;
    r.start = it.start;
    r.len = it.len;
    r.lr_s = a.lr * h.lr_scale;
    r.wd_s = a.wd * h.wd_scale;
    return r;
}

constexpr int kGroupPieces = 4;      // 16-byte groups of every buffer a lane holds at once: a batch
constexpr int kGroupBatches = X3DSTEP_ITEM / (4 * kLanes * kGroupPieces);      // batches that cover a full item: 2

// An element rule of the update walk (rule_lane) says:
//   kBufs         how many flat buffers it takes (all of them are loaded); kStores: the mask of those the walk stores
//   one(x)        the rule on one element of each buffer, x[kBufs]
// and holds what the item's tensor gave it (the rates, the trust).
template <class Rule>
STEP_HD void rule_at(const Rule& rule, float* const* p, int j) {
    float x[Rule::kBufs];
#pragma unroll
    for (int b = 0; b < Rule::kBufs; ++b) x[b] = p[b][j];
    rule.one(x);
#pragma unroll
    for (int b = Rule::kBufs - 1; b >= 0; --b)
        if (Rule::kStores >> b & 1) p[b][j] = x[b];
}

// What lane `lane` of the item's wave updates.  When the addresses of the item in all the buffers are congruent mod 16:
// `head` elements up to the 16-byte grid one by one (lane j the j-th), the 16-byte groups q = lane, lane + 64, .. in batches
// of kGroupPieces (a batch's loads of every buffer before its first store), then the tail one by one.  Otherwise the
// elements j = lane, lane + 64, ...  Every element of the item is stored once per stored buffer, the last buffer first;
// nothing outside the item is read or written.
template <class Rule>
STEP_HD void rule_lane(const Rule& rule, float* const (&base)[Rule::kBufs], int64_t start, int len, int lane) {
    constexpr int B = Rule::kBufs;
    static_assert(B == 3 || B == 4, "the update walk takes three or four buffers");
    float* p[B];
#pragma unroll
    for (int b = 0; b < B; ++b) p[b] = base[b] + start;
    bool same = mod16(p[0]) == mod16(p[1]) && mod16(p[0]) == mod16(p[2]);
    if constexpr (B == 4) same = same && mod16(p[0]) == mod16(p[3]);
    const Plan pl = walk_plan(mod16(p[0]), same, len);
    if (!pl.vec) {
        for (int j = lane; j < len; j += kLanes) rule_at(rule, p, j);
        return;
    }
    const int head = (int)pl.head, groups = (int)pl.groups, tail = (int)pl.tail;
    Vec4* u[B];
#pragma unroll
    for (int b = 0; b < B; ++b) u[b] = (Vec4*)(p[b] + head);
#pragma unroll
    for (int t = 0; t < kGroupBatches; ++t) {        // groups <= X3DSTEP_ITEM / 4 = kGroupBatches * kGroupPieces * kLanes
        const int q0 = lane + t * kGroupPieces * kLanes;
        if (q0 >= groups) break;
        Vec4 v[B][kGroupPieces];
#pragma unroll
        for (int k = 0; k < kGroupPieces; ++k) {
            const int q = q0 + k * kLanes;
            if (q < groups) {
#pragma unroll
                for (int b = 0; b < B; ++b) v[b][k] = u[b][q];
            }
        }
#pragma unroll
        for (int k = 0; k < kGroupPieces; ++k) {
            const int q = q0 + k * kLanes;
            if (q < groups) {
                for (int e = 0; e < 4; ++e) {
                    float x[B];
#pragma unroll
                    for (int b = 0; b < B; ++b) x[b] = v[b][k].v[e];
                    rule.one(x);
#pragma unroll
                    for (int b = 0; b < B; ++b)
                        if (Rule::kStores >> b & 1) v[b][k].v[e] = x[b];
                }
#pragma unroll
                for (int b = B - 1; b >= 0; --b)
                    if (Rule::kStores >> b & 1) u[b][q] = v[b][k];
            }
        }
    }
    if (lane < head) rule_at(rule, p, lane);
    if (lane < len - tail) rule_at(rule, p, tail + lane);
}

// the element rule of x3dstep_apply_groups over w, g, m; kTrust: that of x3dstep_apply_lars, which multiplies by `trust`
template <bool kTrust>
struct SgdRule {
    static constexpr int kBufs = 3;
    static constexpr unsigned kStores = 5;
    float coef;
    SgdArgs a;
    float lr_s, wd_s, trust;
    STEP_HD_MEMBER void one(float (&x)[3]) const { sgd_one<false, kTrust>(x[0], x[1], x[2], coef, a, lr_s, wd_s, trust); }
};

// the grouped update of one lane: rule_lane over w, g and m
template <bool kTrust = false>
STEP_HD void group_lane(float* w, const float* g, float* m, const GroupItem& c, int lane, float coef, const SgdArgs& a,
                        float trust = 1.0f) {
    const SgdRule<kTrust> rule = {coef, a, c.lr_s, c.wd_s, trust};
    float* const base[3] = {w, (float*)g, m};
    rule_lane(rule, base, c.start, c.len, lane);
}

// -- trust ratios (x3dstep_trust, x3dstep_apply_lars) ----------------------------------------------------------------------
// The item tests of group_resolve alone, for the launch that reads w only: an item that fails them gets a NaN partial.
STEP_HD bool trust_item_ok(const X3DStepItem& it, int S, int64_t n) {
    return !(it.seg < 0 || it.seg >= S || it.len < 1 || it.len > X3DSTEP_ITEM || it.start < 0 || it.start > n - it.len);
}

// What lane `lane` adds for an item of w: lane_part's sum of squares, the same elements in the same order (the hash and the
// count of lane_part are never used and fall away).
STEP_HD double trust_lane(const float* w, const X3DStepItem& it, int lane, bool vec) {
    return lane_part(w, it.start, it.len, 0, lane, vec).sumsq;
}

STEP_HD double trust_nan() {
    const uint64_t u = 0x7ff8000000000000ull;
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// the partials of x3dstep_trust as a source of tensor_part: the scratch (far), or the kernel's copy of its head in LDS
struct SumsqSource {
    const double* far_p;
    const double* near_p;
    int cached;
    STEP_HD_MEMBER int near_end(int a, int b) const { return b < cached ? b : (a > cached ? a : cached); }
    STEP_HD_MEMBER Part near(int i) const {
        const Part p = {near_p[i], 0, 0};
        return p;
    }
    STEP_HD_MEMBER Part far(int i) const {
        const Part p = {far_p[i], 0, 0};
        return p;
    }
};

struct TrustArgs {
    float lr, wd, gs, eps;
    int clip;
};

// the tests of tensor s: its rate of trust and its scales finite and >= 0, its items a range of the table
STEP_HD bool trust_tensor_ok(const X3DStepHyper& h, float eta, int a, int b, int64_t nitems) {
    return group_scale_ok(eta) && group_scale_ok(h.lr_scale) && group_scale_ok(h.wd_scale) && a >= 0 && a < b &&
           (int64_t)b <= nitems;
}

// The trust ratio of one tensor: fp64, every operation rounded once.  wss: the sum of squares of its weights; gss, nf: the
// sum of squares and the count of non-finite elements of its gradient in the latest record; coef: the clipping coefficient.
STEP_HD float trust_rule(double wss, double gss, int32_t nf, float eta, const X3DStepHyper& h, float coef, const TrustArgs& t) {
    const double a = sqrt(wss);
    const double b0 = sqrt(gss);
    const double b1 = b0 * (double)t.gs;
    const double b = b1 * (double)coef;
    const float wd_s = t.wd * h.wd_scale;
    const float lr_s = t.lr * h.lr_scale;
    const double dw = (double)wd_s * a;
    const double d0 = b + dw;
    const double den = d0 + (double)t.eps;
    const double num = (double)eta * a;
    double r = num / den;
    if (t.clip) {
        if (lr_s > 0.0f) {
            r = r / (double)lr_s;
            if (r > 1.0) r = 1.0;
        } else {
            r = 1.0;
        }
    }
    const float r32 = (float)r;
    const bool ok = eta > 0.0f && a > 0.0 && b > 0.0 && nf == 0 && r32 >= -3.402823466e38f && r32 <= 3.402823466e38f;
    return ok ? r32 : 1.0f;
}

// What the thread of tensor s does in launch 2 of x3dstep_trust, after the decision (the counter is not 0).
template <class Src>
STEP_HD void trust_tensor(const Src& src, int s, const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper,
                          const float* eta, const Record& rec, float coef, const TrustArgs& t, double* wsumsq, float* trust) {
    const int a = seg_item[s], b = seg_item[s + 1];
    const X3DStepHyper h = hyper[s];
    const float e = eta[s];
    if (!trust_tensor_ok(h, e, a, b, nitems)) return;
    const double wss = tensor_part(src, a, b).sumsq;
    wsumsq[s] = wss;
    trust[s] = trust_rule(wss, rec.sumsq[s], rec.nf[s], e, h, coef, t);
}

// Item i of x3dstep_apply_lars: group_resolve and the tensor's trust, which must be finite and >= 0.
STEP_HD GroupItem lars_resolve(const X3DStepItem* items, int64_t i, const X3DStepHyper* hyper, const float* trust, int S,
                               int64_t n, const SgdArgs& a, float* t) {
    GroupItem r = group_resolve(items, i, hyper, S, n, a);
    if (r.len > 0) {
        *t = trust[items[i].seg];
        if (!group_scale_ok(*t)) r.len = 0;
    }
    return r;
}

// -- second-moment updates (x3dstep_adam, x3dstep_lamb_*) -------------------------------------------------------------------
// b^k for k >= 0, the same bits in the kernel and in the twin: binary exponentiation in which every product is carried as
// an unevaluated sum of two doubles (the exact product of the leading parts by Veltkamp's split, fp64 multiplies and adds
// only, each rounded once), so that the rounding of one squaring is not doubled by the next: the leading part is within
// one ulp of the power.  A libm pow would differ between the two sides.
struct Pair {
    double hi, lo;
};

STEP_HD Pair pair_mul(const Pair& x, const Pair& y) {
    const double p = x.hi * y.hi;
    const double cx = 134217729.0 * x.hi;
    const double xh = cx - (cx - x.hi);
    const double xl = x.hi - xh;
    const double cy = 134217729.0 * y.hi;
    const double yh = cy - (cy - y.hi);
    const double yl = y.hi - yh;
    const double e0 = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl;      // x.hi * y.hi - p, exact above the subnormals
    const double e = e0 + (x.hi * y.lo + x.lo * y.hi);
    Pair r;
    r.hi = p + e;
    r.lo = e - (r.hi - p);
    return r;
}

STEP_HD double pow_count(double b, int64_t k) {
    Pair r = {1.0, 0.0}, x = {b, 0.0};
    while (k > 0) {
        if (k & 1) r = pair_mul(r, x);
        k >>= 1;
        if (k > 0) x = pair_mul(x, x);
    }
    return r.hi;
}

struct AdamArgs {
    float lr, b1, b2, eps, wd, gs;
    int decoupled;
};

STEP_HD int64_t ema_count(const int64_t* state, int64_t count);      // the count rule: the weight average's, below

// b1 and b2 in [0, 1), eps finite and >= 0 (a NaN fails every comparison)
STEP_HD bool adam_args_ok(float b1, float b2, float eps, int decoupled) {
    return b1 >= 0.0f && b1 < 1.0f && b2 >= 0.0f && b2 < 1.0f && eps >= 0.0f && eps <= 3.402823466e38f &&
           (decoupled == 0 || decoupled == 1);
}

// The start of a launch of these updates: the decision rule of apply_begin, then the count rule of ema_count (k: the
// 1-based index of this update among the applied ones).  false: the lane stores nothing.  `counting`: the one thread
// of the launch that writes the three skip words (no launch of x3dstep_lamb_moments / _trust has one).  S_SKIPPED is read
// after the decision, by the lanes of an applied update alone: a skipping launch's counting thread is its only reader.
STEP_HD bool adam_begin(int64_t* state, const void* ring, int R, int S, int64_t count, bool counting, float* coef,
                        int64_t* k) {
    *coef = 1.0f;
    if (!state) {
        *k = count;
        return count >= 1;
    }
    const Decision d = apply_decision(state, ring, R, S);
    if (!d.go) return false;
    if (d.skip) {
        if (counting && ema_count(state, count) >= 1) apply_counters(state, true);
        return false;
    }
    *k = ema_count(state, count);
    if (*k < 1) return false;
    if (counting) apply_counters(state, false);
    *coef = d.coef;
    return true;
}

// the correction rule: fp64, each value rounded once
struct AdamCorr {
    double bc1, bc2;
    float rbc2, omb1, omb2, bc1f, bc2f;
};

STEP_HD AdamCorr adam_corr(int64_t k, float b1, float b2) {
    AdamCorr c;
    c.bc1 = 1.0 - pow_count((double)b1, k);
    c.bc2 = 1.0 - pow_count((double)b2, k);
    c.rbc2 = (float)sqrt(c.bc2);
    c.omb1 = (float)(1.0 - (double)b1);
    c.omb2 = (float)(1.0 - (double)b2);
    c.bc1f = (float)c.bc1;
    c.bc2f = (float)c.bc2;
    return c;
}

STEP_HD float adam_step_size(float lr_s, const AdamCorr& c) { return (float)((double)lr_s / c.bc1); }

// the gradient an element's moments take, before the L2 term: the clipping multiply, then grad_scale
STEP_HD float adam_grad(float g, float coef, float gs) {
    const float gi = coef == 1.0f ? g : scale_one(g, coef);
    return gi * gs;
}

// both moments of one element, fp32, every operation rounded once
STEP_HD void adam_moments(float t, float& m, float& v, const AdamArgs& a, const AdamCorr& c) {
    const float p = c.omb1 * t;
    const float tt = t * t;
    const float q = c.omb2 * tt;
    m = fmaf(a.b1, m, p);
    v = fmaf(a.b2, v, q);
}

// x3dstep_adam over w, g, m, v: torch.optim.Adam / AdamW in the order of torch's single-tensor path
struct AdamRule {
    static constexpr int kBufs = 4;
    static constexpr unsigned kStores = 13;
    AdamArgs a;
    AdamCorr c;
    float coef, wd_s, step_s, lrwd;      // lrwd: lr_s * wd_s, rounded once
    STEP_HD_MEMBER void one(float (&x)[4]) const {
        const float w = x[0];
        float t = adam_grad(x[1], coef, a.gs);
        if (!a.decoupled) t = fmaf(wd_s, w, t);
        adam_moments(t, x[2], x[3], a, c);
        const float sq = sqrtf(x[3]);
        const float d0 = sq / c.rbc2;
        const float den = d0 + a.eps;
        const float w1 = a.decoupled ? fmaf(-lrwd, w, w) : w;
        const float u = x[2] / den;
        const float du = step_s * u;
        x[0] = w1 - du;
    }
};

// the direction of an element of LAMB from its new moments: the corrected Adam quotient plus the decay term
STEP_HD float lamb_dir(float w, float m1, float v1, float eps, float wd_s, const AdamCorr& c) {
    const float mh = m1 / c.bc1f;
    const float vh = v1 / c.bc2f;
    const float sq = sqrtf(vh);
    const float den = sq + eps;
    const float u = mh / den;
    return fmaf(wd_s, w, u);
}

// launch 1 of LAMB over g, m, v: the moments
struct LambMomentsRule {
    static constexpr int kBufs = 3;
    static constexpr unsigned kStores = 6;
    AdamArgs a;
    AdamCorr c;
    float coef;
    STEP_HD_MEMBER void one(float (&x)[3]) const { adam_moments(adam_grad(x[0], coef, a.gs), x[1], x[2], a, c); }
};

// launch 3 of LAMB over w, m, v: the direction again from the stored moments, and the step along it
struct LambApplyRule {
    static constexpr int kBufs = 3;
    static constexpr unsigned kStores = 1;
    AdamArgs a;
    AdamCorr c;
    float wd_s, lrt;                     // lrt: lr_s * trust_s, rounded once
    STEP_HD_MEMBER void one(float (&x)[3]) const {
        const float r = lamb_dir(x[0], x[1], x[2], a.eps, wd_s, c);
        const float dr = lrt * r;
        x[0] = x[0] - dr;
    }
};

struct LambSums {
    double r, w;
};

// What lane `lane` adds for an item in launch 1 of LAMB, before any store: the squares of the direction r (from the
// moments the launch is about to store) and of w, over lane_part's elements in lane_part's order (the groups of four
// elements q = lane, lane + 64, .. by (start mod 4 + j) / 4; `vec`: all four buffers are 16-byte aligned).
STEP_HD LambSums lamb_lane_sums(const float* w, const float* g, const float* m, const float* v, const GroupItem& it, int lane,
                                bool vec, const LambMomentsRule& rule) {
    LambSums s = {0.0, 0.0};
    const int r0 = (int)(it.start & 3);
    const int groups = (r0 + it.len + 3) >> 2;
    for (int q = lane; q < groups; q += kLanes) {
        const int j0 = 4 * q - r0;
        Vec4 wv, gv, mv, vv;
        const bool whole = j0 >= 0 && j0 + 4 <= it.len;
        if (vec && whole) {
            wv = *(const Vec4*)(w + it.start + j0);
            gv = *(const Vec4*)(g + it.start + j0);
            mv = *(const Vec4*)(m + it.start + j0);
            vv = *(const Vec4*)(v + it.start + j0);
        } else {
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                const bool in = j >= 0 && j < it.len;
                wv.v[e] = in ? w[it.start + j] : 0.0f;
                gv.v[e] = in ? g[it.start + j] : 0.0f;
                mv.v[e] = in ? m[it.start + j] : 0.0f;
                vv.v[e] = in ? v[it.start + j] : 0.0f;
            }
        }
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + e;
            if (j < 0 || j >= it.len) continue;
            float x[3] = {gv.v[e], mv.v[e], vv.v[e]};
            rule.one(x);
            const double r = (double)lamb_dir(wv.v[e], x[1], x[2], rule.a.eps, it.wd_s, rule.c);
            const double wd = (double)wv.v[e];
            s.r = s.r + r * r;           // the product of two widened fp32 values is exact
            s.w = s.w + wd * wd;
        }
    }
    return s;
}

// the tests of tensor s in launch 2 of LAMB: its scales finite and >= 0, its items a range of the table
STEP_HD bool lamb_tensor_ok(const X3DStepHyper& h, int a, int b, int64_t nitems) {
    return group_scale_ok(h.lr_scale) && group_scale_ok(h.wd_scale) && a >= 0 && a < b && (int64_t)b <= nitems;
}

// the trust ratio of one tensor of LAMB: |w| / |r| in fp64, rounded to fp32 once; 1 where it does not apply
STEP_HD float lamb_trust_rule(double wss, double rss, int adapt, int32_t nf) {
    const double a = sqrt(wss);
    const double b = sqrt(rss);
    const float q = (float)(a / b);
    const bool ok = adapt != 0 && a > 0.0 && b > 0.0 && nf == 0 && q >= 0.0f && q <= 3.402823466e38f;
    return ok ? q : 1.0f;
}

// What the thread of tensor s does in launch 2 of LAMB, after the decision.  nf: the record's counts, or null without a state.
template <class Src>
STEP_HD void lamb_tensor(const Src& rsrc, const Src& wsrc, int s, const int32_t* seg_item, int64_t nitems,
                         const X3DStepHyper* hyper, const uint8_t* adapt, const int32_t* nf, double* wsumsq, double* rsumsq,
                         float* trust) {
    const int a = seg_item[s], b = seg_item[s + 1];
    if (!lamb_tensor_ok(hyper[s], a, b, nitems)) return;
    const double wss = tensor_part(wsrc, a, b).sumsq;
    const double rss = tensor_part(rsrc, a, b).sumsq;
    wsumsq[s] = wss;
    rsumsq[s] = rss;
    trust[s] = lamb_trust_rule(wss, rss, adapt[s], nf ? nf[s] : 0);
}

// -- the kept buffers (x3dstep_keep) ---------------------------------------------------------------------------------------
constexpr int kKeepPieces = X3DSTEP_ITEM / (4 * kLanes);      // 16-byte groups of a full item per lane: 8

struct KeepCopy {
    float* dst;
    const float* src;
    int len;                         // 0: the item is refused or lies past its buffer's end, nothing is copied
};

// Item i resolved against the table: both ends of the copy, or len 0.  The tests are those x3dstep_keep_host refuses a
// call for; the kernel makes them per item, since the table it reads is device memory nobody has checked.
STEP_HD KeepCopy keep_resolve(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t i, float* snap,
                              int64_t snap_n, int mode, bool* bad) {
    KeepCopy c = {nullptr, nullptr, 0};
    const X3DStepItem it = items[i];
    *bad = true;
    if (it.seg < 0 || it.seg >= nbuf || it.len < 1 || it.len > X3DSTEP_ITEM || it.start < 0 || it.start > snap_n - it.len)
        return c;
    const X3DStepKeep b = table[it.seg];
    const int64_t rel = it.start - b.offset;
    if (b.addr == 0 || (b.addr & 3) != 0 || b.len < 1 || b.offset < 0 || b.offset > snap_n - b.len || rel < 0) return c;
    *bad = false;
    const int64_t left = (int64_t)b.len - rel;               // elements of the buffer from this item's start on
    if (left < 1) return c;                                  // padding past the buffer's end
    float* live = (float*)(uintptr_t)b.addr + rel;
    c.len = left < it.len ? (int)left : it.len;
    c.dst = mode == X3DSTEP_KEEP_SAVE ? snap + it.start : live;
    c.src = mode == X3DSTEP_KEEP_SAVE ? live : snap + it.start;
    return c;
}

// The item walk: what lane `lane` of the item's wave does with buffers 0 (c.dst) and 1 (c.src) of a two-buffer operation.
// The 16-byte groups q = lane, lane + 64, .. when both addresses are 16-byte aligned (all of a lane's loads before its first
// store), the elements j = lane, lane + 64, .. otherwise and for the last len mod 4.
template <class Op>
STEP_HD void item_lane(const Op& op, const KeepCopy& c, int lane) {
    static_assert(Op::kBufs == 2, "the item walk takes two buffers");
    typedef typename Op::Elem Elem;
    typedef typename Op::Group Group;
    Elem* const p[2] = {(Elem*)c.dst, (Elem*)c.src};
    Group* const u[2] = {(Group*)c.dst, (Group*)c.src};
    const bool vec = (mod16(c.dst) | mod16(c.src)) == 0;
    const int groups = vec ? c.len >> 2 : 0;
    Group v[kKeepPieces][2];
#pragma unroll
    for (int k = 0; k < kKeepPieces; ++k) {
        const int q = lane + k * kLanes;
        if (q < groups) {
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (Op::kLoads >> b & 1) v[k][b] = u[b][q];
        }
    }
#pragma unroll
    for (int k = 0; k < kKeepPieces; ++k) {
        const int q = lane + k * kLanes;
        if (q < groups) {
            walk_unit(op, v[k]);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                if (Op::kStores >> b & 1) u[b][q] = v[k][b];
        }
    }
    for (int j = 4 * groups + lane; j < c.len; j += kLanes) walk_at(op, p, (int64_t)j);
}

// x3dstep_keep: buffer 0 <- buffer 1, on bits.  A restore reads the skip word first.
struct CopyOp {
    typedef uint32_t Elem;
    typedef Bits4 Group;
    static constexpr int kBufs = 2;
    static constexpr unsigned kLoads = 2, kStores = 1;
    const int64_t* state;
    int mode;
    STEP_HD_MEMBER bool begin(bool) { return mode != X3DSTEP_KEEP_RESTORE || state[X3DSTEP_S_SKIP] == 1; }
    STEP_HD_MEMBER void one(uint32_t (&x)[2]) const { x[0] = x[1]; }
};

// -- the weight average (x3dstep_ema, x3dstep_ema_keep) --------------------------------------------------------------------
// The number of the update being averaged: the host's `count`, plus (with a state) the updates applied so far, which
// x3dstep_measure / x3dstep_observe and x3dstep_apply counted in earlier launches.  The EMA launches only read the words.
STEP_HD int64_t ema_count(const int64_t* state, int64_t count) {
    return count + (state ? state[X3DSTEP_S_STEP] - state[X3DSTEP_S_SKIPPED] : 0);
}

// the latest x3dstep_apply left the parameters alone: there is nothing new to average
STEP_HD bool ema_skips(const int64_t* state) { return state && state[X3DSTEP_S_SKIP] == 1; }

struct EmaCoef {
    float d, omd;
};

// the decay of update k (k >= 1) and one minus it: fp64, each rounded to fp32 once
STEP_HD EmaCoef ema_coef(int64_t k, float decay, int warmup) {
    double d = (double)decay;
    if (warmup) {
        const double r = (double)(1 + k) / (10.0 + (double)k);
        if (r < d) d = r;
    }
    EmaCoef c;
    c.d = (float)d;
    c.omd = (float)(1.0 - (double)c.d);
    return c;
}

// one element, fp32, each operation rounded once
STEP_HD void ema_one(float& e, float w, const EmaCoef& c) {
    const float p = c.omd * w;
    e = fmaf(c.d, e, p);
}

// x3dstep_ema, x3dstep_ema_keep over e (the average), w: every thread reads the three state words and derives k and the
// two coefficients itself
struct EmaOp {
    typedef float Elem;
    typedef Float4 Group;
    static constexpr int kBufs = 2;
    static constexpr unsigned kLoads = 3, kStores = 1;
    const int64_t* state;
    int64_t count;
    float decay;
    int warmup;
    EmaCoef c;
    static constexpr int mode = X3DSTEP_KEEP_SAVE;
    STEP_HD_MEMBER bool begin(bool) {
        if (ema_skips(state)) return false;
        const int64_t k = ema_count(state, count);
        if (k <= 0) return false;
        c = ema_coef(k, decay, warmup);
        return true;
    }
    STEP_HD_MEMBER void one(float (&x)[2]) const { ema_one(x[0], x[1], c); }
};

// -- the exchange (x3dstep_swap, x3dstep_swap_keep) ------------------------------------------------------------------------
// Bits, not floats: no operation that could quieten a NaN or lose a payload ever sees the values.
struct SwapOp {
    typedef uint32_t Elem;
    typedef Bits4 Group;
    static constexpr int kBufs = 2;
    static constexpr unsigned kLoads = 3, kStores = 3;
    static constexpr int mode = X3DSTEP_KEEP_SAVE;
    STEP_HD_MEMBER bool begin(bool) { return true; }
    STEP_HD_MEMBER void one(uint32_t (&x)[2]) const {
        const uint32_t t = x[0];
        x[0] = x[1];
        x[1] = t;
    }
};

// -- precise BN statistics (x3dstep_pbn_accum, x3dstep_pbn_finish) ---------------------------------------------------------
// One accumulator per channel: the count of cells, the running mean of the cell means, the sum of squared deviations of
// the cell means from it (Welford) and the sum of the cell variances.  fp64, every operation rounded once.
struct PbnAcc {
    double n, mean, m2, vsum;
};

// one cell: the mean and the unbiased variance of one split of one batch
STEP_HD void pbn_cell(PbnAcc& a, float mu32, float v32) {
    const double mu = (double)mu32;
    const double v = (double)v32;
    const double n1 = a.n + 1.0;
    const double d = mu - a.mean;
    const double q = d / n1;
    const double mean1 = a.mean + q;
    const double r = mu - mean1;
    const double p = d * r;
    a.m2 = a.m2 + p;
    a.vsum = a.vsum + v;
    a.mean = mean1;
    a.n = n1;
}

// a <- a then b (the accumulators of two ranks, in rank order)
STEP_HD void pbn_merge(PbnAcc& a, const PbnAcc& b) {
    if (b.n == 0.0) return;
    if (a.n == 0.0) {
        a = b;
        return;
    }
    const double n = a.n + b.n;
    const double d = b.mean - a.mean;
    const double f = b.n / n;
    const double t = d * f;
    const double dd = d * d;
    const double ab = a.n * b.n;
    const double g = ab / n;
    const double u = dd * g;
    const double s = a.m2 + b.m2;
    a.mean = a.mean + t;
    a.m2 = s + u;
    a.vsum = a.vsum + b.vsum;
    a.n = n;
}

// the pooled mean and variance, each rounded to fp32 once; NaN in both when the count is not the expected one
STEP_HD void pbn_result(const PbnAcc& a, int64_t expect_n, float* mean32, float* var32) {
    if (!(a.n == (double)expect_n)) {
        uint32_t u = 0x7fc00000u;
        float q;
        memcpy(&q, &u, 4);
        *mean32 = q;
        *var32 = q;
        return;
    }
    const double s = a.vsum + a.m2;
    *mean32 = (float)a.mean;
    *var32 = (float)(s / a.n);
}

// Work item i resolved against the layer table: the layer, the first channel within it, the count of channels (0: the
// item is refused, nothing is touched) and the first accumulator.  The tests are those the twins refuse a call for; the
// kernels make them per item, since the tables they read are device memory nobody has checked.  snap_n < 0: x3dstep_pbn_accum,
// which does not touch the snapshot.
struct PbnRun {
    X3DStepPbnLayer layer;
    int64_t c0, acc0;
    int len;
};

STEP_HD int64_t pbn_channels(const X3DStepPbnLayer* layers, int nlayers) {
    const X3DStepPbnLayer last = layers[nlayers - 1];
    return last.first + (int64_t)last.C;
}

STEP_HD PbnRun pbn_resolve(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t i, int64_t snap_n) {
    PbnRun r;
    r.len = 0;
    r.c0 = r.acc0 = 0;
    const X3DStepItem it = work[i];
    if (it.seg < 0 || it.seg >= nlayers || it.len < 1 || it.len > X3DSTEP_PBN_RUN) return r;
    r.layer = layers[it.seg];
    const X3DStepPbnLayer& L = r.layer;
    if (L.mean_addr == 0 || L.var_addr == 0 || ((L.mean_addr | L.var_addr) & 3) != 0 || L.C < 1 || L.S < 1 || L.first < 0 ||
        L.first > X3DSTEP_PBN_MAX_CHANNELS - L.C || it.start < L.first || it.start - L.first > (int64_t)L.C - it.len)
        return r;
    const int64_t total = pbn_channels(layers, nlayers);
    if (total > X3DSTEP_PBN_MAX_CHANNELS || L.first + (int64_t)L.C > total) return r;
    if (snap_n >= 0) {
        const int64_t span = (int64_t)L.S * (int64_t)L.C;
        if (L.mean_off < 0 || L.var_off < 0 || span > snap_n || L.mean_off > snap_n - span || L.var_off > snap_n - span)
            return r;
    }
    r.c0 = it.start - L.first;
    r.acc0 = it.start;
    r.len = it.len;
    return r;
}

// what the thread of channel c0 + t of a run does in x3dstep_pbn_accum: one cell update per split, splits in order
STEP_HD void pbn_accum_one(const PbnRun& r, int t, double* acc) {
    const float* mean = (const float*)(uintptr_t)r.layer.mean_addr;
    const float* var = (const float*)(uintptr_t)r.layer.var_addr;
    const int64_t c = r.c0 + t;
    PbnAcc a = *(const PbnAcc*)(acc + 4 * (r.acc0 + t));
    for (int j = 0; j < r.layer.S; ++j) {
        const int64_t at = (int64_t)j * r.layer.C + c;
        pbn_cell(a, mean[at], var[at]);
    }
    *(PbnAcc*)(acc + 4 * (r.acc0 + t)) = a;
}

// ... and in x3dstep_pbn_finish: the W accumulators of the channel merged in rank order, the result into all S slots
STEP_HD void pbn_finish_one(const PbnRun& r, int t, const double* acc_all, int W, int64_t total, int64_t expect_n,
                            float* snap) {
    const int64_t c = r.c0 + t;
    PbnAcc a = *(const PbnAcc*)(acc_all + 4 * (r.acc0 + t));
    for (int w = 1; w < W; ++w) pbn_merge(a, *(const PbnAcc*)(acc_all + 4 * ((int64_t)w * total + r.acc0 + t)));
    float m32, v32;
    pbn_result(a, expect_n, &m32, &v32);
    for (int j = 0; j < r.layer.S; ++j) {
        const int64_t at = (int64_t)j * r.layer.C + c;
        snap[r.layer.mean_off + at] = m32;
        snap[r.layer.var_off + at] = v32;
    }
}

}  // namespace x3ds
