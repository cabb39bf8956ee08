// The host's part of libx3dstep (include/x3dstep.h): error text, sizes, the item-table builder and the *_host twins: the
// launches of the .hip files run serially through the same step_core.h, the two walks included.  Plain C++, no HIP call.
#include <stdarg.h>
#include <stdio.h>

#include "step_priv.h"

static thread_local char g_err[512] = "";

void x3dstep_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* x3dstep_last_error(void) { return g_err; }
extern "C" int x3dstep_abi_version(void) { return X3DSTEP_ABI_VERSION; }
extern "C" size_t x3dstep_item_bytes(void) { return sizeof(X3DStepItem); }
extern "C" size_t x3dstep_header_bytes(void) { return sizeof(X3DStepHeader); }
extern "C" size_t x3dstep_record_bytes(int S) { return S < 1 || S > X3DSTEP_MAX_SEGMENTS ? 0 : x3ds::record_bytes(S); }
extern "C" size_t x3dstep_workspace_bytes(int64_t nitems) {
    return nitems < 1 || nitems > X3DSTEP_MAX_ITEMS ? 0 : x3ds::scratch_bytes(nitems);
}

// counts (items == nullptr) or writes the item table; -1 when the segment table is refused
static int64_t walk_items(const int64_t* seg_off, int S, X3DStepItem* items, int64_t cap, int32_t* seg_item) {
    if (!seg_off || S < 1 || S > X3DSTEP_MAX_SEGMENTS || seg_off[0] != 0) return -1;
    int64_t count = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t len = seg_off[s + 1] - seg_off[s];
        if (len < 1 || len > 0x7fffffff) return -1;
        if (seg_item) seg_item[s] = (int32_t)count;
        for (int64_t at = 0; at < len; at += X3DSTEP_ITEM) {
            if (count >= X3DSTEP_MAX_ITEMS) return -1;
            if (items) {
                if (count >= cap) return -1;
                items[count].start = seg_off[s] + at;
                items[count].seg = s;
                items[count].len = (int32_t)(len - at < X3DSTEP_ITEM ? len - at : X3DSTEP_ITEM);
            }
            ++count;
        }
    }
    if (seg_item) seg_item[S] = (int32_t)count;
    return count;
}

extern "C" int64_t x3dstep_item_count(const int64_t* seg_off, int S) {
    const int64_t c = walk_items(seg_off, S, nullptr, 0, nullptr);
    if (c < 0) {
        x3dstep_set_error("x3dstep_item_count: S %d outside 1 .. %d, seg_off[0] != 0 or a tensor outside 1 .. 2^31 - 1 elements",
                          S, X3DSTEP_MAX_SEGMENTS);
        return X3DSTEP_EINVAL;
    }
    return c;
}

extern "C" int64_t x3dstep_build_items(const int64_t* seg_off, int S, X3DStepItem* items, int64_t cap, int32_t* seg_item) {
    if (!items || !seg_item || cap < 1) {
        x3dstep_set_error("x3dstep_build_items: null table or no capacity");
        return X3DSTEP_EINVAL;
    }
    const int64_t c = walk_items(seg_off, S, items, cap, seg_item);
    if (c < 0) {
        x3dstep_set_error("x3dstep_build_items: the segment table is refused (see x3dstep_item_count) or needs more than "
                          "%lld items", (long long)cap);
        return X3DSTEP_EINVAL;
    }
    return c;
}

static bool ranges_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * 4;
    return x < y + bytes && y < x + bytes;
}

// The flat walk of step_priv.h, serially: the plan decides which element goes through a 16-byte group; the arithmetic is
// per element.
template <class Op>
static void flat_host(const Op& op, const x3ds::Bufs<Op>& bufs, int64_t n) {
    using namespace x3ds;
    const Plan plan = flat_plan(bufs, n);
    if (!plan.vec) {
        for (int64_t i = 0; i < n; ++i) walk_at(op, bufs.p, i);
        return;
    }
    typename Op::Group* u[Op::kBufs];
    for (int b = 0; b < Op::kBufs; ++b) u[b] = (typename Op::Group*)(bufs.p[b] + plan.head);
    for (int64_t i = 0; i < plan.head; ++i) walk_at(op, bufs.p, i);
    for (int64_t q = 0; q < plan.groups; ++q) walk_at(op, u, q);
    for (int64_t i = plan.tail; i < n; ++i) walk_at(op, bufs.p, i);
}

// The tables are host memory in a twin: refuse the call for what the kernel would leave out item by item.
static int table_host_ok(const char* who, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                         float* snap, int64_t snap_n) {
    using namespace x3ds;
    for (int b = 0; b < nbuf; ++b) {
        const X3DStepKeep k = table[b];
        if (k.addr == 0 || (k.addr & 3) != 0 || k.len < 1 || k.offset < 0 || k.offset > snap_n - k.len ||
            (b > 0 && k.offset < table[b - 1].offset + table[b - 1].len)) {
            x3dstep_set_error("%s: buffer %d: a null or unaligned address, or a range outside snap or over the buffer before "
                              "it", who, b);
            return X3DSTEP_EINVAL;
        }
    }
    for (int64_t i = 0; i < nitems; ++i) {
        bool bad;
        (void)keep_resolve(table, nbuf, items, i, snap, snap_n, X3DSTEP_KEEP_SAVE, &bad);
        if (bad) {
            x3dstep_set_error("%s: item %lld lies outside snap or outside its buffer's range", who, (long long)i);
            return X3DSTEP_EINVAL;
        }
    }
    return X3DSTEP_OK;
}

// The item walk of step_priv.h, serially: item after item, lane after lane.
template <class Op>
static void items_host(const Op& op, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                       float* snap, int64_t snap_n) {
    using namespace x3ds;
    for (int64_t i = 0; i < nitems; ++i) {
        bool bad;
        const KeepCopy c = keep_resolve(table, nbuf, items, i, snap, snap_n, op.mode, &bad);
        if (c.len > 0)
            for (int l = 0; l < kLanes; ++l) item_lane(op, c, l);
    }
}

// the argument checks x3dstep_observe and its twin share (step.hip calls it too)
int x3dstep_check_observe(const char* who, const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                          const int32_t* seg_item, int64_t nitems, const void* workspace, const int64_t* state,
                          const void* ring, int R) {
    if (!g || !seg_off || !items || !seg_item || !workspace || !state || !ring || n < 1 || S < 1 ||
        S > X3DSTEP_MAX_SEGMENTS || nitems < S || nitems > X3DSTEP_MAX_ITEMS || R < 1 || ((uintptr_t)g & 3) != 0 ||
        (((uintptr_t)seg_off | (uintptr_t)items | (uintptr_t)workspace | (uintptr_t)state | (uintptr_t)ring) & 7) != 0 ||
        ((uintptr_t)seg_item & 3) != 0) {
        x3dstep_set_error("%s: null or unaligned pointer, n %lld < 1, S %d outside 1 .. %d, nitems %lld outside S .. %d or "
                          "R %d < 1", who, (long long)n, S, X3DSTEP_MAX_SEGMENTS, (long long)nitems, X3DSTEP_MAX_ITEMS, R);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// launches 1 and 2 on the host: what x3dstep_measure_host and x3dstep_observe_host share
static int measure_host(const char* who, const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                        const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring, int R,
                        double max_norm, double inv_world) {
    using namespace x3ds;
    const int rc = x3dstep_check_observe(who, g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R);
    if (rc) return rc;
    // the tables are host memory here: refuse what would read or write outside g, the scratch or the record
    if (seg_off[0] != 0 || seg_off[S] != n || seg_item[0] != 0 || seg_item[S] != nitems) {
        x3dstep_set_error("%s: the tables do not cover n %lld elements and %lld items", who, (long long)n, (long long)nitems);
        return X3DSTEP_EINVAL;
    }
    for (int s = 0; s < S; ++s) {
        bool ok = seg_off[s + 1] > seg_off[s] && seg_item[s + 1] > seg_item[s];
        int64_t at = seg_off[s];
        for (int i = seg_item[s]; ok && i < seg_item[s + 1]; ++i) {
            ok = items[i].seg == s && items[i].start == at && items[i].len >= 1 && items[i].len <= X3DSTEP_ITEM;
            at += items[i].len;
        }
        if (!ok || at != seg_off[s + 1]) {
            x3dstep_set_error("%s: the items of tensor %d do not cover it", who, s);
            return X3DSTEP_EINVAL;
        }
    }
    // launch 1
    const Scratch w = scratch_at(workspace, nitems);
    const bool vec = ((uintptr_t)g & 15) == 0;
    for (int64_t i = 0; i < nitems; ++i) {
        const X3DStepItem it = items[i];
        const uint64_t first = (uint64_t)(it.start - seg_off[it.seg]);
        Part lanes[kLanes];
        for (int l = 0; l < kLanes; ++l) lanes[l] = lane_part(g, it.start, it.len, first, l, vec);
        for (int off = kLanes / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) part_merge(lanes[l], lanes[l + off]);
        w.sumsq[i] = lanes[0].sumsq;
        w.hash[i] = lanes[0].hash;
        w.nf[i] = lanes[0].nf;
    }
    // launch 2
    const int64_t step = state[X3DSTEP_S_STEP];
    const Record r = record_at(ring, R, S, step);
    Sum total = {0.0, 0.0};
    int32_t nf = 0, first_bad = -1;
    for (int s = 0; s < S; ++s) {
        const Part p = tensor_part(ScratchSource{w}, seg_item[s], seg_item[s + 1]);
        r.sumsq[s] = p.sumsq;
        r.hash[s] = p.hash;
        r.nf[s] = p.nf;
        sum_add(total, p.sumsq);
        nf += p.nf;
        if (first_bad < 0 && p.nf > 0) first_bad = s;
    }
    finish_step(r, state, step, S, sum_value(total), nf, first_bad, max_norm, inv_world);
    return X3DSTEP_OK;
}

extern "C" int x3dstep_measure_host(const float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                                    const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring,
                                    int R, double max_norm, double inv_world) {
    return measure_host("x3dstep_measure_host", g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R, max_norm,
                        inv_world);
}

extern "C" int x3dstep_observe_host(float* g, int64_t n, const int64_t* seg_off, int S, const X3DStepItem* items,
                                    const int32_t* seg_item, int64_t nitems, void* workspace, int64_t* state, void* ring,
                                    int R, double max_norm, double inv_world) {
    using namespace x3ds;
    const int rc = measure_host("x3dstep_observe_host", g, n, seg_off, S, items, seg_item, nitems, workspace, state, ring, R,
                                max_norm, inv_world);
    if (rc) return rc;
    // launch 3
    if (max_norm > 0.0) {
        const float coef = state_coef(state);
        if (coef != 1.0f)
            for (int64_t i = 0; i < n; ++i) g[i] = scale_one(g[i], coef);
    }
    return X3DSTEP_OK;
}

extern "C" size_t x3dstep_keep_bytes(void) { return sizeof(X3DStepKeep); }

// the argument checks x3dstep_apply and its twin share (no pointer is followed)
int x3dstep_check_apply(const char* who, const float* w, const float* g, const float* m, int64_t n, const int64_t* state,
                        const void* ring, int R, int S) {
    if (!w || !g || !m || !state || !ring || n < 1 || n > ((int64_t)1 << 40) || R < 1 || S < 1 || S > X3DSTEP_MAX_SEGMENTS ||
        (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m) & 3) != 0 || (((uintptr_t)state | (uintptr_t)ring) & 7) != 0 ||
        w == g || w == m || g == m) {
        x3dstep_set_error("%s: null, unaligned or repeated pointer, n %lld outside 1 .. 2^40, R %d < 1 or S %d outside 1 .. %d",
                          who, (long long)n, R, S, X3DSTEP_MAX_SEGMENTS);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_apply_host(float* w, const float* g, float* m, int64_t n, int64_t* state, const void* ring, int R, int S,
                                  float lr, float momentum, float weight_decay, float grad_scale, int first) {
    using namespace x3ds;
    const int rc = x3dstep_check_apply("x3dstep_apply_host", w, g, m, n, state, ring, R, S);
    if (rc) return rc;
    if (!apply_decision(state, ring, R, S).go) {
        x3dstep_set_error("x3dstep_apply_host: the state's step counter is 0: nothing has been measured");
        return X3DSTEP_EINVAL;
    }
    ApplyOp op = {state, ring, R, S, {lr, momentum, weight_decay, grad_scale, first ? 1 : 0, 0}, 1.0f};
    if (op.begin(true)) flat_host(op, Bufs<ApplyOp>{{w, (float*)g, m}}, n);
    return X3DSTEP_OK;
}

// -- the grouped update -----------------------------------------------------------------------------------------------------
extern "C" size_t x3dstep_hyper_bytes(void) { return sizeof(X3DStepHyper); }

// the argument checks x3dstep_apply_groups and its twin share (no pointer is followed: the tables may be device memory)
int x3dstep_check_groups(const char* who, const float* w, const float* g, const float* m, int64_t n, const X3DStepItem* items,
                         int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state, const void* ring, int R,
                         float momentum, int first, int nesterov) {
    if (!w || !g || !m || !items || !hyper || n < 1 || n > ((int64_t)1 << 40) || nitems < 1 || nitems > X3DSTEP_MAX_ITEMS ||
        S < 1 || S > X3DSTEP_MAX_SEGMENTS || (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)hyper) & 3) != 0 ||
        ((uintptr_t)items & 7) != 0) {
        x3dstep_set_error("%s: null or unaligned pointer, n %lld outside 1 .. 2^40, nitems %lld outside 1 .. %d or S %d outside "
                          "1 .. %d", who, (long long)n, (long long)nitems, X3DSTEP_MAX_ITEMS, S, X3DSTEP_MAX_SEGMENTS);
        return X3DSTEP_EINVAL;
    }
    if (ranges_overlap(w, g, n) || ranges_overlap(w, m, n) || ranges_overlap(g, m, n)) {
        x3dstep_set_error("%s: w, g and m overlap", who);
        return X3DSTEP_EINVAL;
    }
    if (state && (!ring || R < 1 || (((uintptr_t)state | (uintptr_t)ring) & 7) != 0)) {
        x3dstep_set_error("%s: a state without a ring, an unaligned state or ring, or R %d < 1", who, R);
        return X3DSTEP_EINVAL;
    }
    if ((first != 0 && first != 1) || (nesterov != 0 && nesterov != 1) || (nesterov == 1 && !(momentum > 0.0f))) {
        x3dstep_set_error("%s: first %d or nesterov %d outside {0, 1}, or nesterov with momentum %g <= 0", who, first, nesterov,
                          (double)momentum);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// the in-order tiling of [0, n) by the items of S tensors, which the twins that walk an item table ask for
static int tiling_host_ok(const char* who, const X3DStepItem* items, int64_t nitems, int S, int64_t n) {
    int64_t at = 0;
    int32_t seg = 0;
    for (int64_t i = 0; i < nitems; ++i) {
        const X3DStepItem it = items[i];
        if (it.seg < seg || it.seg >= S || it.len < 1 || it.len > X3DSTEP_ITEM || it.start != at || it.start > n - it.len) {
            x3dstep_set_error("%s: item %lld (start %lld, tensor %d, len %d) is not the next piece of the in-order tiling of "
                              "[0, %lld) over %d tensors", who, (long long)i, (long long)it.start, it.seg, it.len, (long long)n,
                              S);
            return X3DSTEP_EINVAL;
        }
        at += it.len;
        seg = it.seg;
    }
    if (at != n) {
        x3dstep_set_error("%s: the items cover %lld of %lld elements", who, (long long)at, (long long)n);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// x3dstep_apply_groups_host (trust null) and x3dstep_apply_lars_host after their argument checks
static int groups_host(const char* who, float* w, const float* g, float* m, int64_t n, const X3DStepItem* items,
                       int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring,
                       int R, float lr, float momentum, float weight_decay, float grad_scale, int first, int nesterov) {
    using namespace x3ds;
    // the tables are host memory here: refuse the call for what the kernel would leave out item by item
    for (int s = 0; s < S; ++s) {
        if (!group_scale_ok(hyper[s].lr_scale) || !group_scale_ok(hyper[s].wd_scale)) {
            x3dstep_set_error("%s: tensor %d: a scale that is negative or not finite (lr_scale %g, wd_scale %g)", who, s,
                              (double)hyper[s].lr_scale, (double)hyper[s].wd_scale);
            return X3DSTEP_EINVAL;
        }
        if (trust && !group_scale_ok(trust[s])) {
            x3dstep_set_error("%s: tensor %d: a trust ratio that is negative or not finite (%g)", who, s, (double)trust[s]);
            return X3DSTEP_EINVAL;
        }
    }
    const int rt = tiling_host_ok(who, items, nitems, S, n);
    if (rt) return rt;
    float coef = 1.0f;
    if (state) {
        if (!apply_decision(state, ring, R, S).go) {
            x3dstep_set_error("%s: the state's step counter is 0: nothing has been measured", who);
            return X3DSTEP_EINVAL;
        }
        if (!apply_begin(state, ring, R, S, true, &coef)) return X3DSTEP_OK;
    }
    const SgdArgs a = {lr, momentum, weight_decay, grad_scale, first, nesterov};
    for (int64_t i = 0; i < nitems; ++i) {
        float t = 1.0f;
        const GroupItem c = trust ? lars_resolve(items, i, hyper, trust, S, n, a, &t) : group_resolve(items, i, hyper, S, n, a);
        if (c.len < 1) continue;
        for (int l = 0; l < kLanes; ++l) {
            if (trust)
                group_lane<true>(w, g, m, c, l, coef, a, t);
            else
                group_lane(w, g, m, c, l, coef, a);
        }
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_apply_groups_host(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items,
                                         int64_t nitems, const X3DStepHyper* hyper, int S, int64_t* state, const void* ring,
                                         int R, float lr, float momentum, float weight_decay, float grad_scale, int first,
                                         int nesterov) {
    const char* who = "x3dstep_apply_groups_host";
    const int rc = x3dstep_check_groups(who, w, g, m, n, items, nitems, hyper, S, state, ring, R, momentum, first, nesterov);
    if (rc) return rc;
    return groups_host(who, w, g, m, n, items, nitems, hyper, nullptr, S, state, ring, R, lr, momentum, weight_decay,
                       grad_scale, first, nesterov);
}

// -- trust ratios -----------------------------------------------------------------------------------------------------------
extern "C" size_t x3dstep_trust_workspace_bytes(int64_t nitems) {
    return nitems < 1 || nitems > X3DSTEP_MAX_ITEMS ? 0 : (size_t)nitems * 8;
}

int x3dstep_check_lars(const char* who, const float* w, const float* g, const float* m, int64_t n, const X3DStepItem* items,
                       int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S, const int64_t* state,
                       const void* ring, int R, float momentum, int first, int nesterov) {
    const int rc = x3dstep_check_groups(who, w, g, m, n, items, nitems, hyper, S, state, ring, R, momentum, first, nesterov);
    if (rc) return rc;
    if (!trust || ((uintptr_t)trust & 3) != 0) {
        x3dstep_set_error("%s: a null or unaligned trust table", who);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_apply_lars_host(float* w, const float* g, float* m, int64_t n, const X3DStepItem* items, int64_t nitems,
                                       const X3DStepHyper* hyper, const float* trust, int S, int64_t* state, const void* ring,
                                       int R, float lr, float momentum, float weight_decay, float grad_scale, int first,
                                       int nesterov) {
    const char* who = "x3dstep_apply_lars_host";
    const int rc = x3dstep_check_lars(who, w, g, m, n, items, nitems, hyper, trust, S, state, ring, R, momentum, first, nesterov);
    if (rc) return rc;
    return groups_host(who, w, g, m, n, items, nitems, hyper, trust, S, state, ring, R, lr, momentum, weight_decay, grad_scale,
                       first, nesterov);
}

// the argument checks x3dstep_trust and its twin share (no pointer is followed: the tables may be device memory)
int x3dstep_check_trust(const char* who, const float* w, int64_t n, const X3DStepItem* items, const int32_t* seg_item,
                        int64_t nitems, const X3DStepHyper* hyper, const float* eta, int S, const int64_t* state,
                        const void* ring, int R, const void* workspace, const double* wsumsq, const float* trust, float eps,
                        int clip) {
    if (!w || !items || !seg_item || !hyper || !eta || !state || !ring || !workspace || !wsumsq || !trust || n < 1 ||
        n > ((int64_t)1 << 40) || S < 1 || S > X3DSTEP_MAX_SEGMENTS || nitems < S || nitems > X3DSTEP_MAX_ITEMS || R < 1 ||
        (((uintptr_t)w | (uintptr_t)seg_item | (uintptr_t)hyper | (uintptr_t)eta | (uintptr_t)trust) & 3) != 0 ||
        (((uintptr_t)items | (uintptr_t)state | (uintptr_t)ring | (uintptr_t)workspace | (uintptr_t)wsumsq) & 7) != 0) {
        x3dstep_set_error("%s: null or unaligned pointer, n %lld outside 1 .. 2^40, S %d outside 1 .. %d, nitems %lld outside "
                          "S .. %d or R %d < 1", who, (long long)n, S, X3DSTEP_MAX_SEGMENTS, (long long)nitems,
                          X3DSTEP_MAX_ITEMS, R);
        return X3DSTEP_EINVAL;
    }
    if (!(eps >= 0.0f && eps <= 3.402823466e38f) || (clip != 0 && clip != 1)) {
        x3dstep_set_error("%s: eps %g negative or not finite, or clip %d outside {0, 1}", who, (double)eps, clip);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_trust_host(const float* w, int64_t n, const X3DStepItem* items, const int32_t* seg_item, int64_t nitems,
                                  const X3DStepHyper* hyper, const float* eta, int S, const int64_t* state, const void* ring,
                                  int R, void* workspace, double* wsumsq, float* trust, float lr, float weight_decay,
                                  float grad_scale, float eps, int clip) {
    using namespace x3ds;
    const char* who = "x3dstep_trust_host";
    const int rc = x3dstep_check_trust(who, w, n, items, seg_item, nitems, hyper, eta, S, state, ring, R, workspace, wsumsq,
                                       trust, eps, clip);
    if (rc) return rc;
    // the tables are host memory here: refuse the call for what the kernels would leave out item by item, tensor by tensor
    const int rt = tiling_host_ok(who, items, nitems, S, n);
    if (rt) return rt;
    for (int s = 0; s < S; ++s) {
        const int a = seg_item[s], b = seg_item[s + 1];
        bool ok = trust_tensor_ok(hyper[s], eta[s], a, b, nitems) && (s > 0 || a == 0) && (s + 1 < S || b == nitems);
        for (int i = a; ok && i < b; ++i) ok = items[i].seg == s;
        if (!ok) {
            x3dstep_set_error("%s: tensor %d: eta %g or a scale (%g, %g) negative or not finite, or items %d .. %d are not its "
                              "own", who, s, (double)eta[s], (double)hyper[s].lr_scale, (double)hyper[s].wd_scale, a, b);
            return X3DSTEP_EINVAL;
        }
    }
    const int64_t step = state[X3DSTEP_S_STEP];
    if (step == 0) {
        x3dstep_set_error("%s: the state's step counter is 0: nothing has been measured", who);
        return X3DSTEP_EINVAL;
    }
    // launch 1
    double* part = (double*)workspace;
    const bool vec = ((uintptr_t)w & 15) == 0;
    for (int64_t i = 0; i < nitems; ++i) {
        double lanes[kLanes];
        for (int l = 0; l < kLanes; ++l) lanes[l] = trust_item_ok(items[i], S, n) ? trust_lane(w, items[i], l, vec) : trust_nan();
        for (int off = kLanes / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) lanes[l] = lanes[l] + lanes[l + off];
        part[i] = lanes[0];
    }
    // launch 2
    const Record rec = record_at((void*)ring, R, S, step - 1);
    const float coef = state_coef(state);
    const TrustArgs t = {lr, weight_decay, grad_scale, eps, clip};
    const SumsqSource src = {part, part, 0};
    for (int s = 0; s < S; ++s) trust_tensor(src, s, seg_item, nitems, hyper, eta, rec, coef, t, wsumsq, trust);
    return X3DSTEP_OK;
}

// -- second-moment updates ----------------------------------------------------------------------------------------------------
extern "C" size_t x3dstep_lamb_workspace_bytes(int64_t nitems) {
    return nitems < 1 || nitems > X3DSTEP_MAX_ITEMS ? 0 : (size_t)nitems * 16;
}

int x3dstep_check_adam(const char* who, const float* w, const float* g, const float* m, const float* v, bool need_g, int64_t n,
                       const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state,
                       const void* ring, int R, int64_t count, float b1, float b2, float eps, int decoupled) {
    if (!w || (need_g && !g) || !m || !v || !items || !hyper || n < 1 || n > ((int64_t)1 << 40) || nitems < 1 ||
        nitems > X3DSTEP_MAX_ITEMS || S < 1 || S > X3DSTEP_MAX_SEGMENTS ||
        (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)hyper) & 3) != 0 ||
        ((uintptr_t)items & 7) != 0) {
        x3dstep_set_error("%s: null or unaligned pointer, n %lld outside 1 .. 2^40, nitems %lld outside 1 .. %d or S %d outside "
                          "1 .. %d", who, (long long)n, (long long)nitems, X3DSTEP_MAX_ITEMS, S, X3DSTEP_MAX_SEGMENTS);
        return X3DSTEP_EINVAL;
    }
    const float* p[4] = {w, g, m, v};
    for (int a = 0; a < 4; ++a)
        for (int b = a + 1; b < 4; ++b)
            if (p[a] && p[b] && ranges_overlap(p[a], p[b], n)) {
                x3dstep_set_error("%s: w, g, m and v overlap", who);
                return X3DSTEP_EINVAL;
            }
    if (state && (!ring || R < 1 || (((uintptr_t)state | (uintptr_t)ring) & 7) != 0)) {
        x3dstep_set_error("%s: a state without a ring, an unaligned state or ring, or R %d < 1", who, R);
        return X3DSTEP_EINVAL;
    }
    if (!x3ds::adam_args_ok(b1, b2, eps, decoupled)) {
        x3dstep_set_error("%s: b1 %g or b2 %g outside [0, 1), eps %g negative or not finite, or decoupled %d outside {0, 1}", who,
                          (double)b1, (double)b2, (double)eps, decoupled);
        return X3DSTEP_EINVAL;
    }
    if (!state && count < 1) {
        x3dstep_set_error("%s: without a state the count %lld is the number of this update: it must be >= 1", who,
                          (long long)count);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

int x3dstep_check_lamb_moments(const char* who, const float* w, const float* g, const float* m, const float* v, int64_t n,
                               const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper, int S,
                               const int64_t* state, const void* ring, int R, int64_t count, float b1, float b2, float eps,
                               const void* workspace) {
    const int rc = x3dstep_check_adam(who, w, g, m, v, true, n, items, nitems, hyper, S, state, ring, R, count, b1, b2, eps, 1);
    if (rc) return rc;
    if (!workspace || ((uintptr_t)workspace & 7) != 0) {
        x3dstep_set_error("%s: a null or unaligned workspace", who);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

int x3dstep_check_lamb_trust(const char* who, const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper,
                             const uint8_t* adapt, int S, const int64_t* state, const void* ring, int R, int64_t count,
                             const void* workspace, const double* wsumsq, const double* rsumsq, const float* trust) {
    if (!seg_item || !hyper || !adapt || !workspace || !wsumsq || !rsumsq || !trust || S < 1 || S > X3DSTEP_MAX_SEGMENTS ||
        nitems < S || nitems > X3DSTEP_MAX_ITEMS || (((uintptr_t)seg_item | (uintptr_t)hyper | (uintptr_t)trust) & 3) != 0 ||
        (((uintptr_t)workspace | (uintptr_t)wsumsq | (uintptr_t)rsumsq) & 7) != 0 || wsumsq == rsumsq) {
        x3dstep_set_error("%s: null, unaligned or repeated pointer, S %d outside 1 .. %d or nitems %lld outside S .. %d", who, S,
                          X3DSTEP_MAX_SEGMENTS, (long long)nitems, X3DSTEP_MAX_ITEMS);
        return X3DSTEP_EINVAL;
    }
    if (state && (!ring || R < 1 || (((uintptr_t)state | (uintptr_t)ring) & 7) != 0)) {
        x3dstep_set_error("%s: a state without a ring, an unaligned state or ring, or R %d < 1", who, R);
        return X3DSTEP_EINVAL;
    }
    if (!state && count < 1) {
        x3dstep_set_error("%s: without a state the count %lld is the number of this update: it must be >= 1", who,
                          (long long)count);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

int x3dstep_check_lamb_apply(const char* who, const float* w, const float* m, const float* v, int64_t n,
                             const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S,
                             const int64_t* state, const void* ring, int R, int64_t count, float b1, float b2, float eps) {
    const int rc = x3dstep_check_adam(who, w, nullptr, m, v, false, n, items, nitems, hyper, S, state, ring, R, count, b1, b2, eps,
                                      1);
    if (rc) return rc;
    if (!trust || ((uintptr_t)trust & 3) != 0) {
        x3dstep_set_error("%s: a null or unaligned trust table", who);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// What the twins of these updates refuse where the kernels leave out or leave at once (the tables and the state are host
// memory here): a scale or a trust that is negative or not finite, an item table that is not the in-order tiling, a
// counter of 0 and k < 1.
static int adam_host_ok(const char* who, const X3DStepItem* items, int64_t nitems, const X3DStepHyper* hyper,
                        const float* trust, int S, int64_t n, const int64_t* state, const void* ring, int R, int64_t count) {
    using namespace x3ds;
    for (int s = 0; s < S; ++s) {
        if (!group_scale_ok(hyper[s].lr_scale) || !group_scale_ok(hyper[s].wd_scale)) {
            x3dstep_set_error("%s: tensor %d: a scale that is negative or not finite (lr_scale %g, wd_scale %g)", who, s,
                              (double)hyper[s].lr_scale, (double)hyper[s].wd_scale);
            return X3DSTEP_EINVAL;
        }
        if (trust && !group_scale_ok(trust[s])) {
            x3dstep_set_error("%s: tensor %d: a trust ratio that is negative or not finite (%g)", who, s, (double)trust[s]);
            return X3DSTEP_EINVAL;
        }
    }
    if (items) {
        const int rt = tiling_host_ok(who, items, nitems, S, n);
        if (rt) return rt;
    }
    if (state && !apply_decision(state, ring, R, S).go) {
        x3dstep_set_error("%s: the state's step counter is 0: nothing has been measured", who);
        return X3DSTEP_EINVAL;
    }
    const int64_t k = ema_count(state, count);
    if (k < 1) {
        x3dstep_set_error("%s: the number of this update among the applied ones is %lld: it must be >= 1", who, (long long)k);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_adam_host(float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items,
                                 int64_t nitems, const X3DStepHyper* hyper, int S, int64_t* state, const void* ring, int R,
                                 int64_t count, float lr, float b1, float b2, float eps, float weight_decay, float grad_scale,
                                 int decoupled) {
    using namespace x3ds;
    const char* who = "x3dstep_adam_host";
    int rc = x3dstep_check_adam(who, w, g, m, v, true, n, items, nitems, hyper, S, state, ring, R, count, b1, b2, eps, decoupled);
    if (!rc) rc = adam_host_ok(who, items, nitems, hyper, nullptr, S, n, state, ring, R, count);
    if (rc) return rc;
    float coef;
    int64_t k;
    if (!adam_begin(state, ring, R, S, count, true, &coef, &k)) return X3DSTEP_OK;
    const AdamArgs a = {lr, b1, b2, eps, weight_decay, grad_scale, decoupled};
    const SgdArgs sa = {a.lr, 0.0f, a.wd, a.gs, 0, 0};
    const AdamCorr corr = adam_corr(k, b1, b2);
    float* const base[4] = {w, (float*)g, m, v};
    for (int64_t i = 0; i < nitems; ++i) {
        const GroupItem c = group_resolve(items, i, hyper, S, n, sa);
        if (c.len < 1) continue;
        const AdamRule rule = {a, corr, coef, c.wd_s, adam_step_size(c.lr_s, corr), c.lr_s * c.wd_s};
        for (int l = 0; l < kLanes; ++l) rule_lane(rule, base, c.start, c.len, l);
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_lamb_moments_host(const float* w, const float* g, float* m, float* v, int64_t n, const X3DStepItem* items,
                                         int64_t nitems, const X3DStepHyper* hyper, int S, const int64_t* state,
                                         const void* ring, int R, int64_t count, float b1, float b2, float eps,
                                         float weight_decay, float grad_scale, void* workspace) {
    using namespace x3ds;
    const char* who = "x3dstep_lamb_moments_host";
    int rc = x3dstep_check_lamb_moments(who, w, g, m, v, n, items, nitems, hyper, S, state, ring, R, count, b1, b2, eps, workspace);
    if (!rc) rc = adam_host_ok(who, items, nitems, hyper, nullptr, S, n, state, ring, R, count);
    if (rc) return rc;
    float coef;
    int64_t k;
    if (!adam_begin((int64_t*)state, ring, R, S, count, false, &coef, &k)) return X3DSTEP_OK;
    const AdamArgs a = {0.0f, b1, b2, eps, weight_decay, grad_scale, 1};
    const SgdArgs sa = {0.0f, 0.0f, a.wd, a.gs, 0, 0};
    const LambMomentsRule rule = {a, adam_corr(k, b1, b2), coef};
    const bool vec = (((uintptr_t)w | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    double* rpart = (double*)workspace;
    double* wpart = rpart + nitems;
    float* const base[3] = {(float*)g, m, v};
    for (int64_t i = 0; i < nitems; ++i) {
        const GroupItem c = group_resolve(items, i, hyper, S, n, sa);
        LambSums lanes[kLanes];
        for (int l = 0; l < kLanes; ++l) {
            const LambSums bad = {trust_nan(), trust_nan()};
            lanes[l] = c.len > 0 ? lamb_lane_sums(w, g, m, v, c, l, vec, rule) : bad;
        }
        for (int off = kLanes / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) {
                lanes[l].r = lanes[l].r + lanes[l + off].r;
                lanes[l].w = lanes[l].w + lanes[l + off].w;
            }
        rpart[i] = lanes[0].r;
        wpart[i] = lanes[0].w;
        if (c.len < 1) continue;
        for (int l = 0; l < kLanes; ++l) rule_lane(rule, base, c.start, c.len, l);
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_lamb_trust_host(const int32_t* seg_item, int64_t nitems, const X3DStepHyper* hyper, const uint8_t* adapt,
                                       int S, const int64_t* state, const void* ring, int R, int64_t count,
                                       const void* workspace, double* wsumsq, double* rsumsq, float* trust) {
    using namespace x3ds;
    const char* who = "x3dstep_lamb_trust_host";
    int rc = x3dstep_check_lamb_trust(who, seg_item, nitems, hyper, adapt, S, state, ring, R, count, workspace, wsumsq, rsumsq,
                                      trust);
    if (rc) return rc;
    for (int s = 0; s < S; ++s) {
        const int a = seg_item[s], b = seg_item[s + 1];
        if (!(lamb_tensor_ok(hyper[s], a, b, nitems) && (s > 0 || a == 0) && (s + 1 < S || b == nitems))) {
            x3dstep_set_error("%s: tensor %d: a scale (%g, %g) negative or not finite, or items %d .. %d are not a range of the "
                              "table", who, s, (double)hyper[s].lr_scale, (double)hyper[s].wd_scale, a, b);
            return X3DSTEP_EINVAL;
        }
    }
    rc = adam_host_ok(who, nullptr, nitems, hyper, nullptr, S, 0, state, ring, R, count);
    if (rc) return rc;
    float coef;
    int64_t k;
    if (!adam_begin((int64_t*)state, ring, R, S, count, false, &coef, &k)) return X3DSTEP_OK;
    const int32_t* nf = state ? record_at((void*)ring, R, S, state[X3DSTEP_S_STEP] - 1).nf : nullptr;
    const double* rpart = (const double*)workspace;
    const SumsqSource rsrc = {rpart, rpart, 0};
    const SumsqSource wsrc = {rpart + nitems, rpart + nitems, 0};
    for (int s = 0; s < S; ++s) lamb_tensor(rsrc, wsrc, s, seg_item, nitems, hyper, adapt, nf, wsumsq, rsumsq, trust);
    return X3DSTEP_OK;
}

extern "C" int x3dstep_lamb_apply_host(float* w, const float* m, const float* v, int64_t n, const X3DStepItem* items,
                                       int64_t nitems, const X3DStepHyper* hyper, const float* trust, int S, int64_t* state,
                                       const void* ring, int R, int64_t count, float lr, float b1, float b2, float eps,
                                       float weight_decay) {
    using namespace x3ds;
    const char* who = "x3dstep_lamb_apply_host";
    int rc = x3dstep_check_lamb_apply(who, w, m, v, n, items, nitems, hyper, trust, S, state, ring, R, count, b1, b2, eps);
    if (!rc) rc = adam_host_ok(who, items, nitems, hyper, trust, S, n, state, ring, R, count);
    if (rc) return rc;
    float coef;
    int64_t k;
    if (!adam_begin(state, ring, R, S, count, true, &coef, &k)) return X3DSTEP_OK;
    const AdamArgs a = {lr, b1, b2, eps, weight_decay, 1.0f, 1};
    const SgdArgs sa = {a.lr, 0.0f, a.wd, a.gs, 0, 0};
    const AdamCorr corr = adam_corr(k, b1, b2);
    float* const base[3] = {w, (float*)m, (float*)v};
    for (int64_t i = 0; i < nitems; ++i) {
        float t = 1.0f;
        const GroupItem c = lars_resolve(items, i, hyper, trust, S, n, sa, &t);
        if (c.len < 1) continue;
        const LambApplyRule rule = {a, corr, c.wd_s, c.lr_s * t};
        for (int l = 0; l < kLanes; ++l) rule_lane(rule, base, c.start, c.len, l);
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_keep_host(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                                 int64_t snap_n, const int64_t* state, int mode) {
    using namespace x3ds;
    const char* who = "x3dstep_keep_host";
    const int rc = x3dstep_check_table(who, table, nbuf, items, nitems, snap, snap_n, state, true, mode, 0.0f);
    if (rc) return rc;
    const int rt = table_host_ok(who, table, nbuf, items, nitems, snap, snap_n);
    if (rt) return rt;
    CopyOp op = {state, mode};
    if (op.begin(false)) items_host(op, table, nbuf, items, nitems, snap, snap_n);
    return X3DSTEP_OK;
}

// -- the weight average and the exchange ----------------------------------------------------------------------------------
// the argument checks x3dstep_ema and its twin share (no pointer is followed)
int x3dstep_check_ema(const char* who, const float* e, const float* w, int64_t n, const int64_t* state, float decay) {
    if (!e || !w || n < 1 || n > ((int64_t)1 << 40) || (((uintptr_t)e | (uintptr_t)w) & 3) != 0 || ((uintptr_t)state & 7) != 0 ||
        !(decay >= 0.0f && decay < 1.0f) || ranges_overlap(e, w, n)) {
        x3dstep_set_error("%s: null, unaligned or overlapping pointers, n %lld outside 1 .. 2^40 or decay %g outside [0, 1)", who,
                          (long long)n, (double)decay);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

int x3dstep_check_swap(const char* who, const float* a, const float* b, int64_t n) {
    if (!a || !b || n < 1 || n > ((int64_t)1 << 40) || (((uintptr_t)a | (uintptr_t)b) & 3) != 0 || ranges_overlap(a, b, n)) {
        x3dstep_set_error("%s: null, unaligned or overlapping pointers or n %lld outside 1 .. 2^40", who, (long long)n);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// The argument checks of the table forms.  need_state: x3dstep_keep, which reads the state whatever the mode (elsewhere it
// may be null); the others pass X3DSTEP_KEEP_SAVE for mode, and x3dstep_keep and x3dstep_swap_keep 0 for decay.
int x3dstep_check_table(const char* who, const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems,
                        const float* snap, int64_t snap_n, const int64_t* state, bool need_state, int mode, float decay) {
    if (!table || !items || !snap || (need_state && !state) || nbuf < 1 || nbuf > X3DSTEP_MAX_SEGMENTS || nitems < nbuf ||
        nitems > X3DSTEP_MAX_ITEMS || snap_n < 1 || (mode != X3DSTEP_KEEP_SAVE && mode != X3DSTEP_KEEP_RESTORE) ||
        (((uintptr_t)table | (uintptr_t)items | (uintptr_t)state) & 7) != 0 || ((uintptr_t)snap & 3) != 0 ||
        !(decay >= 0.0f && decay < 1.0f)) {
        x3dstep_set_error("%s: null or unaligned pointer, nbuf %d outside 1 .. %d, nitems %lld outside nbuf .. %d, snap_n %lld "
                          "< 1, mode %d or decay %g outside [0, 1)", who, nbuf, X3DSTEP_MAX_SEGMENTS, (long long)nitems,
                          X3DSTEP_MAX_ITEMS, (long long)snap_n, mode, (double)decay);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// k of this call, or 0 with the refusal's text: the twin can read the words the kernel alone can read on the device
static int64_t ema_count_host(const char* who, const int64_t* state, int64_t count) {
    const int64_t k = x3ds::ema_count(state, count);
    if (k <= 0) x3dstep_set_error("%s: the count of applied updates is %lld: nothing to average", who, (long long)k);
    return k <= 0 ? 0 : k;
}

extern "C" int x3dstep_ema_host(float* e, const float* w, int64_t n, const int64_t* state, int64_t count, float decay,
                                int warmup) {
    using namespace x3ds;
    const int rc = x3dstep_check_ema("x3dstep_ema_host", e, w, n, state, decay);
    if (rc) return rc;
    if (ema_count_host("x3dstep_ema_host", state, count) == 0) return X3DSTEP_EINVAL;
    EmaOp op = {state, count, decay, warmup ? 1 : 0, {0.0f, 0.0f}};
    if (op.begin(false)) flat_host(op, Bufs<EmaOp>{{e, (float*)w}}, n);
    return X3DSTEP_OK;
}

extern "C" int x3dstep_ema_keep_host(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* esnap,
                                     int64_t snap_n, const int64_t* state, int64_t count, float decay, int warmup) {
    using namespace x3ds;
    const char* who = "x3dstep_ema_keep_host";
    const int rc = x3dstep_check_table(who, table, nbuf, items, nitems, esnap, snap_n, state, false, X3DSTEP_KEEP_SAVE, decay);
    if (rc) return rc;
    const int rt = table_host_ok(who, table, nbuf, items, nitems, esnap, snap_n);
    if (rt) return rt;
    if (ema_count_host(who, state, count) == 0) return X3DSTEP_EINVAL;
    EmaOp op = {state, count, decay, warmup ? 1 : 0, {0.0f, 0.0f}};
    if (op.begin(false)) items_host(op, table, nbuf, items, nitems, esnap, snap_n);
    return X3DSTEP_OK;
}

extern "C" int x3dstep_swap_host(float* a, float* b, int64_t n) {
    using namespace x3ds;
    const int rc = x3dstep_check_swap("x3dstep_swap_host", a, b, n);
    if (rc) return rc;
    flat_host(SwapOp{}, Bufs<SwapOp>{{(uint32_t*)a, (uint32_t*)b}}, n);
    return X3DSTEP_OK;
}

extern "C" int x3dstep_swap_keep_host(const X3DStepKeep* table, int nbuf, const X3DStepItem* items, int64_t nitems, float* snap,
                                      int64_t snap_n) {
    using namespace x3ds;
    const char* who = "x3dstep_swap_keep_host";
    const int rc = x3dstep_check_table(who, table, nbuf, items, nitems, snap, snap_n, nullptr, false, X3DSTEP_KEEP_SAVE, 0.0f);
    if (rc) return rc;
    const int rt = table_host_ok(who, table, nbuf, items, nitems, snap, snap_n);
    if (rt) return rt;
    items_host(SwapOp{}, table, nbuf, items, nitems, snap, snap_n);
    return X3DSTEP_OK;
}

// -- precise BN statistics ----------------------------------------------------------------------------------------------------
extern "C" size_t x3dstep_pbn_layer_bytes(void) { return sizeof(X3DStepPbnLayer); }

extern "C" int64_t x3dstep_pbn_build_layers(const X3DStepKeep* table, int nbuf, const int32_t* splits, int nlayers,
                                            X3DStepPbnLayer* layers) {
    if (!table || !splits || !layers || nlayers < 1 || nlayers > X3DSTEP_MAX_SEGMENTS / 2 || nbuf != 2 * nlayers) {
        x3dstep_set_error("x3dstep_pbn_build_layers: null table, nlayers %d outside 1 .. %d or nbuf %d != 2 * nlayers", nlayers,
                          X3DSTEP_MAX_SEGMENTS / 2, nbuf);
        return X3DSTEP_EINVAL;
    }
    int64_t first = 0;
    for (int l = 0; l < nlayers; ++l) {
        const X3DStepKeep m = table[2 * l], v = table[2 * l + 1];
        const int32_t S = splits[l];
        if (S < 1 || m.len < 1 || m.len != v.len || m.len % S != 0 || first > X3DSTEP_PBN_MAX_CHANNELS - m.len / S) {
            x3dstep_set_error("x3dstep_pbn_build_layers: layer %d: %d splits, buffers of %d and %d elements, or more than %d "
                              "channels in all", l, S, m.len, v.len, X3DSTEP_PBN_MAX_CHANNELS);
            return X3DSTEP_EINVAL;
        }
        X3DStepPbnLayer L;
        L.mean_addr = m.addr;
        L.var_addr = v.addr;
        L.mean_off = m.offset;
        L.var_off = v.offset;
        L.first = first;
        L.C = m.len / S;
        L.S = S;
        layers[l] = L;
        first += L.C;
    }
    return first;
}

// counts (work == nullptr) or writes the work table; -1 when the layer table is refused
static int64_t walk_work(const X3DStepPbnLayer* layers, int nlayers, X3DStepItem* work, int64_t cap) {
    if (!layers || nlayers < 1 || nlayers > X3DSTEP_MAX_SEGMENTS) return -1;
    int64_t count = 0, first = 0;
    for (int l = 0; l < nlayers; ++l) {
        const X3DStepPbnLayer L = layers[l];
        if (L.C < 1 || L.first != first || first > X3DSTEP_PBN_MAX_CHANNELS - L.C) return -1;
        for (int32_t at = 0; at < L.C; at += X3DSTEP_PBN_RUN) {
            if (work) {
                if (count >= cap) return -1;
                work[count].start = first + at;
                work[count].seg = l;
                work[count].len = L.C - at < X3DSTEP_PBN_RUN ? L.C - at : X3DSTEP_PBN_RUN;
            }
            ++count;
        }
        first += L.C;
    }
    return count;
}

extern "C" int64_t x3dstep_pbn_work_count(const X3DStepPbnLayer* layers, int nlayers) {
    const int64_t c = walk_work(layers, nlayers, nullptr, 0);
    if (c < 0) {
        x3dstep_set_error("x3dstep_pbn_work_count: null table, nlayers %d outside 1 .. %d, a layer with C < 1 or whose first "
                          "channel is not the sum of C before it", nlayers, X3DSTEP_MAX_SEGMENTS);
        return X3DSTEP_EINVAL;
    }
    return c;
}

extern "C" int64_t x3dstep_pbn_build_work(const X3DStepPbnLayer* layers, int nlayers, X3DStepItem* work, int64_t cap) {
    if (!work || cap < 1) {
        x3dstep_set_error("x3dstep_pbn_build_work: null table or no capacity");
        return X3DSTEP_EINVAL;
    }
    const int64_t c = walk_work(layers, nlayers, work, cap);
    if (c < 0) {
        x3dstep_set_error("x3dstep_pbn_build_work: the layer table is refused (see x3dstep_pbn_work_count) or needs more than "
                          "%lld items", (long long)cap);
        return X3DSTEP_EINVAL;
    }
    return c;
}

// the argument checks the launches and their twins share (no pointer is followed: the tables may be device memory);
// finish: snap, snap_n, W and expect_n are checked too
int x3dstep_check_pbn(const char* who, const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                      const double* acc, bool finish, int W, int64_t expect_n, const float* snap, int64_t snap_n) {
    if (!layers || !work || !acc || nlayers < 1 || nlayers > X3DSTEP_MAX_SEGMENTS || nwork < nlayers ||
        nwork > X3DSTEP_MAX_ITEMS || (((uintptr_t)layers | (uintptr_t)work | (uintptr_t)acc) & 7) != 0) {
        x3dstep_set_error("%s: null or unaligned pointer, nlayers %d outside 1 .. %d or nwork %lld outside nlayers .. %d", who,
                          nlayers, X3DSTEP_MAX_SEGMENTS, (long long)nwork, X3DSTEP_MAX_ITEMS);
        return X3DSTEP_EINVAL;
    }
    if (finish && (!snap || ((uintptr_t)snap & 3) != 0 || snap_n < 1 || W < 1 || W > 65536 || expect_n < 1)) {
        x3dstep_set_error("%s: null or unaligned snap, snap_n %lld < 1, W %d outside 1 .. 65536 or expect_n %lld < 1", who,
                          (long long)snap_n, W, (long long)expect_n);
        return X3DSTEP_EINVAL;
    }
    return X3DSTEP_OK;
}

// The tables are host memory in a twin: refuse the call for what the kernel would leave out item by item, and for what
// would make two threads store the same element.
static int pbn_host_ok(const char* who, const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                       int64_t snap_n) {
    using namespace x3ds;
    int64_t first = 0, end = 0;
    for (int l = 0; l < nlayers; ++l) {
        const X3DStepPbnLayer L = layers[l];
        if (L.mean_addr == 0 || L.var_addr == 0 || ((L.mean_addr | L.var_addr) & 3) != 0 || L.C < 1 || L.S < 1) {
            x3dstep_set_error("%s: layer %d: a null or unaligned address, C %d < 1 or S %d < 1", who, l, L.C, L.S);
            return X3DSTEP_EINVAL;
        }
        if (L.first != first || first > X3DSTEP_PBN_MAX_CHANNELS - L.C) {
            x3dstep_set_error("%s: layer %d: its first channel is not the sum of C before it, or more than %d channels", who, l,
                              X3DSTEP_PBN_MAX_CHANNELS);
            return X3DSTEP_EINVAL;
        }
        first += L.C;
        if (snap_n >= 0) {
            const int64_t span = (int64_t)L.S * (int64_t)L.C;
            if (span > snap_n || L.mean_off < end || L.mean_off > snap_n - span || L.var_off < L.mean_off + span ||
                L.var_off > snap_n - span) {
                x3dstep_set_error("%s: layer %d: a range outside snap or over the range before it", who, l);
                return X3DSTEP_EINVAL;
            }
            end = L.var_off + span;
        }
    }
    int64_t next = 0;
    for (int64_t i = 0; i < nwork; ++i) {
        const PbnRun r = pbn_resolve(layers, nlayers, work, i, snap_n);
        if (r.len < 1 || work[i].start < next) {
            x3dstep_set_error("%s: work item %lld lies outside its layer or over the item before it", who, (long long)i);
            return X3DSTEP_EINVAL;
        }
        next = work[i].start + work[i].len;
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_pbn_accum_host(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                                      double* acc) {
    using namespace x3ds;
    const int rc = x3dstep_check_pbn("x3dstep_pbn_accum_host", layers, nlayers, work, nwork, acc, false, 1, 1, nullptr, 0);
    if (rc) return rc;
    const int rt = pbn_host_ok("x3dstep_pbn_accum_host", layers, nlayers, work, nwork, -1);
    if (rt) return rt;
    for (int64_t i = 0; i < nwork; ++i) {
        const PbnRun r = pbn_resolve(layers, nlayers, work, i, -1);
        for (int t = 0; t < r.len; ++t) pbn_accum_one(r, t, acc);
    }
    return X3DSTEP_OK;
}

extern "C" int x3dstep_pbn_finish_host(const X3DStepPbnLayer* layers, int nlayers, const X3DStepItem* work, int64_t nwork,
                                       const double* acc_all, int W, int64_t expect_n, float* snap, int64_t snap_n) {
    using namespace x3ds;
    const int rc = x3dstep_check_pbn("x3dstep_pbn_finish_host", layers, nlayers, work, nwork, acc_all, true, W, expect_n, snap,
                                     snap_n);
    if (rc) return rc;
    const int rt = pbn_host_ok("x3dstep_pbn_finish_host", layers, nlayers, work, nwork, snap_n);
    if (rt) return rt;
    const int64_t total = pbn_channels(layers, nlayers);
    for (int64_t i = 0; i < nwork; ++i) {
        const PbnRun r = pbn_resolve(layers, nlayers, work, i, snap_n);
        for (int t = 0; t < r.len; ++t) pbn_finish_one(r, t, acc_all, W, total, expect_n, snap);
    }
    return X3DSTEP_OK;
}
