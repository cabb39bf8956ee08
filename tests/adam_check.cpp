// Stand-alone check of the second-moment updates' host code (csrc_step/step_host.cpp, step_core.h), built by
// tests/test_adam_host.py with -fsanitize=address,undefined and run as a child process.
//
//   adam_check <file>    file: uint32 cases
//     case: uint32 S, R, steps, shift_w, shift_g, shift_m, shift_v; int64 seg_off[S + 1]; X3DStepHyper hyper[S]; uint8
//           adapt[S]; fp32 w[n], m[n], v[n] before the first step; per step fp64 max_norm, int64 count, fp32 lr, b1, b2, eps,
//           weight_decay, grad_scale, uint32 lamb, decoupled, with_state, fp32 g[n], then the expected fp32 w[n], m[n], v[n],
//           fp64 wsumsq[S], rsumsq[S] and fp32 trust[S] after x3dstep_measure_host (with_state) and x3dstep_adam_host or
//           the three x3dstep_lamb_*_host; then the expected state
//
// Every table, the scratch, the ring, the four buffers and the outputs are heap blocks of exactly the size the library is
// told (a buffer starts `shift` elements into a 16-byte aligned block of n + shift), so a read or write outside one stops
// the run.  Everything is compared byte for byte with what the file expects.
//
// After the file's cases: the kernels' own code (x3ds::group_resolve and x3ds::rule_lane with x3ds::AdamRule of
// step_core.h, item by item and lane by lane, as the launch runs them) over tables with one bad item of each kind --
// exactly that item's elements keep their bytes, every other element takes the bytes of the run over the good table.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../x3d-multigrid_amd/csrc_step/step_core.h"

static void rd(FILE* f, void* dst, size_t bytes) {
    if (bytes && fread(dst, 1, bytes, f) != bytes) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
}

template <class T>
static T* block(size_t count) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, count * sizeof(T) ? count * sizeof(T) : 16)) exit(2);
    memset(p, 0, count * sizeof(T));
    return (T*)p;
}

// the tables of a list of tensor lengths, every block of its exact size
struct Tables {
    int S;
    int64_t n, nitems;
    int64_t* seg_off;
    X3DStepItem* items;
    int32_t* seg_item;
    void build() {
        n = seg_off[S];
        nitems = x3dstep_item_count(seg_off, S);
        if (nitems < 1) exit(3);
        items = block<X3DStepItem>((size_t)nitems);
        seg_item = block<int32_t>((size_t)S + 1);
        if (x3dstep_build_items(seg_off, S, items, nitems, seg_item) != nitems) exit(3);
    }
    void release() {
        free(seg_item);
        free(items);
        free(seg_off);
    }
};

static long differs(const char* what, uint32_t c, int s, const void* got, const void* want, size_t bytes) {
    if (memcmp(got, want, bytes) == 0) return 0;
    printf("case %u step %d: %s differs\n", c, s, what);
    return 1;
}

static long file_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[7];
    rd(f, hdr, sizeof(hdr));
    const int S = (int)hdr[0], R = (int)hdr[1], steps = (int)hdr[2];
    Tables t;
    t.S = S;
    t.seg_off = block<int64_t>((size_t)S + 1);
    rd(f, t.seg_off, 8 * ((size_t)S + 1));
    t.build();
    const int64_t n = t.n, nitems = t.nitems;
    X3DStepHyper* hyper = block<X3DStepHyper>((size_t)S);
    rd(f, hyper, sizeof(X3DStepHyper) * (size_t)S);
    uint8_t* adapt = block<uint8_t>((size_t)S);
    rd(f, adapt, (size_t)S);
    uint8_t* ws = block<uint8_t>(x3dstep_workspace_bytes(nitems));
    uint8_t* lws = block<uint8_t>(x3dstep_lamb_workspace_bytes(nitems));
    uint8_t* ring = block<uint8_t>(x3dstep_record_bytes(S) * (size_t)R);
    int64_t* state = block<int64_t>(X3DSTEP_STATE_WORDS);
    state[X3DSTEP_S_BAD_STEP] = state[X3DSTEP_S_BAD_SEG] = -1;
    double* wsumsq = block<double>((size_t)S);
    double* rsumsq = block<double>((size_t)S);
    float* trust = block<float>((size_t)S);
    for (int s = 0; s < S; ++s) {
        wsumsq[s] = rsumsq[s] = -3.0;
        trust[s] = -3.0f;
    }
    double* want_ss = block<double>((size_t)S);
    float* want_tr = block<float>((size_t)S);
    float* blocks[4];
    float* b[4];  // w, g, m, v
    for (int k = 0; k < 4; ++k) {
        blocks[k] = block<float>((size_t)n + hdr[3 + k]);
        b[k] = blocks[k] + hdr[3 + k];
    }
    float *w = b[0], *g = b[1], *m = b[2], *v = b[3];
    float* want = block<float>((size_t)n);
    rd(f, w, 4 * (size_t)n);
    rd(f, m, 4 * (size_t)n);
    rd(f, v, 4 * (size_t)n);
    // nothing measured yet: every guarded call is refused, and nothing is written
    memcpy(want, w, 4 * (size_t)n);
    if (x3dstep_adam_host(w, g, m, v, n, t.items, nitems, hyper, S, state, ring, R, 1, 0.1f, 0.9f, 0.999f, 1e-8f, 0.f, 1.f, 1) !=
            X3DSTEP_EINVAL ||
        x3dstep_lamb_moments_host(w, g, m, v, n, t.items, nitems, hyper, S, state, ring, R, 1, 0.9f, 0.999f, 1e-6f, 0.f, 1.f,
                                  lws) != X3DSTEP_EINVAL ||
        x3dstep_lamb_trust_host(t.seg_item, nitems, hyper, adapt, S, state, ring, R, 1, lws, wsumsq, rsumsq, trust) !=
            X3DSTEP_EINVAL ||
        x3dstep_lamb_apply_host(w, m, v, n, t.items, nitems, hyper, trust, S, state, ring, R, 1, 0.1f, 0.9f, 0.999f, 1e-6f,
                                0.f) != X3DSTEP_EINVAL ||
        memcmp(want, w, 4 * (size_t)n) != 0 || wsumsq[0] != -3.0 || trust[0] != -3.0f) {
        printf("case %u: a call before any measure was not refused\n", c);
        ++failures;
    }
    for (int s = 0; s < steps; ++s) {
        double max_norm;
        int64_t count;
        float par[6];  // lr, b1, b2, eps, weight_decay, grad_scale
        uint32_t flags[3];  // lamb, decoupled, with_state
        rd(f, &max_norm, 8);
        rd(f, &count, 8);
        rd(f, par, sizeof(par));
        rd(f, flags, sizeof(flags));
        rd(f, g, 4 * (size_t)n);
        int64_t* st = flags[2] ? state : nullptr;
        const void* rg = flags[2] ? ring : nullptr;
        const int RR = flags[2] ? R : 0;
        int rc = X3DSTEP_OK;
        if (flags[2]) rc = x3dstep_measure_host(g, n, t.seg_off, S, t.items, t.seg_item, nitems, ws, state, ring, R, max_norm, 1.0);
        if (rc == X3DSTEP_OK) {
            if (flags[0]) {
                rc = x3dstep_lamb_moments_host(w, g, m, v, n, t.items, nitems, hyper, S, st, rg, RR, count, par[1], par[2], par[3],
                                               par[4], par[5], lws);
                if (rc == X3DSTEP_OK)
                    rc = x3dstep_lamb_trust_host(t.seg_item, nitems, hyper, adapt, S, st, rg, RR, count, lws, wsumsq, rsumsq,
                                                 trust);
                if (rc == X3DSTEP_OK)
                    rc = x3dstep_lamb_apply_host(w, m, v, n, t.items, nitems, hyper, trust, S, st, rg, RR, count, par[0], par[1],
                                                 par[2], par[3], par[4]);
            } else {
                rc = x3dstep_adam_host(w, g, m, v, n, t.items, nitems, hyper, S, st, rg, RR, count, par[0], par[1], par[2], par[3],
                                       par[4], par[5], (int)flags[1]);
            }
        }
        if (rc != X3DSTEP_OK) {
            printf("case %u step %d: error %d: %s\n", c, s, rc, x3dstep_last_error());
            ++failures;
        }
        float* bufs[3] = {w, m, v};
        const char* names[3] = {"w", "m", "v"};
        for (int k = 0; k < 3; ++k) {
            rd(f, want, 4 * (size_t)n);
            failures += differs(names[k], c, s, bufs[k], want, 4 * (size_t)n);
        }
        rd(f, want_ss, 8 * (size_t)S);
        failures += differs("wsumsq", c, s, wsumsq, want_ss, 8 * (size_t)S);
        rd(f, want_ss, 8 * (size_t)S);
        failures += differs("rsumsq", c, s, rsumsq, want_ss, 8 * (size_t)S);
        rd(f, want_tr, 4 * (size_t)S);
        failures += differs("trust", c, s, trust, want_tr, 4 * (size_t)S);
    }
    int64_t want_state[X3DSTEP_STATE_WORDS];
    rd(f, want_state, sizeof(want_state));
    failures += differs("state", c, steps, state, want_state, sizeof(want_state));
    free(want);
    for (int k = 0; k < 4; ++k) free(blocks[k]);
    free(want_tr);
    free(want_ss);
    free(trust);
    free(rsumsq);
    free(wsumsq);
    free(state);
    free(ring);
    free(lws);
    free(ws);
    free(adapt);
    free(hyper);
    t.release();
    return failures;
}

// the launch of x3dstep_adam (no state) as the kernel runs it: per item, per lane
static void run_items(float* w, const float* g, float* m, float* v, const Tables& t, const X3DStepItem* items,
                      const X3DStepHyper* hyper) {
    using namespace x3ds;
    const AdamArgs a = {0.01f, 0.9f, 0.999f, 1e-8f, 0.01f, 0.5f, 1};
    const SgdArgs sa = {a.lr, 0.0f, a.wd, a.gs, 0, 0};
    const AdamCorr corr = adam_corr(3, a.b1, a.b2);
    float* const base[4] = {w, (float*)g, m, v};
    for (int64_t i = 0; i < t.nitems; ++i) {
        const GroupItem c = group_resolve(items, i, hyper, t.S, t.n, sa);
        if (c.len < 1) continue;
        const AdamRule rule = {a, corr, 1.0f, c.wd_s, adam_step_size(c.lr_s, corr), c.lr_s * c.wd_s};
        for (int l = 0; l < kLanes; ++l) rule_lane(rule, base, c.start, c.len, l);
    }
}

static long bad_items(long* count) {
    long failures = 0;
    const int64_t lens[] = {1, 2, 3, 24, 63, 64, 65, 2047, 2048, 2049, 4097, 16384 - 12443};
    Tables t;
    t.S = 12;
    t.seg_off = block<int64_t>(13);
    for (int s = 0; s < 12; ++s) t.seg_off[s + 1] = t.seg_off[s] + lens[s];
    t.build();
    const int64_t n = t.n;
    X3DStepHyper* hyper = block<X3DStepHyper>(12);
    for (int s = 0; s < 12; ++s) {
        hyper[s].lr_scale = 1.0f + 0.25f * (float)(s % 3);
        hyper[s].wd_scale = (float)(s % 2);
    }
    float* w0 = block<float>((size_t)n);
    float* g = block<float>((size_t)n);
    float* m0 = block<float>((size_t)n);
    float* v0 = block<float>((size_t)n);
    uint32_t z = 12345;
    for (int64_t i = 0; i < n; ++i) {
        float x[4];
        for (int k = 0; k < 4; ++k) {
            z = z * 1664525u + 1013904223u;
            x[k] = (float)(int32_t)(z >> 8) / 8388608.0f - 1.0f;
        }
        w0[i] = x[0];
        g[i] = x[1];
        m0[i] = 0.1f * x[2];
        v0[i] = 0.01f * x[3] * x[3];
    }
    float* good[3] = {block<float>((size_t)n), block<float>((size_t)n), block<float>((size_t)n)};
    float* got[3] = {block<float>((size_t)n), block<float>((size_t)n), block<float>((size_t)n)};
    const float* init[3] = {w0, m0, v0};
    for (int k = 0; k < 3; ++k) memcpy(good[k], init[k], 4 * (size_t)n);
    run_items(good[0], g, good[1], good[2], t, t.items, hyper);
    const int64_t k = t.nitems - 2;       // an inner item of the last tensor
    const float nanv = nanf(""), infv = INFINITY;
    for (int kind = 0; kind < 10; ++kind) {
        X3DStepItem* items = block<X3DStepItem>((size_t)t.nitems);
        memcpy(items, t.items, sizeof(X3DStepItem) * (size_t)t.nitems);
        X3DStepHyper* hy = block<X3DStepHyper>(12);
        memcpy(hy, hyper, sizeof(X3DStepHyper) * 12);
        int64_t lo = t.items[k].start, hi = lo + t.items[k].len;      // the elements that must stay
        switch (kind) {
            case 0: items[k].seg = -1; break;
            case 1: items[k].seg = t.S; break;
            case 2: items[k].len = 0; break;
            case 3: items[k].len = X3DSTEP_ITEM + 1; break;
            case 4: items[k].start = -4; break;
            case 5: items[k].start = n - items[k].len + 1; break;
            default: {
                const int s = 9;          // X3DSTEP_ITEM + 1 elements: two items
                if (kind == 6) hy[s].lr_scale = -1.0f;
                if (kind == 7) hy[s].lr_scale = nanv;
                if (kind == 8) hy[s].wd_scale = infv;
                if (kind == 9) hy[s].wd_scale = -0.5f;
                lo = t.seg_off[s];
                hi = t.seg_off[s + 1];
            }
        }
        for (int b = 0; b < 3; ++b) memcpy(got[b], init[b], 4 * (size_t)n);
        run_items(got[0], g, got[1], got[2], t, items, hy);
        bool ok = true;
        for (int b = 0; b < 3; ++b)
            for (int64_t i = 0; i < n; ++i) {
                const float* want = (i >= lo && i < hi) ? init[b] : good[b];
                ok = ok && memcmp(&got[b][i], &want[i], 4) == 0;
            }
        if (!ok) {
            printf("bad item of kind %d: not exactly that item was left untouched\n", kind);
            ++failures;
        }
        ++*count;
        free(hy);
        free(items);
    }
    for (int b = 0; b < 3; ++b) {
        free(got[b]);
        free(good[b]);
    }
    free(v0);
    free(m0);
    free(g);
    free(w0);
    free(hyper);
    t.release();
    return failures;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: adam_check <file>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t cases = 0;
    rd(f, &cases, 4);
    long failures = 0;
    for (uint32_t c = 0; c < cases; ++c) failures += file_case(f, c);
    fclose(f);
    long items = 0;
    failures += bad_items(&items);
    printf("adam %u items %ld %ld\n", cases, items, failures);
    return failures ? 1 : 0;
}
