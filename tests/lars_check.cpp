// Stand-alone check of the trust ratios' host code (csrc_step/step_host.cpp, step_core.h), built by
// tests/test_lars_host.py with -fsanitize=address,undefined and run as a child process.
//
//   lars_check <file>    file: uint32 cases
//     case: uint32 S, R, steps, shift_w, shift_g, shift_m; int64 seg_off[S + 1]; X3DStepHyper hyper[S]; fp32 eta[S]; fp32
//           w[n], m[n] before the first step; per step fp64 max_norm, fp32 lr, momentum, weight_decay, grad_scale, eps,
//           uint32 first, nesterov, with_state, clip, fp32 g[n], then the expected fp64 wsumsq[S], fp32 trust[S], w[n] and
//           m[n] after x3dstep_measure_host, x3dstep_trust_host and x3dstep_apply_lars_host (with_state: with the state);
//           then the expected state
//
// Every table, the scratch, the ring, w, g, m and the outputs are heap blocks of exactly the size the library is told (a
// buffer starts `shift` elements into a 16-byte aligned block of n + shift), so a read or write outside one stops the run.
// Everything is compared byte for byte with what the file expects.
//
// After the file's cases: the kernels' own code (x3ds::lars_resolve and x3ds::group_lane<true>, x3ds::trust_item_ok,
// x3ds::trust_lane and x3ds::trust_tensor of step_core.h, item by item, lane by lane and tensor by tensor, as the launches
// run them) over tables with one bad item, one bad trust or one bad tensor of each kind -- exactly that item's elements,
// or that tensor's outputs, keep their bytes.
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

static long file_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[6];
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
    float* eta = block<float>((size_t)S);
    rd(f, eta, 4 * (size_t)S);
    uint8_t* ws = block<uint8_t>(x3dstep_workspace_bytes(nitems));
    uint8_t* tws = block<uint8_t>(x3dstep_trust_workspace_bytes(nitems));
    uint8_t* ring = block<uint8_t>(x3dstep_record_bytes(S) * (size_t)R);
    int64_t* state = block<int64_t>(X3DSTEP_STATE_WORDS);
    state[X3DSTEP_S_BAD_STEP] = state[X3DSTEP_S_BAD_SEG] = -1;
    double* wsumsq = block<double>((size_t)S);
    float* trust = block<float>((size_t)S);
    double* want_ss = block<double>((size_t)S);
    float* want_tr = block<float>((size_t)S);
    float* blocks[3];
    float* v[3];  // w, g, m
    for (int k = 0; k < 3; ++k) {
        blocks[k] = block<float>((size_t)n + hdr[3 + k]);
        v[k] = blocks[k] + hdr[3 + k];
    }
    float *w = v[0], *g = v[1], *m = v[2];
    float* want = block<float>((size_t)n);
    rd(f, w, 4 * (size_t)n);
    rd(f, m, 4 * (size_t)n);
    // nothing measured yet: both refused, and nothing is written
    memcpy(want, w, 4 * (size_t)n);
    if (x3dstep_trust_host(w, n, t.items, t.seg_item, nitems, hyper, eta, S, state, ring, R, tws, wsumsq, trust, 0.1f, 0.f, 1.f,
                           0.f, 0) != X3DSTEP_EINVAL ||
        x3dstep_apply_lars_host(w, g, m, n, t.items, nitems, hyper, trust, S, state, ring, R, 0.1f, 0.9f, 0.f, 1.f, 0, 0) !=
            X3DSTEP_EINVAL ||
        memcmp(want, w, 4 * (size_t)n) != 0 || wsumsq[0] != 0.0 || trust[0] != 0.0f) {
        printf("case %u: a call before any measure was not refused\n", c);
        ++failures;
    }
    for (int s = 0; s < steps; ++s) {
        double max_norm;
        float par[5];
        uint32_t flags[4];
        rd(f, &max_norm, 8);
        rd(f, par, sizeof(par));
        rd(f, flags, sizeof(flags));
        rd(f, g, 4 * (size_t)n);
        memcpy(want, g, 4 * (size_t)n);
        int rc = x3dstep_measure_host(g, n, t.seg_off, S, t.items, t.seg_item, nitems, ws, state, ring, R, max_norm, 1.0);
        if (rc == X3DSTEP_OK)
            rc = x3dstep_trust_host(w, n, t.items, t.seg_item, nitems, hyper, eta, S, state, ring, R, tws, wsumsq, trust, par[0],
                                    par[2], par[3], par[4], (int)flags[3]);
        if (rc == X3DSTEP_OK)
            rc = x3dstep_apply_lars_host(w, g, m, n, t.items, nitems, hyper, trust, S, flags[2] ? state : nullptr,
                                         flags[2] ? ring : nullptr, flags[2] ? R : 0, par[0], par[1], par[2], par[3],
                                         (int)flags[0], (int)flags[1]);
        if (rc != X3DSTEP_OK || memcmp(want, g, 4 * (size_t)n) != 0) {
            printf("case %u step %d: call %d (%s), or g was written\n", c, s, rc, x3dstep_last_error());
            ++failures;
        }
        rd(f, want_ss, 8 * (size_t)S);
        rd(f, want_tr, 4 * (size_t)S);
        if (memcmp(want_ss, wsumsq, 8 * (size_t)S) != 0 || memcmp(want_tr, trust, 4 * (size_t)S) != 0) {
            printf("case %u step %d: other sums of squares or trust ratios than expected\n", c, s);
            ++failures;
        }
        rd(f, want, 4 * (size_t)n);
        if (memcmp(want, w, 4 * (size_t)n) != 0) {
            printf("case %u step %d: another w than expected\n", c, s);
            ++failures;
        }
        rd(f, want, 4 * (size_t)n);
        if (memcmp(want, m, 4 * (size_t)n) != 0) {
            printf("case %u step %d: another m than expected\n", c, s);
            ++failures;
        }
    }
    int64_t want_state[X3DSTEP_STATE_WORDS];
    rd(f, want_state, sizeof(want_state));
    if (memcmp(state, want_state, sizeof(want_state)) != 0) {
        printf("case %u: state differs\n", c);
        ++failures;
    }
    // refused calls write nothing
    memcpy(want, w, 4 * (size_t)n);
    memcpy(want_tr, trust, 4 * (size_t)S);
    int refused = 0;
    refused += x3dstep_trust_host(w, n, t.items, t.seg_item, nitems, hyper, eta, S, state, ring, R, tws, wsumsq, trust, 0.1f, 0.f,
                                  1.f, -1.f, 0) == X3DSTEP_EINVAL;
    refused += x3dstep_trust_host(w, n, t.items, t.seg_item, nitems, hyper, eta, S, state, ring, R, tws, wsumsq, trust, 0.1f, 0.f,
                                  1.f, 0.f, 2) == X3DSTEP_EINVAL;
    refused += x3dstep_trust_host(w, n, t.items, t.seg_item, nitems - 1, hyper, eta, S, state, ring, R, tws, wsumsq, trust, 0.1f,
                                  0.f, 1.f, 0.f, 0) == X3DSTEP_EINVAL;
    const float e0 = eta[S - 1];
    eta[S - 1] = -e0 - 1.0f;
    refused += x3dstep_trust_host(w, n, t.items, t.seg_item, nitems, hyper, eta, S, state, ring, R, tws, wsumsq, trust, 0.1f, 0.f,
                                  1.f, 0.f, 0) == X3DSTEP_EINVAL;
    eta[S - 1] = e0;
    refused += x3dstep_apply_lars_host(w, g, m, n, t.items, nitems, hyper, nullptr, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f,
                                       0, 0) == X3DSTEP_EINVAL;
    trust[0] = NAN;
    refused += x3dstep_apply_lars_host(w, g, m, n, t.items, nitems, hyper, trust, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f, 0,
                                       0) == X3DSTEP_EINVAL;
    trust[0] = want_tr[0];
    if (refused != 6 || memcmp(want, w, 4 * (size_t)n) != 0 || memcmp(want_tr, trust, 4 * (size_t)S) != 0 ||
        memcmp(state, want_state, sizeof(want_state)) != 0) {
        printf("case %u: a bad call was not refused (%d of 6), or wrote\n", c, refused);
        ++failures;
    }
    free(want);
    for (int k = 0; k < 3; ++k) free(blocks[k]);
    free(want_tr);
    free(want_ss);
    free(trust);
    free(wsumsq);
    free(state);
    free(ring);
    free(tws);
    free(ws);
    free(eta);
    free(hyper);
    t.release();
    return failures;
}

// -- the per-item and per-tensor tests on the kernels' own code ---------------------------------------------------------------
static const int kLengths[] = {1, 2, 3, 24, 63, 64, 65, 2047, 2048, 2049, 4097, 5921};      // tests/step_ref.py
static const float kLrScales[] = {1.0f, 0.0f, 0.5f, 10.0f, 0.1f};                           // tests/group_cases.py
static const float kWdScales[] = {1.0f, 0.0f, 2.0f};
static const float kEtas[] = {0.001f, 0.0f, 0.02f, 1.0f, 0.5f, 0.25f, 0.125f};              // tests/lars_cases.py
static const int kBadSeg = 9;

static Tables synthetic(X3DStepHyper** hyper, float** eta) {
    Tables t;
    t.S = (int)(sizeof(kLengths) / sizeof(kLengths[0]));
    t.seg_off = block<int64_t>((size_t)t.S + 1);
    for (int s = 0; s < t.S; ++s) t.seg_off[s + 1] = t.seg_off[s] + kLengths[s];
    t.build();
    *hyper = block<X3DStepHyper>((size_t)t.S);
    *eta = block<float>((size_t)t.S);
    for (int s = 0; s < t.S; ++s) {
        (*hyper)[s].lr_scale = kLrScales[s % 5];
        (*hyper)[s].wd_scale = kWdScales[s % 3];
        (*eta)[s] = kEtas[s % 7];
    }
    return t;
}

static float lcg(uint32_t& z, float div) {
    z = z * 1664525u + 1013904223u;
    return (float)((int)(z >> 8) % 2001 - 1000) / div;
}

// kinds 0 .. 9: the bad items of tests/group_check.cpp; 10 .. 12: the trust of tensor kBadSeg negative, NaN, infinite
static long item_case(int kind, int shift) {
    using namespace x3ds;
    X3DStepHyper* hyper;
    float* eta;
    Tables t = synthetic(&hyper, &eta);
    const int S = t.S;
    const int64_t n = t.n, nitems = t.nitems;
    float* trust = block<float>((size_t)S);
    for (int s = 0; s < S; ++s) trust[s] = s % 4 == 1 ? 1.0f : 0.25f + 0.125f * (float)s;
    std::vector<char> frozen((size_t)n, 0);
    const int64_t k = nitems - 2;
    const X3DStepItem good = t.items[k];
    if (kind < 6) {
        for (int j = 0; j < good.len; ++j) frozen[(size_t)(good.start + j)] = 1;
        if (kind == 0) t.items[k].seg = -1;
        if (kind == 1) t.items[k].seg = S;
        if (kind == 2) t.items[k].len = 0;
        if (kind == 3) t.items[k].len = X3DSTEP_ITEM + 1;
        if (kind == 4) t.items[k].start = -4;
        if (kind == 5) t.items[k].start = n - good.len + 1;
    } else {
        for (int64_t j = t.seg_off[kBadSeg]; j < t.seg_off[kBadSeg + 1]; ++j) frozen[(size_t)j] = 1;
        if (kind == 6) hyper[kBadSeg].lr_scale = -1.0f;
        if (kind == 7) hyper[kBadSeg].lr_scale = NAN;
        if (kind == 8) hyper[kBadSeg].wd_scale = INFINITY;
        if (kind == 9) hyper[kBadSeg].wd_scale = -0.5f;
        if (kind == 10) trust[kBadSeg] = -0.5f;
        if (kind == 11) trust[kBadSeg] = NAN;
        if (kind == 12) trust[kBadSeg] = INFINITY;
    }
    float* blocks[3];
    float* v[3];
    for (int b = 0; b < 3; ++b) {
        blocks[b] = block<float>((size_t)n + shift);
        v[b] = blocks[b] + shift;
    }
    float *w = v[0], *g = v[1], *m = v[2];
    std::vector<float> w0((size_t)n), m0((size_t)n);
    uint32_t z = 12345u + (uint32_t)kind;
    for (int64_t i = 0; i < n; ++i) {
        w[i] = w0[(size_t)i] = lcg(z, 512.0f);
        g[i] = lcg(z, 1024.0f);
        m[i] = m0[(size_t)i] = lcg(z, 4096.0f);
    }
    const SgdArgs a = {0.05f, 0.9f, 5e-5f, 0.5f, 0, 1};
    long failures = 0;
    // the twin refuses the table ...
    if (x3dstep_apply_lars_host(w, g, m, n, t.items, nitems, hyper, trust, S, nullptr, nullptr, 0, a.lr, a.mu, a.wd, a.gs, 0, 1) !=
            X3DSTEP_EINVAL ||
        memcmp(w, w0.data(), 4 * (size_t)n) != 0 || memcmp(m, m0.data(), 4 * (size_t)n) != 0) {
        printf("item kind %d: the twin did not refuse the table, or wrote\n", kind);
        ++failures;
    }
    // ... and the launch's walk leaves exactly the bad item out
    for (int64_t i = 0; i < nitems; ++i) {
        float ratio = 1.0f;
        const GroupItem c = lars_resolve(t.items, i, hyper, trust, S, n, a, &ratio);
        if (c.len > 0)
            for (int l = 0; l < kLanes; ++l) group_lane<true>(w, g, m, c, l, 1.0f, a, ratio);
    }
    long wrong = 0, moved = 0;
    for (int s = 0; s < S; ++s) {
        const float lr_s = a.lr * kLrScales[s % 5], wd_s = a.wd * kWdScales[s % 3];
        for (int64_t i = t.seg_off[s]; i < t.seg_off[s + 1]; ++i) {
            float we = w0[(size_t)i], me = m0[(size_t)i];
            if (!frozen[(size_t)i]) sgd_one<false, true>(we, g[i], me, 1.0f, a, lr_s, wd_s, trust[s]);
            wrong += memcmp(&we, &w[i], 4) != 0 || memcmp(&me, &m[i], 4) != 0;
            moved += memcmp(&m0[(size_t)i], &m[i], 4) != 0;
        }
    }
    if (wrong || moved == 0) {
        printf("item kind %d shift %d: %ld elements differ from the per-element rule (%ld moved)\n", kind, shift, wrong, moved);
        ++failures;
    }
    // launch 1 of x3dstep_trust on the same table: a bad item's partial is a NaN, every other is the lanes' sum
    if (kind < 6) {
        for (int64_t i = 0; i < nitems; ++i) {
            double lanes[kLanes];
            const bool ok = trust_item_ok(t.items[i], S, n);
            for (int l = 0; l < kLanes; ++l) lanes[l] = ok ? trust_lane(w, t.items[i], l, shift == 0) : trust_nan();
            for (int off = kLanes / 2; off > 0; off >>= 1)
                for (int l = 0; l < off; ++l) lanes[l] = lanes[l] + lanes[l + off];
            if ((i == k) != (lanes[0] != lanes[0])) {
                printf("item kind %d: the partial of item %lld is %g\n", kind, (long long)i, lanes[0]);
                ++failures;
            }
        }
    }
    for (int b = 0; b < 3; ++b) free(blocks[b]);
    free(trust);
    free(eta);
    free(hyper);
    t.release();
    return failures;
}

// launch 2 of x3dstep_trust, tensor by tensor, over the partials of a clean launch 1; `kind` spoils one tensor
static void trust_walk(const Tables& t, const int32_t* seg_item, const X3DStepHyper* hyper, const float* eta, const double* part,
                       const x3ds::Record& rec, double* wsumsq, float* trust) {
    using namespace x3ds;
    const TrustArgs a = {0.05f, 5e-5f, 0.5f, 1e-8f, 0};
    const SumsqSource src = {part, part, 0};
    for (int s = 0; s < t.S; ++s) trust_tensor(src, s, seg_item, t.nitems, hyper, eta, rec, 1.0f, a, wsumsq, trust);
}

static long tensor_case(int kind) {
    using namespace x3ds;
    X3DStepHyper* hyper;
    float* eta;
    Tables t = synthetic(&hyper, &eta);
    const int S = t.S;
    const int64_t n = t.n, nitems = t.nitems;
    float* w = block<float>((size_t)n);
    float* g = block<float>((size_t)n);
    uint32_t z = 777u + (uint32_t)kind;
    for (int64_t i = 0; i < n; ++i) {
        w[i] = lcg(z, 512.0f);
        g[i] = lcg(z, 1024.0f);
    }
    uint8_t* ws = block<uint8_t>(x3dstep_workspace_bytes(nitems));
    uint8_t* ring = block<uint8_t>(x3dstep_record_bytes(S));
    int64_t* state = block<int64_t>(X3DSTEP_STATE_WORDS);
    state[X3DSTEP_S_BAD_STEP] = state[X3DSTEP_S_BAD_SEG] = -1;
    if (x3dstep_measure_host(g, n, t.seg_off, S, t.items, t.seg_item, nitems, ws, state, ring, 1, 0.0, 1.0) != X3DSTEP_OK) exit(3);
    const Record rec = record_at(ring, 1, S, 0);
    double* part = block<double>((size_t)nitems);
    for (int64_t i = 0; i < nitems; ++i) {
        double lanes[kLanes];
        for (int l = 0; l < kLanes; ++l) lanes[l] = trust_lane(w, t.items[i], l, true);
        for (int off = kLanes / 2; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) lanes[l] = lanes[l] + lanes[l + off];
        part[i] = lanes[0];
    }
    double* clean_ss = block<double>((size_t)S);
    float* clean_tr = block<float>((size_t)S);
    trust_walk(t, t.seg_item, hyper, eta, part, rec, clean_ss, clean_tr);
    int32_t* seg_item = block<int32_t>((size_t)S + 1);
    memcpy(seg_item, t.seg_item, 4 * ((size_t)S + 1));
    int bad = kBadSeg, other = -1;
    if (kind == 0) eta[bad] = -0.001f;
    if (kind == 1) eta[bad] = NAN;
    if (kind == 2) eta[bad] = INFINITY;
    if (kind == 3) hyper[bad].lr_scale = NAN;
    if (kind == 4) hyper[bad].wd_scale = -0.5f;
    if (kind == 5) {
        seg_item[bad + 1] = seg_item[bad];      // no items; the next tensor takes them over and is not compared
        other = bad + 1;
    }
    if (kind == 6) {
        bad = S - 1;
        seg_item[S] = (int32_t)nitems + 1;
    }
    double* wsumsq = block<double>((size_t)S);
    float* trust = block<float>((size_t)S);
    for (int s = 0; s < S; ++s) {
        wsumsq[s] = -3.0;
        trust[s] = -3.0f;
    }
    long failures = 0;
    double* tws = block<double>((size_t)nitems);
    if (x3dstep_trust_host(w, n, t.items, seg_item, nitems, hyper, eta, S, state, ring, 1, tws, wsumsq, trust, 0.05f, 5e-5f, 0.5f,
                           1e-8f, 0) != X3DSTEP_EINVAL ||
        wsumsq[0] != -3.0 || trust[0] != -3.0f) {
        printf("tensor kind %d: the twin did not refuse the tables, or wrote\n", kind);
        ++failures;
    }
    trust_walk(t, seg_item, hyper, eta, part, rec, wsumsq, trust);
    for (int s = 0; s < S; ++s) {
        if (s == other) continue;
        const bool kept = wsumsq[s] == -3.0 && trust[s] == -3.0f;
        const bool same = memcmp(&wsumsq[s], &clean_ss[s], 8) == 0 && memcmp(&trust[s], &clean_tr[s], 4) == 0;
        if (s == bad ? !kept : !same) {
            printf("tensor kind %d: tensor %d has wsumsq %g trust %g\n", kind, s, wsumsq[s], (double)trust[s]);
            ++failures;
        }
    }
    free(tws);
    free(trust);
    free(wsumsq);
    free(seg_item);
    free(clean_tr);
    free(clean_ss);
    free(part);
    free(state);
    free(ring);
    free(ws);
    free(g);
    free(w);
    free(eta);
    free(hyper);
    t.release();
    return failures;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    rd(f, &count, sizeof(count));
    long failures = 0;
    for (uint32_t c = 0; c < count; ++c) failures += file_case(f, c);
    fclose(f);
    int kinds = 0, tensors = 0;
    for (int kind = 0; kind < 13; ++kind, ++kinds) failures += item_case(kind, kind % 4);
    for (int kind = 0; kind < 7; ++kind, ++tensors) failures += tensor_case(kind);
    printf("lars %u items %d tensors %d failures %ld\n", count, kinds, tensors, failures);
    return failures ? 1 : 0;
}
