// Stand-alone check of the grouped update's host code (csrc_step/step_host.cpp, step_core.h), built by
// tests/test_group_host.py with -fsanitize=address,undefined and run as a child process.
//
//   group_check <file>    file: uint32 cases
//     case: uint32 S, R, steps, shift_w, shift_g, shift_m; int64 seg_off[S + 1]; X3DStepHyper hyper[S]; fp32 w[n], m[n] before
//           the first step; per step fp64 max_norm, fp32 lr, momentum, weight_decay, grad_scale, uint32 first, nesterov,
//           with_state, fp32 g[n], then the expected w[n] and m[n] after (with_state: x3dstep_measure_host and)
//           x3dstep_apply_groups_host; then the expected state
//
// Every table, the scratch, the ring, w, g, m are heap blocks of exactly the size the library is told (a buffer starts
// `shift` elements into a 16-byte aligned block of n + shift), so a read or write outside one stops the run.  Everything is
// compared byte for byte with what the file expects.
//
// After the file's cases: the kernel's own walk (x3ds::group_resolve and x3ds::group_lane of step_core.h, item by item and
// lane by lane, as the launch runs them) over a table with one bad item of each kind -- exactly the elements of that item
// keep their bytes, and every other element is what x3ds::sgd_one gives with its tensor's scales.
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

static long file_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[6];
    rd(f, hdr, sizeof(hdr));
    const int S = (int)hdr[0], R = (int)hdr[1], steps = (int)hdr[2];
    int64_t* seg_off = block<int64_t>((size_t)S + 1);
    rd(f, seg_off, 8 * ((size_t)S + 1));
    X3DStepHyper* hyper = block<X3DStepHyper>((size_t)S);
    rd(f, hyper, sizeof(X3DStepHyper) * (size_t)S);
    const int64_t n = seg_off[S];
    const int64_t nitems = x3dstep_item_count(seg_off, S);
    if (nitems < 1) exit(3);
    X3DStepItem* items = block<X3DStepItem>((size_t)nitems);
    int32_t* seg_item = block<int32_t>((size_t)S + 1);
    if (x3dstep_build_items(seg_off, S, items, nitems, seg_item) != nitems) exit(3);
    const size_t rb = x3dstep_record_bytes(S), wb = x3dstep_workspace_bytes(nitems);
    uint8_t* ws = block<uint8_t>(wb);
    uint8_t* ring = block<uint8_t>(rb * (size_t)R);
    int64_t* state = block<int64_t>(X3DSTEP_STATE_WORDS);
    state[X3DSTEP_S_BAD_STEP] = state[X3DSTEP_S_BAD_SEG] = -1;
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
    // nothing measured yet: refused with a state, and nothing is written
    memcpy(want, w, 4 * (size_t)n);
    if (x3dstep_apply_groups_host(w, g, m, n, items, nitems, hyper, S, state, ring, R, 0.1f, 0.9f, 0.f, 1.f, 0, 0) !=
            X3DSTEP_EINVAL ||
        memcmp(want, w, 4 * (size_t)n) != 0) {
        printf("case %u: an update before any measure was not refused\n", c);
        ++failures;
    }
    for (int s = 0; s < steps; ++s) {
        double max_norm;
        float par[4];
        uint32_t flags[3];
        rd(f, &max_norm, 8);
        rd(f, par, sizeof(par));
        rd(f, flags, sizeof(flags));
        rd(f, g, 4 * (size_t)n);
        memcpy(want, g, 4 * (size_t)n);
        int rc = X3DSTEP_OK;
        if (flags[2]) rc = x3dstep_measure_host(g, n, seg_off, S, items, seg_item, nitems, ws, state, ring, R, max_norm, 1.0);
        if (rc == X3DSTEP_OK)
            rc = x3dstep_apply_groups_host(w, g, m, n, items, nitems, hyper, S, flags[2] ? state : nullptr,
                                           flags[2] ? ring : nullptr, flags[2] ? R : 0, par[0], par[1], par[2], par[3],
                                           (int)flags[0], (int)flags[1]);
        if (rc != X3DSTEP_OK || memcmp(want, g, 4 * (size_t)n) != 0) {
            printf("case %u step %d: call %d (%s), or g was written\n", c, s, rc, x3dstep_last_error());
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
        printf("case %u: state differs (skip %lld skipped %lld run %lld)\n", c, (long long)state[X3DSTEP_S_SKIP],
               (long long)state[X3DSTEP_S_SKIPPED], (long long)state[X3DSTEP_S_RUN]);
        ++failures;
    }
    // refused calls write nothing
    memcpy(want, w, 4 * (size_t)n);
    const float bad_scale = hyper[S - 1].lr_scale;
    int refused = 0;
    refused += x3dstep_apply_groups_host(w, g, m, 0, items, nitems, hyper, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f, 0, 0) ==
               X3DSTEP_EINVAL;
    refused += x3dstep_apply_groups_host(nullptr, g, m, n, items, nitems, hyper, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f, 0,
                                         0) == X3DSTEP_EINVAL;
    refused += x3dstep_apply_groups_host(w, g, m, n, items, nitems - 1, hyper, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f, 0,
                                         0) == X3DSTEP_EINVAL;      /* every case has several items: [0, n) is not covered */
    refused += x3dstep_apply_groups_host(w, g, m, n, items, nitems, hyper, S, nullptr, nullptr, 0, 0.1f, 0.f, 0.f, 1.f, 0, 1) ==
               X3DSTEP_EINVAL;
    refused += x3dstep_apply_groups_host(w, g, w + (n - 1), n, items, nitems, hyper, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f,
                                         0, 0) == X3DSTEP_EINVAL;
    hyper[S - 1].lr_scale = -1.0f;
    refused += x3dstep_apply_groups_host(w, g, m, n, items, nitems, hyper, S, nullptr, nullptr, 0, 0.1f, 0.9f, 0.f, 1.f, 0, 0) ==
               X3DSTEP_EINVAL;
    hyper[S - 1].lr_scale = bad_scale;
    if (refused != 6 || memcmp(want, w, 4 * (size_t)n) != 0 || memcmp(state, want_state, sizeof(want_state)) != 0) {
        printf("case %u: a bad call was not refused (%d of 6), or wrote\n", c, refused);
        ++failures;
    }
    free(want);
    for (int k = 0; k < 3; ++k) free(blocks[k]);
    free(state);
    free(ring);
    free(ws);
    free(seg_item);
    free(items);
    free(hyper);
    free(seg_off);
    return failures;
}

// -- the per-item tests on the kernel's own walk ------------------------------------------------------------------------------
static const int kLengths[] = {1, 2, 3, 24, 63, 64, 65, 2047, 2048, 2049, 4097, 5921};      // tests/step_ref.py
static const float kLrScales[] = {1.0f, 0.0f, 0.5f, 10.0f, 0.1f};                           // tests/group_cases.py
static const float kWdScales[] = {1.0f, 0.0f, 2.0f};

static long item_case(int kind, int shift) {
    using namespace x3ds;
    const int S = (int)(sizeof(kLengths) / sizeof(kLengths[0]));
    int64_t* seg_off = block<int64_t>((size_t)S + 1);
    for (int s = 0; s < S; ++s) seg_off[s + 1] = seg_off[s] + kLengths[s];
    const int64_t n = seg_off[S];
    const int64_t nitems = x3dstep_item_count(seg_off, S);
    X3DStepItem* items = block<X3DStepItem>((size_t)nitems);
    int32_t* seg_item = block<int32_t>((size_t)S + 1);
    if (x3dstep_build_items(seg_off, S, items, nitems, seg_item) != nitems) exit(3);
    X3DStepHyper* hyper = block<X3DStepHyper>((size_t)S);
    for (int s = 0; s < S; ++s) {
        hyper[s].lr_scale = kLrScales[s % 5];
        hyper[s].wd_scale = kWdScales[s % 3];
    }
    // which elements must keep their bytes
    std::vector<char> frozen((size_t)n, 0);
    const int64_t k = nitems - 2;
    const X3DStepItem good = items[k];
    const int bad_seg = 9;
    if (kind < 6) {
        for (int j = 0; j < good.len; ++j) frozen[(size_t)(good.start + j)] = 1;
        if (kind == 0) items[k].seg = -1;
        if (kind == 1) items[k].seg = S;
        if (kind == 2) items[k].len = 0;
        if (kind == 3) items[k].len = X3DSTEP_ITEM + 1;
        if (kind == 4) items[k].start = -4;
        if (kind == 5) items[k].start = n - good.len + 1;
    } else {
        for (int64_t j = seg_off[bad_seg]; j < seg_off[bad_seg + 1]; ++j) frozen[(size_t)j] = 1;
        if (kind == 6) hyper[bad_seg].lr_scale = -1.0f;
        if (kind == 7) hyper[bad_seg].lr_scale = NAN;
        if (kind == 8) hyper[bad_seg].wd_scale = INFINITY;
        if (kind == 9) hyper[bad_seg].wd_scale = -0.5f;
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
        z = z * 1664525u + 1013904223u;
        w[i] = w0[(size_t)i] = (float)((int)(z >> 8) % 2001 - 1000) / 512.0f;
        z = z * 1664525u + 1013904223u;
        g[i] = (float)((int)(z >> 8) % 2001 - 1000) / 1024.0f;
        z = z * 1664525u + 1013904223u;
        m[i] = m0[(size_t)i] = (float)((int)(z >> 8) % 2001 - 1000) / 4096.0f;
    }
    const SgdArgs a = {0.05f, 0.9f, 5e-5f, 0.5f, 0, 1};
    // the twin refuses the table ...
    long failures = 0;
    if (x3dstep_apply_groups_host(w, g, m, n, items, nitems, hyper, S, nullptr, nullptr, 0, a.lr, a.mu, a.wd, a.gs, 0, 1) !=
            X3DSTEP_EINVAL ||
        memcmp(w, w0.data(), 4 * (size_t)n) != 0 || memcmp(m, m0.data(), 4 * (size_t)n) != 0) {
        printf("item kind %d: the twin did not refuse the table, or wrote\n", kind);
        ++failures;
    }
    // ... and the launch's walk leaves exactly the bad item out
    for (int64_t i = 0; i < nitems; ++i) {
        const GroupItem c = group_resolve(items, i, hyper, S, n, a);
        if (c.len > 0)
            for (int l = 0; l < kLanes; ++l) group_lane(w, g, m, c, l, 1.0f, a);
    }
    long wrong = 0, moved = 0;
    for (int s = 0; s < S; ++s) {
        const float lr_s = a.lr * kLrScales[s % 5], wd_s = a.wd * kWdScales[s % 3];
        for (int64_t i = seg_off[s]; i < seg_off[s + 1]; ++i) {
            float we = w0[(size_t)i], me = m0[(size_t)i];
            if (!frozen[(size_t)i]) sgd_one(we, g[i], me, 1.0f, a, lr_s, wd_s);
            wrong += memcmp(&we, &w[i], 4) != 0 || memcmp(&me, &m[i], 4) != 0;
            moved += memcmp(&m0[(size_t)i], &m[i], 4) != 0;
        }
    }
    if (wrong || moved == 0) {
        printf("item kind %d shift %d: %ld elements differ from the per-element rule (%ld moved)\n", kind, shift, wrong, moved);
        ++failures;
    }
    for (int b = 0; b < 3; ++b) free(blocks[b]);
    free(hyper);
    free(seg_item);
    free(items);
    free(seg_off);
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
    int kinds = 0;
    for (int kind = 0; kind < 10; ++kind, ++kinds) failures += item_case(kind, kind % 4);
    printf("groups %u items %d failures %ld\n", count, kinds, failures);
    return failures ? 1 : 0;
}
