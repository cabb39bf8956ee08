// Stand-alone check of the guarded update's host code (csrc_step/step_host.cpp, step_core.h), built by
// tests/test_guard_host.py with -fsanitize=address,undefined and run as a child process.
//
//   guard_check <file>    file: uint32 apply cases, uint32 keep cases
//     apply case: uint32 S, R, steps, shift_w, shift_g, shift_m; int64 seg_off[S + 1]; fp32 w[n], m[n] before the first step;
//                 per step fp64 max_norm, inv_world, fp32 lr, momentum, weight_decay, grad_scale, uint32 first, fp32 g[n],
//                 then the expected w[n] and m[n] after x3dstep_measure_host + x3dstep_apply_host; then the expected state
//     keep case:  uint32 nbuf, stagger, skip word; int32 len[nbuf]; the live buffers; the expected snapshot after a save
//                 (every buffer starts on a multiple of four elements); new contents of the live buffers; what they hold
//                 after a restore with that skip word
//
// Every table, the scratch, the ring, w, g, m and every live buffer are heap blocks of exactly the size the library is told
// (a buffer starts `shift` elements into a 16-byte aligned block of n + shift), so a read or write outside one stops the
// run.  Everything is compared byte for byte with what the file expects.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "x3dstep.h"

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

struct StepPar {
    double max_norm, inv_world;
    float lr, mu, wd, gs;
    uint32_t first;
};

static long apply_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[6];
    rd(f, hdr, sizeof(hdr));
    const int S = (int)hdr[0], R = (int)hdr[1], steps = (int)hdr[2];
    int64_t* seg_off = block<int64_t>((size_t)S + 1);
    rd(f, seg_off, 8 * ((size_t)S + 1));
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
    // nothing measured yet: refused, and nothing is written
    memcpy(want, w, 4 * (size_t)n);
    if (x3dstep_apply_host(w, g, m, n, state, ring, R, S, 0.1f, 0.9f, 0.f, 1.f, 0) != X3DSTEP_EINVAL ||
        memcmp(want, w, 4 * (size_t)n) != 0) {
        printf("apply case %u: an apply before any measure was not refused\n", c);
        ++failures;
    }
    for (int s = 0; s < steps; ++s) {
        StepPar p;
        rd(f, &p.max_norm, 8);
        rd(f, &p.inv_world, 8);
        rd(f, &p.lr, 16);
        rd(f, &p.first, 4);
        rd(f, g, 4 * (size_t)n);
        memcpy(want, g, 4 * (size_t)n);
        int rc = x3dstep_measure_host(g, n, seg_off, S, items, seg_item, nitems, ws, state, ring, R, p.max_norm, p.inv_world);
        if (rc == X3DSTEP_OK)
            rc = x3dstep_apply_host(w, g, m, n, state, ring, R, S, p.lr, p.mu, p.wd, p.gs, (int)p.first);
        if (rc != X3DSTEP_OK || memcmp(want, g, 4 * (size_t)n) != 0) {
            printf("apply case %u step %d: call %d (%s), or g was written\n", c, s, rc, x3dstep_last_error());
            ++failures;
        }
        rd(f, want, 4 * (size_t)n);
        if (memcmp(want, w, 4 * (size_t)n) != 0) {
            printf("apply case %u step %d: another w than expected\n", c, s);
            ++failures;
        }
        rd(f, want, 4 * (size_t)n);
        if (memcmp(want, m, 4 * (size_t)n) != 0) {
            printf("apply case %u step %d: another m than expected\n", c, s);
            ++failures;
        }
    }
    int64_t want_state[X3DSTEP_STATE_WORDS];
    rd(f, want_state, sizeof(want_state));
    if (memcmp(state, want_state, sizeof(want_state)) != 0) {
        printf("apply case %u: state differs (skip %lld skipped %lld run %lld)\n", c, (long long)state[X3DSTEP_S_SKIP],
               (long long)state[X3DSTEP_S_SKIPPED], (long long)state[X3DSTEP_S_RUN]);
        ++failures;
    }
    // refused calls write nothing
    if (x3dstep_apply_host(w, g, m, 0, state, ring, R, S, 0.1f, 0.9f, 0.f, 1.f, 0) != X3DSTEP_EINVAL ||
        x3dstep_apply_host(w, g, m, n, state, ring, 0, S, 0.1f, 0.9f, 0.f, 1.f, 0) != X3DSTEP_EINVAL ||
        x3dstep_apply_host(w, g, m, n, state, ring, R, 0, 0.1f, 0.9f, 0.f, 1.f, 0) != X3DSTEP_EINVAL ||
        x3dstep_apply_host(nullptr, g, m, n, state, ring, R, S, 0.1f, 0.9f, 0.f, 1.f, 0) != X3DSTEP_EINVAL ||
        memcmp(state, want_state, sizeof(want_state)) != 0) {
        printf("apply case %u: a bad call was not refused\n", c);
        ++failures;
    }
    free(want);
    for (int k = 0; k < 3; ++k) free(blocks[k]);
    free(state);
    free(ring);
    free(ws);
    free(seg_item);
    free(items);
    free(seg_off);
    return failures;
}

static long keep_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[3];
    rd(f, hdr, sizeof(hdr));
    const int nbuf = (int)hdr[0];
    const bool stagger = hdr[1] != 0;
    std::vector<int32_t> len((size_t)nbuf);
    rd(f, len.data(), 4 * (size_t)nbuf);
    std::vector<float*> blocks((size_t)nbuf), live((size_t)nbuf);
    X3DStepKeep* table = block<X3DStepKeep>((size_t)nbuf);
    int64_t* seg_off = block<int64_t>((size_t)nbuf + 1);
    for (int b = 0; b < nbuf; ++b) {
        const int shift = stagger ? b % 4 : 0;
        blocks[b] = block<float>((size_t)len[b] + shift);
        live[b] = blocks[b] + shift;
        rd(f, live[b], 4 * (size_t)len[b]);
        seg_off[b + 1] = seg_off[b] + (len[b] + 3) / 4 * 4;
        table[b].addr = (int64_t)(uintptr_t)live[b];
        table[b].offset = seg_off[b];
        table[b].len = len[b];
        table[b].pad = 0;
    }
    const int64_t snap_n = seg_off[nbuf];
    const int64_t nitems = x3dstep_item_count(seg_off, nbuf);
    if (nitems < 1) exit(3);
    X3DStepItem* items = block<X3DStepItem>((size_t)nitems);
    int32_t* seg_item = block<int32_t>((size_t)nbuf + 1);
    if (x3dstep_build_items(seg_off, nbuf, items, nitems, seg_item) != nitems) exit(3);
    float* snap = block<float>((size_t)snap_n);
    float* want = block<float>((size_t)snap_n);
    int64_t* state = block<int64_t>(X3DSTEP_STATE_WORDS);
    int rc = x3dstep_keep_host(table, nbuf, items, nitems, snap, snap_n, state, X3DSTEP_KEEP_SAVE);
    rd(f, want, 4 * (size_t)snap_n);
    if (rc != X3DSTEP_OK || memcmp(want, snap, 4 * (size_t)snap_n) != 0) {
        printf("keep case %u: save %d (%s), or another snapshot than expected\n", c, rc, x3dstep_last_error());
        ++failures;
    }
    for (int b = 0; b < nbuf; ++b) rd(f, live[b], 4 * (size_t)len[b]);
    state[X3DSTEP_S_SKIP] = (int64_t)hdr[2];
    rc = x3dstep_keep_host(table, nbuf, items, nitems, snap, snap_n, state, X3DSTEP_KEEP_RESTORE);
    if (rc != X3DSTEP_OK) {
        printf("keep case %u: restore %d (%s)\n", c, rc, x3dstep_last_error());
        ++failures;
    }
    for (int b = 0; b < nbuf; ++b) {
        rd(f, want, 4 * (size_t)len[b]);
        if (memcmp(want, live[b], 4 * (size_t)len[b]) != 0) {
            printf("keep case %u: buffer %d differs after the restore\n", c, b);
            ++failures;
        }
    }
    // refused: a null address, an unaligned one, a range outside snap; a snapshot one element short
    X3DStepKeep saved = table[nbuf - 1];
    table[nbuf - 1].addr = 0;
    if (x3dstep_keep_host(table, nbuf, items, nitems, snap, snap_n, state, X3DSTEP_KEEP_SAVE) != X3DSTEP_EINVAL) ++failures;
    table[nbuf - 1].addr = saved.addr + 2;
    if (x3dstep_keep_host(table, nbuf, items, nitems, snap, snap_n, state, X3DSTEP_KEEP_SAVE) != X3DSTEP_EINVAL) ++failures;
    table[nbuf - 1] = saved;
    table[nbuf - 1].offset = snap_n;
    if (x3dstep_keep_host(table, nbuf, items, nitems, snap, snap_n, state, X3DSTEP_KEEP_SAVE) != X3DSTEP_EINVAL) ++failures;
    table[nbuf - 1] = saved;
    if (x3dstep_keep_host(table, nbuf, items, nitems, snap, snap_n - 1, state, X3DSTEP_KEEP_SAVE) != X3DSTEP_EINVAL) ++failures;
    free(state);
    free(want);
    free(snap);
    free(seg_item);
    free(items);
    free(seg_off);
    free(table);
    for (int b = 0; b < nbuf; ++b) free(blocks[b]);
    return failures;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t counts[2] = {0, 0};
    rd(f, counts, sizeof(counts));
    long failures = 0;
    for (uint32_t c = 0; c < counts[0]; ++c) failures += apply_case(f, c);
    for (uint32_t c = 0; c < counts[1]; ++c) failures += keep_case(f, c);
    fclose(f);
    printf("apply %u keep %u failures %ld\n", counts[0], counts[1], failures);
    return failures ? 1 : 0;
}
