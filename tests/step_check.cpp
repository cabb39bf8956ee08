// Stand-alone check of the step library's host code (csrc_step/step_host.cpp, step_core.h), built by
// tests/test_step_host.py with -fsanitize=address,undefined and run as a child process.
//
//   step_check <file>     file: uint32 cases; per case uint32 S, R, steps, misalign, int64 seg_off[S + 1]; per step fp64
//                         max_norm, fp64 inv_world, fp32 g[n], fp32 expected g[n] after the call; then the expected state
//                         (int64 [X3DSTEP_STATE_WORDS]) and the expected ring (R records)
//
// Every table, the scratch, the ring and g are heap blocks of exactly the size the library is told (g starts `misalign`
// elements into a 16-byte aligned block of n + misalign), so a read or write outside one stops the run.  Per case the
// item table is built here, every step goes through x3dstep_observe_host, and the gradient after each step, the final
// state and the final ring are compared byte for byte with what the file expects.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t cases = 0;
    rd(f, &cases, 4);
    long steps_run = 0, failures = 0;
    for (uint32_t c = 0; c < cases; ++c) {
        uint32_t hdr[4];
        rd(f, hdr, sizeof(hdr));
        const int S = (int)hdr[0], R = (int)hdr[1], steps = (int)hdr[2], mis = (int)hdr[3];
        int64_t* seg_off = block<int64_t>((size_t)S + 1);
        rd(f, seg_off, 8 * ((size_t)S + 1));
        const int64_t n = seg_off[S];
        const int64_t nitems = x3dstep_item_count(seg_off, S);
        if (nitems < 1) return 3;
        X3DStepItem* items = block<X3DStepItem>((size_t)nitems);
        int32_t* seg_item = block<int32_t>((size_t)S + 1);
        if (x3dstep_build_items(seg_off, S, items, nitems, seg_item) != nitems) return 3;
        if (x3dstep_build_items(seg_off, S, items, nitems - 1, seg_item) != X3DSTEP_EINVAL && nitems > 1) return 3;
        if (x3dstep_build_items(seg_off, S, items, nitems, seg_item) != nitems) return 3;
        const size_t rb = x3dstep_record_bytes(S), wb = x3dstep_workspace_bytes(nitems);
        if (rb != (sizeof(X3DStepHeader) + 20 * (size_t)S + 7) / 8 * 8 || wb < 20 * (size_t)nitems) return 3;
        uint8_t* ws = block<uint8_t>(wb);
        uint8_t* ring = block<uint8_t>(rb * (size_t)R);
        int64_t* state = block<int64_t>(X3DSTEP_STATE_WORDS);
        state[X3DSTEP_S_BAD_STEP] = state[X3DSTEP_S_BAD_SEG] = -1;
        float* gblock = block<float>((size_t)n + mis);
        float* g = gblock + mis;
        float* want = block<float>((size_t)n);
        for (int s = 0; s < steps; ++s) {
            double par[2];
            rd(f, par, sizeof(par));
            rd(f, g, 4 * (size_t)n);
            rd(f, want, 4 * (size_t)n);
            const int rc = x3dstep_observe_host(g, n, seg_off, S, items, seg_item, nitems, ws, state, ring, R, par[0], par[1]);
            ++steps_run;
            if (rc != X3DSTEP_OK || memcmp(g, want, 4 * (size_t)n) != 0) {
                printf("case %u step %d: call %d (%s), or another gradient than expected\n", c, s, rc, x3dstep_last_error());
                ++failures;
            }
        }
        int64_t* want_state = block<int64_t>(X3DSTEP_STATE_WORDS);
        uint8_t* want_ring = block<uint8_t>(rb * (size_t)R);
        rd(f, want_state, 8 * X3DSTEP_STATE_WORDS);
        rd(f, want_ring, rb * (size_t)R);
        if (memcmp(state, want_state, 8 * X3DSTEP_STATE_WORDS) != 0) {
            printf("case %u: state differs (step %lld, bad %lld / %lld)\n", c, (long long)state[0], (long long)state[1],
                   (long long)state[2]);
            ++failures;
        }
        if (memcmp(ring, want_ring, rb * (size_t)R) != 0) {
            printf("case %u: ring differs\n", c);
            ++failures;
        }
        // a refused call writes nothing
        if (x3dstep_observe_host(g, n, seg_off, S, items, seg_item, nitems, ws, state, ring, 0, 0.0, 1.0) != X3DSTEP_EINVAL ||
            x3dstep_observe_host(g, n + 1, seg_off, S, items, seg_item, nitems, ws, state, ring, R, 0.0, 1.0) != X3DSTEP_EINVAL ||
            memcmp(state, want_state, 8 * X3DSTEP_STATE_WORDS) != 0) {
            printf("case %u: a bad call was not refused\n", c);
            ++failures;
        }
        free(want_ring);
        free(want_state);
        free(want);
        free(gblock);
        free(state);
        free(ring);
        free(ws);
        free(seg_item);
        free(items);
        free(seg_off);
    }
    fclose(f);
    printf("cases %u steps %ld failures %ld\n", cases, steps_run, failures);
    return failures ? 1 : 0;
}
