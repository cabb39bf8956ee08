// Stand-alone check of the weight average's host code (csrc_step/step_host.cpp, step_core.h), built by
// tests/test_ema_host.py with -fsanitize=address,undefined and run as a child process.
//
//   ema_check <file>    file: uint32 ema cases, uint32 keep cases, uint32 swap cases
//     ema case:  uint32 n, shift_e, shift_w, warmup, has_state; int64 count; int64 state[8]; fp32 decay; fp32 e[n], w[n];
//                the expected e[n] after x3dstep_ema_host
//     keep case: uint32 nbuf, rot, warmup, has_state; int64 count; int64 state[8]; fp32 decay; int32 len[nbuf]; the live
//                buffers; the averaged snapshot before (every buffer starts on a multiple of four elements) and the expected
//                one after x3dstep_ema_keep_host; the program then exchanges live and snapshot twice
//     swap case: uint32 n, shift_a, shift_b; fp32 a[n], b[n]
//
// Every table, e, w and every live buffer are heap blocks of exactly the size the library is told (a buffer starts `shift`
// elements into a 16-byte aligned block of n + shift), so a read or write outside one stops the run.  Everything is
// compared byte for byte with what the file expects.
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

static long ema_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[5];
    int64_t count, state[X3DSTEP_STATE_WORDS];
    float decay;
    rd(f, hdr, sizeof(hdr));
    rd(f, &count, 8);
    rd(f, state, sizeof(state));
    rd(f, &decay, 4);
    const int64_t n = hdr[0];
    float* eb = block<float>((size_t)n + hdr[1]);
    float* wb = block<float>((size_t)n + hdr[2]);
    float *e = eb + hdr[1], *w = wb + hdr[2];
    float* want = block<float>((size_t)n);
    rd(f, e, 4 * (size_t)n);
    rd(f, w, 4 * (size_t)n);
    memcpy(want, w, 4 * (size_t)n);
    const int64_t* st = hdr[4] ? state : nullptr;
    // an update count of zero or less is refused and nothing is written
    const int64_t applied = st ? st[X3DSTEP_S_STEP] - st[X3DSTEP_S_SKIPPED] : 0;
    float* e0 = block<float>((size_t)n);
    memcpy(e0, e, 4 * (size_t)n);
    if (x3dstep_ema_host(e, w, n, st, -applied, decay, (int)hdr[3]) != X3DSTEP_EINVAL || memcmp(e0, e, 4 * (size_t)n) != 0) {
        printf("ema case %u: k = 0 was not refused\n", c);
        ++failures;
    }
    const int rc = x3dstep_ema_host(e, w, n, st, count, decay, (int)hdr[3]);
    if (rc != X3DSTEP_OK || memcmp(want, w, 4 * (size_t)n) != 0) {
        printf("ema case %u: call %d (%s), or w was written\n", c, rc, x3dstep_last_error());
        ++failures;
    }
    rd(f, want, 4 * (size_t)n);
    if (memcmp(want, e, 4 * (size_t)n) != 0) {
        printf("ema case %u: another e than expected\n", c);
        ++failures;
    }
    free(eb);
    free(wb);
    free(want);
    free(e0);
    return failures;
}

static long keep_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[4];
    int64_t count, state[X3DSTEP_STATE_WORDS];
    float decay;
    rd(f, hdr, sizeof(hdr));
    rd(f, &count, 8);
    rd(f, state, sizeof(state));
    rd(f, &decay, 4);
    const int nbuf = (int)hdr[0];
    const uint32_t rot = hdr[1];
    std::vector<int32_t> len((size_t)nbuf);
    rd(f, len.data(), 4 * (size_t)nbuf);
    int64_t* seg_off = block<int64_t>((size_t)nbuf + 1);
    for (int b = 0; b < nbuf; ++b) seg_off[b + 1] = seg_off[b] + (len[b] + 3) / 4 * 4;
    const int64_t snap_n = seg_off[nbuf];
    const int64_t nitems = x3dstep_item_count(seg_off, nbuf);
    if (nitems < 1) exit(3);
    X3DStepItem* items = block<X3DStepItem>((size_t)nitems);
    int32_t* seg_item = block<int32_t>((size_t)nbuf + 1);
    if (x3dstep_build_items(seg_off, nbuf, items, nitems, seg_item) != nitems) exit(3);
    X3DStepKeep* table = block<X3DStepKeep>((size_t)nbuf);
    std::vector<float*> blocks((size_t)nbuf), live((size_t)nbuf), live0((size_t)nbuf);
    for (int b = 0; b < nbuf; ++b) {
        const size_t shift = ((size_t)b + rot) % 4;
        blocks[b] = block<float>((size_t)len[b] + shift);
        live[b] = blocks[b] + shift;
        live0[b] = block<float>((size_t)len[b]);
        rd(f, live[b], 4 * (size_t)len[b]);
        memcpy(live0[b], live[b], 4 * (size_t)len[b]);
        table[b].addr = (int64_t)(uintptr_t)live[b];
        table[b].offset = seg_off[b];
        table[b].len = len[b];
    }
    float* esnap = block<float>((size_t)snap_n);
    float* snap0 = block<float>((size_t)snap_n);
    float* want = block<float>((size_t)snap_n);
    rd(f, esnap, 4 * (size_t)snap_n);
    memcpy(snap0, esnap, 4 * (size_t)snap_n);
    rd(f, want, 4 * (size_t)snap_n);
    const int64_t* st = hdr[3] ? state : nullptr;
    const int rc = x3dstep_ema_keep_host(table, nbuf, items, nitems, esnap, snap_n, st, count, decay, (int)hdr[2]);
    if (rc != X3DSTEP_OK || memcmp(want, esnap, 4 * (size_t)snap_n) != 0) {
        printf("keep case %u: call %d (%s), or another averaged snapshot than expected\n", c, rc, x3dstep_last_error());
        ++failures;
    }
    for (int b = 0; b < nbuf; ++b)
        if (memcmp(live[b], live0[b], 4 * (size_t)len[b]) != 0) {
            printf("keep case %u: live buffer %d was written\n", c, b);
            ++failures;
        }
    // the exchange: the live buffers take the averaged values and back
    if (x3dstep_swap_keep_host(table, nbuf, items, nitems, esnap, snap_n) != X3DSTEP_OK) ++failures;
    for (int b = 0; b < nbuf; ++b)
        if (memcmp(live[b], want + seg_off[b], 4 * (size_t)len[b]) != 0 ||
            memcmp(esnap + seg_off[b], live0[b], 4 * (size_t)len[b]) != 0) {
            printf("keep case %u: buffer %d was not exchanged\n", c, b);
            ++failures;
        }
    if (x3dstep_swap_keep_host(table, nbuf, items, nitems, esnap, snap_n) != X3DSTEP_OK) ++failures;
    if (memcmp(want, esnap, 4 * (size_t)snap_n) != 0) {
        printf("keep case %u: two exchanges are not the identity\n", c);
        ++failures;
    }
    for (int b = 0; b < nbuf; ++b) {
        if (memcmp(live[b], live0[b], 4 * (size_t)len[b]) != 0) ++failures;
        free(blocks[b]);
        free(live0[b]);
    }
    free(seg_off);
    free(items);
    free(seg_item);
    free(table);
    free(esnap);
    free(snap0);
    free(want);
    return failures;
}

static long swap_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[3];
    rd(f, hdr, sizeof(hdr));
    const size_t n = hdr[0];
    float* ab = block<float>(n + hdr[1]);
    float* bb = block<float>(n + hdr[2]);
    float *a = ab + hdr[1], *b = bb + hdr[2];
    float* a0 = block<float>(n);
    float* b0 = block<float>(n);
    rd(f, a0, 4 * n);
    rd(f, b0, 4 * n);
    memcpy(a, a0, 4 * n);
    memcpy(b, b0, 4 * n);
    if (x3dstep_swap_host(a, b, (int64_t)n) != X3DSTEP_OK || memcmp(a, b0, 4 * n) != 0 || memcmp(b, a0, 4 * n) != 0) {
        printf("swap case %u: not exchanged (%s)\n", c, x3dstep_last_error());
        ++failures;
    }
    if (x3dstep_swap_host(a, b, (int64_t)n) != X3DSTEP_OK || memcmp(a, a0, 4 * n) != 0 || memcmp(b, b0, 4 * n) != 0) {
        printf("swap case %u: two exchanges are not the identity\n", c);
        ++failures;
    }
    if (x3dstep_swap_host(a, a, (int64_t)n) != X3DSTEP_EINVAL) ++failures;
    free(ab);
    free(bb);
    free(a0);
    free(b0);
    return failures;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: ema_check <cases file>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t counts[3];
    rd(f, counts, sizeof(counts));
    long failures = 0;
    for (uint32_t c = 0; c < counts[0]; ++c) failures += ema_case(f, c);
    for (uint32_t c = 0; c < counts[1]; ++c) failures += keep_case(f, c);
    for (uint32_t c = 0; c < counts[2]; ++c) failures += swap_case(f, c);
    fclose(f);
    printf("ema %u keep %u swap %u failures %ld\n", counts[0], counts[1], counts[2], failures);
    return failures ? 1 : 0;
}
