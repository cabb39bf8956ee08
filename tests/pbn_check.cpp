// Stand-alone check of the precise-BN host code (csrc_step/step_host.cpp, step_core.h), built by tests/test_pbn_host.py
// with -fsanitize=address,undefined and run as a child process.
//
//   pbn_check <file>    file: uint32 cases
//     case: uint32 nlayers, rot, W; int32 miscount; int32 (C, S)[nlayers]; int32 batches[W]; then for every rank and every
//           one of its batches the contents of the live buffers (means, variances of layer 0, of layer 1, ..); fp32 the
//           snapshot's fill; int64 expect_n; fp64 the expected accumulators [W][4 * T]; fp32 the expected snapshot
//
// Every table, accumulator array and live buffer is a heap block of exactly the size the library is told (a buffer starts
// `shift` elements into a 16-byte aligned block of len + shift), so a read or write outside one stops the run.  Everything
// is compared byte for byte with what the file expects.
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

static long pbn_case(FILE* f, uint32_t c) {
    long failures = 0;
    uint32_t hdr[3];
    int32_t miscount;
    rd(f, hdr, sizeof(hdr));
    rd(f, &miscount, 4);
    const int nlayers = (int)hdr[0], W = (int)hdr[2];
    const uint32_t rot = hdr[1];
    const int nbuf = 2 * nlayers;
    std::vector<int32_t> shape(2 * (size_t)nlayers), batches((size_t)W);
    rd(f, shape.data(), 8 * (size_t)nlayers);
    rd(f, batches.data(), 4 * (size_t)W);
    X3DStepKeep* table = block<X3DStepKeep>((size_t)nbuf);
    int32_t* splits = block<int32_t>((size_t)nlayers);
    std::vector<float*> blocks((size_t)nbuf), live((size_t)nbuf);
    int64_t snap_n = 0;
    for (int b = 0; b < nbuf; ++b) {
        const int32_t len = shape[2 * (b / 2)] * shape[2 * (b / 2) + 1];
        const size_t shift = ((size_t)b + rot) % 4;
        blocks[b] = block<float>((size_t)len + shift);
        live[b] = blocks[b] + shift;
        table[b].addr = (int64_t)(uintptr_t)live[b];
        table[b].offset = snap_n;
        table[b].len = len;
        snap_n += (len + 3) / 4 * 4;
        splits[b / 2] = shape[2 * (b / 2) + 1];
    }
    X3DStepPbnLayer* layers = block<X3DStepPbnLayer>((size_t)nlayers);
    const int64_t T = x3dstep_pbn_build_layers(table, nbuf, splits, nlayers, layers);
    const int64_t nwork = x3dstep_pbn_work_count(layers, nlayers);
    if (T < 1 || nwork < 1) exit(3);
    X3DStepItem* work = block<X3DStepItem>((size_t)nwork);
    if (x3dstep_pbn_build_work(layers, nlayers, work, nwork) != nwork) exit(3);
    double* acc_all = block<double>((size_t)W * 4 * (size_t)T);
    for (int r = 0; r < W; ++r) {
        double* acc = block<double>(4 * (size_t)T);          // a rank's own block: exactly 4 * T doubles
        for (int k = 0; k < batches[r]; ++k) {
            for (int b = 0; b < nbuf; ++b) rd(f, live[b], 4 * (size_t)table[b].len);
            const int rc = x3dstep_pbn_accum_host(layers, nlayers, work, nwork, acc);
            if (rc != X3DSTEP_OK) {
                printf("case %u: accum %d (%s)\n", c, rc, x3dstep_last_error());
                ++failures;
            }
        }
        memcpy(acc_all + (size_t)r * 4 * (size_t)T, acc, 32 * (size_t)T);
        free(acc);
    }
    float fill;
    int64_t expect_n;
    rd(f, &fill, 4);
    rd(f, &expect_n, 8);
    double* want_acc = block<double>((size_t)W * 4 * (size_t)T);
    rd(f, want_acc, (size_t)W * 32 * (size_t)T);
    if (memcmp(want_acc, acc_all, (size_t)W * 32 * (size_t)T) != 0) {
        printf("case %u: other accumulators than expected\n", c);
        ++failures;
    }
    float* snap = block<float>((size_t)snap_n);
    float* want = block<float>((size_t)snap_n);
    for (int64_t i = 0; i < snap_n; ++i) snap[i] = fill;
    rd(f, want, 4 * (size_t)snap_n);
    // refusals first: nothing is written
    if (x3dstep_pbn_finish_host(layers, nlayers, work, nwork, acc_all, 0, expect_n, snap, snap_n) != X3DSTEP_EINVAL ||
        x3dstep_pbn_finish_host(layers, nlayers, work, nwork, acc_all, W, expect_n, snap, snap_n - 4) != X3DSTEP_EINVAL ||
        x3dstep_pbn_accum_host(layers, nlayers, work, nwork, nullptr) != X3DSTEP_EINVAL) {
        printf("case %u: a bad call was not refused\n", c);
        ++failures;
    }
    for (int64_t i = 0; i < snap_n; ++i)
        if (snap[i] != fill) {
            printf("case %u: a refused call wrote\n", c);
            ++failures;
            break;
        }
    const int rc = x3dstep_pbn_finish_host(layers, nlayers, work, nwork, acc_all, W, expect_n, snap, snap_n);
    if (rc != X3DSTEP_OK || memcmp(want, snap, 4 * (size_t)snap_n) != 0) {
        printf("case %u: finish %d (%s), or another snapshot than expected\n", c, rc, x3dstep_last_error());
        ++failures;
    }
    if (miscount != 0) {                                     // every statistic a NaN, the padding untouched
        for (int b = 0; b < nbuf; ++b)
            for (int32_t i = 0; i < table[b].len; ++i)
                if (snap[table[b].offset + i] == snap[table[b].offset + i]) ++failures;
    }
    for (int b = 0; b < nbuf; ++b) free(blocks[b]);
    free(table);
    free(splits);
    free(layers);
    free(work);
    free(acc_all);
    free(want_acc);
    free(snap);
    free(want);
    return failures;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: pbn_check <cases file>\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t count;
    rd(f, &count, 4);
    long failures = 0;
    for (uint32_t c = 0; c < count; ++c) failures += pbn_case(f, c);
    fclose(f);
    printf("pbn %u failures %ld\n", count, failures);
    return failures ? 1 : 0;
}
