// Stand-alone check of the stage step of the frame store's host tier on the host (csrc_jpeg/stage_host.cpp, stage_core.h,
// with store_host.cpp, host.cpp and scan.cpp), built by tests/test_jpeg_tier_host.py with -fsanitize=address,undefined and
// run as a child process.
//
//   jpeg_tier_check <file>     file: uint32 count, then per frame uint32 length and the bytes of a JPEG file; uint32 runs,
//                              then per run int32 n, the request the staging capacity is one byte short of (-1: the
//                              capacity is the total), the expected stage status and n int32 ids
//
// The store is built here: per frame one heap block for the prepared scan and one for its segment table, each of exactly
// the size written; the staging buffer and every table x3djpeg_stage_host writes is a heap block of exactly the size the
// library is told, so a read or write outside one stops the run.  Per run: the status is the expected one; a served
// request's staged bytes are its source's with a zero tail, a refused one has a zero record and id -1; the staged tables,
// taken through x3djpeg_store_build_jobs_host and x3djpeg_entropy_decode_parallel_host, give the coefficients of
// x3djpeg_entropy_decode.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "x3djpeg.h"

static const int kSubBits = 128;

static uint32_t rd32(FILE* f) {
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24);
}

template <class T>
static T* block(size_t count) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, count * sizeof(T) ? count * sizeof(T) : 16)) exit(2);
    return (T*)p;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    std::vector<uint8_t*> scans(count);
    std::vector<X3DJpegScanSeg*> segs(count);
    std::vector<int16_t*> want(count);
    std::vector<X3DJpegInfo> infos(count);
    X3DJpegStoreRec* recs = block<X3DJpegStoreRec>(count);
    X3DJpegStoreHeader* headers = block<X3DJpegStoreHeader>(count);
    memset(headers, 0, count * sizeof(X3DJpegStoreHeader));
    size_t max_frame = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t len = rd32(f);
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(data, 1, len, f) != len) return 2;
        X3DJpegInfo& I = infos[i];
        if (x3djpeg_parse(data, len, &I) != X3DJPEG_OK) return 3;
        want[i] = (int16_t*)malloc((size_t)I.coef_count * 2);
        if (x3djpeg_entropy_decode(data, len, &I, want[i], (size_t)I.coef_count * 2) != X3DJPEG_OK) return 3;
        const size_t nmcu = (size_t)I.mcus_x * I.mcus_y;
        const size_t seg_cap = I.restart_interval ? (nmcu + I.restart_interval - 1) / I.restart_interval : 1;
        const size_t scan_cap = len - (size_t)I.scan_off + X3DJPEG_SCAN_PAD;
        uint8_t* tmp = (uint8_t*)malloc(scan_cap);
        segs[i] = block<X3DJpegScanSeg>(seg_cap);
        size_t scan_bytes = 0, nseg = 0;
        if (x3djpeg_scan_prepare(data, len, &I, tmp, scan_cap, segs[i], seg_cap, &scan_bytes, &nseg) != X3DJPEG_OK) return 3;
        scans[i] = block<uint8_t>(scan_bytes + X3DJPEG_SCAN_PAD);  // not rounded up: the twin reads no byte past the padding
        memcpy(scans[i], tmp, scan_bytes + X3DJPEG_SCAN_PAD);
        free(tmp);
        free(data);
        recs[i].scan = scans[i];
        recs[i].segs = segs[i];
        recs[i].scan_bytes = (int32_t)scan_bytes;
        recs[i].nseg = (int32_t)nseg;
        recs[i].header = (int32_t)i;
        recs[i].pad = 0;
        const size_t b = x3djpeg_stage_bytes((int)scan_bytes, (int)nseg);
        if (b != (scan_bytes + X3DJPEG_SCAN_PAD + 15) / 16 * 16 + 16 * nseg) return 3;
        if (b > max_frame) max_frame = b;
        X3DJpegFrameJob& F = headers[i].frame;
        X3DJpegScanJob& S = headers[i].scan;
        F.width = I.width;
        F.height = I.height;
        F.ncomp = I.ncomp;
        F.hmax = I.hmax;
        F.vmax = I.vmax;
        F.nblocks = I.nblocks;
        S.coef_count = I.coef_count;
        S.ncomp = I.ncomp;
        S.mcus_x = I.mcus_x;
        S.mcus_y = I.mcus_y;
        S.restart_interval = I.restart_interval;
        for (int c = 0; c < 3; ++c) {
            F.blocks_w[c] = I.blocks_w[c];
            F.blocks_h[c] = I.blocks_h[c];
            F.cw[c] = I.cw[c];
            F.ch[c] = I.ch[c];
            F.block_start[c] = I.block_start[c];
            memcpy(F.qt[c], I.qt[I.comp_tq[c]], sizeof(F.qt[c]));
            S.comp_h[c] = I.comp_h[c];
            S.comp_v[c] = I.comp_v[c];
            S.comp_td[c] = I.comp_td[c];
            S.comp_ta[c] = I.comp_ta[c];
            S.blocks_w[c] = I.blocks_w[c];
            S.block_start[c] = I.block_start[c];
        }
        memcpy(S.huff_bits, I.huff_bits, sizeof(S.huff_bits));
        memcpy(S.huff_vals, I.huff_vals, sizeof(S.huff_vals));
    }

    const uint32_t runs = rd32(f);
    long served = 0, refused = 0, failures = 0;
    for (uint32_t l = 0; l < runs; ++l) {
        const int n = (int)rd32(f), cap_short = (int)rd32(f), expect = (int)rd32(f);
        int32_t* ids = block<int32_t>(n);
        X3DJpegStoreDst* dsts = block<X3DJpegStoreDst>(n);
        int64_t total = 0, cap = -1, coef_total = 0, ws_total = 0;
        for (int i = 0; i < n; ++i) {
            ids[i] = (int32_t)rd32(f);
            const bool ok = ids[i] >= 0 && (uint32_t)ids[i] < count;
            const int64_t b = ok ? (int64_t)x3djpeg_stage_bytes(recs[ids[i]].scan_bytes, recs[ids[i]].nseg) : 0;
            if (i == cap_short) cap = total + b - 1;
            total += b;
            dsts[i].dst = (uint8_t*)(uintptr_t)(0x1000 + 4096 * (size_t)i);  // an address only: the builder never follows it
            dsts[i].width = ok ? infos[ids[i]].width : 8;
            dsts[i].height = ok ? infos[ids[i]].height : 8;
            dsts[i].dst_stride = 3 * (int64_t)dsts[i].width;
            coef_total += ok ? infos[ids[i]].coef_count : 0;
            ws_total += ok ? (int64_t)x3djpeg_entropy_workspace_bytes(recs[ids[i]].scan_bytes, recs[ids[i]].nseg, kSubBits) : 0;
        }
        if (cap < 0) cap = total;
        uint8_t* staging = block<uint8_t>((size_t)cap);  // exactly the capacity: a byte past it stops the run
        X3DJpegStoreRec* srecs = block<X3DJpegStoreRec>(n);
        int32_t* sids = block<int32_t>(n);
        int64_t* offsets = block<int64_t>((size_t)n + 1);
        int32_t* status = block<int32_t>(1);
        memset(staging, 0x3C, (size_t)cap);
        const int rc = x3djpeg_stage_host(recs, (int)count, ids, n, max_frame, staging, (size_t)cap, srecs, sids, offsets, status);
        if (rc != X3DJPEG_OK || *status != expect) {
            printf("run %u: call %d, status %d (expected %d)\n", l, rc, rc ? -1 : *status, expect);
            ++failures;
        } else {
            int64_t at = 0;
            static const uint8_t zeros[sizeof(X3DJpegStoreRec)] = {0};
            for (int i = 0; i < n; ++i) {
                bool good = offsets[i] == at;
                if (sids[i] < 0) {
                    ++refused;
                    good = good && sids[i] == -1 && memcmp(srecs + i, zeros, sizeof(zeros)) == 0;
                } else {
                    ++served;
                    const X3DJpegStoreRec& R = recs[ids[i]];
                    const size_t valid = (size_t)R.scan_bytes + X3DJPEG_SCAN_PAD, scan_len = (valid + 15) / 16 * 16;
                    good = good && sids[i] == i && srecs[i].scan == staging + at && (const uint8_t*)srecs[i].segs == staging + at + scan_len &&
                           srecs[i].scan_bytes == R.scan_bytes && srecs[i].nseg == R.nseg && srecs[i].header == R.header &&
                           memcmp(staging + at, R.scan, valid) == 0 && memcmp(staging + at + scan_len, R.segs, 16 * (size_t)R.nseg) == 0;
                    for (size_t k = valid; k < scan_len; ++k) good = good && staging[at + k] == 0;
                    at += (int64_t)x3djpeg_stage_bytes(R.scan_bytes, R.nseg);
                }
                if (!good) {
                    printf("run %u request %d (id %d): staged id %d at %lld\n", l, i, ids[i], sids[i], (long long)offsets[i]);
                    ++failures;
                }
            }
            if (offsets[n] != at) ++failures;
            for (int64_t k = at; k < cap; ++k)
                if (staging[k] != 0x3C) {
                    printf("run %u: byte %lld past the total %lld written\n", l, (long long)k, (long long)at);
                    ++failures;
                    break;
                }
            // the staged tables are a store of n frames: build and decode
            int16_t* coef = block<int16_t>((size_t)coef_total);
            uint8_t* planes = block<uint8_t>((size_t)coef_total);
            uint8_t* ws = block<uint8_t>((size_t)ws_total);
            int64_t* plan = block<int64_t>(3 * (size_t)n + 2);
            X3DJpegScanJob* sj = block<X3DJpegScanJob>(n);
            X3DJpegFrameJob* fj = block<X3DJpegFrameJob>(n);
            int32_t* bst = block<int32_t>(1);
            int32_t* st = block<int32_t>(n);
            if (x3djpeg_store_build_jobs_host(srecs, n, headers, (int)count, sids, n, kSubBits, coef, (size_t)coef_total, planes,
                                              (size_t)coef_total, (size_t)ws_total, dsts, plan, sj, fj, bst) != X3DJPEG_OK ||
                x3djpeg_entropy_decode_parallel_host(sj, n, kSubBits, ws, (size_t)ws_total, st, nullptr) != X3DJPEG_OK) {
                printf("run %u: the builder or the decoder refused the staged tables\n", l);
                ++failures;
            } else {
                for (int i = 0; i < n; ++i) {
                    const bool good = sids[i] < 0 ? (plan[2 * n + i] == X3DJPEG_STORE_BAD_ID && st[i] == X3DJPEG_EINVAL)
                                                  : (plan[2 * n + i] == 0 && st[i] == 0 &&
                                                     memcmp(sj[i].coef, want[ids[i]], (size_t)infos[ids[i]].coef_count * 2) == 0);
                    if (!good) {
                        printf("run %u request %d (id %d): flags %lld, status %d\n", l, i, ids[i], (long long)plan[2 * n + i], st[i]);
                        ++failures;
                    }
                }
            }
            free(st);
            free(bst);
            free(fj);
            free(sj);
            free(plan);
            free(ws);
            free(planes);
            free(coef);
        }
        free(status);
        free(offsets);
        free(sids);
        free(srecs);
        free(staging);
        free(dsts);
        free(ids);
    }
    fclose(f);
    for (uint32_t i = 0; i < count; ++i) {
        free(scans[i]);
        free(segs[i]);
        free(want[i]);
    }
    free(recs);
    free(headers);
    printf("frames %u runs %u served %ld refused %ld failures %ld\n", count, runs, served, refused, failures);
    return failures ? 1 : 0;
}
