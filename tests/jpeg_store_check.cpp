// Stand-alone check of the frame store's job builder on the host (csrc_jpeg/store_host.cpp, store_core.h, with host.cpp
// and scan.cpp), built by tests/test_jpeg_store_host.py with -fsanitize=address,undefined and run as a child process.
//
//   jpeg_store_check <file>     file: uint32 count, then per frame uint32 length and the bytes of a JPEG file; uint32 lists,
//                               then per list int32 n, sub_bits, coef_short, ws_short, expected build status and n pairs
//                               (int32 id, int32 extra width of the destination)
//
// The store is built here: per frame one heap block for the prepared scan and one for its segment table, each of exactly
// the size written; every table and every output of x3djpeg_store_build_jobs_host is a heap block of exactly the size the
// library is told, so a read or write outside one stops the run.  coef_short / ws_short name the request whose
// coefficients / workspace the capacity is one element short of (-1: the capacity is the total).  Per list: the build
// status is the expected one; a request the plan flags has both jobs zero, byte for byte; the scan jobs of the others,
// run through x3djpeg_entropy_decode_parallel_host, give the coefficients of x3djpeg_entropy_decode.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "x3djpeg.h"

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
        scans[i] = block<uint8_t>(scan_bytes + X3DJPEG_SCAN_PAD);
        memcpy(scans[i], tmp, scan_bytes + X3DJPEG_SCAN_PAD);
        free(tmp);
        free(data);
        recs[i].scan = scans[i];
        recs[i].segs = segs[i];
        recs[i].scan_bytes = (int32_t)scan_bytes;
        recs[i].nseg = (int32_t)nseg;
        recs[i].header = (int32_t)i;
        recs[i].pad = 0;
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

    const uint32_t lists = rd32(f);
    long served = 0, refused = 0, failures = 0;
    for (uint32_t l = 0; l < lists; ++l) {
        const int n = (int)rd32(f), sub_bits = (int)rd32(f), coef_short = (int)rd32(f), ws_short = (int)rd32(f);
        const int expect = (int)rd32(f);
        int32_t* ids = block<int32_t>(n);
        X3DJpegStoreDst* dsts = block<X3DJpegStoreDst>(n);
        int64_t coef_total = 0, ws_total = 0, coef_cap = -1, ws_cap = -1;
        for (int i = 0; i < n; ++i) {
            ids[i] = (int32_t)rd32(f);
            const int extra = (int)rd32(f);
            const bool ok = ids[i] >= 0 && (uint32_t)ids[i] < count;
            dsts[i].dst = (uint8_t*)(uintptr_t)(0x1000 + 4096 * (size_t)i);  // an address only: the builder never follows it
            dsts[i].width = (ok ? infos[ids[i]].width : 8) + extra;
            dsts[i].height = ok ? infos[ids[i]].height : 8;
            dsts[i].dst_stride = 3 * (int64_t)dsts[i].width;
            const int64_t cc = ok ? infos[ids[i]].coef_count : 0;
            const int64_t ws = ok ? (int64_t)x3djpeg_entropy_workspace_bytes(recs[ids[i]].scan_bytes, recs[ids[i]].nseg, sub_bits) : 0;
            if (i == coef_short) coef_cap = coef_total + cc - 1;
            if (i == ws_short) ws_cap = ws_total + ws - 1;
            coef_total += cc;
            ws_total += ws;
        }
        if (coef_cap < 0) coef_cap = coef_total;
        if (ws_cap < 0) ws_cap = ws_total;
        int16_t* coef = block<int16_t>((size_t)coef_cap);
        uint8_t* planes = block<uint8_t>((size_t)coef_cap);
        uint8_t* ws = block<uint8_t>((size_t)ws_cap);
        int64_t* plan = block<int64_t>(3 * (size_t)n + 2);
        if (x3djpeg_store_plan_bytes(n) != sizeof(int64_t) * (3 * (size_t)n + 2)) ++failures;
        X3DJpegScanJob* sj = block<X3DJpegScanJob>(n);
        X3DJpegFrameJob* fj = block<X3DJpegFrameJob>(n);
        int32_t* status = block<int32_t>(1);
        memset(coef, 0x5A, (size_t)coef_cap * 2);
        const int rc = x3djpeg_store_build_jobs_host(recs, (int)count, headers, (int)count, ids, n, sub_bits, coef,
                                                     (size_t)coef_cap, planes, (size_t)coef_cap, (size_t)ws_cap, dsts, plan, sj,
                                                     fj, status);
        if (rc != X3DJPEG_OK || *status != expect || plan[3 * n] != coef_total || plan[3 * n + 1] != ws_total) {
            printf("list %u: call %d, status %d (expected %d), totals %lld %lld\n", l, rc, rc ? -1 : *status, expect,
                   (long long)plan[3 * n], (long long)plan[3 * n + 1]);
            ++failures;
        } else {
            int32_t* st = block<int32_t>(n);
            if (x3djpeg_entropy_decode_parallel_host(sj, n, sub_bits, ws, (size_t)ws_cap, st, nullptr) != X3DJPEG_OK) ++failures;
            static const uint8_t zeros[sizeof(X3DJpegScanJob)] = {0};
            for (int i = 0; i < n; ++i) {
                bool good;
                if (plan[2 * n + i]) {
                    ++refused;
                    good = memcmp(sj + i, zeros, sizeof(X3DJpegScanJob)) == 0 && memcmp(fj + i, zeros, sizeof(X3DJpegFrameJob)) == 0 &&
                           st[i] == X3DJPEG_EINVAL;
                } else {
                    ++served;
                    const X3DJpegInfo& I = infos[ids[i]];
                    good = st[i] == 0 && sj[i].coef == coef + plan[i] && fj[i].coef == sj[i].coef && fj[i].planes == planes + plan[i] &&
                           fj[i].dst == dsts[i].dst && fj[i].width == I.width && fj[i].nblocks == I.nblocks &&
                           memcmp(sj[i].coef, want[ids[i]], (size_t)I.coef_count * 2) == 0;
                }
                if (!good) {
                    printf("list %u request %d (id %d): flags %lld, status %d\n", l, i, ids[i], (long long)plan[2 * n + i], st[i]);
                    ++failures;
                }
            }
            free(st);
        }
        free(status);
        free(fj);
        free(sj);
        free(plan);
        free(ws);
        free(planes);
        free(coef);
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
    printf("frames %u lists %u served %ld refused %ld failures %ld\n", count, lists, served, refused, failures);
    return failures ? 1 : 0;
}
