// The host's part of the sync index of libx3djpeg (include/x3djpeg.h): x3djpeg_index_build, one serial pass per segment of
// a prepared scan, and x3djpeg_entropy_decode_indexed_host, the scheme of entropy_indexed.hip run serially through the
// same index_core.h.  Plain C++, no HIP call, no global state.
#include <stdlib.h>
#include <string.h>

#include "index_core.h"

void x3djpeg_set_error(const char* fmt, ...);  // host.cpp

extern "C" size_t x3djpeg_index_rec_bytes(void) { return sizeof(X3DJpegIndexRec); }

extern "C" size_t x3djpeg_index_count(const X3DJpegScanSeg* segs, size_t nseg, int index_bits) {
    if (!segs || !x3dj::index_bits_ok(index_bits)) return 0;
    size_t n = 0;
    for (size_t s = 0; s < nseg; ++s) n += (size_t)x3dj::seg_nsub(segs[s].byte_len, index_bits);
    return n;
}

extern "C" int x3djpeg_index_build(const uint8_t* scan, size_t scan_bytes, const X3DJpegScanSeg* segs, size_t nseg,
                                   const X3DJpegInfo* info, int index_bits, uint64_t* entries, size_t cap, size_t* n) {
    using namespace x3dj;
    if (n) *n = 0;
    if (!scan || !segs || !info || !entries || !n || !index_bits_ok(index_bits) ||
        scan_bytes > (size_t)X3DJPEG_SCAN_MAX_BYTES || nseg < 1 || nseg > ((size_t)1 << 26)) {
        x3djpeg_set_error("x3djpeg_index_build: null pointer, a scan too large, or index_bits %d not a multiple of 32",
                          index_bits);
        return X3DJPEG_EINVAL;
    }
    X3DJpegScanJob J;
    memset(&J, 0, sizeof J);
    J.scan = scan;
    J.segs = segs;
    J.coef_count = info->coef_count;
    J.scan_bytes = (int32_t)scan_bytes;
    J.nseg = (int32_t)nseg;
    J.ncomp = info->ncomp;
    J.mcus_x = info->mcus_x;
    J.mcus_y = info->mcus_y;
    J.restart_interval = info->restart_interval;
    for (int c = 0; c < 3; ++c) {
        J.comp_h[c] = info->comp_h[c];
        J.comp_v[c] = info->comp_v[c];
        J.comp_td[c] = info->comp_td[c];
        J.comp_ta[c] = info->comp_ta[c];
        J.blocks_w[c] = info->blocks_w[c];
        J.block_start[c] = info->block_start[c];
    }
    memcpy(J.huff_bits, info->huff_bits, sizeof J.huff_bits);
    memcpy(J.huff_vals, info->huff_vals, sizeof J.huff_vals);
    HuffTable* tables = (HuffTable*)malloc(8 * sizeof(HuffTable));
    if (!tables) {
        x3djpeg_set_error("x3djpeg_index_build: out of memory");
        return X3DJPEG_EINVAL;
    }
    FrameCtx C;
    int32_t sum = 0;
    int rc = setup_frame(J, index_bits, tables, &C);
    if (!rc) rc = seg_count(C, 0, 1, &sum);
    if (rc) {
        free(tables);
        x3djpeg_set_error("x3djpeg_index_build: the segment table or the info is not this scan's");
        return X3DJPEG_EINVAL;
    }
    if (build_tables(J, C, tables, 0, 1)) {
        free(tables);
        x3djpeg_set_error("corrupt JPEG: over-subscribed Huffman table");
        return X3DJPEG_ECORRUPT;
    }
    size_t at = 0;
    for (size_t s = 0; s < nseg && !rc; ++s) {
        const int32_t k = seg_nsub(segs[s].byte_len, index_bits);
        if ((int64_t)segs[s].mcu_count * C.bpm >= X3DJPEG_INDEX_MAX_BLOCKS) {
            x3djpeg_set_error("unsupported JPEG: segment %zu of %lld blocks, the sync index takes fewer than %d", s,
                              (long long)segs[s].mcu_count * C.bpm, X3DJPEG_INDEX_MAX_BLOCKS);
            rc = X3DJPEG_EUNSUPPORTED;
        } else if ((size_t)k > cap - at) {
            x3djpeg_set_error("x3djpeg_index_build: more than %zu entries", cap);
            rc = X3DJPEG_EINVAL;
        } else {
            const int e = index_segment(C, (int32_t)s, (uint32_t*)(entries + at), k);
            if (e) {
                x3djpeg_set_error("corrupt JPEG: the scan does not decode (segment %zu)", s);
                rc = e == X3DJPEG_ECORRUPT ? X3DJPEG_ECORRUPT : X3DJPEG_EINVAL;
            }
            at += (size_t)k;
        }
    }
    free(tables);
    if (rc) return rc;
    *n = at;
    return X3DJPEG_OK;
}

namespace {

// One frame through the phases of index_core.h with kWorkers workers taken in turn: what a workgroup does in
// entropy_indexed.hip, a loop where it has a barrier.
constexpr int kWorkers = 7;

int frame_host(const X3DJpegScanJob& J, int32_t id, const X3DJpegIndexRec* recs, int nrecs, const uint32_t* entries,
               int64_t entries_total, int index_bits, x3dj::HuffTable* tables, int32_t* scratch) {
    using namespace x3dj;
    FrameCtx C;
    IndexCtx X;
    const int nt = kWorkers;
    int err = idx_setup(J, id, recs, nrecs, entries, entries_total, index_bits, tables, &C, &X);
    if (err) return err;
    int bad_table = 0, bad_seg = 0, bits = 0;
    for (int t = 0; t < nt; ++t) bad_table |= build_tables(J, C, tables, t, nt);
    for (int t = 0; t < nt; ++t) bad_seg |= seg_count(C, t, nt, scratch);
    if (bad_seg) return X3DJPEG_EINVAL;
    if (bad_table) return X3DJPEG_ECORRUPT;
    err = idx_total(&C, X, nt, scratch);
    if (err) return err;
    for (int t = 0; t < nt; ++t) zero(C, t, nt);
    for (int t = 0; t < nt; ++t) bits |= idx_write(C, X, t, nt, scratch);
    for (int t = 0; t < nt; ++t) dc_sum(C, t, nt, scratch);
    for (int c = 0; c < C.ncomp; ++c) carry_scan(scratch + 2 * c * nt, nt);
    for (int t = 0; t < nt; ++t) dc_place(C, t, nt, scratch);
    return idx_status(bits);
}

}  // namespace

extern "C" int x3djpeg_entropy_decode_indexed_host(const void* jobs, int njobs, const void* ids, const void* index_recs,
                                                   int nrecs, const void* entries, size_t entries_total, int index_bits,
                                                   void* status) {
    if (!jobs || !ids || !index_recs || !entries || !status || njobs < 1 || nrecs < 1 || !x3dj::index_bits_ok(index_bits) ||
        ((uintptr_t)entries & 7) != 0 || ((uintptr_t)index_recs & 7) != 0 || entries_total > ((size_t)1 << 59)) {
        x3djpeg_set_error("x3djpeg_entropy_decode_indexed_host: null pointer, unaligned tables, or index_bits %d not a "
                          "multiple of 32", index_bits);
        return X3DJPEG_EINVAL;
    }
    x3dj::HuffTable* tables = (x3dj::HuffTable*)malloc(8 * sizeof(x3dj::HuffTable));
    int32_t* scratch = (int32_t*)malloc(x3dj::kScratchInts * sizeof(int32_t));
    if (!tables || !scratch) {
        free(tables);
        free(scratch);
        x3djpeg_set_error("x3djpeg_entropy_decode_indexed_host: out of memory");
        return X3DJPEG_EINVAL;
    }
    for (int j = 0; j < njobs; ++j)
        ((int32_t*)status)[j] = frame_host(((const X3DJpegScanJob*)jobs)[j], ((const int32_t*)ids)[j],
                                           (const X3DJpegIndexRec*)index_recs, nrecs, (const uint32_t*)entries,
                                           (int64_t)entries_total, index_bits, tables, scratch);
    free(tables);
    free(scratch);
    return X3DJPEG_OK;
}
