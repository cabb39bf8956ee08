// The indexed Huffman decoder of libx3djpeg (include/x3djpeg.h), shared word for word by the HIP kernel
// (entropy_indexed.hip) and by its serial CPU twin (index_host.cpp), and the rule of the sync index itself.  Plain C++ on
// top of entropy_core.h: the same bit reader, tables, decode_span, zero and DC phases; nothing here touches a workspace.
//
// The relaxation decoder finds the state (p, b, k) and the first block of every subsequence again for every batch.  For a
// stored frame they depend on the stored bytes alone: index_segment computes them once, and a frame is then decoded in one
// pass -- every worker starts its subsequences in the states the index gives and compares the state it ends in with the
// next entry of the segment.  Entry 0 of a segment is compared with the start state.  If every comparison holds, every
// subsequence was decoded from the state the serial decoder is in at its start, by induction over the segment: the result
// is the serial decode.  If one does not, the frame reports X3DJPEG_EINDEX.
//
// Whatever an entry holds, decode_span checks every scan read against the segment's length and every store against
// coef_count, and each of its loops consumes at least one bit per turn up to the segment's bits; an entry whose p lies
// beyond the segment is refused before it is decoded from (the reader's bit position would wrap).
//
//   idx_setup              the job checked against itself; id, record and entry range checked
//   seg_count / idx_total  entries per segment summed per worker (entropy_core.h), their total against the record
//   idx_write              zero first; then each worker: its contiguous share of the entries, decoded and compared
//   dc_sum / dc_place      as in the relaxation decoder
#pragma once
#include "entropy_core.h"

namespace x3dj {

// what a frame's failures are collected as, one bit each, OR-ed over the workers
enum { kIdxStale = 1, kIdxCorrupt = 2, kIdxInvalid = 4 };

X3DJ_HD static inline uint32_t idx_word1(uint32_t b, uint32_t k, uint32_t first) {
    return (b & 7u) | ((k & 127u) << 3) | (first << 10);
}

X3DJ_HD static inline bool index_bits_ok(int index_bits) {
    return index_bits >= 32 && index_bits % 32 == 0 && index_bits <= (1 << 20);
}

// The frame's entries: two uint32 words each.
struct IndexCtx {
    const uint32_t* ent;
    int32_t nent;
};

// By one worker.  The context without a workspace, and the frame's part of the index.
X3DJ_HD static inline int idx_setup(const X3DJpegScanJob& J, int32_t id, const X3DJpegIndexRec* recs, int32_t nrecs,
                                    const uint32_t* entries, int64_t entries_total, int index_bits, const HuffTable* tables,
                                    FrameCtx* C, IndexCtx* X) {
    if (!J.coef) return X3DJPEG_EINVAL;
    const int err = setup_frame(J, index_bits, tables, C);
    if (err) return err;
    if (id < 0 || id >= nrecs) return X3DJPEG_EINVAL;
    const X3DJpegIndexRec r = recs[id];
    if (r.first_entry < 0 || r.nentries < 1 || r.first_entry > entries_total || r.nentries > entries_total - r.first_entry)
        return X3DJPEG_EINVAL;
    X->ent = entries + 2 * r.first_entry;
    X->nent = r.nentries;
    return X3DJPEG_OK;
}

// By one worker, after seg_count: exclusive sum of scratch[0, nt) (the first entry of each worker's share of the
// segments); the total must be the record's count.
X3DJ_HD static inline int idx_total(FrameCtx* C, const IndexCtx& X, int nt, int32_t* scratch) {
    int64_t run = 0;
    for (int t = 0; t < nt; ++t) {
        const int32_t v = scratch[t];
        scratch[t] = (int32_t)(run > 0x7FFFFFFF ? 0x7FFFFFFF : run);
        run += v;
    }
    if (run > 0x3FFFFFFF || run != X.nent) return X3DJPEG_EINVAL;
    C->nsub = (int32_t)run;
    return X3DJPEG_OK;
}

// The worker's contiguous share of the entries: each decoded from its state, the state it ends in compared with the next
// entry of its segment, the first of a segment with the start state.  scratch: what idx_total left.  Returns kIdx* bits.
X3DJ_HD static inline int idx_write(const FrameCtx& C, const IndexCtx& X, int tid, int nt, const int32_t* scratch) {
    int64_t lo, hi;
    chunk(C.nsub, tid, nt, &lo, &hi);
    if (lo >= hi) return 0;
    // the last worker whose share of the segments starts at or before entry lo holds its segment (scratch does not fall)
    int a = 0, z = nt - 1;
    while (a < z) {
        const int m = (a + z + 1) >> 1;
        if (scratch[m] <= lo) a = m; else z = m - 1;
    }
    int64_t slo, shi;
    chunk(C.nseg, a, nt, &slo, &shi);
    int64_t s = slo, at = scratch[a];
    X3DJpegScanSeg g = C.segs[s];
    int32_t n = seg_nsub(g.byte_len, C.sub_bits);
    while (at + n <= lo && s + 1 < C.nseg) {
        at += n;
        ++s;
        g = C.segs[s];
        n = seg_nsub(g.byte_len, C.sub_bits);
    }
    int32_t local = (int32_t)(lo - at);
    int bad = 0;
    for (int64_t i = lo; i < hi; ++i) {
        if (local >= n) {
            if (s + 1 >= C.nseg) return bad | kIdxInvalid;  // cannot be: the entries are the segments' sum
            ++s;
            g = C.segs[s];
            n = seg_nsub(g.byte_len, C.sub_bits);
            local = 0;
        }
        uint32_t p = X.ent[2 * i];
        const uint32_t w = X.ent[2 * i + 1];
        const bool last = local + 1 == n;
        if ((local == 0 && (p != 0 || w != 0)) || p > g.byte_len * 8u) {
            bad |= kIdxStale;
        } else {
            uint32_t bk = (w & 7u) | (((w >> 3) & 127u) << 8);
            const int32_t first = (int32_t)(w >> 10);
            int32_t blocks = 0;
            const int e = decode_span<kWrite>(C, (int32_t)s, g, local, last, &p, &bk, first, &blocks);
            if (e) {
                bad |= e == X3DJPEG_ECORRUPT ? kIdxCorrupt : kIdxInvalid;
            } else if (!last) {
                const int64_t end_block = (int64_t)first + blocks;
                const uint32_t want = idx_word1(bk & 255u, (bk >> 8) & 255u, (uint32_t)end_block);
                if (end_block >= X3DJPEG_INDEX_MAX_BLOCKS || X.ent[2 * i + 2] != p || X.ent[2 * i + 3] != want)
                    bad |= kIdxStale;
            }
        }
        ++local;
    }
    return bad;
}

// what the frame reports for the OR of its workers' bits
X3DJ_HD static inline int idx_status(int bits) {
    return bits & kIdxStale ? X3DJPEG_EINDEX : bits & kIdxInvalid ? X3DJPEG_EINVAL : bits & kIdxCorrupt ? X3DJPEG_ECORRUPT : 0;
}

// The entries of segment s of a prepared scan, n of them, into ent[0, 2 * n): one serial pass in check mode.  Nonzero
// where the host decoder refuses the segment.
X3DJ_HD static inline int index_segment(const FrameCtx& C, int32_t s, uint32_t* ent, int32_t n) {
    const X3DJpegScanSeg g = C.segs[s];
    uint32_t p = 0, bk = 0;
    int32_t first = 0;
    for (int32_t local = 0; local < n; ++local) {
        ent[2 * local] = p;
        ent[2 * local + 1] = idx_word1(bk & 255u, (bk >> 8) & 255u, (uint32_t)first);
        int32_t blocks = 0;
        const int e = decode_span<kCheck>(C, s, g, local, local + 1 == n, &p, &bk, first, &blocks);
        if (e) return e;
        first += blocks;
    }
    return 0;
}

}  // namespace x3dj
