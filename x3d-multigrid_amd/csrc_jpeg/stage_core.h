// The stage step of libx3djpeg's two-tier frame store (include/x3djpeg.h), shared word for word by the HIP kernels
// (stage.hip) and by their serial CPU twin (x3djpeg_stage_host in stage_host.cpp).  Plain C++, every table through plain
// pointers.
//
// A host-tier store keeps its arena in pinned host memory; a batch first gathers the frames it draws into a staging buffer
// on the device.  That has two steps:
//
//   plan   per request: the bytes it takes (stage_request; zero for a request refused by itself); the exclusive sum of
//          those over the requests gives each one its offset; the capacity is checked against offset + bytes
//          (stage_place), which writes the request's staged record, staged id and offset.  The sums run over what every
//          request asks for, served or not: they grow with i, so a request that does not fit leaves no room for any later
//          one, the served requests lie without a gap in [0, total), and total is the smallest offset refused for lack of
//          room (stage_total).  The sum is the only thing that couples requests: the kernel runs it in one workgroup,
//          the twin in a loop.
//   copy   per request and 16-byte piece of its staged bytes: one load from the arena (stage_load), one store.  The
//          last piece of the scan is masked to zero past scan_bytes + X3DJPEG_SCAN_PAD, so the staged tail does not
//          depend on what the arena holds there.
//
// Nothing is read through an index that was not checked first: a record only for an id in [0, nrecs), arena bytes only
// for a served request and only inside the sizes its record states.
#pragma once
#include "store_core.h"

namespace x3dj {

// The tables of one call.
struct StageArgs {
    const X3DJpegStoreRec* recs;
    const int32_t* ids;
    int32_t nrecs, n;
    int64_t max_frame_bytes;
    uint8_t* staging;
    int64_t cap;
    X3DJpegStoreRec* staged_recs;
    int32_t* staged_ids;
    int64_t* offsets;  // [n + 1]
};

constexpr int64_t kStageNever = INT64_MAX;  // "no request was refused for lack of room"

X3DJ_HD static inline int64_t stage_scan_len(int32_t scan_bytes) { return ((int64_t)scan_bytes + X3DJPEG_SCAN_PAD + 15) & ~(int64_t)15; }
X3DJ_HD static inline int64_t stage_frame_bytes(int32_t scan_bytes, int32_t nseg) {
    if (scan_bytes < 0 || nseg < 0) return 0;
    return stage_scan_len(scan_bytes) + (int64_t)nseg * (int64_t)sizeof(X3DJpegScanSeg);
}
static_assert(sizeof(X3DJpegScanSeg) == 16, "a segment is one piece");

// Request i by itself: the bytes it asks for (zero when it is refused here) and its flags short of the capacity.
X3DJ_HD static inline int stage_request(const StageArgs& A, int i, int64_t* bytes) {
    *bytes = 0;
    const int32_t id = A.ids[i];
    if (id < 0 || id >= A.nrecs) return X3DJPEG_STAGE_BAD_ID;
    const X3DJpegStoreRec& R = A.recs[id];
    if (!R.scan || !R.segs || R.scan_bytes < 0 || R.nseg < 0) return X3DJPEG_STAGE_BAD_ID;
    const int64_t b = stage_frame_bytes(R.scan_bytes, R.nseg);
    if (b > A.max_frame_bytes) return X3DJPEG_STAGE_NO_ROOM;  // the copy grid would not cover it
    *bytes = b;
    return 0;
}

// Request i with its offset in the sums: the capacity.  Returns the request's final flags and writes its staged record and
// id; its line of `offsets` is written by stage_offset once the total so far is known.
X3DJ_HD static inline int stage_place(const StageArgs& A, int i, int flags, int64_t off, int64_t bytes) {
    if (!flags && bytes > A.cap - off) flags = X3DJPEG_STAGE_NO_ROOM;
    X3DJpegStoreRec out;
    if (flags) {
        out.scan = nullptr;
        out.segs = nullptr;
        out.scan_bytes = out.nseg = out.header = 0;
    } else {
        const X3DJpegStoreRec& R = A.recs[A.ids[i]];
        out.scan = A.staging + off;
        out.segs = (const X3DJpegScanSeg*)(A.staging + off + stage_scan_len(R.scan_bytes));
        out.scan_bytes = R.scan_bytes;
        out.nseg = R.nseg;
        out.header = R.header;
    }
    out.pad = 0;
    A.staged_recs[i] = out;
    A.staged_ids[i] = flags ? -1 : i;
    return flags;
}

// What a request refused with `flags` at `off` and asking for `bytes` says about the total: its offset if it was the
// capacity that refused it (it asked for bytes, and got none), nothing otherwise.
X3DJ_HD static inline int64_t stage_total(int flags, int64_t off, int64_t bytes) {
    return (flags & X3DJPEG_STAGE_NO_ROOM) && bytes > 0 ? off : kStageNever;
}

// offsets[i]: the request's place in the sums, or the total for everything from the first one without room on.
X3DJ_HD static inline void stage_offset(const StageArgs& A, int i, int64_t off, int64_t first_refused) {
    A.offsets[i] = off < first_refused ? off : first_refused;
}

// Request i as the copy sees it: where from, where to, how much.  The plan is complete.
struct StageFrame {
    const uint8_t* scan;
    const uint8_t* segs;
    uint8_t* dst;
    int64_t valid, scan_len, bytes;  // scan bytes with their padding; the same rounded up to 16; all staged bytes
};

// false for a refused request: it has no bytes, and nothing of the arena is read for it.
X3DJ_HD static inline bool stage_frame(const StageArgs& A, int i, StageFrame* F) {
    if (A.staged_ids[i] < 0) return false;
    const X3DJpegStoreRec& S = A.staged_recs[i];  // where to; the sizes are the source's
    const X3DJpegStoreRec& R = A.recs[A.ids[i]];
    F->scan = R.scan;
    F->segs = (const uint8_t*)R.segs;
    F->dst = const_cast<uint8_t*>(S.scan);
    F->valid = (int64_t)S.scan_bytes + X3DJPEG_SCAN_PAD;
    F->scan_len = stage_scan_len(S.scan_bytes);
    F->bytes = F->scan_len + (int64_t)S.nseg * 16;
    return true;
}

// The 16 staged bytes at `at` (a multiple of 16 below F.bytes).
X3DJ_HD static inline Piece stage_load(const StageFrame& F, int64_t at) {
    if (at >= F.scan_len) return load_piece(F.segs + (at - F.scan_len));
    if (at + 16 <= F.valid) return load_piece(F.scan + at);
    const int keep = (int)(F.valid - at);  // the scan's last piece: 1 .. 15 bytes of it, then zeros
    Piece v;
#ifdef __HIP_DEVICE_COMPILE__
    v = load_piece(F.scan + at);  // readable to the rounded-up end (include/x3djpeg.h)
    if (keep <= 8) {
        v.a &= keep == 8 ? ~(uint64_t)0 : (((uint64_t)1 << (8 * keep)) - 1);
        v.b = 0;
    } else {
        v.b &= ((uint64_t)1 << (8 * (keep - 8))) - 1;
    }
#else
    v.a = v.b = 0;
    memcpy(&v, F.scan + at, (size_t)keep);
#endif
    return v;
}

}  // namespace x3dj
