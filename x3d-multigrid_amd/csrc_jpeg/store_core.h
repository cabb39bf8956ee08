// The job builder of libx3djpeg's frame store (include/x3djpeg.h), shared word for word by the HIP kernels (store.hip)
// and by their serial CPU twin (x3djpeg_store_build_jobs_host in store_host.cpp).  Plain C++, every table through plain
// pointers.
//
// A batch is n requests (frame id, destination).  Building its two job tables has two steps:
//
//   plan   per request: what it needs (coefficients, workspace) and why it cannot be served, if so (plan_request); the
//          exclusive sums of both needs over the requests give each request its ranges; the capacities are checked against
//          the ranges (plan_place).  The sums are the only thing that couples requests: the kernel runs them in one
//          workgroup, the twin in a loop.
//   emit   per request: both job structs, written as 16-byte pieces (emit_request): the header entry is the two structs
//          with the per-request fields zero, so a piece is either a copy or one of six patched ones.  A refused request
//          gets zeros.  `lane` of `lanes` workers share a request; piece p is written by lane p % lanes, once.
//
// Nothing is read through an index that was not checked first: a record only for an id in [0, nrecs), a header only for
// a record whose header index is in [0, nheaders).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "entropy_core.h"

namespace x3dj {

struct alignas(16) Piece {
    uint64_t a, b;
};

static_assert(sizeof(X3DJpegFrameJob) == 512 && sizeof(X3DJpegFrameJob) % 16 == 0, "X3DJpegFrameJob");
static_assert(sizeof(X3DJpegScanJob) % 16 == 0 && sizeof(X3DJpegStoreHeader) == sizeof(X3DJpegFrameJob) + sizeof(X3DJpegScanJob),
              "X3DJpegStoreHeader");
static_assert(sizeof(X3DJpegStoreRec) == 32 && sizeof(X3DJpegStoreDst) == 24, "store records");
// the patched pieces: frame job 0 (coef, planes) and 1 (dst, dst_stride); scan job 0 (scan, segs), 1 (coef, coef_count),
// 2 (ws_off, ws_bytes) and 3 (scan_bytes, nseg | ncomp, mcus_x)
static_assert(offsetof(X3DJpegFrameJob, dst) == 16 && offsetof(X3DJpegFrameJob, width) == 32, "X3DJpegFrameJob");
static_assert(offsetof(X3DJpegScanJob, coef) == 16 && offsetof(X3DJpegScanJob, ws_off) == 32 &&
                  offsetof(X3DJpegScanJob, scan_bytes) == 48 && offsetof(X3DJpegScanJob, ncomp) == 56 &&
                  offsetof(X3DJpegScanJob, comp_h) == 72,
              "X3DJpegScanJob");

constexpr int kFramePieces = (int)(sizeof(X3DJpegFrameJob) / 16);
constexpr int kScanPieces = (int)(sizeof(X3DJpegScanJob) / 16);
constexpr int kPlanThreads = X3DJPEG_STORE_PLAN_THREADS;
constexpr int kPlanPerThread = X3DJPEG_STORE_PLAN_CHUNK / X3DJPEG_STORE_PLAN_THREADS;
static_assert(kPlanPerThread * kPlanThreads == X3DJPEG_STORE_PLAN_CHUNK, "the plan chunk is whole requests per thread");

X3DJ_HD static inline Piece load_piece(const void* p) {
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const Piece*>(p);  // one 16-byte load: the tables are 16-byte aligned
#else
    Piece v;
    memcpy(&v, p, sizeof(v));
    return v;
#endif
}

X3DJ_HD static inline void store_piece(void* p, Piece v) {
#ifdef __HIP_DEVICE_COMPILE__
    *reinterpret_cast<Piece*>(p) = v;
#else
    memcpy(p, &v, sizeof(v));
#endif
}

// The tables and capacities of one call.
struct StoreArgs {
    const X3DJpegStoreRec* recs;
    const X3DJpegStoreHeader* headers;
    const int32_t* ids;
    const X3DJpegStoreDst* dsts;
    int32_t nrecs, nheaders, n, sub_bits;
    int16_t* coef;
    uint8_t* planes;
    int64_t coef_cap, planes_cap, ws_cap;
    int64_t* plan;  // [3 * n + 2]
    X3DJpegScanJob* scan_jobs;
    X3DJpegFrameJob* frame_jobs;
};

X3DJ_HD static inline int64_t* plan_coef_off(const StoreArgs& A) { return A.plan; }
X3DJ_HD static inline int64_t* plan_ws_off(const StoreArgs& A) { return A.plan + A.n; }
X3DJ_HD static inline int64_t* plan_flags(const StoreArgs& A) { return A.plan + 2 * (int64_t)A.n; }
X3DJ_HD static inline int64_t* plan_totals(const StoreArgs& A) { return A.plan + 3 * (int64_t)A.n; }

// Request i by itself: its needs (zero for a bad id) and its flags short of the capacities.
X3DJ_HD static inline int plan_request(const StoreArgs& A, int i, int64_t* coef_count, int64_t* ws_need) {
    *coef_count = 0;
    *ws_need = 0;
    const int32_t id = A.ids[i];
    if (id < 0 || id >= A.nrecs) return X3DJPEG_STORE_BAD_ID;
    const X3DJpegStoreRec& R = A.recs[id];
    if (R.header < 0 || R.header >= A.nheaders || !R.scan || !R.segs) return X3DJPEG_STORE_BAD_ID;
    const X3DJpegStoreHeader& H = A.headers[R.header];
    const int64_t ws = frame_workspace_bytes(R.scan_bytes, R.nseg, A.sub_bits);
    if (ws == 0 || H.scan.coef_count < 0 || H.scan.coef_count != (int64_t)H.frame.nblocks * 64) return X3DJPEG_STORE_BAD_ID;
    *coef_count = H.scan.coef_count;
    *ws_need = ws;
    const X3DJpegStoreDst& D = A.dsts[i];
    return (H.frame.width != D.width || H.frame.height != D.height) ? X3DJPEG_STORE_BAD_SIZE : 0;
}

// Request i with its ranges: the capacities.  Returns the request's final flags and writes its line of the plan.
X3DJ_HD static inline int plan_place(const StoreArgs& A, int i, int flags, int64_t coef_off, int64_t coef_count, int64_t ws_off,
                                     int64_t ws_need) {
    if (!(flags & X3DJPEG_STORE_BAD_ID)) {
        if (coef_count > A.coef_cap - coef_off || coef_count > A.planes_cap - coef_off) flags |= X3DJPEG_STORE_NO_COEF;
        if (ws_need > A.ws_cap - ws_off) flags |= X3DJPEG_STORE_NO_WS;
    }
    plan_coef_off(A)[i] = coef_off;
    plan_ws_off(A)[i] = ws_off;
    plan_flags(A)[i] = flags;
    return flags;
}

// Both jobs of request i, lane's pieces of them.  The plan is complete.
X3DJ_HD static inline void emit_request(const StoreArgs& A, int i, int lane, int lanes) {
    uint8_t* fj = (uint8_t*)(A.frame_jobs + i);
    uint8_t* sj = (uint8_t*)(A.scan_jobs + i);
    if (plan_flags(A)[i] != 0) {  // refused: nothing of the tables is read
        const Piece zero = {0, 0};
        for (int p = lane; p < kFramePieces + kScanPieces; p += lanes)
            store_piece(p < kFramePieces ? fj + 16 * p : sj + 16 * (p - kFramePieces), zero);
        return;
    }
    const X3DJpegStoreRec& R = A.recs[A.ids[i]];
    const uint8_t* hf = (const uint8_t*)&A.headers[R.header].frame;
    const uint8_t* hs = (const uint8_t*)&A.headers[R.header].scan;
    const int64_t coef_off = plan_coef_off(A)[i], ws_off = plan_ws_off(A)[i];
    for (int p = lane; p < kFramePieces + kScanPieces; p += lanes) {
        Piece v;
        if (p < kFramePieces) {
            if (p == 0) {
                v.a = (uint64_t)(uintptr_t)(A.coef + coef_off);
                v.b = (uint64_t)(uintptr_t)(A.planes + coef_off);
            } else if (p == 1) {
                v.a = (uint64_t)(uintptr_t)A.dsts[i].dst;
                v.b = (uint64_t)A.dsts[i].dst_stride;
            } else {
                v = load_piece(hf + 16 * p);
            }
            store_piece(fj + 16 * p, v);
        } else {
            const int q = p - kFramePieces;
            if (q == 0) {
                v.a = (uint64_t)(uintptr_t)R.scan;
                v.b = (uint64_t)(uintptr_t)R.segs;
            } else if (q == 1) {
                v.a = (uint64_t)(uintptr_t)(A.coef + coef_off);
                v.b = load_piece(hs + 16).b;  // coef_count
            } else if (q == 2) {
                v.a = (uint64_t)ws_off;
                v.b = (uint64_t)frame_workspace_bytes(R.scan_bytes, R.nseg, A.sub_bits);
            } else if (q == 3) {
                v.a = (uint64_t)(uint32_t)R.scan_bytes | ((uint64_t)(uint32_t)R.nseg << 32);
                v.b = load_piece(hs + 48).b;  // ncomp, mcus_x
            } else {
                v = load_piece(hs + 16 * q);
            }
            store_piece(sj + 16 * q, v);
        }
    }
}

}  // namespace x3dj
