// The host's part of the two-tier frame store (include/x3djpeg.h): the size query and x3djpeg_stage_host, the stage step
// of stage.hip run serially through the same stage_core.h.  Plain C++, no HIP call, no global state.
#include "stage_core.h"

void x3djpeg_set_error(const char* fmt, ...);  // host.cpp

extern "C" size_t x3djpeg_stage_bytes(int scan_bytes, int nseg) { return (size_t)x3dj::stage_frame_bytes(scan_bytes, nseg); }

extern "C" int x3djpeg_stage_host(const void* recs, int nrecs, const void* ids, int n, size_t max_frame_bytes, void* staging,
                                  size_t staging_cap, void* staged_recs, void* staged_ids, void* offsets, void* stage_status) {
    using namespace x3dj;
    if (!recs || !ids || !staging || !staged_recs || !staged_ids || !offsets || !stage_status || nrecs < 1 || n < 1 ||
        n > 65535 || max_frame_bytes < 1 || max_frame_bytes >= ((size_t)1 << 40) || staging_cap > ((size_t)1 << 60) ||
        (uint64_t)n * (uint64_t)max_frame_bytes >= ((uint64_t)1 << 44) ||
        (((uintptr_t)recs | (uintptr_t)staged_recs | (uintptr_t)offsets) & 7) != 0 || ((uintptr_t)staging & 15) != 0 ||
        (((uintptr_t)ids | (uintptr_t)staged_ids | (uintptr_t)stage_status) & 3) != 0) {
        x3djpeg_set_error("x3djpeg_stage_host: null or unaligned pointer, n %d outside 1 .. 65535, or max_frame_bytes %zu "
                          "outside 1 .. 2^40 or 2^44 / n", n, max_frame_bytes);
        return X3DJPEG_EINVAL;
    }
    StageArgs A;
    A.recs = (const X3DJpegStoreRec*)recs;
    A.ids = (const int32_t*)ids;
    A.nrecs = nrecs;
    A.n = n;
    A.max_frame_bytes = (int64_t)max_frame_bytes;
    A.staging = (uint8_t*)staging;
    A.cap = (int64_t)staging_cap;
    A.staged_recs = (X3DJpegStoreRec*)staged_recs;
    A.staged_ids = (int32_t*)staged_ids;
    A.offsets = (int64_t*)offsets;
    int64_t off = 0, first_refused = kStageNever;
    int seen = 0;
    for (int i = 0; i < n; ++i) {
        int64_t b;
        const int asked = stage_request(A, i, &b);
        const int fl = stage_place(A, i, asked, off, b);
        seen |= fl;
        const int64_t t = stage_total(fl, off, b);
        first_refused = t < first_refused ? t : first_refused;
        stage_offset(A, i, off, first_refused);
        off += b;
    }
    stage_offset(A, n, off, first_refused);
    *(int32_t*)stage_status = seen;
    for (int i = 0; i < n; ++i) {
        StageFrame F;
        if (!stage_frame(A, i, &F)) continue;
        for (int64_t at = 0; at < F.bytes; at += 16) store_piece(F.dst + at, stage_load(F, at));
    }
    return X3DJPEG_OK;
}
