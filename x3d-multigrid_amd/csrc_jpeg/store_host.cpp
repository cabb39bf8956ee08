// The host's part of libx3djpeg's frame store (include/x3djpeg.h): the size queries and x3djpeg_store_build_jobs_host,
// the job builder of store.hip run serially through the same store_core.h.  Plain C++, no HIP call, no global state.
#include "store_core.h"

void x3djpeg_set_error(const char* fmt, ...);  // host.cpp

extern "C" size_t x3djpeg_store_header_bytes(void) { return sizeof(X3DJpegStoreHeader); }
extern "C" size_t x3djpeg_store_rec_bytes(void) { return sizeof(X3DJpegStoreRec); }
extern "C" size_t x3djpeg_store_dst_bytes(void) { return sizeof(X3DJpegStoreDst); }
extern "C" size_t x3djpeg_store_plan_bytes(int n) { return n < 1 ? 0 : sizeof(int64_t) * (3 * (size_t)n + 2); }

extern "C" int x3djpeg_store_build_jobs_host(const void* recs, int nrecs, const void* headers, int nheaders, const void* ids,
                                             int n, int sub_bits, void* coef, size_t coef_cap, void* planes, size_t planes_cap,
                                             size_t workspace_bytes, const void* dsts, void* plan, void* scan_jobs,
                                             void* frame_jobs, void* build_status) {
    using namespace x3dj;
    if (!recs || !headers || !ids || !coef || !planes || !dsts || !plan || !scan_jobs || !frame_jobs || !build_status ||
        nrecs < 1 || nheaders < 1 || n < 1 || n > 65535 || sub_bits < 32 || sub_bits % 32 != 0 || sub_bits > (1 << 20) ||
        coef_cap > ((size_t)1 << 60) || planes_cap > ((size_t)1 << 60) || workspace_bytes > ((size_t)1 << 62) ||
        (((uintptr_t)recs | (uintptr_t)headers | (uintptr_t)dsts | (uintptr_t)plan | (uintptr_t)scan_jobs |
          (uintptr_t)frame_jobs) & 7) != 0 ||
        (((uintptr_t)ids | (uintptr_t)build_status) & 3) != 0) {
        x3djpeg_set_error("x3djpeg_store_build_jobs_host: null or unaligned pointer, n %d outside 1 .. 65535, or sub_bits %d "
                          "not a multiple of 32", n, sub_bits);
        return X3DJPEG_EINVAL;
    }
    StoreArgs A;
    A.recs = (const X3DJpegStoreRec*)recs;
    A.headers = (const X3DJpegStoreHeader*)headers;
    A.ids = (const int32_t*)ids;
    A.dsts = (const X3DJpegStoreDst*)dsts;
    A.nrecs = nrecs;
    A.nheaders = nheaders;
    A.n = n;
    A.sub_bits = sub_bits;
    A.coef = (int16_t*)coef;
    A.planes = (uint8_t*)planes;
    A.coef_cap = (int64_t)coef_cap;
    A.planes_cap = (int64_t)planes_cap;
    A.ws_cap = (int64_t)workspace_bytes;
    A.plan = (int64_t*)plan;
    A.scan_jobs = (X3DJpegScanJob*)scan_jobs;
    A.frame_jobs = (X3DJpegFrameJob*)frame_jobs;
    int64_t off_coef = 0, off_ws = 0;
    int seen = 0;
    for (int i = 0; i < n; ++i) {
        int64_t cc, ws;
        const int fl = plan_request(A, i, &cc, &ws);
        seen |= plan_place(A, i, fl, off_coef, cc, off_ws, ws);
        off_coef += cc;
        off_ws += ws;
    }
    plan_totals(A)[0] = off_coef;
    plan_totals(A)[1] = off_ws;
    *(int32_t*)build_status = seen;
    constexpr int kLanes = 5;  // any number gives the same bytes; more than one walks the lane stride
    for (int i = 0; i < n; ++i)
        for (int lane = 0; lane < kLanes; ++lane) emit_request(A, i, lane, kLanes);
    return X3DJPEG_OK;
}
