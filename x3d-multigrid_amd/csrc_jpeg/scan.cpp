// The host's part of the parallel Huffman decoder of libx3djpeg (include/x3djpeg.h): x3djpeg_scan_prepare, one pass over
// the entropy-coded bytes of a file, and x3djpeg_entropy_decode_parallel_host, the scheme of entropy.hip run serially
// through the same entropy_core.h.  Plain C++, no HIP call, no global state.
#include <stdlib.h>
#include <string.h>

#include "entropy_core.h"

void x3djpeg_set_error(const char* fmt, ...);  // host.cpp

extern "C" size_t x3djpeg_scan_seg_bytes(void) { return sizeof(X3DJpegScanSeg); }
extern "C" size_t x3djpeg_scan_job_bytes(void) { return sizeof(X3DJpegScanJob); }

namespace {

int corrupt(const char* what) {
    x3djpeg_set_error("corrupt JPEG: %s", what);
    return X3DJPEG_ECORRUPT;
}

// what x3djpeg_entropy_decode asks of an info too
bool info_ok(const X3DJpegInfo* info, size_t len) {
    const int nc = info->ncomp;
    bool ok = (nc == 1 || nc == 3) && info->mcus_x > 0 && info->mcus_y > 0 && info->mcus_x <= 8192 && info->mcus_y <= 8192 &&
              info->scan_off >= 0 && (uint64_t)info->scan_off <= len && info->restart_interval >= 0;
    int64_t nb = 0;
    for (int c = 0; ok && c < nc; ++c) {
        ok = info->comp_h[c] >= 1 && info->comp_h[c] <= 2 && info->comp_v[c] >= 1 && info->comp_v[c] <= 2 &&
             info->blocks_w[c] == info->mcus_x * info->comp_h[c] && info->blocks_h[c] == info->mcus_y * info->comp_v[c] &&
             info->block_start[c] == nb && info->coef_off[c] == nb * 64 && info->comp_td[c] >= 0 && info->comp_td[c] <= 3 &&
             info->comp_ta[c] >= 0 && info->comp_ta[c] <= 3;
        if (ok) nb += (int64_t)info->blocks_w[c] * info->blocks_h[c];
    }
    return ok && nb == info->nblocks && info->coef_count == nb * 64;
}

}  // namespace

extern "C" int x3djpeg_scan_prepare(const uint8_t* d, size_t len, const X3DJpegInfo* info, uint8_t* scan, size_t scan_cap,
                                    X3DJpegScanSeg* segs, size_t seg_cap, size_t* scan_bytes, size_t* nseg) {
    if (!d || !info || !scan || !segs || !scan_bytes || !nseg) {
        x3djpeg_set_error("x3djpeg_scan_prepare: null pointer");
        return X3DJPEG_EINVAL;
    }
    *scan_bytes = *nseg = 0;
    if (!info_ok(info, len)) {
        x3djpeg_set_error("x3djpeg_scan_prepare: info is not what x3djpeg_parse wrote");
        return X3DJPEG_EINVAL;
    }
    {
        x3dj::HuffTable t;
        for (int c = 0; c < info->ncomp; ++c) {
            const int td = info->comp_td[c], ta = 4 + info->comp_ta[c];
            if (!x3dj::build_table(info->huff_bits[td], info->huff_vals[td], &t) ||
                !x3dj::build_table(info->huff_bits[ta], info->huff_vals[ta], &t))
                return corrupt("over-subscribed Huffman table");
        }
    }
    const int64_t nmcu = (int64_t)info->mcus_x * info->mcus_y, ri = info->restart_interval;
    const int64_t want = ri ? (nmcu + ri - 1) / ri : 1;
    if ((uint64_t)want > seg_cap || scan_cap < X3DJPEG_SCAN_PAD) {
        x3djpeg_set_error("x3djpeg_scan_prepare: %lld segments and the padding do not fit (%zu entries, %zu bytes)",
                          (long long)want, seg_cap, scan_cap);
        return X3DJPEG_EINVAL;
    }
    const size_t room = scan_cap - X3DJPEG_SCAN_PAD;  // for data
    size_t pos = (size_t)info->scan_off, out = 0;
    for (int64_t s = 0; s < want; ++s) {
        const size_t start = out;
        while (pos < len) {  // up to a marker or the end of the file
            const uint8_t* f = (const uint8_t*)memchr(d + pos, 0xFF, len - pos);
            const size_t run = f ? (size_t)(f - (d + pos)) : len - pos;
            const bool stuffed = f && pos + run + 1 < len && d[pos + run + 1] == 0x00;
            if (run + (stuffed ? 1 : 0) > room - out) {
                x3djpeg_set_error("x3djpeg_scan_prepare: scan buffer of %zu bytes too small", scan_cap);
                return X3DJPEG_EINVAL;
            }
            memcpy(scan + out, d + pos, run);
            out += run;
            pos += run;
            if (!stuffed) break;  // on a marker, or at the end
            scan[out++] = 0xFF;
            pos += 2;
        }
        if (out > (size_t)X3DJPEG_SCAN_MAX_BYTES) {
            x3djpeg_set_error("unsupported JPEG: scan of more than %d bytes on the parallel path", X3DJPEG_SCAN_MAX_BYTES);
            return X3DJPEG_EUNSUPPORTED;
        }
        segs[s].byte_off = (uint32_t)start;
        segs[s].byte_len = (uint32_t)(out - start);
        segs[s].first_mcu = (int32_t)(s * ri);
        segs[s].mcu_count = (int32_t)(ri ? (nmcu - s * ri < ri ? nmcu - s * ri : ri) : nmcu);
        if (s + 1 < want) {  // RSTn, after any fill bytes, and nothing else
            size_t p = pos;
            while (p + 1 < len && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
            if (p + 2 > len || d[p] != 0xFF || d[p + 1] != 0xD0 + (int)(s & 7)) return corrupt("restart marker missing");
            pos = p + 2;
        }
    }
    memset(scan + out, 0, X3DJPEG_SCAN_PAD);
    *scan_bytes = out;
    *nseg = (size_t)want;
    return X3DJPEG_OK;
}

extern "C" size_t x3djpeg_entropy_workspace_bytes(size_t scan_bytes, size_t nseg, int sub_bits) {
    if (scan_bytes > (size_t)X3DJPEG_SCAN_MAX_BYTES || nseg > (size_t)1 << 26) return 0;
    return (size_t)x3dj::frame_workspace_bytes((int64_t)scan_bytes, (int64_t)nseg, sub_bits);
}

namespace {

// One frame through the phases of entropy_core.h with kWorkers workers taken in turn: what a workgroup does in entropy.hip,
// a loop where it has a barrier.
constexpr int kWorkers = 7;

int frame_host(const X3DJpegScanJob& J, int sub_bits, uint8_t* ws, int64_t ws_bytes, x3dj::HuffTable* tables,
               int32_t* scratch, int32_t* rounds) {
    using namespace x3dj;
    FrameCtx C;
    const int nt = kWorkers;
    int err = setup(J, sub_bits, ws, ws_bytes, tables, &C);
    if (err) return err;
    int bad_table = 0, bad_seg = 0;
    for (int t = 0; t < nt; ++t) bad_table |= build_tables(J, C, tables, t, nt);
    for (int t = 0; t < nt; ++t) bad_seg |= seg_count(C, t, nt, scratch);
    if (bad_seg) return X3DJPEG_EINVAL;
    if (bad_table) return X3DJPEG_ECORRUPT;
    err = seg_total(&C, nt, scratch);
    if (err) return err;
    for (int t = 0; t < nt; ++t) seg_place(C, t, nt, scratch);
    for (int t = 0; t < nt; ++t) init(C, t, nt);
    int r = 0;
    while (r < C.nsub) {
        ++r;
        int changed = 0;
        for (int t = 0; t < nt; ++t) changed |= relax_take(C, t, nt);
        if (!changed) break;
        for (int t = 0; t < nt; ++t) relax_run(C, t, nt);
    }
    C.head[0] = r;
    if (rounds) *rounds = r;
    for (int t = 0; t < nt; ++t) count_sum(C, t, nt, scratch);
    carry_scan(scratch, nt);
    for (int t = 0; t < nt; ++t) count_place(C, t, nt, scratch);
    for (int t = 0; t < nt; ++t) zero(C, t, nt);
    for (int t = 0; t < nt; ++t) err |= write_coef(C, t, nt);
    for (int t = 0; t < nt; ++t) dc_sum(C, t, nt, scratch);
    for (int c = 0; c < C.ncomp; ++c) carry_scan(scratch + 2 * c * nt, nt);
    for (int t = 0; t < nt; ++t) dc_place(C, t, nt, scratch);
    return err ? X3DJPEG_ECORRUPT : X3DJPEG_OK;
}

}  // namespace

extern "C" int x3djpeg_entropy_decode_parallel_host(const X3DJpegScanJob* jobs, int njobs, int sub_bits, void* workspace,
                                                    size_t workspace_bytes, int32_t* status, int32_t* rounds) {
    if (!jobs || !workspace || !status || njobs < 1 || sub_bits < 32 || sub_bits % 32 != 0 || sub_bits > (1 << 20) ||
        ((uintptr_t)workspace & 15) != 0 || workspace_bytes > ((size_t)1 << 62)) {
        x3djpeg_set_error("x3djpeg_entropy_decode_parallel_host: null pointer, unaligned workspace, or sub_bits %d not a "
                          "multiple of 32", sub_bits);
        return X3DJPEG_EINVAL;
    }
    x3dj::HuffTable* tables = (x3dj::HuffTable*)malloc(8 * sizeof(x3dj::HuffTable));
    int32_t* scratch = (int32_t*)malloc(x3dj::kScratchInts * sizeof(int32_t));
    if (!tables || !scratch) {
        free(tables);
        free(scratch);
        x3djpeg_set_error("x3djpeg_entropy_decode_parallel_host: out of memory");
        return X3DJPEG_EINVAL;
    }
    for (int j = 0; j < njobs; ++j) {
        if (rounds) rounds[j] = 0;
        status[j] = frame_host(jobs[j], sub_bits, (uint8_t*)workspace, (int64_t)workspace_bytes, tables, scratch,
                               rounds ? rounds + j : nullptr);
    }
    free(tables);
    free(scratch);
    return X3DJPEG_OK;
}
