// The parallel Huffman decoder of libx3djpeg (include/x3djpeg.h), shared word for word by the HIP kernel (entropy.hip) and
// by its serial CPU twin (x3djpeg_entropy_decode_parallel_host in scan.cpp).  Plain C++: no HIP intrinsic, every table and
// buffer through plain pointers.
//
// A prepared scan (x3djpeg_scan_prepare) is cut into segments, one per restart interval, and each segment into
// subsequences of sub_bits bits.  A decoder's state at a bit position is (p, b, k): p the bit position within the segment,
// b the block within the MCU (it selects the component and so the tables), k the zigzag index, 0 when a DC code comes
// next.  The frame is decoded in phases, each a function of (context, tid, nt): `nt` workers run a phase, then all of them
// meet before the next one (a workgroup barrier on the device, the end of a plain loop over tid on the CPU).
//
//   seg_count / seg_place   subsequences per segment, their exclusive sum, the subsequence -> segment map
//   init                    entry[i] = (i * sub_bits, 0, 0) (exact for the first of a segment); exit[i] = run(entry[i])
//   relax_take / relax_run  while anything changed, at most nsub rounds: entry[i] takes exit[i - 1], changed ones rerun.
//                           After round r the first r + 1 subsequences of a segment are exact.
//   count_sum / count_place blocks completed per subsequence -> first block of each (exclusive sum within the segment)
//   zero, write             coefficients: nonzero ACs in natural order, the DC *difference* in element 0
//   dc_sum / dc_place       per component and segment, the inclusive sum of the DC differences in scan order (mod 2^16,
//                           as the host's (int16_t)(pred + diff))
//
// In speculative mode (run) a bad code is no error: the decoder skips one bit and expects a DC code.  In write mode it is
// the host decoder's error.  Every read of the scan is checked against the segment's byte length and yields zero bits
// past it; every loop is bounded by the bits of the segment (a symbol consumes at least one); every coefficient store is
// checked against the frame's coef_count.
#pragma once
#include <stdint.h>

#include "../../include/x3djpeg.h"

#ifdef __HIP__
#define X3DJ_HD __host__ __device__
#else
#define X3DJ_HD
#endif

namespace x3dj {

constexpr int kMaxWorkers = 256;                   // the kernel's workgroup; the CPU twin uses fewer
constexpr int kScratchInts = 2 * 3 * kMaxWorkers;  // (flag, sum) per worker and component
constexpr uint32_t kDirty = 0x80000000u;           // in the second word of an entry state: rerun it

// Huffman table in libjpeg's form: a 9-bit lookahead table for the short codes, maxcode / valoffset for the rest.
struct HuffTable {
    static constexpr int LOOK = 9;
    uint16_t look[1 << LOOK];  // (length << 8) | symbol; 0: longer than LOOK bits
    int32_t maxcode[18];       // largest code of each length, -1 if none; [17] is a sentinel
    int32_t valoff[17];        // index of the first value of the length minus its first code
    uint8_t vals[256];
};

// false for an over-subscribed table (more codes of a length than the length holds)
X3DJ_HD static inline bool build_table(const uint8_t* bits, const uint8_t* vals, HuffTable* t) {
    for (int i = 0; i < (1 << HuffTable::LOOK); ++i) t->look[i] = 0;
    for (int i = 0; i < 256; ++i) t->vals[i] = vals[i];
    int code = 0, k = 0;
    t->valoff[0] = 0;
    t->maxcode[0] = -1;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (code + n > (1 << l)) return false;
        t->valoff[l] = k - code;
        if (n) {
            if (l <= HuffTable::LOOK) {
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (HuffTable::LOOK - l);
                    for (int j = 0; j < (1 << (HuffTable::LOOK - l)); ++j)
                        t->look[first + j] = (uint16_t)((l << 8) | vals[(k + i) & 255]);
                }
            }
            code += n;
            k += n;
            t->maxcode[l] = code - 1;
        } else {
            t->maxcode[l] = -1;
        }
        code <<= 1;
    }
    t->maxcode[17] = 0x7FFFFFFF;
    return true;
}

// Bit reader over one segment of unstuffed bytes, from any bit position; zero bits past the segment.
struct Bits {
    const uint8_t* d;
    uint32_t nbytes, pos;
    uint64_t acc;  // the low n bits are valid
    int n;

    X3DJ_HD void seek(uint32_t p) {
        pos = p >> 3;
        acc = 0;
        n = 0;
        fill();
        n -= (int)(p & 7);
    }
    X3DJ_HD void fill() {
        while (n <= 56) {
            const uint32_t b = pos < nbytes ? d[pos] : 0u;
            ++pos;
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    X3DJ_HD uint32_t bitpos() const { return pos * 8u - (uint32_t)n; }
    X3DJ_HD int peek(int k) const { return (int)((acc >> (n - k)) & ((1u << k) - 1)); }
    X3DJ_HD void skip(int k) { n -= k; }
};

X3DJ_HD static inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one symbol; -1 for a code no length matches.  Needs >= 16 bits in the reader.
X3DJ_HD static inline int decode_symbol(Bits& br, const HuffTable& t) {
    const int e = t.look[br.peek(HuffTable::LOOK)];
    if (e) {
        br.skip(e >> 8);
        return e & 255;
    }
    int l = HuffTable::LOOK + 1;
    int code = br.peek(l);
    while (l <= 16 && code > t.maxcode[l]) {
        ++l;
        code = br.peek(l);
    }
    if (l > 16) return -1;
    br.skip(l);
    return t.vals[(code + t.valoff[l]) & 255];
}

// What one frame's phases share: written by setup() and the *_place phases, read by everybody after a meeting point.
struct FrameCtx {
    const uint8_t* scan;
    const X3DJpegScanSeg* segs;
    int16_t* coef;
    int64_t coef_count;
    int32_t scan_bytes, nseg, nsub, sub_bits, ncomp, bpm, mcus_x, nmcu, ri;
    int32_t blk_comp[6], blk_by[6], blk_bx[6];  // block b of an MCU: component, row and column among the component's
    int32_t comp_h[3], comp_v[3], blocks_w[3];
    int64_t coef_off[3];
    const HuffTable* dc[3];
    const HuffTable* ac[3];
    int64_t ws_bytes;
    int32_t* head;       // [0]: relaxation rounds used, [1]: nsub
    int32_t* seg_first;  // [nseg]: first subsequence of the segment
    int32_t* sub_seg;    // [nsub]: segment of the subsequence
    uint32_t* entry;     // [nsub][2]: p, b | k << 8 | kDirty
    uint32_t* exits;     // [nsub][2]
    int32_t* cnt;        // [nsub]: blocks completed, then (count_place) the first block within the segment
    uint8_t zigzag[64];
};

X3DJ_HD static inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// bytes of workspace for nsub subsequences in nseg segments
X3DJ_HD static inline int64_t workspace_need(int64_t nsub, int64_t nseg) {
    return 16 + align16(4 * nseg) + align16(4 * nsub) + 2 * align16(8 * nsub) + align16(4 * nsub);
}

// What x3djpeg_entropy_workspace_bytes answers, for the host and for the job builder of store_core.h: 0 for a sub_bits or a
// scan the decoder does not take.  A segment has at most floor(bits / sub_bits) + 1 subsequences.
X3DJ_HD static inline int64_t frame_workspace_bytes(int64_t scan_bytes, int64_t nseg, int sub_bits) {
    if (sub_bits < 32 || sub_bits % 32 != 0 || scan_bytes < 0 || scan_bytes > (int64_t)X3DJPEG_SCAN_MAX_BYTES || nseg < 0 ||
        nseg > ((int64_t)1 << 26))
        return 0;
    return workspace_need(scan_bytes * 8 / sub_bits + nseg, nseg);
}

X3DJ_HD static inline int32_t seg_nsub(uint32_t byte_len, int32_t sub_bits) {
    const int64_t n = ((int64_t)byte_len * 8 + sub_bits - 1) / sub_bits;
    return n < 1 ? 1 : (int32_t)n;
}

// By one worker.  Checks the job against itself (the rest of the code relies on nothing else) and derives the context;
// X3DJPEG_EINVAL if it does not hold together.  tables: storage for 8 HuffTables (DC 0-3, AC 0-3).  WS: with the frame's
// part of the workspace and its coefficient buffer (setup); without, neither is looked at and every workspace pointer of
// the context is null (setup_frame: the indexed decoder of index_core.h starts from that alone).
template <bool WS>
X3DJ_HD static inline int setup_any(const X3DJpegScanJob& J, int sub_bits, uint8_t* workspace, int64_t workspace_bytes,
                                    const HuffTable* tables, FrameCtx* C) {
    const int nc = J.ncomp;
    bool ok = (nc == 1 || nc == 3) && J.mcus_x > 0 && J.mcus_y > 0 && J.mcus_x <= 8192 && J.mcus_y <= 8192 && J.scan &&
              J.segs && (!WS || J.coef) && J.scan_bytes >= 0 && J.scan_bytes <= X3DJPEG_SCAN_MAX_BYTES &&
              J.restart_interval >= 0 && sub_bits >= 32 && sub_bits % 32 == 0 && sub_bits <= (1 << 20) &&
              (!WS || (J.ws_off >= 0 && J.ws_off % 16 == 0 && J.ws_bytes >= 16 && J.ws_off <= workspace_bytes &&
                       J.ws_bytes <= workspace_bytes - J.ws_off && workspace));
    if (!ok) return X3DJPEG_EINVAL;
    int64_t nb = 0;
    int bpm = 0;
    for (int c = 0; c < nc; ++c) {
        const int h = J.comp_h[c], v = J.comp_v[c];
        ok = h >= 1 && h <= 2 && v >= 1 && v <= 2 && J.blocks_w[c] == J.mcus_x * h && J.block_start[c] == nb &&
             J.comp_td[c] >= 0 && J.comp_td[c] <= 3 && J.comp_ta[c] >= 0 && J.comp_ta[c] <= 3 && (c == 0 || (h == 1 && v == 1));
        if (!ok) return X3DJPEG_EINVAL;
        for (int by = 0; by < v; ++by)
            for (int bx = 0; bx < h; ++bx) {
                C->blk_comp[bpm] = c;
                C->blk_by[bpm] = by;
                C->blk_bx[bpm] = bx;
                ++bpm;
            }
        C->comp_h[c] = h;
        C->comp_v[c] = v;
        C->blocks_w[c] = J.blocks_w[c];
        C->coef_off[c] = nb * 64;
        C->dc[c] = tables + J.comp_td[c];
        C->ac[c] = tables + 4 + J.comp_ta[c];
        nb += (int64_t)J.blocks_w[c] * J.mcus_y * v;
    }
    C->nmcu = J.mcus_x * J.mcus_y;
    C->ri = J.restart_interval;
    const int64_t want_seg = C->ri ? ((int64_t)C->nmcu + C->ri - 1) / C->ri : 1;
    if (J.coef_count != nb * 64 || J.nseg != want_seg) return X3DJPEG_EINVAL;
    if (WS && workspace_need(J.nseg, J.nseg) > J.ws_bytes) return X3DJPEG_EINVAL;  // at least one subsequence per segment
    C->scan = J.scan;
    C->segs = J.segs;
    C->coef = J.coef;
    C->coef_count = J.coef_count;
    C->scan_bytes = J.scan_bytes;
    C->nseg = J.nseg;
    C->nsub = 0;
    C->sub_bits = sub_bits;
    C->ncomp = nc;
    C->bpm = bpm;
    C->mcus_x = J.mcus_x;
    if (WS) {
        C->ws_bytes = J.ws_bytes;
        C->head = (int32_t*)(workspace + J.ws_off);
        C->seg_first = C->head + 4;
        C->head[0] = 0;
        C->head[1] = 0;
    } else {
        C->ws_bytes = 0;
        C->head = nullptr;
        C->seg_first = nullptr;
        C->sub_seg = nullptr;
        C->entry = nullptr;
        C->exits = nullptr;
        C->cnt = nullptr;
    }
    const uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    for (int i = 0; i < 64; ++i) C->zigzag[i] = zz[i];
    return X3DJPEG_OK;
}

X3DJ_HD static inline int setup(const X3DJpegScanJob& J, int sub_bits, uint8_t* workspace, int64_t workspace_bytes,
                                const HuffTable* tables, FrameCtx* C) {
    return setup_any<true>(J, sub_bits, workspace, workspace_bytes, tables, C);
}

X3DJ_HD static inline int setup_frame(const X3DJpegScanJob& J, int sub_bits, const HuffTable* tables, FrameCtx* C) {
    return setup_any<false>(J, sub_bits, nullptr, 0, tables, C);
}

// worker tid's share of [0, n): contiguous, in order of tid
X3DJ_HD static inline void chunk(int64_t n, int tid, int nt, int64_t* lo, int64_t* hi) {
    *lo = n * tid / nt;
    *hi = n * (tid + 1) / nt;
}

// The Huffman tables the frame uses, one per worker.  Nonzero for an over-subscribed one.
X3DJ_HD static inline int build_tables(const X3DJpegScanJob& J, const FrameCtx& C, HuffTable* tables, int tid, int nt) {
    int err = 0;
    for (int t = tid; t < 8; t += nt) {
        bool used = false;
        for (int c = 0; c < C.ncomp; ++c) used = used || (t < 4 ? J.comp_td[c] == t : J.comp_ta[c] == t - 4);
        if (used && !build_table(J.huff_bits[t], J.huff_vals[t], tables + t)) err = X3DJPEG_ECORRUPT;
    }
    return err;
}

// Subsequences of the worker's segments, summed into scratch[tid]; the segment table checked against the job.
X3DJ_HD static inline int seg_count(const FrameCtx& C, int tid, int nt, int32_t* scratch) {
    int64_t lo, hi, sum = 0;
    int err = 0;
    chunk(C.nseg, tid, nt, &lo, &hi);
    for (int64_t s = lo; s < hi; ++s) {
        const X3DJpegScanSeg g = C.segs[s];
        const int64_t first = C.ri ? s * C.ri : 0;
        const int64_t count = C.ri ? (C.nmcu - first < C.ri ? C.nmcu - first : C.ri) : C.nmcu;
        if ((int64_t)g.byte_off + g.byte_len > C.scan_bytes || g.first_mcu != first || g.mcu_count != count) err = X3DJPEG_EINVAL;
        sum += seg_nsub(g.byte_len, C.sub_bits);
    }
    scratch[tid] = (int32_t)(sum > 0x7FFFFFFF ? 0x7FFFFFFF : sum);
    return err;
}

// By one worker: exclusive sum of scratch[0, nt), nsub, and the workspace laid out for it.
X3DJ_HD static inline int seg_total(FrameCtx* C, int nt, int32_t* scratch) {
    int64_t run = 0;
    for (int t = 0; t < nt; ++t) {
        const int32_t v = scratch[t];
        scratch[t] = (int32_t)(run > 0x7FFFFFFF ? 0x7FFFFFFF : run);
        run += v;
    }
    if (run > 0x3FFFFFFF || workspace_need(run, C->nseg) > C->ws_bytes) return X3DJPEG_EINVAL;
    C->nsub = (int32_t)run;
    uint8_t* p = (uint8_t*)C->seg_first + align16(4 * (int64_t)C->nseg);
    C->sub_seg = (int32_t*)p;
    p += align16(4 * run);
    C->entry = (uint32_t*)p;
    p += align16(8 * run);
    C->exits = (uint32_t*)p;
    p += align16(8 * run);
    C->cnt = (int32_t*)p;
    C->head[1] = C->nsub;
    return X3DJPEG_OK;
}

X3DJ_HD static inline void seg_place(const FrameCtx& C, int tid, int nt, const int32_t* scratch) {
    int64_t lo, hi;
    chunk(C.nseg, tid, nt, &lo, &hi);
    int32_t at = scratch[tid];
    for (int64_t s = lo; s < hi; ++s) {
        const int32_t n = seg_nsub(C.segs[s].byte_len, C.sub_bits);
        C.seg_first[s] = at;
        for (int32_t j = 0; j < n; ++j) C.sub_seg[at + j] = (int32_t)s;
        at += n;
    }
}

enum { kRun = 0, kWrite = 1, kCheck = 2 };

// Decodes subsequence `local` of segment s (g: its table entry; last: it is the segment's last) from state (*p, *bk).
// kRun: until the subsequence ends; bad codes are skipped; *blocks gets the blocks completed.  kWrite: from an exact
// state, with first_block the index within the segment of the block the state is in; stores coefficients, stops at the
// subsequence's end or at the segment's last block (the last subsequence of a segment runs on until then), returns nonzero
// where the host decoder does.  kCheck: kWrite in every check and every state it leaves, without the stores (C.coef is
// not touched).
template <int MODE>
X3DJ_HD static inline int decode_span(const FrameCtx& C, int32_t s, const X3DJpegScanSeg g, int32_t local, bool last,
                                      uint32_t* p_io, uint32_t* bk_io, int32_t first_block, int32_t* blocks) {
    const uint32_t seg_bits = g.byte_len * 8u;
    const uint32_t end = last ? seg_bits : (uint32_t)(local + 1) * (uint32_t)C.sub_bits;
    const int32_t total = g.mcu_count * C.bpm;  // blocks of the segment
    Bits br;
    br.d = C.scan + g.byte_off;
    br.nbytes = g.byte_len;
    br.seek(*p_io);
    int b = (int)(*bk_io & 255u), k = (int)((*bk_io >> 8) & 255u);
    if (b >= C.bpm) b = 0;
    int32_t done = 0;
    // where the current block is stored (kWrite)
    int16_t* blk = nullptr;
    int32_t mcu = 0;
    auto locate = [&](int32_t block) -> bool {
        mcu = g.first_mcu + block / C.bpm;
        const int c = C.blk_comp[b];
        const int my = mcu / C.mcus_x, mx = mcu - my * C.mcus_x;
        const int64_t off = C.coef_off[c] +
                            ((int64_t)(my * C.comp_v[c] + C.blk_by[b]) * C.blocks_w[c] + (mx * C.comp_h[c] + C.blk_bx[b])) * 64;
        if (off < 0 || off + 64 > C.coef_count) return false;
        if (MODE == kWrite) blk = C.coef + off;
        return true;
    };
    if (MODE != kRun) {
        if (first_block >= total) return 0;  // the segment's blocks ended in an earlier subsequence
        if (!locate(first_block)) return X3DJPEG_EINVAL;
    }
    uint32_t p = br.bitpos();
    for (;;) {
        if (MODE != kRun) {
            if (last) {
                if (p > seg_bits) return X3DJPEG_ECORRUPT;  // scan data ends inside an MCU
            } else if (p >= end) {
                break;
            }
        } else if (p >= end) {
            break;
        }
        br.fill();
        const int c = C.blk_comp[b];
        bool bad = false;
        if (k == 0) {
            const int sym = decode_symbol(br, *C.dc[c]);
            if (sym < 0 || sym > 15) {
                bad = true;  // bad DC Huffman code
            } else {
                if (sym) {
                    const int bits = br.peek(sym);
                    br.skip(sym);
                    if (MODE == kWrite) blk[0] = (int16_t)extend(bits, sym);
                }
                k = 1;
            }
        } else {
            const int rs = decode_symbol(br, *C.ac[c]);
            if (rs < 0) {
                bad = true;  // bad AC Huffman code
            } else {
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    k = r == 15 ? k + 16 : 64;  // ZRL, or the end of the block
                } else {
                    k += r;
                    if (k > 63) {
                        bad = true;  // coefficient index past 63
                    } else {
                        const int bits = br.peek(sz);
                        br.skip(sz);
                        if (MODE == kWrite) blk[C.zigzag[k]] = (int16_t)extend(bits, sz);
                        ++k;
                    }
                }
            }
        }
        if (bad) {
            if (MODE != kRun) return X3DJPEG_ECORRUPT;
            br.seek(p + 1);
            k = 0;
        } else if (k >= 64) {
            k = 0;
            ++done;
            b = b + 1 == C.bpm ? 0 : b + 1;
            if (MODE != kRun) {
                if (first_block + done >= total) {
                    // the segment's last block: the host's checks at a restart marker and at the end of the scan
                    p = br.bitpos();
                    if (p > seg_bits) return X3DJPEG_ECORRUPT;                        // scan data ends inside an MCU
                    if (s + 1 < C.nseg && seg_bits - p >= 8) return X3DJPEG_ECORRUPT;  // data where a marker is due
                    break;
                }
                if (!locate(first_block + done)) return X3DJPEG_EINVAL;
            }
        }
        p = br.bitpos();
    }
    *p_io = p;
    *bk_io = (uint32_t)b | ((uint32_t)k << 8);
    *blocks = done;
    return 0;
}

// Subsequence i of the frame, through the workspace's subsequence -> segment map.
template <int MODE>
X3DJ_HD static inline int decode_sub(const FrameCtx& C, int32_t i, uint32_t* p_io, uint32_t* bk_io, int32_t first_block,
                                     int32_t* blocks) {
    const int32_t s = C.sub_seg[i];
    const X3DJpegScanSeg g = C.segs[s];
    const int32_t local = i - C.seg_first[s];
    const bool last = i + 1 == C.nsub || C.sub_seg[i + 1] != s;
    return decode_span<MODE>(C, s, g, local, last, p_io, bk_io, first_block, blocks);
}

X3DJ_HD static inline void run_sub(const FrameCtx& C, int32_t i) {
    uint32_t p = C.entry[2 * i], bk = C.entry[2 * i + 1] & ~kDirty;
    int32_t blocks = 0;
    decode_sub<kRun>(C, i, &p, &bk, 0, &blocks);
    C.exits[2 * i] = p;
    C.exits[2 * i + 1] = bk;
    C.cnt[i] = blocks;
}

X3DJ_HD static inline void init(const FrameCtx& C, int tid, int nt) {
    for (int32_t i = tid; i < C.nsub; i += nt) {
        const int32_t local = i - C.seg_first[C.sub_seg[i]];
        C.entry[2 * i] = (uint32_t)local * (uint32_t)C.sub_bits;
        C.entry[2 * i + 1] = 0;
        run_sub(C, i);
    }
}

// entry[i] takes exit[i - 1] where they differ.  Reads exits, writes the worker's own entries.  Nonzero if any changed.
X3DJ_HD static inline int relax_take(const FrameCtx& C, int tid, int nt) {
    int changed = 0;
    for (int32_t i = tid; i < C.nsub; i += nt) {
        if (i == 0 || C.sub_seg[i] != C.sub_seg[i - 1]) continue;
        const uint32_t p = C.exits[2 * i - 2], bk = C.exits[2 * i - 1];
        if (p != C.entry[2 * i] || bk != C.entry[2 * i + 1]) {
            C.entry[2 * i] = p;
            C.entry[2 * i + 1] = bk | kDirty;
            changed = 1;
        }
    }
    return changed;
}

// Reruns the changed ones.  Reads the worker's own entries, writes its own exits.
X3DJ_HD static inline void relax_run(const FrameCtx& C, int tid, int nt) {
    for (int32_t i = tid; i < C.nsub; i += nt) {
        if (!(C.entry[2 * i + 1] & kDirty)) continue;
        C.entry[2 * i + 1] &= ~kDirty;
        run_sub(C, i);
    }
}

// Segmented sums over contiguous chunks: a worker reduces its chunk to (flag: a segment starts in it, sum since the last
// start), one worker turns these into what each chunk starts from, the workers walk their chunks again.
X3DJ_HD static inline void carry_scan(int32_t* fs, int nt) {
    uint32_t carry = 0;
    for (int t = 0; t < nt; ++t) {
        const uint32_t sum = (uint32_t)fs[2 * t + 1];
        const bool flag = fs[2 * t] != 0;
        fs[2 * t + 1] = (int32_t)carry;
        carry = flag ? sum : carry + sum;
    }
}

X3DJ_HD static inline void count_sum(const FrameCtx& C, int tid, int nt, int32_t* scratch) {
    int64_t lo, hi;
    chunk(C.nsub, tid, nt, &lo, &hi);
    uint32_t sum = 0;
    int flag = 0;
    for (int64_t i = lo; i < hi; ++i) {
        if (i == 0 || C.sub_seg[i] != C.sub_seg[i - 1]) {
            flag = 1;
            sum = 0;
        }
        sum += (uint32_t)C.cnt[i];
    }
    scratch[2 * tid] = flag;
    scratch[2 * tid + 1] = (int32_t)sum;
}

X3DJ_HD static inline void count_place(const FrameCtx& C, int tid, int nt, const int32_t* scratch) {
    int64_t lo, hi;
    chunk(C.nsub, tid, nt, &lo, &hi);
    uint32_t at = (uint32_t)scratch[2 * tid + 1];
    for (int64_t i = lo; i < hi; ++i) {
        if (i == 0 || C.sub_seg[i] != C.sub_seg[i - 1]) at = 0;
        const uint32_t n = (uint32_t)C.cnt[i];
        C.cnt[i] = (int32_t)(at > 0x7FFFFFFFu ? 0x7FFFFFFFu : at);
        at += n;
    }
}

X3DJ_HD static inline void zero(const FrameCtx& C, int tid, int nt) {
    if (((uintptr_t)C.coef & 7) == 0) {  // coef_count is a multiple of 64
        uint64_t* q = (uint64_t*)C.coef;
        for (int64_t i = tid; i < C.coef_count / 4; i += nt) q[i] = 0;
    } else {
        for (int64_t i = tid; i < C.coef_count; i += nt) C.coef[i] = 0;
    }
}

X3DJ_HD static inline int write_coef(const FrameCtx& C, int tid, int nt) {
    int err = 0;
    for (int32_t i = tid; i < C.nsub; i += nt) {
        uint32_t p = C.entry[2 * i], bk = C.entry[2 * i + 1] & ~kDirty;
        int32_t blocks = 0;
        const int e = decode_sub<kWrite>(C, i, &p, &bk, C.cnt[i], &blocks);
        if (e && !err) err = e;
    }
    return err;
}

// element t of component c in scan order -> its block's DC coefficient; *start: a segment begins with it
X3DJ_HD static inline int16_t* dc_at(const FrameCtx& C, int c, int64_t t, bool* start) {
    const int hv = C.comp_h[c] * C.comp_v[c];
    const int32_t mcu = (int32_t)(t / hv), j = (int32_t)(t - (int64_t)mcu * hv);
    const int by = j / C.comp_h[c], bx = j - by * C.comp_h[c];
    const int my = mcu / C.mcus_x, mx = mcu - my * C.mcus_x;
    *start = j == 0 && (C.ri ? mcu % C.ri == 0 : mcu == 0);
    return C.coef + C.coef_off[c] + ((int64_t)(my * C.comp_v[c] + by) * C.blocks_w[c] + (mx * C.comp_h[c] + bx)) * 64;
}

X3DJ_HD static inline void dc_sum(const FrameCtx& C, int tid, int nt, int32_t* scratch) {
    for (int c = 0; c < C.ncomp; ++c) {
        int64_t lo, hi;
        chunk((int64_t)C.nmcu * C.comp_h[c] * C.comp_v[c], tid, nt, &lo, &hi);
        uint32_t sum = 0;
        int flag = 0;
        for (int64_t t = lo; t < hi; ++t) {
            bool start;
            const int16_t* q = dc_at(C, c, t, &start);
            if (start) {
                flag = 1;
                sum = 0;
            }
            sum += (uint32_t)(int32_t)*q;
        }
        scratch[2 * (c * nt + tid)] = flag;
        scratch[2 * (c * nt + tid) + 1] = (int32_t)sum;
    }
}

X3DJ_HD static inline void dc_place(const FrameCtx& C, int tid, int nt, const int32_t* scratch) {
    for (int c = 0; c < C.ncomp; ++c) {
        int64_t lo, hi;
        chunk((int64_t)C.nmcu * C.comp_h[c] * C.comp_v[c], tid, nt, &lo, &hi);
        uint32_t pred = (uint32_t)scratch[2 * (c * nt + tid) + 1];
        for (int64_t t = lo; t < hi; ++t) {
            bool start;
            int16_t* q = dc_at(C, c, t, &start);
            if (start) pred = 0;
            pred += (uint32_t)(int32_t)*q;
            *q = (int16_t)(uint16_t)(pred & 0xFFFFu);
        }
    }
}

}  // namespace x3dj
