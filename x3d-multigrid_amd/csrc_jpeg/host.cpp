// Host stage of libx3djpeg (include/x3djpeg.h): marker parsing and Huffman decoding.  Plain C++, no HIP call, no global
// state besides the thread-local error message, so that several threads decode different frames at once.
//
// Every read of the file goes through a bounds check against `len`; every coefficient store is inside the frame's
// nblocks * 64 elements by construction (block indices come from the MCU loops over the parsed block counts, the
// position inside a block is checked against 63).  A stream that asks for bits the file does not hold is ECORRUPT: no
// zero-padding recovery as libjpeg has it.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "../../include/x3djpeg.h"

static thread_local char g_err[512] = "";

void x3djpeg_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* x3djpeg_last_error(void) { return g_err; }
extern "C" int x3djpeg_abi_version(void) { return X3DJPEG_ABI_VERSION; }
extern "C" size_t x3djpeg_info_bytes(void) { return sizeof(X3DJpegInfo); }
extern "C" size_t x3djpeg_frame_job_bytes(void) { return sizeof(X3DJpegFrameJob); }

namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

int corrupt(const char* what) {
    x3djpeg_set_error("corrupt JPEG: %s", what);
    return X3DJPEG_ECORRUPT;
}

int unsupported(const char* what) {
    x3djpeg_set_error("unsupported JPEG: %s", what);
    return X3DJPEG_EUNSUPPORTED;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

}  // namespace

extern "C" int x3djpeg_parse(const uint8_t* d, size_t len, X3DJpegInfo* info) {
    if (!d || !info) {
        x3djpeg_set_error("x3djpeg_parse: null pointer");
        return X3DJPEG_EINVAL;
    }
    memset(info, 0, sizeof(*info));
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) return corrupt("no SOI marker");
    size_t pos = 2;
    int adobe_transform = -1, comp_id[3] = {0, 0, 0};
    bool have_sof = false;
    for (;;) {
        if (pos + 4 > len) return corrupt("file ends before the scan");
        if (d[pos] != 0xFF) return corrupt("marker expected");
        const int m = d[pos + 1];
        if (m == 0xFF) {  // fill byte
            ++pos;
            continue;
        }
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) {  // markers without a segment
            pos += 2;
            continue;
        }
        if (m == 0xD9) return corrupt("EOI before the scan");
        const size_t L = ((size_t)d[pos + 2] << 8) | d[pos + 3];
        if (L < 2 || pos + 2 + L > len) return corrupt("segment runs past the end of the file");
        const uint8_t* s = d + pos + 4;
        const size_t n = L - 2;
        pos += 2 + L;
        if (m == 0xDB) {  // DQT
            size_t i = 0;
            while (i < n) {
                const int pq = s[i] >> 4, tq = s[i] & 15;
                ++i;
                if (pq > 1 || tq > 3) return corrupt("quantisation table header");
                const size_t need = pq ? 128 : 64;
                if (i + need > n) return corrupt("quantisation table runs past its segment");
                for (int k = 0; k < 64; ++k)
                    info->qt[tq][kZigzag[k]] = pq ? (uint16_t)((s[i + 2 * k] << 8) | s[i + 2 * k + 1]) : s[i + k];
                info->qt_set[tq] = 1;
                i += need;
            }
        } else if (m == 0xC0 || m == 0xC1) {  // SOF0 / SOF1
            if (have_sof) return corrupt("two frame headers");
            if (n < 6) return corrupt("frame header too short");
            if (s[0] == 12) return unsupported("12-bit samples");
            if (s[0] != 8) return unsupported("sample precision other than 8 bits");
            info->height = (s[1] << 8) | s[2];
            info->width = (s[3] << 8) | s[4];
            const int nc = s[5];
            if (nc == 4) return unsupported("4 components (CMYK / YCCK)");
            if (nc != 1 && nc != 3) return unsupported("component count other than 1 or 3");
            if (n < (size_t)(6 + 3 * nc)) return corrupt("frame header too short");
            if (info->width == 0) return corrupt("zero width");
            if (info->height == 0) return unsupported("height given by a DNL marker");
            info->ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = s[6 + 3 * c];
                info->comp_h[c] = s[7 + 3 * c] >> 4;
                info->comp_v[c] = s[7 + 3 * c] & 15;
                info->comp_tq[c] = s[8 + 3 * c];
                if (info->comp_tq[c] > 3) return corrupt("quantisation table index");
                if (info->comp_h[c] < 1 || info->comp_h[c] > 4 || info->comp_v[c] < 1 || info->comp_v[c] > 4)
                    return corrupt("sampling factor");
            }
            have_sof = true;
        } else if (m == 0xC2) {
            return unsupported("progressive (SOF2)");
        } else if (m == 0xC3 || m == 0xC7 || m == 0xCB || m == 0xCF) {
            return unsupported("lossless");
        } else if (m == 0xC5 || m == 0xC6) {
            return unsupported("hierarchical (differential frames)");
        } else if (m == 0xC9 || m == 0xCA || m == 0xCD || m == 0xCE || m == 0xCC) {
            return unsupported("arithmetic coding");
        } else if (m == 0xC4) {  // DHT
            size_t i = 0;
            while (i < n) {
                const int tc = s[i] >> 4, th = s[i] & 15;
                if (tc > 1 || th > 3) return corrupt("Huffman table header");
                if (i + 17 > n) return corrupt("Huffman table runs past its segment");
                int total = 0;
                for (int k = 0; k < 16; ++k) total += s[i + 1 + k];
                if (total > 256 || i + 17 + total > n) return corrupt("Huffman table runs past its segment");
                const int t = tc * 4 + th;
                memcpy(info->huff_bits[t], s + i + 1, 16);
                memset(info->huff_vals[t], 0, 256);
                memcpy(info->huff_vals[t], s + i + 17, total);
                info->huff_set[t] = 1;
                i += 17 + total;
            }
        } else if (m == 0xDD) {  // DRI
            if (n < 2) return corrupt("restart interval segment too short");
            info->restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xEE) {  // APP14
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) adobe_transform = s[11];
        } else if (m == 0xDA) {  // SOS
            if (!have_sof) return corrupt("scan before the frame header");
            if (n < 1) return corrupt("scan header too short");
            const int ns = s[0];
            if (ns < 1 || ns > 4) return corrupt("scan component count");
            if (ns != info->ncomp) return unsupported("multi-scan file (a scan that does not hold all components)");
            if (n < (size_t)(1 + 2 * ns + 3)) return corrupt("scan header too short");
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return unsupported("scan components out of frame order");
                info->comp_td[c] = s[2 + 2 * c] >> 4;
                info->comp_ta[c] = s[2 + 2 * c] & 15;
                if (info->comp_td[c] > 3 || info->comp_ta[c] > 3) return corrupt("Huffman table index");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return unsupported("spectral selection / successive approximation in a sequential scan");
            break;
        }
        // everything else (APPn, COM, ...) is skipped
    }
    const int nc = info->ncomp;
    if (nc == 1) {
        info->comp_h[0] = info->comp_v[0] = 1;  // a single-component scan is never interleaved: one block per MCU
    } else {
        if (adobe_transform >= 0 && adobe_transform != 1) return unsupported("Adobe APP14 colour transform other than YCbCr");
        if (adobe_transform < 0 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
            return unsupported("RGB colour space");
        const int h = info->comp_h[0], v = info->comp_v[0];
        const bool luma_ok = (h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2);
        if (!luma_ok || info->comp_h[1] != 1 || info->comp_v[1] != 1 || info->comp_h[2] != 1 || info->comp_v[2] != 1)
            return unsupported("sampling factors other than 4:4:4, 4:2:2 (2x1) and 4:2:0 (2x2)");
    }
    info->hmax = info->comp_h[0];
    info->vmax = info->comp_v[0];
    info->mcus_x = cdiv(info->width, 8 * info->hmax);
    info->mcus_y = cdiv(info->height, 8 * info->vmax);
    int nb = 0;
    for (int c = 0; c < nc; ++c) {
        if (!info->qt_set[info->comp_tq[c]]) return corrupt("quantisation table missing");
        if (!info->huff_set[info->comp_td[c]] || !info->huff_set[4 + info->comp_ta[c]]) return corrupt("Huffman table missing");
        info->blocks_w[c] = info->mcus_x * info->comp_h[c];
        info->blocks_h[c] = info->mcus_y * info->comp_v[c];
        info->cw[c] = cdiv(info->width * info->comp_h[c], info->hmax);
        info->ch[c] = cdiv(info->height * info->comp_v[c], info->vmax);
        info->block_start[c] = nb;
        info->coef_off[c] = (int64_t)nb * 64;
        nb += info->blocks_w[c] * info->blocks_h[c];  // <= 3 * 8192 * 8192 / ... : width, height <= 65535 keeps it in int32
    }
    info->nblocks = nb;
    info->coef_count = (int64_t)nb * 64;
    info->scan_off = (int64_t)pos;
    return X3DJPEG_OK;
}

namespace {

// Huffman table in libjpeg's form: a 9-bit lookahead table for the short codes, maxcode / valoffset for the rest.
struct HuffTable {
    static constexpr int LOOK = 9;
    uint16_t look[1 << LOOK];  // (length << 8) | symbol; 0: longer than LOOK bits
    int32_t maxcode[18];       // largest code of each length, -1 if none; [17] is a sentinel
    int32_t valoff[17];        // index of the first value of the length minus its first code
    uint8_t vals[256];
};

bool build_table(const uint8_t* bits, const uint8_t* vals, HuffTable* t) {
    memset(t->look, 0, sizeof(t->look));
    memcpy(t->vals, vals, 256);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = bits[l - 1];
        if (code + n > (1 << l)) return false;  // more codes than the length holds
        t->valoff[l] = k - code;
        if (n) {
            if (l <= HuffTable::LOOK) {
                for (int i = 0; i < n; ++i) {
                    const int first = (code + i) << (HuffTable::LOOK - l);
                    for (int j = 0; j < (1 << (HuffTable::LOOK - l)); ++j)
                        t->look[first + j] = (uint16_t)((l << 8) | vals[k + i]);
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

// Bit reader over the entropy-coded segment: removes byte stuffing, stops at a marker or at the end of the file and
// then feeds zero bits, counted in `fake`, so that a caller that consumed any of them can tell.
struct BitReader {
    const uint8_t* d;
    size_t pos, len;
    uint64_t acc = 0;  // the low `n` bits are valid
    int n = 0;
    int fake = 0;      // zero bits appended after the data ran out that are still in acc

    void fill() {
        while (n <= 56) {
            int b = 0;
            if (pos < len) {
                b = d[pos];
                if (b == 0xFF) {
                    if (pos + 1 < len && d[pos + 1] == 0x00) {
                        pos += 2;  // a stuffed 0xFF
                    } else {
                        b = -1;    // a marker (or the end of the file): stay on it
                    }
                } else {
                    ++pos;
                }
            } else {
                b = -1;
            }
            if (b < 0) {
                acc <<= 8;
                fake += 8;
            } else {
                acc = (acc << 8) | (uint64_t)b;
            }
            n += 8;
        }
    }
    // true when bits beyond the data were consumed
    bool overrun() const { return fake > n; }
    inline int peek(int k) { return (int)((acc >> (n - k)) & ((1u << k) - 1)); }
    inline void skip(int k) { n -= k; }
};

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// one symbol; -1 for a code no length matches.  Needs >= 16 bits in the reader.
inline int decode_symbol(BitReader& br, const HuffTable& t) {
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

}  // namespace

extern "C" int x3djpeg_entropy_decode(const uint8_t* d, size_t len, const X3DJpegInfo* info, int16_t* coef,
                                      size_t coef_bytes) {
    if (!d || !info || !coef) {
        x3djpeg_set_error("x3djpeg_entropy_decode: null pointer");
        return X3DJPEG_EINVAL;
    }
    const int nc = info->ncomp;
    // the info must be what x3djpeg_parse wrote: re-derive what the loops below rely on
    bool ok = (nc == 1 || nc == 3) && info->mcus_x > 0 && info->mcus_y > 0 && info->scan_off >= 0 &&
              (uint64_t)info->scan_off <= len;
    int64_t nb = 0;
    for (int c = 0; ok && c < nc; ++c) {
        ok = info->comp_h[c] >= 1 && info->comp_h[c] <= 2 && info->comp_v[c] >= 1 && info->comp_v[c] <= 2 &&
             info->blocks_w[c] == info->mcus_x * info->comp_h[c] && info->blocks_h[c] == info->mcus_y * info->comp_v[c] &&
             info->block_start[c] == nb && info->coef_off[c] == nb * 64 && info->comp_td[c] >= 0 && info->comp_td[c] <= 3 && info->comp_ta[c] >= 0 &&
             info->comp_ta[c] <= 3 && info->mcus_x <= 8192 && info->mcus_y <= 8192;
        if (ok) nb += (int64_t)info->blocks_w[c] * info->blocks_h[c];
    }
    if (!ok || nb != info->nblocks || info->coef_count != nb * 64) {
        x3djpeg_set_error("x3djpeg_entropy_decode: info is not what x3djpeg_parse wrote");
        return X3DJPEG_EINVAL;
    }
    if (coef_bytes < (size_t)info->coef_count * sizeof(int16_t)) {
        x3djpeg_set_error("x3djpeg_entropy_decode: coefficient buffer of %zu bytes, %lld needed", coef_bytes,
                          (long long)info->coef_count * 2);
        return X3DJPEG_EINVAL;
    }
    memset(coef, 0, (size_t)info->coef_count * sizeof(int16_t));

    HuffTable dc[3], ac[3];
    for (int c = 0; c < nc; ++c) {
        const int td = info->comp_td[c], ta = 4 + info->comp_ta[c];
        if (!build_table(info->huff_bits[td], info->huff_vals[td], &dc[c]) ||
            !build_table(info->huff_bits[ta], info->huff_vals[ta], &ac[c]))
            return corrupt("over-subscribed Huffman table");
    }

    BitReader br{d, (size_t)info->scan_off, len};
    int pred[3] = {0, 0, 0};
    const int ri = info->restart_interval;
    int64_t mcu = 0;
    for (int my = 0; my < info->mcus_y; ++my) {
        for (int mx = 0; mx < info->mcus_x; ++mx, ++mcu) {
            if (ri && mcu && mcu % ri == 0) {
                // the reader sits on the marker once the bits before it are used up (the rest of the last byte is padding)
                if (br.overrun()) return corrupt("scan data ends inside an MCU");
                br.fill();
                if (br.n - br.fake >= 8) return corrupt("data where a restart marker is expected");
                size_t p = br.pos;
                while (p + 1 < len && d[p] == 0xFF && d[p + 1] == 0xFF) ++p;
                if (p + 2 > len || d[p] != 0xFF || d[p + 1] != 0xD0 + (int)((mcu / ri - 1) & 7))
                    return corrupt("restart marker missing");
                br.pos = p + 2;
                br.acc = 0;
                br.n = br.fake = 0;
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < nc; ++c) {
                const int bw = info->blocks_w[c], h = info->comp_h[c], v = info->comp_v[c];
                int16_t* base = coef + info->coef_off[c];
                for (int by = 0; by < v; ++by) {
                    for (int bx = 0; bx < h; ++bx) {
                        int16_t* blk = base + ((size_t)(my * v + by) * bw + (mx * h + bx)) * 64;
                        br.fill();
                        int s = decode_symbol(br, dc[c]);
                        if (s < 0 || s > 15) return corrupt("bad DC Huffman code");
                        if (s) {
                            br.fill();
                            const int bits = br.peek(s);
                            br.skip(s);
                            pred[c] = (int16_t)(pred[c] + extend(bits, s));
                        }
                        blk[0] = (int16_t)pred[c];
                        int k = 1;
                        while (k < 64) {
                            br.fill();  // >= 57 bits: a code (<= 16) and its value bits (<= 15) fit
                            const int rs = decode_symbol(br, ac[c]);
                            if (rs < 0) return corrupt("bad AC Huffman code");
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;  // end of block
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) return corrupt("coefficient index past 63");
                            const int bits = br.peek(s);
                            br.skip(s);
                            blk[kZigzag[k]] = (int16_t)extend(bits, s);
                            ++k;
                        }
                        if (br.overrun()) return corrupt("scan data ends inside an MCU");
                    }
                }
            }
        }
    }
    return X3DJPEG_OK;
}
