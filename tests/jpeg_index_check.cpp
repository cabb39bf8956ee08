// Stand-alone check of the sync index's host code (csrc_jpeg/host.cpp, scan.cpp, index_host.cpp, index_core.h,
// entropy_core.h), built by tests/test_jpeg_index_host.py with -fsanitize=address,undefined and run as a child process.
//
//   jpeg_index_check <file>      file: uint32 count, then per case int32 base, uint32 length and the bytes of a JPEG.
//                                base -1: a good file, decoded with its own index; base >= 0: a damaged copy of case
//                                `base` (a good one, earlier in the file), decoded with the index of that good file
//
// Every buffer is a heap block of exactly the size the library is told, so a read or write outside it stops the run.
// Good file, per index_bits: x3djpeg_index_build gives x3djpeg_index_count entries, x3djpeg_entropy_decode_indexed_host
// gives status 0 and the coefficients of x3djpeg_entropy_decode, and with one bit of the entries flipped it gives
// X3DJPEG_EINDEX.  Damaged file: x3djpeg_index_build fails exactly where x3djpeg_entropy_decode does; decoded with the
// stale index, whenever the status is 0 the coefficients are those of x3djpeg_entropy_decode_parallel_host.
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

// one heap block of exactly n elements (at least one byte), 8-byte aligned by malloc
template <typename T>
static T* block(size_t n) {
    T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
    if (!p) exit(2);
    return p;
}

struct Prepared {
    bool ok = false;
    X3DJpegInfo info;
    uint8_t* scan = nullptr;
    X3DJpegScanSeg* segs = nullptr;
    size_t scan_bytes = 0, nseg = 0;
};

static Prepared prepare(const uint8_t* data, uint32_t len, const X3DJpegInfo& info, int* rc_out) {
    Prepared P;
    P.info = info;
    const size_t nmcu = (size_t)info.mcus_x * info.mcus_y;
    const size_t seg_cap = info.restart_interval ? (nmcu + info.restart_interval - 1) / info.restart_interval : 1;
    const size_t scan_cap = len - (size_t)info.scan_off + X3DJPEG_SCAN_PAD;
    P.scan = block<uint8_t>(scan_cap);
    P.segs = block<X3DJpegScanSeg>(seg_cap);
    *rc_out = x3djpeg_scan_prepare(data, len, &info, P.scan, scan_cap, P.segs, seg_cap, &P.scan_bytes, &P.nseg);
    P.ok = *rc_out == X3DJPEG_OK;
    return P;
}

static X3DJpegScanJob job_of(const Prepared& P, int16_t* coef) {
    X3DJpegScanJob job;
    memset(&job, 0, sizeof(job));
    job.scan = P.scan;
    job.segs = P.segs;
    job.coef = coef;
    job.coef_count = P.info.coef_count;
    job.scan_bytes = (int32_t)P.scan_bytes;
    job.nseg = (int32_t)P.nseg;
    job.ncomp = P.info.ncomp;
    job.mcus_x = P.info.mcus_x;
    job.mcus_y = P.info.mcus_y;
    job.restart_interval = P.info.restart_interval;
    for (int c = 0; c < 3; ++c) {
        job.comp_h[c] = P.info.comp_h[c];
        job.comp_v[c] = P.info.comp_v[c];
        job.comp_td[c] = P.info.comp_td[c];
        job.comp_ta[c] = P.info.comp_ta[c];
        job.blocks_w[c] = P.info.blocks_w[c];
        job.block_start[c] = P.info.block_start[c];
    }
    memcpy(job.huff_bits, P.info.huff_bits, sizeof(job.huff_bits));
    memcpy(job.huff_vals, P.info.huff_vals, sizeof(job.huff_vals));
    return job;
}

struct Index {
    uint64_t* entries = nullptr;
    size_t n = 0;
};

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    const int bits[3] = {32, 128, 1024};
    long good = 0, stale = 0, stale_zero = 0, flips = 0, unparsed = 0, failures = 0;
    std::vector<Prepared> kept(count);
    std::vector<Index> index(3 * (size_t)count);
    for (uint32_t n = 0; n < count; ++n) {
        const int32_t base = (int32_t)rd32(f);
        const uint32_t len = rd32(f);
        uint8_t* data = block<uint8_t>(len);
        if (len && fread(data, 1, len, f) != len) return 2;
        X3DJpegInfo info;
        if (x3djpeg_parse(data, len, &info) != X3DJPEG_OK) {
            ++unparsed;
            free(data);
            continue;
        }
        const size_t cc = (size_t)info.coef_count;
        int16_t* want = block<int16_t>(cc);
        const int rc = x3djpeg_entropy_decode(data, len, &info, want, cc * 2);
        int prc = 0;
        Prepared P = prepare(data, len, info, &prc);
        if (base >= 0 && ((uint32_t)base >= n || !kept[base].ok)) return 2;
        for (int k = 0; k < 3 && P.ok; ++k) {
            // the index of this very scan: fails exactly where the host decoder does
            const size_t cap = x3djpeg_index_count(P.segs, P.nseg, bits[k]);
            uint64_t* own = block<uint64_t>(cap);
            size_t wrote = 0;
            const int irc = x3djpeg_index_build(P.scan, P.scan_bytes, P.segs, P.nseg, &info, bits[k], own, cap, &wrote);
            if ((irc == X3DJPEG_OK) != (rc == X3DJPEG_OK) || (irc != X3DJPEG_OK && irc != X3DJPEG_ECORRUPT) ||
                (irc == X3DJPEG_OK && wrote != cap) || cap == 0) {
                printf("case %u index_bits %d: the indexer gives %d (%zu of %zu entries), the host decoder %d\n", n, bits[k],
                       irc, wrote, cap, rc);
                ++failures;
            }
            const Index use = base < 0 ? Index{own, cap} : index[3 * (size_t)base + k];
            if (base < 0 && irc != X3DJPEG_OK) {
                free(own);
                continue;
            }
            int16_t* got = block<int16_t>(cc);
            memset(got, 0x5A, cc * 2);
            X3DJpegScanJob job = job_of(P, got);
            X3DJpegIndexRec rec = {0, (int32_t)use.n, 0};
            int32_t id = 0, status = 77;
            int erc = x3djpeg_entropy_decode_indexed_host(&job, 1, &id, &rec, 1, use.entries, use.n, bits[k], &status);
            if (base < 0) {
                ++good;
                if (erc != X3DJPEG_OK || status != 0 || memcmp(got, want, cc * 2) != 0) {
                    printf("case %u index_bits %d: call %d, status %d with its own index\n", n, bits[k], erc, status);
                    ++failures;
                }
                // one flipped bit of the entries, in a copy: the same call must report it
                uint64_t* bad = block<uint64_t>(cap);
                memcpy(bad, own, cap * 8);
                const size_t bit = ((size_t)n * 2654435761u + (size_t)k * 40503u) % (cap * 64);
                bad[bit / 64] ^= (uint64_t)1 << (bit % 64);
                status = 77;
                erc = x3djpeg_entropy_decode_indexed_host(&job, 1, &id, &rec, 1, bad, cap, bits[k], &status);
                ++flips;
                if (erc != X3DJPEG_OK || status != X3DJPEG_EINDEX) {
                    printf("case %u index_bits %d: bit %zu flipped gives call %d, status %d\n", n, bits[k], bit, erc, status);
                    ++failures;
                }
                free(bad);
                index[3 * (size_t)n + k] = Index{own, cap};
            } else {
                ++stale;
                if (erc != X3DJPEG_OK) {
                    printf("case %u index_bits %d: call %d with a stale index\n", n, bits[k], erc);
                    ++failures;
                } else if (status == 0) {
                    ++stale_zero;
                    const size_t wsb = x3djpeg_entropy_workspace_bytes(P.scan_bytes, P.nseg, bits[k]);
                    void* ws = nullptr;
                    if (posix_memalign(&ws, 16, wsb)) return 2;
                    int16_t* ref = block<int16_t>(cc);
                    memset(ref, 0x5A, cc * 2);
                    X3DJpegScanJob rjob = job_of(P, ref);
                    rjob.ws_bytes = (int64_t)wsb;
                    int32_t rstatus = 77;
                    const int prc2 = x3djpeg_entropy_decode_parallel_host(&rjob, 1, bits[k], ws, wsb, &rstatus, nullptr);
                    if (prc2 != X3DJPEG_OK || rstatus != 0 || memcmp(got, ref, cc * 2) != 0) {
                        printf("case %u index_bits %d: status 0 with a stale index, the relaxation decoder gives %d\n", n,
                               bits[k], rstatus);
                        ++failures;
                    }
                    free(ref);
                    free(ws);
                }
                free(own);
            }
            free(got);
        }
        if (base < 0 && P.ok) {
            kept[n] = P;
        } else {
            free(P.scan);
            free(P.segs);
        }
        free(want);
        free(data);
    }
    fclose(f);
    for (Prepared& P : kept) {
        free(P.scan);
        free(P.segs);
    }
    for (Index& I : index) free(I.entries);
    printf("cases %u good %ld flips %ld stale %ld zero %ld unparsed %ld failures %ld\n", count, good, flips, stale, stale_zero,
           unparsed, failures);
    return failures ? 1 : 0;
}
