// Stand-alone check of the parallel Huffman decoder's host code (csrc_jpeg/host.cpp, scan.cpp, entropy_core.h), built by
// tests/test_jpeg_entropy_host.py with -fsanitize=address,undefined and run as a child process.
//
//   jpeg_entropy_check <file>      file: uint32 count, then per case uint32 length and the bytes of a (possibly damaged) JPEG
//
// Every buffer is a heap block of exactly the size the library is told, so a read or write outside it stops the run.
// Per case and sub_bits: where x3djpeg_entropy_decode succeeds, prepare + x3djpeg_entropy_decode_parallel_host must give
// the same coefficients; where it fails with X3DJPEG_ECORRUPT, prepare or the status must fail too.
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

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const uint32_t count = rd32(f);
    const int sub_bits[3] = {32, 128, X3DJPEG_SUB_BITS_DEFAULT};
    long ok = 0, corrupt = 0, unparsed = 0, failures = 0;
    for (uint32_t n = 0; n < count; ++n) {
        const uint32_t len = rd32(f);
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(data, 1, len, f) != len) return 2;
        X3DJpegInfo info;
        if (x3djpeg_parse(data, len, &info) != X3DJPEG_OK) {
            ++unparsed;
            free(data);
            continue;
        }
        const size_t cc = (size_t)info.coef_count;
        int16_t* want = (int16_t*)malloc(cc * 2);
        const int rc = x3djpeg_entropy_decode(data, len, &info, want, cc * 2);
        rc == X3DJPEG_OK ? ++ok : ++corrupt;

        const size_t nmcu = (size_t)info.mcus_x * info.mcus_y;
        const size_t seg_cap = info.restart_interval ? (nmcu + info.restart_interval - 1) / info.restart_interval : 1;
        const size_t scan_cap = len - (size_t)info.scan_off + X3DJPEG_SCAN_PAD;
        uint8_t* scan = (uint8_t*)malloc(scan_cap);
        X3DJpegScanSeg* segs = (X3DJpegScanSeg*)malloc(seg_cap * sizeof(X3DJpegScanSeg));
        size_t scan_bytes = 0, nseg = 0;
        const int prc = x3djpeg_scan_prepare(data, len, &info, scan, scan_cap, segs, seg_cap, &scan_bytes, &nseg);
        if (prc != X3DJPEG_OK) {
            if (rc == X3DJPEG_OK || prc != X3DJPEG_ECORRUPT) {
                printf("case %u: prepare gives %d, the host decoder %d\n", n, prc, rc);
                ++failures;
            }
        } else {
            for (int k = 0; k < 3; ++k) {
                const size_t wsb = x3djpeg_entropy_workspace_bytes(scan_bytes, nseg, sub_bits[k]);
                void* ws = nullptr;
                if (posix_memalign(&ws, 16, wsb)) return 2;
                int16_t* got = (int16_t*)malloc(cc * 2);
                memset(got, 0x5A, cc * 2);
                X3DJpegScanJob job;
                memset(&job, 0, sizeof(job));
                job.scan = scan;
                job.segs = segs;
                job.coef = got;
                job.coef_count = info.coef_count;
                job.ws_off = 0;
                job.ws_bytes = (int64_t)wsb;
                job.scan_bytes = (int32_t)scan_bytes;
                job.nseg = (int32_t)nseg;
                job.ncomp = info.ncomp;
                job.mcus_x = info.mcus_x;
                job.mcus_y = info.mcus_y;
                job.restart_interval = info.restart_interval;
                for (int c = 0; c < 3; ++c) {
                    job.comp_h[c] = info.comp_h[c];
                    job.comp_v[c] = info.comp_v[c];
                    job.comp_td[c] = info.comp_td[c];
                    job.comp_ta[c] = info.comp_ta[c];
                    job.blocks_w[c] = info.blocks_w[c];
                    job.block_start[c] = info.block_start[c];
                }
                memcpy(job.huff_bits, info.huff_bits, sizeof(job.huff_bits));
                memcpy(job.huff_vals, info.huff_vals, sizeof(job.huff_vals));
                int32_t status = 77, rounds = -1;
                const int erc = x3djpeg_entropy_decode_parallel_host(&job, 1, sub_bits[k], ws, wsb, &status, &rounds);
                bool good = erc == X3DJPEG_OK && rounds >= 1 && rounds <= ((int32_t*)ws)[1];
                if (rc == X3DJPEG_OK)
                    good = good && status == 0 && memcmp(got, want, cc * 2) == 0;
                else
                    good = good && status == X3DJPEG_ECORRUPT;
                if (!good) {
                    printf("case %u sub_bits %d: host %d, call %d, status %d, rounds %d\n", n, sub_bits[k], rc, erc, status,
                           rounds);
                    ++failures;
                }
                free(got);
                free(ws);
            }
        }
        free(segs);
        free(scan);
        free(want);
        free(data);
    }
    fclose(f);
    printf("cases %u ok %ld corrupt %ld unparsed %ld failures %ld\n", count, ok, corrupt, unparsed, failures);
    return failures ? 1 : 0;
}
