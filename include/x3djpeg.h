/*
 * x3djpeg.h -- C ABI of libx3djpeg.so: a baseline JPEG decoder for the frame folders the reference reads with PIL
 * (kinetics.py:43-51), bit-exact with Pillow's libjpeg-turbo.  Hybrid: the serial part (marker parsing, Huffman decoding)
 * is plain C++ on the host, callable from several threads at once; everything per pixel (dequantisation, the "islow"
 * integer IDCT, "fancy" chroma upsampling, YCbCr -> RGB) runs as two HIP kernels (gfx950 / MI355X) per batch of frames,
 * which store straight into the caller's uint8 [H, W, 3] frames.
 *
 * A separate library from libx3dhip.so on purpose: tools/stamp.py and the gradient-hash record hash the training library's
 * sources, and nothing here runs inside a training step.
 *
 * Conventions (as include/x3ddata.h)
 *   - plain pointers and sizes; the caller owns every buffer; every kernel is enqueued on the hipStream_t passed as
 *     `stream`; no device entry point allocates or synchronises
 *   - return 0 on success, negative X3DJPEG_E* on failure; x3djpeg_last_error() gives the message (thread-local)
 *   - the host stage keeps no global state and makes no HIP call; it never reads outside [bytes, bytes + len) and never
 *     writes outside the coefficient buffer it is given
 *   - deterministic bit for bit: every output byte is written exactly once by a plain vector store
 *
 * Accepted files: SOF0 / SOF1 with 8-bit samples, Huffman coded, one interleaved scan; 1 component (greyscale, written to
 * all three channels) or 3 components (YCbCr) with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; restart intervals;
 * 8- and 16-bit quantisation tables.  Everything else is X3DJPEG_EUNSUPPORTED with the feature named in the message.
 *
 * Coefficients: int16 in natural (de-zigzagged) order, per component [blocks_h][blocks_w][64] with the block counts
 * padded to whole MCUs, the components one after the other (coef_off).  Planes: uint8, per component
 * [blocks_h * 8][blocks_w * 8], the components one after the other: block b of a frame has its coefficients at element
 * 64 * b and its component's plane starts at byte 64 * block_start.
 *
 * Huffman decoding has two paths that fill the same coefficient buffer bit for bit.  x3djpeg_entropy_decode is the serial
 * host decoder.  The device path: x3djpeg_scan_prepare (host, one pass over the file) removes the byte stuffing and the
 * restart markers and cuts the scan into one segment per restart interval; x3djpeg_entropy_decode_batch decodes a batch,
 * one workgroup per frame, by many decoders that start at fixed bit offsets (every sub_bits bits of a segment) and are
 * relaxed until each starts in the state its predecessor ended in (JPEG Huffman streams self-synchronise; Weissenberger
 * & Schmidt, "Accelerating JPEG decompression on GPUs").  x3djpeg_entropy_decode_parallel_host runs the same scheme
 * through the same code (csrc_jpeg/entropy_core.h) serially on the CPU.  For frames that are stored, the states the
 * relaxation converges to can be computed once and kept (x3djpeg_index_build): x3djpeg_entropy_decode_indexed then fills
 * the same buffer in one pass and checks the index as it goes ("Sync index" below).
 */
#ifndef X3DJPEG_H
#define X3DJPEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X3DJPEG_ABI_VERSION 2

#define X3DJPEG_OK 0
#define X3DJPEG_EINVAL (-1)        /* bad shape / null pointer / buffer too small */
#define X3DJPEG_ELAUNCH (-2)       /* hipLaunch error */
#define X3DJPEG_EUNSUPPORTED (-3)  /* a valid file of a kind this decoder does not take; the message names the feature */
#define X3DJPEG_ECORRUPT (-4)      /* truncated or inconsistent stream */
#define X3DJPEG_EINDEX (-5)        /* a sync index that does not describe the scan it is used with */

/* What x3djpeg_parse reads from the headers of one file. */
typedef struct X3DJpegInfo {
    int32_t width, height, ncomp;
    int32_t hmax, vmax;          /* the luma sampling factors */
    int32_t mcus_x, mcus_y;
    int32_t restart_interval;    /* in MCUs; 0: none */
    int32_t comp_h[3], comp_v[3], comp_tq[3], comp_td[3], comp_ta[3];
    int32_t blocks_w[3], blocks_h[3];   /* padded to whole MCUs */
    int32_t cw[3], ch[3];               /* the component's true size: ceil(width * h / hmax), ceil(height * v / vmax) */
    int32_t block_start[3];             /* first block of the component among the frame's blocks */
    int32_t nblocks;                    /* of all components */
    int64_t coef_off[3];                /* in int16 elements: 64 * block_start */
    int64_t coef_count;                 /* int16 elements of the frame: 64 * nblocks */
    int64_t scan_off;                   /* byte offset of the entropy-coded data */
    uint16_t qt[4][64];                 /* natural order */
    uint8_t huff_bits[8][16];           /* [class * 4 + id][length - 1]: codes per length (class 0 DC, 1 AC) */
    uint8_t huff_vals[8][256];
    uint8_t qt_set[4];
    uint8_t huff_set[8];
    uint8_t pad[4];
} X3DJpegInfo;

/* One frame of a batch, on the device. */
typedef struct X3DJpegFrameJob {
    const int16_t* coef;   /* the frame's coefficients (nblocks * 64) */
    uint8_t* planes;       /* the frame's planes (nblocks * 64 bytes) */
    uint8_t* dst;          /* uint8 [height][width][3]; only bytes [0, 3 * width) of each row are written */
    int64_t dst_stride;    /* bytes between rows, >= 3 * width */
    int32_t width, height, ncomp, hmax, vmax, nblocks;
    int32_t blocks_w[3], blocks_h[3], cw[3], ch[3], block_start[3];
    int32_t pad[3];        /* qt is 16-byte aligned, the struct 512 bytes */
    uint16_t qt[3][64];    /* per component, natural order */
} X3DJpegFrameJob;

/* One restart interval of a prepared scan (a file without DRI has one).  Its bit length is 8 * byte_len: the decoder
 * ignores the pad bits of the last byte. */
typedef struct X3DJpegScanSeg {
    uint32_t byte_off, byte_len;   /* in the frame's unstuffed scan bytes */
    int32_t first_mcu, mcu_count;
} X3DJpegScanSeg;

#define X3DJPEG_SCAN_PAD 16               /* zero bytes x3djpeg_scan_prepare appends to the unstuffed scan */
#define X3DJPEG_SCAN_MAX_BYTES (1 << 27)  /* largest scan the parallel path takes: bit positions stay below 2^30 */
#define X3DJPEG_SUB_BITS_DEFAULT 1024     /* profiles/jpeg_entropy/README.md */

/* One frame of a batch of x3djpeg_entropy_decode_batch, on the device (host pointers for ..._parallel_host). */
typedef struct X3DJpegScanJob {
    const uint8_t* scan;           /* what x3djpeg_scan_prepare wrote: scan_bytes bytes and X3DJPEG_SCAN_PAD zeros */
    const X3DJpegScanSeg* segs;    /* nseg entries */
    int16_t* coef;                 /* the frame's coefficients (coef_count elements), written in full */
    int64_t coef_count;
    int64_t ws_off, ws_bytes;      /* the frame's part of the workspace: ws_off a multiple of 16, ws_bytes at least
                                      x3djpeg_entropy_workspace_bytes(scan_bytes, nseg, sub_bits) */
    int32_t scan_bytes, nseg;
    int32_t ncomp, mcus_x, mcus_y, restart_interval;
    int32_t comp_h[3], comp_v[3], comp_td[3], comp_ta[3], blocks_w[3], block_start[3];
    uint8_t huff_bits[8][16];      /* as in X3DJpegInfo */
    uint8_t huff_vals[8][256];
} X3DJpegScanJob;

/* Frame store: frames kept on the device in the form the device path decodes from -- the output of x3djpeg_scan_prepare
 * and its segment table, in arena chunks that are never moved -- so that a batch's two job tables can be built on the
 * device from a list of frame ids (x3djpeg_store_build_jobs).  The caller fills all three tables with plain copies. */

/* What a frame's jobs take from its headers, laid out as the jobs themselves: `frame` and `scan` are the two job structs
 * with every pointer, dst_stride, ws_off, ws_bytes, scan_bytes and nseg zero (scan.coef_count is set).  Frames with equal
 * headers share one entry.  16-byte aligned, a multiple of 16 bytes. */
typedef struct X3DJpegStoreHeader {
    X3DJpegFrameJob frame;
    X3DJpegScanJob scan;
} X3DJpegStoreHeader;

/* One stored frame: device addresses (16-byte aligned) of its prepared scan and segment table. */
typedef struct X3DJpegStoreRec {
    const uint8_t* scan;           /* scan_bytes bytes and X3DJPEG_SCAN_PAD zeros */
    const X3DJpegScanSeg* segs;    /* nseg entries */
    int32_t scan_bytes, nseg;
    int32_t header;                /* index into the header table */
    int32_t pad;
} X3DJpegStoreRec;

/* Where one request of a batch is decoded to. */
typedef struct X3DJpegStoreDst {
    uint8_t* dst;                  /* as X3DJpegFrameJob.dst */
    int64_t dst_stride;
    int32_t width, height;         /* the size the caller expects; a frame of another size is refused */
} X3DJpegStoreDst;

/* Bits of the build status, and of a request's flags in the plan. */
#define X3DJPEG_STORE_BAD_ID 1     /* id outside [0, nrecs), or a record whose header index is outside the header table */
#define X3DJPEG_STORE_BAD_SIZE 2   /* the frame is not width x height of its destination */
#define X3DJPEG_STORE_NO_COEF 4    /* its coefficients or planes do not fit the capacities given */
#define X3DJPEG_STORE_NO_WS 8      /* its workspace does not fit */

#define X3DJPEG_STORE_PLAN_THREADS 256   /* the plan kernel's one workgroup */
#define X3DJPEG_STORE_PLAN_CHUNK 1024    /* requests it sums per pass; a carry joins the passes */

/* Bits of the stage status (x3djpeg_stage): why a request was not copied into the staging buffer. */
#define X3DJPEG_STAGE_BAD_ID 1     /* id outside [0, nrecs), or a record without addresses or with sizes below zero */
#define X3DJPEG_STAGE_NO_ROOM 2    /* the frame does not fit what is left of the staging buffer, or max_frame_bytes */

int x3djpeg_abi_version(void);
const char* x3djpeg_last_error(void);
size_t x3djpeg_info_bytes(void);
size_t x3djpeg_frame_job_bytes(void);
size_t x3djpeg_scan_seg_bytes(void);
size_t x3djpeg_scan_job_bytes(void);

/* Host stage. */
int x3djpeg_parse(const uint8_t* bytes, size_t len, X3DJpegInfo* info);
/* Huffman decoding (byte stuffing, DC prediction, restart intervals) of the scan `info` describes into coef
 * (info->coef_count int16, zero-filled first).  coef_bytes < 2 * coef_count is X3DJPEG_EINVAL. */
int x3djpeg_entropy_decode(const uint8_t* bytes, size_t len, const X3DJpegInfo* info, int16_t* coef, size_t coef_bytes);

/* The host's part of the device path: copies the entropy-coded data of the scan `info` describes into scan[0, scan_cap)
 * with the byte stuffing (FF 00 -> FF) and the restart markers removed, X3DJPEG_SCAN_PAD zero bytes after it, and writes
 * one X3DJpegScanSeg per restart interval into segs[0, seg_cap).  Markers are handled as x3djpeg_entropy_decode does:
 * fill FFs before a marker are skipped, RSTn must be the expected one at the end of its interval, anything else ends
 * the data; fewer segments than ceil(mcus / restart_interval), or an over-subscribed Huffman table, is X3DJPEG_ECORRUPT.
 * scan_cap >= len - info->scan_off + X3DJPEG_SCAN_PAD and seg_cap >= the number of restart intervals always suffice;
 * too small a buffer is X3DJPEG_EINVAL.  *scan_bytes (without the padding) and *nseg receive what was written. */
int x3djpeg_scan_prepare(const uint8_t* bytes, size_t len, const X3DJpegInfo* info, uint8_t* scan, size_t scan_cap,
                         X3DJpegScanSeg* segs, size_t seg_cap, size_t* scan_bytes, size_t* nseg);
/* Workspace one frame needs, a multiple of 16.  sub_bits: a multiple of 32 (0 if not). */
size_t x3djpeg_entropy_workspace_bytes(size_t scan_bytes, size_t nseg, int sub_bits);
/* The scheme of x3djpeg_entropy_decode_batch, serially on the CPU through the same code; every pointer (in the jobs too)
 * is a host pointer.  rounds (may be null): relaxation rounds used per frame. */
int x3djpeg_entropy_decode_parallel_host(const X3DJpegScanJob* jobs, int njobs, int sub_bits, void* workspace,
                                         size_t workspace_bytes, int32_t* status, int32_t* rounds);

/* Device stage.  Huffman decoding of njobs prepared scans into their coefficient ranges: one workgroup per frame, one
 * launch.  jobs: X3DJpegScanJob [njobs] on the device; workspace: device memory, 16-byte aligned; status: int32 [njobs] on
 * the device, per frame 0, X3DJPEG_ECORRUPT (a stream the host decoder refuses too) or X3DJPEG_EINVAL (a job that does not
 * fit its own sizes or the workspace).  A failed frame's coefficients are unspecified but stay inside its own range, and
 * the other frames are not affected.  The first int32 of a frame's workspace receives the relaxation rounds it used. */
int x3djpeg_entropy_decode_batch(const void* jobs, int njobs, int sub_bits, void* workspace, size_t workspace_bytes,
                                 void* status, void* stream);

/* jobs: X3DJpegFrameJob [njobs] on the device; max_blocks, max_w, max_h: the maxima of nblocks, width and
 * height over the jobs (they size the grids).  Frames of a batch may differ in size and subsampling. */
/* dequantisation + IDCT + 128, clamped: coef -> planes */
int x3djpeg_idct(const void* jobs, int njobs, int max_blocks, void* stream);
/* chroma upsampling + colour conversion: planes -> dst */
int x3djpeg_to_rgb(const void* jobs, int njobs, int max_w, int max_h, void* stream);
/* both, in two launches whatever njobs is */
int x3djpeg_decode_batch(const void* jobs, int njobs, int max_blocks, int max_w, int max_h, void* stream);

/* Frame store. */
size_t x3djpeg_store_header_bytes(void);
size_t x3djpeg_store_rec_bytes(void);
size_t x3djpeg_store_dst_bytes(void);
/* bytes of the plan of n requests: int64 [3 * n + 2] -- coefficient offsets (int16 elements) [n], workspace offsets
 * (bytes) [n], flags [n], then the two totals */
size_t x3djpeg_store_plan_bytes(int n);

/* Builds the job tables of a batch from frame ids, on the device: two launches whatever n is, no synchronisation, no
 * allocation.  recs: X3DJpegStoreRec [nrecs]; headers: X3DJpegStoreHeader [nheaders]; ids: int32 [n], n in 1 .. 65535;
 * dsts: X3DJpegStoreDst [n]; coef: int16 [coef_cap]; planes: uint8 [planes_cap]; workspace_bytes: the capacity of the
 * workspace x3djpeg_entropy_decode_batch will be given.  All on the device, the tables 16-byte aligned.
 *
 * Request i gets the coefficient range [off_i, off_i + coef_count_i) of coef, the same range of planes in bytes, and
 * workspace [ws_i, ws_i + x3djpeg_entropy_workspace_bytes(...)_i), where off and ws are the exclusive sums over the
 * requests before it (a request with a bad id counts as zero, every other one in full whether it is served or not: a
 * refused request does not move anybody else's range).  The sums, each request's flags and the totals go to `plan`
 * (x3djpeg_store_plan_bytes(n) bytes).  scan_jobs: X3DJpegScanJob [n], frame_jobs: X3DJpegFrameJob [n]: every byte of both
 * is written exactly once.  A request that cannot be served (X3DJPEG_STORE_* says why) gets a refused pair -- every byte
 * of both jobs zero -- for which x3djpeg_entropy_decode_batch reports X3DJPEG_EINVAL and the kernels of
 * x3djpeg_decode_batch leave at once; *build_status (int32) receives the OR of all requests' flags, 0 if all are served. */
int x3djpeg_store_build_jobs(const void* recs, int nrecs, const void* headers, int nheaders, const void* ids, int n,
                             int sub_bits, void* coef, size_t coef_cap, void* planes, size_t planes_cap,
                             size_t workspace_bytes, const void* dsts, void* plan, void* scan_jobs, void* frame_jobs,
                             void* build_status, void* stream);
/* The same through the same code (csrc_jpeg/store_core.h) serially on the CPU; every pointer is a host pointer. */
int x3djpeg_store_build_jobs_host(const void* recs, int nrecs, const void* headers, int nheaders, const void* ids, int n,
                                  int sub_bits, void* coef, size_t coef_cap, void* planes, size_t planes_cap,
                                  size_t workspace_bytes, const void* dsts, void* plan, void* scan_jobs, void* frame_jobs,
                                  void* build_status);

/* Second tier of the frame store: the arena may lie in host memory the device can read (x3djpeg_pinned_alloc), with the
 * record and header tables still on the device.  A batch then first gathers the frames it draws into a small staging
 * buffer on the device (x3djpeg_stage), and the builder and the decoders run on the staged copy:
 *     x3djpeg_stage(recs, nrecs, ids, n, ..., staged_recs, staged_ids, ...)
 *     x3djpeg_store_build_jobs(staged_recs, n, headers, nheaders, staged_ids, n, ...)
 *     x3djpeg_entropy_decode_batch, x3djpeg_decode_batch as ever.
 * (These entry points are not named x3djpeg_store_*: that family is closed at the six above.) */

/* bytes one frame takes in a staging buffer: its scan + X3DJPEG_SCAN_PAD rounded up to 16, then its segment table (16
 * bytes per segment); 0 for sizes below zero */
size_t x3djpeg_stage_bytes(int scan_bytes, int nseg);

/* Copies the frames `ids` name into `staging` and writes the tables that make the staged copies a store of n frames: two
 * launches whatever n (1 .. 65535) is, no synchronisation, no allocation.  recs: X3DJpegStoreRec [nrecs], ids: int32 [n],
 * staging (16-byte aligned, staging_cap bytes) and the four outputs are on the device; only the addresses inside the
 * records may point into host memory the device can read.  A scan is read in whole 16-byte pieces: scan_bytes +
 * X3DJPEG_SCAN_PAD rounded up to 16 is readable at rec.scan.  max_frame_bytes: the largest x3djpeg_stage_bytes among the
 * frames the caller can be asked for (it sizes the copy kernel's grid; n * max_frame_bytes < 2^44).
 *
 * Request i is served at offsets[i], the exclusive sum of x3djpeg_stage_bytes over the requests before it (a bad id and a
 * frame beyond max_frame_bytes count as zero), if it ends at or before staging_cap.  Since a request that does not fit
 * leaves no room for any after it either, the served requests take staging[0, total) without a gap: a refused request
 * takes no staging bytes, offsets[i] of a request refused for lack of room is total, and offsets[n] is total.  A served
 * request gets staged_ids[i] = i and staged_recs[i] = its record with scan and segs rebased into staging; a refused one
 * staged_ids[i] = -1 and a record of zeros, which x3djpeg_store_build_jobs answers with X3DJPEG_STORE_BAD_ID.  Repeated ids
 * are staged once per request.  Every byte of staging[0, total) is written exactly once by a plain store, the round-up
 * tail of each scan as zeros; no byte at or after total is written.  *stage_status (int32) receives the OR of the
 * X3DJPEG_STAGE_* bits of the refused requests. */
int x3djpeg_stage(const void* recs, int nrecs, const void* ids, int n, size_t max_frame_bytes, void* staging,
                  size_t staging_cap, void* staged_recs, void* staged_ids, void* offsets, void* stage_status, void* stream);
/* The same through the same code (csrc_jpeg/stage_core.h) serially on the CPU; every pointer is a host pointer. */
int x3djpeg_stage_host(const void* recs, int nrecs, const void* ids, int n, size_t max_frame_bytes, void* staging,
                       size_t staging_cap, void* staged_recs, void* staged_ids, void* offsets, void* stage_status);

/* Pinned host memory the device can read, for the arena of a host-tier store: mapped and portable.  *host is the address
 * the CPU writes through, *dev the one the runtime reports for the device: kernels are given *dev, never *host.  These two
 * are the only entry points that allocate, and they are not for a step's path.  A failure (no device, a limit reached)
 * is X3DJPEG_ELAUNCH with the byte count in the message. */
int x3djpeg_pinned_alloc(size_t bytes, void** host, void** dev);
int x3djpeg_pinned_free(void* host);

/* Sync index: what the relaxation of x3djpeg_entropy_decode_batch finds out again for every batch -- the decoder state at
 * the start of every subsequence -- depends only on the stored bytes, so it can be computed once, on the host, when a
 * frame is stored.  An index covers one frame at one granularity index_bits (as sub_bits: a multiple of 32, 32 .. 2^20)
 * and holds one 8-byte entry per subsequence of every segment, in the order the relaxation decoder numbers them
 * (x3djpeg_index_count of them).  An entry is two uint32 words:
 *     word 0   p, the bit position within the segment
 *     word 1   b (bits 0-2, the block within the MCU) | k << 3 (bits 3-9, the zigzag index) | first << 10 (bits 10-31,
 *              the index within the segment of the block the state is in)
 * Entry 0 of a segment is all zero.  Entry i + 1 is the state in which the serial decoder stands at the first symbol
 * boundary (a Huffman code with its extra bits is one symbol) at or after bit (i + 1) * index_bits of the segment, or, if
 * the segment's last block ends before that bit, the state at that end (b 0, k 0, first the segment's block count).
 * A segment of 2^22 blocks or more cannot be indexed.
 *
 * Cost: 8 bytes per index_bits bits of scan -- 6.25 % of the scan bytes at 1024, 12.5 % at 512. */
#define X3DJPEG_INDEX_BITS_DEFAULT 512    /* the fastest end to end: profiles/jpeg_index/README.md */
#define X3DJPEG_INDEX_MAX_BLOCKS (1 << 22)

/* Where a stored frame's entries are: entries [first_entry, first_entry + nentries) of the entry array.  The table
 * [nrecs] is parallel to the store's record table: it is indexed by frame id. */
typedef struct X3DJpegIndexRec {
    int64_t first_entry;
    int32_t nentries;
    int32_t pad;
} X3DJpegIndexRec;

size_t x3djpeg_index_rec_bytes(void);
/* Entries of a frame with these segments; 0 for an index_bits the decoder does not take (or segs null). */
size_t x3djpeg_index_count(const X3DJpegScanSeg* segs, size_t nseg, int index_bits);
/* Host, no HIP call: the index of one prepared scan (what x3djpeg_scan_prepare wrote for `info`), one serial pass per
 * segment through csrc_jpeg/entropy_core.h, into entries[0, cap); *n receives the count.  X3DJPEG_ECORRUPT exactly where
 * x3djpeg_entropy_decode refuses the file; X3DJPEG_EUNSUPPORTED for a segment of X3DJPEG_INDEX_MAX_BLOCKS blocks or more;
 * X3DJPEG_EINVAL for a null pointer, a bad index_bits, a segment table that is not the scan's, or cap too small. */
int x3djpeg_index_build(const uint8_t* scan, size_t scan_bytes, const X3DJpegScanSeg* segs, size_t nseg,
                        const X3DJpegInfo* info, int index_bits, uint64_t* entries, size_t cap, size_t* n);

/* Huffman decoding of njobs prepared scans from their sync indices: one workgroup per frame, one launch, one pass over
 * each scan, no workspace.  jobs: the X3DJpegScanJob [njobs] x3djpeg_store_build_jobs wrote (ws_off and ws_bytes are not
 * read); ids: int32 [njobs], the frame id of each job in the index tables (for a host-tier store the ids before
 * x3djpeg_stage, not the staged ones); index_recs: X3DJpegIndexRec [nrecs]; entries: the entry array, entries_total
 * entries, 8-byte aligned; status: int32 [njobs].  All on the device.
 *
 * Per frame the status is 0, X3DJPEG_EINVAL (a job that does not fit its own sizes; an id outside [0, nrecs); a record
 * outside the entry array; nentries that is not x3djpeg_index_count of the job's own segment table), X3DJPEG_EINDEX (an
 * entry that is not what the index rule gives for this scan) or X3DJPEG_ECORRUPT (a stream the host decoder refuses too).
 * Every worker decodes its subsequences from their entries and compares the state it ends in -- p, b, k and the block --
 * with the next entry of the segment; the first entry of a segment is compared with the start state.  So status 0 means:
 * entry 0 was exact and every hand-over matched, and by induction the coefficients are the serial decoder's.  Whatever
 * the entries hold, every scan read is checked against the segment, every store against coef_count and every loop is
 * bounded by the segment's bits: a failed frame's coefficients are unspecified but stay inside its own range, and the
 * other frames are not affected. */
int x3djpeg_entropy_decode_indexed(const void* jobs, int njobs, const void* ids, const void* index_recs, int nrecs,
                                   const void* entries, size_t entries_total, int index_bits, void* status, void* stream);
/* The same through the same code (csrc_jpeg/index_core.h) serially on the CPU; every pointer is a host pointer. */
int x3djpeg_entropy_decode_indexed_host(const void* jobs, int njobs, const void* ids, const void* index_recs, int nrecs,
                                        const void* entries, size_t entries_total, int index_bits, void* status);

#ifdef __cplusplus
}
#endif

#endif /* X3DJPEG_H */
