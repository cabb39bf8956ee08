/*
 * x3ddata.h -- C ABI of libx3ddata.so: HIP kernels (gfx950 / MI355X) of the input paths, what the reference's datasets
 * do per sample on CPU workers: for Charades (charades.py:68-189) the per-frame label windows cut from dense host arrays,
 * the clip transforms, and the zero padding of custom_collate_fn; for Kinetics (kinetics_multigrid.py:240-253) the clip
 * transforms.
 *
 * A separate library from libx3dhip.so on purpose: tools/stamp.py and the gradient-hash record hash the training library's
 * sources, and nothing here runs inside a training step.
 *
 * Conventions (as include/x3deval.h)
 *   - plain pointers and sizes; the caller (torch) owns every buffer; every kernel is enqueued on the hipStream_t passed
 *     as `stream`; no entry point allocates or synchronises (they may be captured into a graph)
 *   - return 0 on success, negative X3DDATA_E* on failure; x3ddata_last_error() gives the message (thread-local)
 *   - deterministic bit for bit: every output element is written exactly once by a plain vector store; no memset pass,
 *     no atomics
 *
 * The annotation table (device resident for the lifetime of a dataset; a CSR table over the dataset's videos)
 *   ann_off  int32 [V + 1]   annotations of video v are ann_off[v] .. ann_off[v + 1] - 1
 *   ann_cls  int32 [A]       class of each annotation
 *   ann_lo   int32 [A]       half-open range [lo, hi) of the 0-based frames on which the annotation is on; computed on
 *   ann_hi   int32 [A]       the host with the reference's double-precision expression (charades.py:93-97)
 */
#ifndef X3DDATA_H
#define X3DDATA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X3DDATA_ABI_VERSION 1

#define X3DDATA_OK 0
#define X3DDATA_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define X3DDATA_ELAUNCH (-2)  /* hipLaunch error */

/* One label window: frames [start, start + n) of video `video` (an index into ann_off). */
typedef struct X3DDataLabelJob {
    int32_t video;
    int32_t start; /* first frame, 0-based */
    int32_t n;     /* window length, 0 <= n <= TLmax */
    int32_t pad;
} X3DDataLabelJob;

/* One video (or one clip) of a batch: T frames, listed in frames[frames_off ..], are cropped, resized to out x out with
 * Pillow's 8-bit bilinear resample, optionally flipped, and normalised.  Frame t lands at
 *     dst[w * dst_ws + c * dst_cs + (t - w * win_step) * dst_ts + y * out + x]
 * for every window w < nwin with w * win_step <= t < w * win_step + win_len (a frame is resized once, however many windows
 * hold it).  With nwin == 1 (win_step 0, win_len >= T) that is one clip, and frames T <= t < Tpad of it are written as
 * +0.0f.  Strides are in floats. */
typedef struct X3DDataClipJob {
    const uint8_t* src;     /* [Tsrc][Hs][Ws][3] decoded frames */
    float* dst;
    const int32_t* kk;      /* [out][ksize] coefficients (one table for both passes: square crop, square output) */
    const int32_t* bounds;  /* [out][2]  (first input index, tap count) */
    int64_t dst_cs, dst_ts, dst_ws;
    int64_t tmp_off;        /* byte offset of this job's [T][crop][out][3] horizontal-pass intermediate in `scratch` */
    int32_t frames_off;     /* offset of this job's T source-frame indices (0-based) in `frames` */
    int32_t Hs, Ws, x1, y1, crop, out, ksize;
    int32_t T, Tpad, flip;
    int32_t nwin, win_step, win_len;
} X3DDataClipJob;

int x3ddata_abi_version(void);
const char* x3ddata_last_error(void);
size_t x3ddata_label_job_bytes(void);
size_t x3ddata_clip_job_bytes(void);

/* Per-frame labels, masks and clip-level labels of B windows in one launch.  Replaces the dense [K, n_frames] host arrays
 * of make_dataset (charades.py:91-97), the window slice and the task='class' max of __getitem__ (:140-143) and the label
 * and mask padding of custom_collate_fn (:174-185).
 *   jobs    X3DDataLabelJob [B] on the device
 *   labels  fp32 [B, K, TLmax]  1 iff an annotation of class k covers frame start_b + t and t < n_b, else 0
 *   masks   fp32 [B, TLmax]     1 iff t < n_b
 *   cls     fp32 [B, K]         max_t labels[b, k, t]
 * Any output may be NULL (not all three).  A job whose video is outside [0, V) gives zeros. */
int x3ddata_charades_labels(const int32_t* ann_off, const int32_t* ann_cls, const int32_t* ann_lo, const int32_t* ann_hi,
                            int V, const void* jobs, int B, int K, int TLmax, float* labels, float* masks, float* cls,
                            void* stream);

/* njobs X3DDataClipJob (on the device) in two launches, whatever njobs is: the horizontal pass into the uint8 intermediate
 * in `scratch`, then the vertical pass + flip + ToTensor(255) + Normalize(mean, std) + the zero padding.  Replaces
 * load_rgb_frames and the spatial transforms of __getitem__ (charades.py:139,145-148; transforms/spatial_transforms.py
 * :44-83,106-116,214-228,334-346,480-495), the window slicing of the testing split (:150-157) and the clip padding of
 * custom_collate_fn (:179-183); and, for Kinetics, the per-sample CPU work of kinetics_multigrid.py:240-253 (frame
 * selection by TemporalRandomCrop, transforms/temporal_transforms.py:94-117, with the indices computed by the host;
 * MultiScaleRandomCropMultigrid; RandomHorizontalFlip; ToTensor(255) + Normalize; stack / permute to [3][T][S][S]): one
 * job per sample with dst_cs = T * S * S, dst_ts = S * S, no padding and one window.  Bit-exact with Pillow's 8-bit
 * bilinear resample given the host-built coefficient table (x3dhip/clip_input.py:resize_coeffs = Resample.c
 * precompute_coeffs + normalize_coeffs_8bpc).
 * max_T / max_Tpad / max_crop / max_out: the maxima over the jobs (they size the grid).  mean, stdv: 3 floats each on the
 * host. */
int x3ddata_clip_batch(const void* jobs, int njobs, const int32_t* frames, uint8_t* scratch, int max_T, int max_Tpad,
                       int max_crop, int max_out, const float* mean, const float* stdv, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* X3DDATA_H */
