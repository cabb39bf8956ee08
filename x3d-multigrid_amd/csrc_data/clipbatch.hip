// The clip kernels of every input path: the fixed-length batches of the Kinetics dataset (kinetics_multigrid.py:240-253,
// through clip_input.ClipPreprocessor) and the variable-length ones of the Charades dataset (charades.py:139,145-157 and
// custom_collate_fn :167-189), over decoded uint8 frames resident in HBM: crop, Pillow's 8-bit bilinear resample,
// optional flip, ToTensor(255), Normalize, each sample into its slice of a batch, padded where the job asks for it (the
// tail written as +0.0f here, not by a memset), or into the windows of a multi-window testing batch (a frame resized once
// and stored to every window that holds it).
//
// This is the only copy of the resample.  It lives here and not in csrc/ because nothing that runs outside a training
// step goes into the sources that tools/stamp.csrc_sha16() hashes and the gradient-hash record is keyed on (DESIGN.md
// section 7).  Bit-exact with Pillow (libImaging/Resample.c): separable, horizontal pass first into
// a uint8 intermediate, 22-bit fixed-point coefficient tables built on the host (clip_input.resize_coeffs), round half
// up, clip to [0, 255].  The intermediate lives in caller-provided HBM scratch: the rounding to uint8 between the passes
// is what makes the result Pillow's, and the plain two-pass form is the only one.
// Byte/integer work, HBM bound: one thread per output pixel (3 channels), coalesced along x.
#include "data_common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// horizontal pass: tmp[t][y][xx][c] = clip8(sum_i src[frame t][y1 + y][x1 + x0 + i][c] * kk[xx][i])
__global__ __launch_bounds__(256) void clip_batch_hpass_kernel(const X3DDataClipJob* __restrict__ jobs,
                                                               const int32_t* __restrict__ frames,
                                                               uint8_t* __restrict__ scratch) {
    const X3DDataClipJob J = jobs[blockIdx.z];
    const int t = blockIdx.y;
    if (t >= J.T) return;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= J.crop * J.out) return;
    const int y = idx / J.out, xx = idx - y * J.out;
    const int x0 = J.bounds[xx * 2], n = J.bounds[xx * 2 + 1];
    const int32_t* k = J.kk + (size_t)xx * J.ksize;
    const uint8_t* row = J.src + (((size_t)frames[J.frames_off + t] * J.Hs + (J.y1 + y)) * J.Ws + (J.x1 + x0)) * 3;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < n; ++i) {
        const int kv = k[i];
        a0 += (int)row[i * 3] * kv;
        a1 += (int)row[i * 3 + 1] * kv;
        a2 += (int)row[i * 3 + 2] * kv;
    }
    uint8_t* o = scratch + J.tmp_off + (((size_t)t * J.crop + y) * J.out + xx) * 3;
    o[0] = (uint8_t)clip8(a0); o[1] = (uint8_t)clip8(a1); o[2] = (uint8_t)clip8(a2);
}

// vertical pass + flip + ToTensor(255) + Normalize: ((v / 255) - mean[c]) / std[c], stored to every window holding frame
// t; frames T <= t < Tpad of a padded clip are zeros.
__global__ __launch_bounds__(256) void clip_batch_vpass_kernel(const X3DDataClipJob* __restrict__ jobs,
                                                               const uint8_t* __restrict__ scratch, float m0, float m1,
                                                               float m2, float s0, float s1, float s2) {
    const X3DDataClipJob J = jobs[blockIdx.z];
    const int t = blockIdx.y;
    if (t >= J.Tpad) return;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= J.out * J.out) return;
    const int yy = idx / J.out, xx = idx - yy * J.out;
    if (t >= J.T) {                                     // the padding of custom_collate_fn (only nwin == 1 has one)
        float* d = J.dst + (size_t)t * J.dst_ts + (size_t)yy * J.out + xx;
        d[0] = 0.0f;
        d[J.dst_cs] = 0.0f;
        d[2 * J.dst_cs] = 0.0f;
        return;
    }
    const int y0 = J.bounds[yy * 2], n = J.bounds[yy * 2 + 1];
    const int32_t* k = J.kk + (size_t)yy * J.ksize;
    const uint8_t* col = scratch + J.tmp_off + (((size_t)t * J.crop + y0) * J.out + xx) * 3;
    const size_t pitch = (size_t)J.out * 3;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < n; ++i) {
        const int kv = k[i];
        a0 += (int)col[i * pitch] * kv;
        a1 += (int)col[i * pitch + 1] * kv;
        a2 += (int)col[i * pitch + 2] * kv;
    }
    // img.float().div(255) ; t.sub_(m).div_(s)  -- three separately rounded fp32 operations
    const float v0 = ((float)clip8(a0) / 255.0f - m0) / s0;
    const float v1 = ((float)clip8(a1) / 255.0f - m1) / s1;
    const float v2 = ((float)clip8(a2) / 255.0f - m2) / s2;
    const int xo = J.flip ? J.out - 1 - xx : xx;
    const size_t pix = (size_t)yy * J.out + xo;
    for (int w = 0; w < J.nwin; ++w) {
        const int tw = t - w * J.win_step;
        if (tw < 0) break;
        if (tw >= J.win_len) continue;
        float* d = J.dst + (size_t)w * J.dst_ws + (size_t)tw * J.dst_ts + pix;
        d[0] = v0;
        d[J.dst_cs] = v1;
        d[2 * J.dst_cs] = v2;
    }
}

}  // namespace

extern "C" int x3ddata_clip_batch(const void* jobs, int njobs, const int32_t* frames, uint8_t* scratch, int max_T,
                                  int max_Tpad, int max_crop, int max_out, const float* mean, const float* stdv,
                                  void* stream) {
    X3DDATA_CHECK_ARG(jobs && frames && scratch && mean && stdv);
    X3DDATA_CHECK_ARG(njobs > 0 && njobs <= 65535 && max_T > 0 && max_Tpad >= max_T && max_Tpad <= 65535);
    X3DDATA_CHECK_ARG(max_crop > 0 && max_out > 0 && (long long)max_crop * max_out < (1LL << 31));
    X3DDATA_CHECK_ARG((long long)max_out * max_out < (1LL << 31));
    hipStream_t s = (hipStream_t)stream;
    const X3DDataClipJob* J = (const X3DDataClipJob*)jobs;
    hipLaunchKernelGGL(clip_batch_hpass_kernel, dim3(data_cdiv(max_crop * max_out, 256), max_T, njobs), dim3(256), 0, s, J,
                       frames, scratch);
    hipLaunchKernelGGL(clip_batch_vpass_kernel, dim3(data_cdiv(max_out * max_out, 256), max_Tpad, njobs), dim3(256), 0, s,
                       J, (const uint8_t*)scratch, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
    X3DDATA_LAUNCH_CHECK();
    return X3DDATA_OK;
}
