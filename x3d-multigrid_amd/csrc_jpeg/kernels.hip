// Device stage of libx3djpeg (include/x3djpeg.h): two kernels per batch of frames.
//
// idct: dequantisation in int32 and libjpeg's "islow" integer IDCT (jidctint.c: CONST_BITS 13, PASS1_BITS 2, column pass
// first), + 128, clamped.  libjpeg's zero-AC shortcuts give the same integers as the full butterfly, so there is no
// branch.  One workgroup of 256 threads takes 32 blocks: thread (block, r) loads coefficient row r as one 16-byte load,
// dequantises it into an int32 LDS workspace, runs the column pass on column r, then the row pass on row r, and stores
// the 8 output bytes of that row as one 8-byte store.  The workspace is 72 dwords per block: the column pass reads and
// writes dwords (32 banks, per half-wave = 4 blocks), and 72 = 8 mod 32 puts the 4 blocks on disjoint banks.
// Integer and LDS work, no MFMA.
//
// to_rgb: libjpeg's "fancy" (triangle) chroma upsampling on the component's true size, plain replication when the chroma
// width is <= 2, then the fixed-point YCbCr -> RGB conversion; 4 pixels per thread, stored as three dwords where the
// destination is dword aligned and as bytes otherwise (row strides are the caller's).
#include "jpeg_common.h"

namespace {

constexpr int BLOCKS_PER_WG = 32;
constexpr int WS_STRIDE = 72;

constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270;
constexpr int FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137;
constexpr int FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

// One 1-D pass of jidctint.c: v[0..7] in, v[0..7] out, descaled by SHIFT with rounding.
template <int SHIFT>
__device__ __forceinline__ void idct_1d(int* v) {
    int z1 = (v[2] + v[6]) * FIX_0_541196100;
    const int tmp2 = z1 - v[6] * FIX_1_847759065;
    const int tmp3 = z1 + v[2] * FIX_0_765366865;
    const int e0 = (v[0] + v[4]) * 8192;
    const int e1 = (v[0] - v[4]) * 8192;
    const int tmp10 = e0 + tmp3, tmp13 = e0 - tmp3, tmp11 = e1 + tmp2, tmp12 = e1 - tmp2;
    int t0 = v[7], t1 = v[5], t2 = v[3], t3 = v[1];
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    t0 *= FIX_0_298631336;
    t1 *= FIX_2_053119869;
    t2 *= FIX_3_072711026;
    t3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223;
    z2 *= -FIX_2_562915447;
    z3 = z3 * -FIX_1_961570560 + z5;
    z4 = z4 * -FIX_0_390180644 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    v[0] = (tmp10 + t3 + R) >> SHIFT;
    v[7] = (tmp10 - t3 + R) >> SHIFT;
    v[1] = (tmp11 + t2 + R) >> SHIFT;
    v[6] = (tmp11 - t2 + R) >> SHIFT;
    v[2] = (tmp12 + t1 + R) >> SHIFT;
    v[5] = (tmp12 - t1 + R) >> SHIFT;
    v[3] = (tmp13 + t0 + R) >> SHIFT;
    v[4] = (tmp13 - t0 + R) >> SHIFT;
}

__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

union Row8 {
    int4 q;
    int16_t s[8];
    uint16_t u[8];
};

__global__ __launch_bounds__(256) void idct_kernel(const X3DJpegFrameJob* __restrict__ jobs) {
    __shared__ __attribute__((aligned(16))) int ws[BLOCKS_PER_WG * WS_STRIDE];
    const X3DJpegFrameJob* J = jobs + blockIdx.y;
    const int nblocks = J->nblocks;
    if ((int)blockIdx.x * BLOCKS_PER_WG >= nblocks) return;  // the whole workgroup leaves: no barrier is skipped by a part
    const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
    const int b = blockIdx.x * BLOCKS_PER_WG + lb;
    const bool live = b < nblocks;
    int c = 0;
    if (J->ncomp == 3) c = b >= J->block_start[2] ? 2 : (b >= J->block_start[1] ? 1 : 0);
    int* w = ws + lb * WS_STRIDE;
    int v[8];
    if (live) {
        Row8 co, q;
        co.q = *reinterpret_cast<const int4*>(J->coef + (size_t)b * 64 + r * 8);
        q.q = *reinterpret_cast<const int4*>(&J->qt[c][r * 8]);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (int)co.s[i] * (int)q.u[i];
        *reinterpret_cast<int4*>(w + r * 8) = make_int4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<int4*>(w + r * 8 + 4) = make_int4(v[4], v[5], v[6], v[7]);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[k * 8 + r];
        idct_1d<11>(v);  // CONST_BITS - PASS1_BITS
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k * 8 + r] = v[k];
    }
    __syncthreads();
    if (live) {
        const int4 a = *reinterpret_cast<const int4*>(w + r * 8);
        const int4 d = *reinterpret_cast<const int4*>(w + r * 8 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = d.x; v[5] = d.y; v[6] = d.z; v[7] = d.w;
        idct_1d<18>(v);  // CONST_BITS + PASS1_BITS + 3
        uint2 o;
        o.x = (uint32_t)clamp8(v[0] + 128) | ((uint32_t)clamp8(v[1] + 128) << 8) | ((uint32_t)clamp8(v[2] + 128) << 16) |
              ((uint32_t)clamp8(v[3] + 128) << 24);
        o.y = (uint32_t)clamp8(v[4] + 128) | ((uint32_t)clamp8(v[5] + 128) << 8) | ((uint32_t)clamp8(v[6] + 128) << 16) |
              ((uint32_t)clamp8(v[7] + 128) << 24);
        const int start = J->block_start[c], bw = J->blocks_w[c];
        const int k = b - start, by = k / bw, bx = k - by * bw;
        uint8_t* plane = J->planes + (size_t)start * 64;
        *reinterpret_cast<uint2*>(plane + ((size_t)(by * 8 + r) * bw + bx) * 8) = o;
    }
}

// The chroma sample libjpeg's upsampler gives output pixel (x, y).  P: the component's plane, `stride` bytes per row;
// cw, ch: the component's true size.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ P, int stride, int cw, int ch, int hs, int vs, int x,
                                         int y) {
    if (hs == 1) return P[(size_t)y * stride + x];
    const int j = x >> 1;
    const int jn = (x & 1) ? min(j + 1, cw - 1) : max(j - 1, 0);
    if (vs == 1) {
        const uint8_t* row = P + (size_t)y * stride;
        if (cw <= 2) return row[j];
        return (3 * (int)row[j] + (int)row[jn] + 1 + (x & 1)) >> 2;
    }
    const int i = y >> 1;
    const uint8_t* near = P + (size_t)i * stride;
    if (cw <= 2) return near[j];
    const uint8_t* far = P + (size_t)((y & 1) ? min(i + 1, ch - 1) : max(i - 1, 0)) * stride;
    const int s = 3 * (int)near[j] + (int)far[j];
    const int sn = 3 * (int)near[jn] + (int)far[jn];
    return (3 * s + sn + 8 - (x & 1)) >> 4;
}

constexpr int G_1_402 = 91881, G_1_772 = 116130, G_0_34414 = 22554, G_0_71414 = 46802;

__global__ __launch_bounds__(256) void to_rgb_kernel(const X3DJpegFrameJob* __restrict__ jobs) {
    const X3DJpegFrameJob* J = jobs + blockIdx.y;
    const int W = J->width, H = J->height;
    const int gw = jpeg_cdiv(W, 4);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= gw * H) return;
    const int y = idx / gw, x0 = (idx - y * gw) * 4;
    const int nc = J->ncomp, hs = J->hmax, vs = J->vmax;
    const int ystride = J->blocks_w[0] * 8;
    const uint8_t* Y = J->planes + (size_t)y * ystride;
    const uint8_t *Cb = nullptr, *Cr = nullptr;
    int cstride = 0, cw = 0, ch = 0;
    if (nc == 3) {
        Cb = J->planes + (size_t)J->block_start[1] * 64;
        Cr = J->planes + (size_t)J->block_start[2] * 64;
        cstride = J->blocks_w[1] * 8;
        cw = J->cw[1];
        ch = J->ch[1];
    }
    uint8_t px[12];
    const int n = min(4, W - x0);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = min(x0 + p, W - 1);
        const int yy = Y[x];
        int r = yy, g = yy, b = yy;
        if (nc == 3) {
            const int cb = chroma_at(Cb, cstride, cw, ch, hs, vs, x, y) - 128;
            const int cr = chroma_at(Cr, cstride, cw, ch, hs, vs, x, y) - 128;
            r = clamp8(yy + ((G_1_402 * cr + 32768) >> 16));
            b = clamp8(yy + ((G_1_772 * cb + 32768) >> 16));
            g = clamp8(yy + ((-G_0_34414 * cb - G_0_71414 * cr + 32768) >> 16));
        }
        px[p * 3] = (uint8_t)r;
        px[p * 3 + 1] = (uint8_t)g;
        px[p * 3 + 2] = (uint8_t)b;
    }
    uint8_t* o = J->dst + (size_t)y * J->dst_stride + (size_t)x0 * 3;
    if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) |
                    ((uint32_t)px[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * n) o[k] = px[k];
    }
}

int launch_idct(const void* jobs, int njobs, int max_blocks, hipStream_t s) {
    hipLaunchKernelGGL(idct_kernel, dim3(jpeg_cdiv(max_blocks, BLOCKS_PER_WG), njobs), dim3(256), 0, s,
                       (const X3DJpegFrameJob*)jobs);
    X3DJPEG_LAUNCH_CHECK();
    return X3DJPEG_OK;
}

int launch_to_rgb(const void* jobs, int njobs, int max_w, int max_h, hipStream_t s) {
    hipLaunchKernelGGL(to_rgb_kernel, dim3(jpeg_cdiv(jpeg_cdiv(max_w, 4) * max_h, 256), njobs), dim3(256), 0, s,
                       (const X3DJpegFrameJob*)jobs);
    X3DJPEG_LAUNCH_CHECK();
    return X3DJPEG_OK;
}

}  // namespace

// grid.y holds the jobs (<= 65535); grid.x the blocks / pixel groups of the largest frame
#define X3DJPEG_CHECK_BLOCKS() X3DJPEG_CHECK_ARG(jobs && njobs > 0 && njobs <= 65535 && max_blocks > 0)
#define X3DJPEG_CHECK_PIXELS() \
    X3DJPEG_CHECK_ARG(jobs && njobs > 0 && njobs <= 65535 && max_w > 0 && max_h > 0 && max_w <= 65535 && max_h <= 65535 && \
                      (long long)jpeg_cdiv(max_w, 4) * max_h < (1LL << 31))

extern "C" int x3djpeg_idct(const void* jobs, int njobs, int max_blocks, void* stream) {
    X3DJPEG_CHECK_BLOCKS();
    return launch_idct(jobs, njobs, max_blocks, (hipStream_t)stream);
}

extern "C" int x3djpeg_to_rgb(const void* jobs, int njobs, int max_w, int max_h, void* stream) {
    X3DJPEG_CHECK_PIXELS();
    return launch_to_rgb(jobs, njobs, max_w, max_h, (hipStream_t)stream);
}

extern "C" int x3djpeg_decode_batch(const void* jobs, int njobs, int max_blocks, int max_w, int max_h, void* stream) {
    X3DJPEG_CHECK_BLOCKS();
    X3DJPEG_CHECK_PIXELS();
    const int rc = launch_idct(jobs, njobs, max_blocks, (hipStream_t)stream);
    if (rc != X3DJPEG_OK) return rc;
    return launch_to_rgb(jobs, njobs, max_w, max_h, (hipStream_t)stream);
}
