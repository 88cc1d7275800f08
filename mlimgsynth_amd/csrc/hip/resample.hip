// Resampling of NCHW fp32 planes (mlsd_resample2d, include/mlsd_kernels.h): the latent upscaler between the two passes of the hires fix.
// One thread per output pixel, x fastest: stores are coalesced along the row, the 1 / 4 / 16 taps of neighbouring threads fall into the same or
// adjacent cache lines.  The data is a few megabytes at most and the launch happens once per generation: nothing here is worth LDS.
// Coordinates are pixel centres (torch's align_corners=False): src = (d + 0.5) s_in / s_out - 0.5.  Its integer part and its fraction come from
// the exact integer division of (2 d + 1) s_in - s_out by 2 s_out: a coordinate computed in fp32 carries an error of 2^-24 * extent in the
// fraction (1.5e-5 of the neighbours' difference at 256 pixels), the quotient and remainder carry none.  Weights and sums are fp32, not contracted.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

// floor of the source coordinate of output pixel d, and its fraction in [0, 1)
__device__ __forceinline__ int src_coord(int d, int s_in, int s_out, float* t)
{
    const long num = (2L * d + 1) * s_in - s_out, den = 2L * s_out;      // src = num / den, num >= -den + 1
    long q = num / den, r = num - q * den;
    if (r < 0) { r += den; q -= 1; }
    *t = __fdiv_rn((float)r, (float)den);
    return (int)q;
}

// tap index i (any int within one extent of the plane) inside [0, n): modulo n on a wrapped axis, clamped otherwise
__device__ __forceinline__ int tap(int i, int n, int wrap)
{
    if (wrap) { i %= n; return i < 0 ? i + n : i; }
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// Keys cubic convolution, a = -0.75: |x| <= 1 and 1 < |x| < 2
__device__ __forceinline__ float cubic1(float x) { const float a = -0.75f; return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(a + 2.f, x), a + 3.f), x), x), 1.f); }
__device__ __forceinline__ float cubic2(float x) { const float a = -0.75f; return __fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(__fmul_rn(a, x), 5.f * a), x), 8.f * a), x), 4.f * a); }
__device__ __forceinline__ void cubic_weights(float t, float w[4])
{
    w[0] = cubic2(__fadd_rn(t, 1.f)); w[1] = cubic1(t); w[2] = cubic1(__fsub_rn(1.f, t)); w[3] = cubic2(__fsub_rn(2.f, t));
}

template <int MODE>
__global__ void resample2d_kernel(const float* __restrict__ src, int sw, int sh, float* __restrict__ dst, int dw, int dh, int planes, int wrap)
{
    const long total = (long)planes * dh * dw;
    GRID_LOOP(i, total) {
        const int x = (int)(i % dw);
        const long r = i / dw;
        const int y = (int)(r % dh);
        const float* p = src + (r / dh) * ((long)sh * sw);
        float tx, ty;
        const int ix = src_coord(x, sw, dw, &tx), iy = src_coord(y, sh, dh, &ty);
        float v;
        if (MODE == MLSD_RESAMPLE_NEAREST) {
            // floor((d + 0.5) s_in / s_out), in integers; never outside the plane
            const int nx = (int)(((2L * x + 1) * sw) / (2L * dw)), ny = (int)(((2L * y + 1) * sh) / (2L * dh));
            v = p[(long)(ny < sh ? ny : sh - 1) * sw + (nx < sw ? nx : sw - 1)];
        } else if (MODE == MLSD_RESAMPLE_BILINEAR) {
            const int x0 = tap(ix, sw, wrap & 1), x1 = tap(ix + 1, sw, wrap & 1);
            const float* r0 = p + (long)tap(iy, sh, wrap & 2) * sw;
            const float* r1 = p + (long)tap(iy + 1, sh, wrap & 2) * sw;
            const float ux = __fsub_rn(1.f, tx), uy = __fsub_rn(1.f, ty);
            const float a = __fadd_rn(__fmul_rn(ux, r0[x0]), __fmul_rn(tx, r0[x1]));
            const float b = __fadd_rn(__fmul_rn(ux, r1[x0]), __fmul_rn(tx, r1[x1]));
            v = __fadd_rn(__fmul_rn(uy, a), __fmul_rn(ty, b));
        } else {
            float wx[4], wy[4];
            cubic_weights(tx, wx); cubic_weights(ty, wy);
            int xs[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) xs[k] = tap(ix - 1 + k, sw, wrap & 1);
            v = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* row = p + (long)tap(iy - 1 + j, sh, wrap & 2) * sw;
                float s = __fmul_rn(wx[0], row[xs[0]]);
#pragma unroll
                for (int k = 1; k < 4; ++k) s = __fadd_rn(s, __fmul_rn(wx[k], row[xs[k]]));
                v = __fadd_rn(v, __fmul_rn(wy[j], s));
            }
        }
        dst[i] = v;
    }
}

}  // namespace

extern "C" MLSD_API int mlsd_resample2d(const float* src, int sw, int sh, float* dst, int dw, int dh, int planes, int mode, int wrap, void* stream)
{
    if (!src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || planes < 1) return mlsd_set_error(-1, "mlsd_resample2d: bad size %dx%d -> %dx%d, %d planes", sw, sh, dw, dh, planes);
    // src_coord's fraction r / (2 s_out) stays below 1 only while 2 s_out is exact in fp32 (2^24): beyond it (float)r can round up to the divisor
    if (sw > MLSD_RESAMPLE_MAX_EXTENT || sh > MLSD_RESAMPLE_MAX_EXTENT || dw > MLSD_RESAMPLE_MAX_EXTENT || dh > MLSD_RESAMPLE_MAX_EXTENT)
        return mlsd_set_error(-1, "mlsd_resample2d: extent above %d in %dx%d -> %dx%d", MLSD_RESAMPLE_MAX_EXTENT, sw, sh, dw, dh);
    if (mode < MLSD_RESAMPLE_NEAREST || mode > MLSD_RESAMPLE_BICUBIC || (wrap & ~3)) return mlsd_set_error(-1, "mlsd_resample2d: bad mode %d / wrap %d", mode, wrap);
    const long n_src = (long)planes * sh * sw, n_dst = (long)planes * dh * dw;
    if (n_src >= (1L << 31) || n_dst >= (1L << 31)) return mlsd_set_error(-1, "mlsd_resample2d: more than 2^31 elements");
    if (src < dst + n_dst && dst < src + n_src) return mlsd_set_error(-1, "mlsd_resample2d: src and dst overlap");
    // equal sizes: every coordinate is a pixel centre; the nearest kernel copies it whatever its bits (-0, NaN payloads)
    if (sw == dw && sh == dh) mode = MLSD_RESAMPLE_NEAREST;
    const dim3 grid(nblk(n_dst)), block(256);
    switch (mode) {
    case MLSD_RESAMPLE_NEAREST: hipLaunchKernelGGL(resample2d_kernel<MLSD_RESAMPLE_NEAREST>, grid, block, 0, (hipStream_t)stream, src, sw, sh, dst, dw, dh, planes, wrap); break;
    case MLSD_RESAMPLE_BILINEAR: hipLaunchKernelGGL(resample2d_kernel<MLSD_RESAMPLE_BILINEAR>, grid, block, 0, (hipStream_t)stream, src, sw, sh, dst, dw, dh, planes, wrap); break;
    default: hipLaunchKernelGGL(resample2d_kernel<MLSD_RESAMPLE_BICUBIC>, grid, block, 0, (hipStream_t)stream, src, sw, sh, dst, dw, dh, planes, wrap); break;
    }
    return mlsd_check_launch("resample2d");
}
