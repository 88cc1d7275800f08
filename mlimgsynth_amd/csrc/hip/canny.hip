// Canny edge detection of NCHW fp32 planes (mlsd_canny, include/mlsd_kernels.h): the preprocessor of a ControlNet's control image, run at the pass's own pixel
// size.  Integer arithmetic from the quantised 8-bit value to the edge bit (the rules are stated at the prototype), so the result is a function of the input
// alone: no tolerance, no dependence on the order the hysteresis runs in.  Everything is bandwidth-bound and byte-sized behind the first read of src.
//
//   canny_classify   one block per 64 x 32 tile: the quantised patch with a 2-pixel halo in LDS (one pixel for Sobel, one for the neighbours' magnitudes), the
//                    magnitude and the gradient of tile + 1 in LDS, non-maximum suppression, one class byte per pixel (0 none, 1 weak, 2 strong).  Reads src once
//                    (the halo: 1.2x).
//   canny_sweep      one hysteresis sweep, one block per 128 x 128 tile: the tile's classes with a 1-pixel halo in LDS, weak pixels next to a strong one are
//                    promoted in LDS until the tile stops changing (__syncthreads_or; at most one round per tile pixel), the tile goes to the OTHER class buffer
//                    (ping-pong: a sweep reads what the previous launch wrote and nothing else, so its result and the sweep count do not depend on block order),
//                    thread 0 stores 1 into the sweep's flag when the block promoted anything.  No atomics, no block waits on another.
//   canny_output     class 2 -> 1.0f, else 0.0f, into every plane of dst.
// The host launches sweeps in groups of CANNY_SWEEP_GROUP with one flag each, reads the group's flags back once, and stops at the first sweep that raised none:
// such a sweep copied its input, so whichever buffer was written last holds the fixed point.  A sweep that raises its flag promotes at least one pixel, so
// w h + 1 sweeps is a true upper bound; it is the hard cap of the host's for loop.
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

enum { C_TX = 64, C_TY = 32,                          // classify: tile, 256 threads
       C_QW = C_TX + 4, C_QH = C_TY + 4,              // quantised patch (halo 2)
       C_MW = C_TX + 2, C_MH = C_TY + 2,              // magnitudes (halo 1)
       S_TX = 128, S_TY = 128,                        // sweep: tile, 256 threads
       S_LD = S_TX + 8, S_X0 = 4,                     // LDS row of the sweep: the tile's first pixel at byte 4, the halo at bytes 3 and S_TX + 4
       SWEEP_GROUP = 4 };

// coordinate j of an axis of extent n as a tap of the Sobel filter: wrapped or clamped to the border
__device__ __forceinline__ int tap_coord(int j, int n, int wrap)
{
    if (wrap) { j %= n; return j < 0 ? j + n : j; }
    return j < 0 ? 0 : (j >= n ? n - 1 : j);
}
// coordinate j as a pixel: wrapped, or -1 outside the image
__device__ __forceinline__ int pixel_coord(int j, int n, int wrap)
{
    if (wrap) { j %= n; return j < 0 ? j + n : j; }
    return (j < 0 || j >= n) ? -1 : j;
}

__device__ __forceinline__ int quantise(float v)
{
    const float t = floorf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f));
    return (int)fminf(fmaxf(t, 0.0f), 255.0f);      // clamped as a float: the same integers, and no conversion of a value an int cannot hold (NaN -> 0)
}

template <int PLANES>
__global__ void __launch_bounds__(256) canny_classify(const float* __restrict__ src, int w, int h, int lo, int hi, int l2, int wrap, unsigned char* __restrict__ cls)
{
    __shared__ unsigned char s_q[PLANES][C_QH][C_QW];
    __shared__ int s_m[C_MH][C_MW];
    __shared__ int s_g[C_MH][C_MW];       // dx in the high half, dy in the low half (|dx|, |dy| <= 1020)
    const int x0 = blockIdx.x * C_TX, y0 = blockIdx.y * C_TY;
    const int wx = wrap & 1, wy = (wrap >> 1) & 1;
    const long plane = (long)w * h;
    // (a) the quantised patch, rows y0 - 2 .. y0 + C_TY + 1, columns x0 - 2 .. x0 + C_TX + 1, taps outside the image replicated or wrapped
    for (int i = threadIdx.x; i < C_QH * C_QW; i += 256) {
        const int py = i / C_QW, px = i % C_QW;
        const int sx = tap_coord(x0 - 2 + px, w, wx), sy = tap_coord(y0 - 2 + py, h, wy);
        const long at = (long)sy * w + sx;
#pragma unroll
        for (int p = 0; p < PLANES; ++p) s_q[p][py][px] = (unsigned char)quantise(src[p * plane + at]);
    }
    __syncthreads();
    // (c), (d) gradient and magnitude of rows y0 - 1 .. y0 + C_TY, columns x0 - 1 .. x0 + C_TX; 0 outside the image on an axis that does not wrap
    for (int i = threadIdx.x; i < C_MH * C_MW; i += 256) {
        const int my = i / C_MW, mx = i % C_MW;
        int m = 0, g = 0;
        if (pixel_coord(x0 - 1 + mx, w, wx) >= 0 && pixel_coord(y0 - 1 + my, h, wy) >= 0) {
            m = -1;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) {
                const unsigned char (*q)[C_QW] = s_q[p];
                const int cy = my + 1, cx = mx + 1;
                const int dx = (q[cy - 1][cx + 1] + 2 * q[cy][cx + 1] + q[cy + 1][cx + 1]) - (q[cy - 1][cx - 1] + 2 * q[cy][cx - 1] + q[cy + 1][cx - 1]);
                const int dy = (q[cy + 1][cx - 1] + 2 * q[cy + 1][cx] + q[cy + 1][cx + 1]) - (q[cy - 1][cx - 1] + 2 * q[cy - 1][cx] + q[cy - 1][cx + 1]);
                const int mp = l2 ? dx * dx + dy * dy : abs(dx) + abs(dy);
                if (mp > m) { m = mp; g = (int)(((unsigned)dx << 16) | ((unsigned)dy & 0xffffu)); }      // the lowest plane wins ties
            }
        }
        s_m[my][mx] = m; s_g[my][mx] = g;
    }
    __syncthreads();
    // (e) suppression and classification of the tile's own pixels
    for (int i = threadIdx.x; i < C_TY * C_TX; i += 256) {
        const int ty = i / C_TX, tx = i % C_TX;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx >= w || gy >= h) continue;
        const int cy = ty + 1, cx = tx + 1;
        const int m = s_m[cy][cx], g = s_g[cy][cx];
        const int dx = g >> 16, dy = (int)(short)(g & 0xffff);
        int c = 0;
        if (m > lo) {
            const int ax = abs(dx), ay = abs(dy) << 15;
            const int t22 = ax * 13573, t67 = t22 + (ax << 16);
            bool keep;
            if (ay < t22) keep = m > s_m[cy][cx - 1] && m >= s_m[cy][cx + 1];
            else if (ay > t67) keep = m > s_m[cy - 1][cx] && m >= s_m[cy + 1][cx];
            else { const int s = ((dx ^ dy) < 0) ? -1 : 1; keep = m > s_m[cy - 1][cx - s] && m > s_m[cy + 1][cx + s]; }
            if (keep) c = m > hi ? 2 : 1;
        }
        cls[(long)gy * w + gx] = (unsigned char)c;
    }
}

__global__ void __launch_bounds__(256) canny_sweep(const unsigned char* __restrict__ in, unsigned char* __restrict__ out, int w, int h, int wrap, int* __restrict__ flag)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_c[S_TY + 2][S_LD];
    const int x0 = blockIdx.x * S_TX, y0 = blockIdx.y * S_TY;
    const int wx = wrap & 1, wy = (wrap >> 1) & 1;
    // rows y0 - 1 .. y0 + S_TY, columns x0 - 1 .. x0 + S_TX.  The column (row) just outside the image stands for the wrapped neighbour, or 0 on an axis that does
    // not wrap; anything further out is 0.  Only pixels of the image are promoted and written below.
    for (int i = threadIdx.x; i < (S_TY + 2) * (S_TX + 2); i += 256) {
        const int ly = i / (S_TX + 2), lx = i % (S_TX + 2);
        const int gx = x0 - 1 + lx, gy = y0 - 1 + ly;
        const int sx = (gx >= 0 && gx < w) ? gx : ((gx == -1 || gx == w) ? pixel_coord(gx, w, wx) : -1);
        const int sy = (gy >= 0 && gy < h) ? gy : ((gy == -1 || gy == h) ? pixel_coord(gy, h, wy) : -1);
        s_c[ly][S_X0 - 1 + lx] = (sx >= 0 && sy >= 0) ? in[(long)sy * w + sx] : (unsigned char)0;
    }
    __syncthreads();
    int promoted = 0;
    // a round promotes every weak pixel of the tile that has a strong neighbour; promotions of the same round may or may not be seen (1 -> 2 only, the fixed
    // point is the same).  A round that changes something promotes at least one pixel: at most S_TX S_TY rounds change something.
    for (int round = 0; round <= S_TX * S_TY; ++round) {
        int changed = 0;
        for (int i = threadIdx.x; i < S_TY * (S_TX / 4); i += 256) {
            const int ly = 1 + i / (S_TX / 4), lx = S_X0 + 4 * (i % (S_TX / 4));
            const unsigned four = *(const unsigned*)&s_c[ly][lx];
            if (!(four & 0x01010101u) || y0 + ly - 1 >= h) continue;      // no weak pixel among the four, or a row below the image
            for (int k = 0; k < 4; ++k) {
                const int x = lx + k;
                if (s_c[ly][x] != 1 || x0 + x - S_X0 >= w) continue;
                const int any = (s_c[ly - 1][x - 1] | s_c[ly - 1][x] | s_c[ly - 1][x + 1] | s_c[ly][x - 1] | s_c[ly][x + 1] | s_c[ly + 1][x - 1] | s_c[ly + 1][x] | s_c[ly + 1][x + 1]) & 2;
                if (any) { s_c[ly][x] = 2; changed = 1; }
            }
        }
        if (!__syncthreads_or(changed)) break;
        promoted = 1;
    }
    for (int i = threadIdx.x; i < S_TY * S_TX; i += 256) {
        const int ly = i / S_TX, lx = i % S_TX;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < w && gy < h) out[(long)gy * w + gx] = s_c[1 + ly][S_X0 + lx];
    }
    if (promoted && threadIdx.x == 0) *flag = 1;
}

__global__ void __launch_bounds__(256) canny_output(const unsigned char* __restrict__ cls, float* __restrict__ dst, long n, int planes_out)
{
    GRID_LOOP(i, n) {
        const float v = cls[i] == 2 ? 1.0f : 0.0f;
        for (int p = 0; p < planes_out; ++p) dst[p * n + i] = v;
    }
}

__global__ void __launch_bounds__(256) invert_kernel(const float* __restrict__ src, float* __restrict__ dst, long n)
{
    GRID_LOOP(i, n) dst[i] = __fsub_rn(1.0f, src[i]);
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" MLSD_API int mlsd_canny_tile(int which)
{
    switch (which) { case 0: return C_TX; case 1: return C_TY; case 2: return S_TX; case 3: return S_TY; case 4: return SWEEP_GROUP; }
    return -1;
}

// two class buffers (ping-pong) and the flags of one group of sweeps
extern "C" MLSD_API size_t mlsd_canny_ws_bytes(int w, int h)
{
    if (w < 1 || h < 1 || w > MLSD_CANNY_MAX_EXTENT || h > MLSD_CANNY_MAX_EXTENT || (long)w * h * 3 >= (1L << 31)) return 0;
    return 2 * align256((size_t)w * h) + 256;
}

extern "C" MLSD_API int mlsd_canny_thresholds(double low, double high, int l2, int* lo, int* hi)
{
    if (!lo || !hi || low != low || high != high) return mlsd_set_error(-1, "mlsd_canny_thresholds: bad argument");
    if (low > high) { const double t = low; low = high; high = t; }
    double v[2] = { low, high };
    int o[2];
    for (int i = 0; i < 2; ++i) {
        if (l2) {      // compared with squared magnitudes: no square root anywhere
            const double c = v[i] > 32767.0 ? 32767.0 : v[i];
            const long f = c < 0.0 ? 0 : (long)floor(c);
            o[i] = (int)(f * f);
        } else {
            const double f = floor(v[i]);
            o[i] = f > (double)INT_MAX ? INT_MAX : (f < (double)INT_MIN ? INT_MIN : (int)f);
        }
    }
    *lo = o[0]; *hi = o[1];
    return 0;
}

extern "C" MLSD_API int mlsd_canny(const float* src, int w, int h, int planes, int low, int high, int l2, int wrap, float* dst, int planes_out, void* ws, int* n_passes,
                                   void* stream)
{
    if (n_passes) *n_passes = 0;
    if (!src || !dst || w < 1 || h < 1 || w > MLSD_CANNY_MAX_EXTENT || h > MLSD_CANNY_MAX_EXTENT) return mlsd_set_error(-1, "mlsd_canny: bad size %dx%d", w, h);
    if (planes != 1 && planes != 3) return mlsd_set_error(-1, "mlsd_canny: %d source planes (1 or 3)", planes);
    if (planes_out != 1 && planes_out != 3) return mlsd_set_error(-1, "mlsd_canny: %d output planes (1 or 3)", planes_out);
    if ((wrap & ~3) || (l2 & ~1)) return mlsd_set_error(-1, "mlsd_canny: bad wrap %d / l2 %d", wrap, l2);
    const long n = (long)w * h;
    if (n * 3 >= (1L << 31)) return mlsd_set_error(-1, "mlsd_canny: more than 2^31 elements");
    if (!ws) return mlsd_set_error(-1, "mlsd_canny: no workspace");
    const size_t ws_bytes = mlsd_canny_ws_bytes(w, h), n_src = (size_t)n * planes * 4, n_dst = (size_t)n * planes_out * 4;
    if (overlap(src, n_src, dst, n_dst) || overlap(src, n_src, ws, ws_bytes) || overlap(dst, n_dst, ws, ws_bytes)) return mlsd_set_error(-1, "mlsd_canny: src, dst and ws overlap");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("canny");      // the dry runtime's buffers are host memory: refuse before the launch
    hipStream_t st = (hipStream_t)stream;
    unsigned char* buf[2] = { (unsigned char*)ws, (unsigned char*)ws + align256((size_t)n) };
    int* flags = (int*)((unsigned char*)ws + 2 * align256((size_t)n));

    const dim3 cgrid((unsigned)((w + C_TX - 1) / C_TX), (unsigned)((h + C_TY - 1) / C_TY));
    if (planes == 3) hipLaunchKernelGGL(canny_classify<3>, cgrid, dim3(256), 0, st, src, w, h, low, high, l2, wrap, buf[0]);
    else hipLaunchKernelGGL(canny_classify<1>, cgrid, dim3(256), 0, st, src, w, h, low, high, l2, wrap, buf[0]);
    { const int r = mlsd_check_launch("canny classify"); if (r) return r; }

    const dim3 sgrid((unsigned)((w + S_TX - 1) / S_TX), (unsigned)((h + S_TY - 1) / S_TY));
    const long cap = n + 1;      // every sweep but the last promotes a pixel
    long launched = 0, needed = -1;
    int cur = 0;
    while (needed < 0 && launched < cap) {
        const int k = (int)(cap - launched < SWEEP_GROUP ? cap - launched : SWEEP_GROUP);
        int h_flags[SWEEP_GROUP];
        MLSD_HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int) * k, st));
        for (int i = 0; i < k; ++i, cur ^= 1) {
            hipLaunchKernelGGL(canny_sweep, sgrid, dim3(256), 0, st, (const unsigned char*)buf[cur], buf[cur ^ 1], w, h, wrap, flags + i);
            const int r = mlsd_check_launch("canny sweep"); if (r) return r;
        }
        MLSD_HIP_TRY(hipMemcpyAsync(h_flags, flags, sizeof(int) * k, hipMemcpyDeviceToHost, st));
        MLSD_HIP_TRY(hipStreamSynchronize(st));
        for (int i = 0; i < k && needed < 0; ++i) if (!h_flags[i]) needed = launched + i + 1;
        launched += k;
    }
    if (needed < 0) return mlsd_set_error(-1, "mlsd_canny: %ld hysteresis sweeps of a %dx%d image did not settle", launched, w, h);
    if (n_passes) *n_passes = (int)(needed > INT_MAX ? INT_MAX : needed);

    hipLaunchKernelGGL(canny_output, dim3(nblk(n)), dim3(256), 0, st, (const unsigned char*)buf[cur], dst, n, planes_out);
    return mlsd_check_launch("canny output");
}

extern "C" MLSD_API int mlsd_invert(const float* src, float* dst, int64_t n, void* stream)
{
    if (!src || !dst || n < 1) return mlsd_set_error(-1, "mlsd_invert: bad argument");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("invert");
    hipLaunchKernelGGL(invert_kernel, dim3(nblk((long)n)), dim3(256), 0, (hipStream_t)stream, src, dst, (long)n);
    return mlsd_check_launch("invert");
}
