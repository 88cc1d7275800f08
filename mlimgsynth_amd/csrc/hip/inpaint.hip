// Image-space pieces of region inpainting (include/mlsd_kernels.h, "region inpainting"): the repaint weight of a mask, its growth by a square maximum / minimum,
// a Gaussian blur, the bounding box of what is to be repainted and the paste of a repainted patch into the untouched original.  fp32 planes [planes][h][w].
// An index outside a plane replicates the border pixel, or is taken modulo the extent on an axis named in `wrap` (a true modulo: a radius may exceed the extent).
//
// Blur, horizontal pass: an output needs 2 r + 1 neighbours of its row, r up to 160, so a block stages the span of its tile's columns, tx + 2 r floats of up to 16
// rows, in LDS together with the taps (coalesced reads, each source float fetched once per tile; lane x reads word x + k: no bank conflicts, the tap is a broadcast).
// tx is 64, 128 or 256 with the image's width: at r = 160 a 256-column tile reads 576 floats per row for 256 outputs (2.25 x), a 64-column one would read 6 x.
// A tile may use 32 KiB; where even 4 rows of the span do not fit (a test's lowered limit) the launch reads global memory directly.
// Blur, vertical pass: a block owns 256 columns of four output rows, one thread per column; the taps are uniform over the block, every load and store is
// coalesced, and a source row is loaded once for the four outputs it feeds.  No LDS.
// Every sum is fp32 in ascending tap order, products and additions rounded one by one: the result is a function of the taps alone, whatever the tile.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

enum { B_WAVES = 4, B_TY_MAX = 16, B_LDS_BYTES = 32 * 1024, B_MIN_TILES = 1024, V_TX = 256, V_ROWS = 4, MAX_BLOCKS = 65536 };

// index on one axis: modulo the extent when it wraps, else clamped to the border
__device__ __forceinline__ int axis_index(long j, int n, int wrap)
{
    if (wrap) { j %= n; return (int)(j < 0 ? j + n : j); }
    return (int)(j < 0 ? 0 : (j >= n ? n - 1 : j));
}

__global__ void __launch_bounds__(256) mask_weight_kernel(const float* __restrict__ m, float* __restrict__ p, long n, int invert)
{
    GRID_LOOP(i, n) {
        const float v = invert ? m[i] : __fsub_rn(1.0f, m[i]);
        p[i] = fminf(fmaxf(v, 0.0f), 1.0f);      // fmaxf(NaN, 0) = 0
    }
}

// maximum (grow) or minimum over 2 r + 1 neighbours along x (stride 1) or y (stride w) of a plane [h][w]
__global__ void __launch_bounds__(256) grow_axis_kernel(const float* __restrict__ src, float* __restrict__ dst, int w, int h, int r, int is_min, int along_y, int wrap)
{
    const long total = (long)w * h;
    GRID_LOOP(i, total) {
        const int x = (int)(i % w), y = (int)(i / w);
        float v = src[i];
        for (int k = -r; k <= r; ++k) {
            const float s = along_y ? src[(long)axis_index((long)y + k, h, wrap) * w + x] : src[(long)y * w + axis_index((long)x + k, w, wrap)];
            v = is_min ? fminf(v, s) : fmaxf(v, s);
        }
        dst[i] = v;
    }
}

// Horizontal blur from LDS.  rows = planes * h rows of w floats.  Tile t covers columns [tx cx, tx cx + tx) of rows [ty cy, ty cy + ty); its span starts r columns
// to the left.  Thread (lx, ly) = (tid % tx, tid / tx) stages and computes the rows ly, ly + 256 / tx, ...
__global__ void __launch_bounds__(256) blur_rows_lds(const float* __restrict__ src, float* __restrict__ dst, int w, long rows, const float* __restrict__ taps, int r,
                                                     int tx, int ty, int wrap, long n_tiles, int tiles_x)
{
    extern __shared__ float lds[];
    const int K = 2 * r + 1, span = tx + 2 * r;
    float* s_w = lds;                 // [K]
    float* s_src = lds + K;           // [ty][span]
    const int lx = threadIdx.x % tx, ly = threadIdx.x / tx, step = 256 / tx;
    for (int k = threadIdx.x; k < K; k += 256) s_w[k] = taps[k];
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int x0 = (int)(t % tiles_x) * tx;
        const long r0 = (t / tiles_x) * ty;
        const int nx = w - x0 < tx ? w - x0 : tx, len = nx + 2 * r;
        __syncthreads();              // the previous tile's reads are done (and, the first time, nothing)
        for (int j = ly; j < ty && r0 + j < rows; j += step) {
            const float* row = src + (r0 + j) * w;
            for (int c = lx; c < len; c += tx) s_src[j * span + c] = row[axis_index((long)x0 - r + c, w, wrap)];
        }
        __syncthreads();
        if (lx < nx) for (int j = ly; j < ty && r0 + j < rows; j += step) {
            const float* p = s_src + j * span + lx;
            float acc = __fmul_rn(s_w[0], p[0]);
            for (int k = 1; k < K; ++k) acc = __fadd_rn(acc, __fmul_rn(s_w[k], p[k]));
            dst[(r0 + j) * w + x0 + lx] = acc;
        }
    }
}

// Horizontal blur reading global memory: one thread per output, x fastest
__global__ void __launch_bounds__(256) blur_rows_direct(const float* __restrict__ src, float* __restrict__ dst, int w, long rows, const float* __restrict__ taps, int r, int wrap)
{
    const long total = rows * w;
    const int K = 2 * r + 1;
    GRID_LOOP(i, total) {
        const int x = (int)(i % w);
        const float* p = src + (i / w) * w;
        float acc = __fmul_rn(taps[0], p[axis_index((long)x - r, w, wrap)]);
        for (int k = 1; k < K; ++k) acc = __fadd_rn(acc, __fmul_rn(taps[k], p[axis_index((long)x - r + k, w, wrap)]));
        dst[i] = acc;
    }
}

// Vertical blur: tile t covers columns [256 cx, 256 cx + 256) of the V_ROWS output rows of group t / tiles_x (groups_y groups per plane).  A thread walks the
// K + V_ROWS - 1 source rows its outputs need once: source row y0 - r + s is tap k = s - o of output o, so each output still sums its taps in ascending order
__global__ void __launch_bounds__(256) blur_cols(const float* __restrict__ src, float* __restrict__ dst, int w, int h, const float* __restrict__ taps, int r, int wrap,
                                                 long n_tiles, int tiles_x, int groups_y)
{
    const int K = 2 * r + 1;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int x = (int)(t % tiles_x) * V_TX + threadIdx.x;
        const long g = t / tiles_x;
        const int y0 = (int)(g % groups_y) * V_ROWS;
        const long plane = (g / groups_y) * ((long)h * w);
        const float* p = src + plane;
        if (x < w) {
            float acc[V_ROWS];
#pragma unroll
            for (int o = 0; o < V_ROWS; ++o) acc[o] = 0.0f;
            for (int s = 0; s < K + V_ROWS - 1; ++s) {
                const float v = p[(long)axis_index((long)y0 - r + s, h, wrap) * w + x];
#pragma unroll
                for (int o = 0; o < V_ROWS; ++o) {
                    const int k = s - o;      // uniform over the block
                    if (k == 0) acc[o] = __fmul_rn(taps[0], v);
                    else if (k > 0 && k < K) acc[o] = __fadd_rn(acc[o], __fmul_rn(taps[k], v));
                }
            }
#pragma unroll
            for (int o = 0; o < V_ROWS; ++o) if (y0 + o < h) dst[plane + (long)(y0 + o) * w + x] = acc[o];
        }
    }
}

// bounding box: out = { min x, min y, max x + 1, max y + 1 } of the pixels with p > 0, by integer atomics on a box initialised to { INT_MAX, INT_MAX, 0, 0 }
__global__ void bbox_init_kernel(int* out) { if (threadIdx.x < 4) out[threadIdx.x] = threadIdx.x < 2 ? INT_MAX : 0; }

__global__ void __launch_bounds__(256) bbox_kernel(const float* __restrict__ p, int w, long n, int* __restrict__ out)
{
    int x0 = INT_MAX, y0 = INT_MAX, x1 = 0, y1 = 0;
    GRID_LOOP(i, n) if (p[i] > 0.0f) {
        const int x = (int)(i % w), y = (int)(i / w);
        x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x + 1); y1 = max(y1, y + 1);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && x1 > 0) { atomicMin(out + 0, x0); atomicMin(out + 1, y0); atomicMax(out + 2, x1); atomicMax(out + 3, y1); }
}

// nothing found: the box is 0, 0, 0, 0
__global__ void bbox_finish_kernel(int* out) { if (threadIdx.x == 0 && out[2] == 0) out[0] = out[1] = out[3] = 0; }

// dst [B][planes][H][W] = orig outside the rectangle, orig (1 - p) + patch p inside (mask_apply_kernel's arithmetic: two rounded products, one rounded sum)
__global__ void __launch_bounds__(256) composite_kernel(float* dst, const float* orig /* may be dst */, int n_orig, const float* __restrict__ patch,
                                                        const float* __restrict__ p, int W, int H, int planes, long total, int x0, int y0, int cw, int ch)
{
    const long hw = (long)H * W, per = hw * planes;
    GRID_LOOP(i, total) {
        const long q = i % hw, bc = i / hw;      // pixel; image * planes + plane
        const int x = (int)(q % W), y = (int)(q / W);
        const float o = orig[n_orig == 1 ? i % per : i];
        float v = o;
        if (x >= x0 && x < x0 + cw && y >= y0 && y < y0 + ch) {
            const float pv = p[q], t = patch[(bc * ch + (y - y0)) * cw + (x - x0)];
            v = __fadd_rn(__fmul_rn(o, __fsub_rn(1.0f, pv)), __fmul_rn(t, pv));
        }
        dst[i] = v;
    }
}

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

int g_lds_limit = B_LDS_BYTES;      // mlsd_gauss_blur_lds_limit

unsigned grid_for(long n_tiles) { return (unsigned)(n_tiles < 1 ? 1 : (n_tiles > MAX_BLOCKS ? MAX_BLOCKS : n_tiles)); }

int gauss_radius(float sigma) { return (int)(2.5 * (double)sigma + 0.5); }

bool plane_args_ok(int w, int h, long planes) { return w >= 1 && h >= 1 && planes >= 1 && w <= MLSD_INPAINT_MAX_EXTENT && h <= MLSD_INPAINT_MAX_EXTENT && planes * (long)w * h < (1L << 31); }

}  // namespace

extern "C" MLSD_API int mlsd_mask_weight(const float* mask, float* p, int64_t n, int invert, void* stream)
{
    if (!mask || !p || n < 1 || (invert & ~1)) return mlsd_set_error(-1, "mlsd_mask_weight: bad argument");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("mask_weight");
    hipLaunchKernelGGL(mask_weight_kernel, dim3(nblk((long)n)), dim3(256), 0, (hipStream_t)stream, mask, p, (long)n, invert);
    return mlsd_check_launch("mask_weight");
}

extern "C" MLSD_API int mlsd_mask_grow(const float* src, float* dst, int w, int h, int radius, int wrap, void* ws, void* stream)
{
    if (!src || !dst || !plane_args_ok(w, h, 1)) return mlsd_set_error(-1, "mlsd_mask_grow: bad size %dx%d", w, h);
    if (radius < -MLSD_MASK_GROW_MAX || radius > MLSD_MASK_GROW_MAX || (wrap & ~3)) return mlsd_set_error(-1, "mlsd_mask_grow: bad radius %d / wrap %d", radius, wrap);
    const size_t bytes = (size_t)w * h * 4;
    if (!ws) return mlsd_set_error(-1, "mlsd_mask_grow: no workspace");
    if (overlap(src, bytes, dst, bytes) || overlap(src, bytes, ws, bytes) || overlap(dst, bytes, ws, bytes)) return mlsd_set_error(-1, "mlsd_mask_grow: src, dst and ws overlap");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("mask_grow");
    hipStream_t st = (hipStream_t)stream;
    if (radius == 0) { MLSD_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)); return 0; }
    const int r = radius < 0 ? -radius : radius, is_min = radius < 0;
    const unsigned grid = nblk((long)w * h);
    hipLaunchKernelGGL(grow_axis_kernel, dim3(grid), dim3(256), 0, st, src, (float*)ws, w, h, r, is_min, 0, wrap & 1);
    { const int e = mlsd_check_launch("mask_grow rows"); if (e) return e; }
    hipLaunchKernelGGL(grow_axis_kernel, dim3(grid), dim3(256), 0, st, (const float*)ws, dst, w, h, r, is_min, 1, (wrap >> 1) & 1);
    return mlsd_check_launch("mask_grow columns");
}

extern "C" MLSD_API int mlsd_gauss_taps(float sigma, float* w, int k_max)
{
    if (!(sigma >= 0.0f && sigma <= (float)MLSD_GAUSS_MAX_SIGMA) || !w) return -1;
    const int r = gauss_radius(sigma), K = 2 * r + 1;
    if (K > k_max) return -1;
    if (r == 0) { w[0] = 1.0f; return 1; }
    double* tmp = (double*)malloc(sizeof(double) * (size_t)K);
    if (!tmp) return -1;
    const double s = (double)sigma, d = 2.0 * s * s;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) { const double x = (double)(k - r); tmp[k] = exp(-(x * x) / d); sum += tmp[k]; }
    for (int k = 0; k < K; ++k) w[k] = (float)(tmp[k] / sum);
    free(tmp);
    return K;
}

extern "C" MLSD_API int mlsd_gauss_blur_lds_limit(int bytes)
{
    const int was = g_lds_limit;
    if (bytes >= 0) g_lds_limit = bytes < B_LDS_BYTES ? bytes : B_LDS_BYTES;
    return was;
}

extern "C" MLSD_API size_t mlsd_gauss_blur_ws_bytes(int w, int h, int planes)
{
    if (!plane_args_ok(w, h, planes)) return 0;
    return align256(sizeof(float) * MLSD_GAUSS_MAX_TAPS) + align256(sizeof(float) * (size_t)planes * w * h);
}

extern "C" MLSD_API int mlsd_gauss_blur(const float* src, float* dst, int w, int h, int planes, float sigma, int wrap, void* ws, void* stream)
{
    if (!src || !dst || !plane_args_ok(w, h, planes)) return mlsd_set_error(-1, "mlsd_gauss_blur: bad size %dx%d, %d planes", w, h, planes);
    if (!(sigma >= 0.0f && sigma <= (float)MLSD_GAUSS_MAX_SIGMA) || (wrap & ~3)) return mlsd_set_error(-1, "mlsd_gauss_blur: bad sigma %g / wrap %d", (double)sigma, wrap);
    if (!ws) return mlsd_set_error(-1, "mlsd_gauss_blur: no workspace");
    const size_t bytes = (size_t)planes * w * h * 4, ws_bytes = mlsd_gauss_blur_ws_bytes(w, h, planes);
    if (overlap(src, bytes, dst, bytes) || overlap(src, bytes, ws, ws_bytes) || overlap(dst, bytes, ws, ws_bytes)) return mlsd_set_error(-1, "mlsd_gauss_blur: src, dst and ws overlap");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("gauss_blur");
    hipStream_t st = (hipStream_t)stream;
    float taps[MLSD_GAUSS_MAX_TAPS];
    const int K = mlsd_gauss_taps(sigma, taps, MLSD_GAUSS_MAX_TAPS), r = K / 2;
    if (K < 1) return mlsd_set_error(-1, "mlsd_gauss_blur: taps of sigma %g", (double)sigma);
    if (r == 0) { MLSD_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st)); return 0; }      // one tap of 1: a copy of the bits
    // the taps: uploaded on the stream, which is waited for before the host array goes out of scope
    hipError_t e = hipMemcpyAsync(ws, taps, sizeof(float) * (size_t)K, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipGetLastError(); return mlsd_set_error(-(int)e - 1000, "mlsd_gauss_blur: tap upload failed: %s", hipGetErrorString(e)); }
    const float* d_taps = (const float*)ws;
    float* mid = (float*)((char*)ws + align256(sizeof(float) * MLSD_GAUSS_MAX_TAPS));
    const long rows = (long)planes * h;
    const int tx = w > 128 ? 256 : (w > 64 ? 128 : 64), span = tx + 2 * r;
    int ty = B_TY_MAX;
    const int tiles_rx = (w + tx - 1) / tx;
    while (ty > B_WAVES && sizeof(float) * ((size_t)ty * span + K) > (size_t)g_lds_limit) ty /= 2;
    while (ty > B_WAVES && ((rows + ty - 1) / ty) * tiles_rx < B_MIN_TILES) ty /= 2;      // a small image: rather more tiles than rows per tile (256 CUs)
    const size_t lds = sizeof(float) * ((size_t)ty * span + K);
    if (lds <= (size_t)g_lds_limit) {
        const long n_tiles = ((rows + ty - 1) / ty) * tiles_rx;
        hipLaunchKernelGGL(blur_rows_lds, dim3(grid_for(n_tiles)), dim3(256), lds, st, src, mid, w, rows, d_taps, r, tx, ty, wrap & 1, n_tiles, tiles_rx);
    } else {
        hipLaunchKernelGGL(blur_rows_direct, dim3(nblk(rows * w)), dim3(256), 0, st, src, mid, w, rows, d_taps, r, wrap & 1);
    }
    { const int c = mlsd_check_launch("gauss_blur rows"); if (c) return c; }
    const int tiles_x = (w + V_TX - 1) / V_TX, groups_y = (h + V_ROWS - 1) / V_ROWS;
    const long n_tiles = (long)planes * groups_y * tiles_x;
    hipLaunchKernelGGL(blur_cols, dim3(grid_for(n_tiles)), dim3(256), 0, st, (const float*)mid, dst, w, h, d_taps, r, (wrap >> 1) & 1, n_tiles, tiles_x, groups_y);
    return mlsd_check_launch("gauss_blur columns");
}

extern "C" MLSD_API int mlsd_mask_bbox(const float* p, int w, int h, int* out4_dev, void* stream)
{
    if (!p || !out4_dev || !plane_args_ok(w, h, 1)) return mlsd_set_error(-1, "mlsd_mask_bbox: bad size %dx%d", w, h);
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("mask_bbox");
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)w * h;
    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, st, out4_dev);
    hipLaunchKernelGGL(bbox_kernel, dim3(nblk(n)), dim3(256), 0, st, p, w, n, out4_dev);
    hipLaunchKernelGGL(bbox_finish_kernel, dim3(1), dim3(64), 0, st, out4_dev);
    return mlsd_check_launch("mask_bbox");
}

extern "C" MLSD_API int mlsd_composite(float* dst, const float* orig, int n_orig, const float* patch, const float* p, int W, int H, int planes, int B, int x0, int y0,
                                       int cw, int ch, void* stream)
{
    if (!dst || !orig || !patch || !p || B < 1 || planes < 1 || (n_orig != 1 && n_orig != B) || !plane_args_ok(W, H, (long)planes * B))
        return mlsd_set_error(-1, "mlsd_composite: bad argument (%dx%d, %d planes, %d images, %d originals)", W, H, planes, B, n_orig);
    if (cw < 1 || ch < 1 || x0 < 0 || y0 < 0 || cw > W - x0 || ch > H - y0) return mlsd_set_error(-1, "mlsd_composite: rectangle %dx%d at (%d, %d) of a %dx%d image", cw, ch, x0, y0, W, H);
    const size_t per = (size_t)planes * W * H * 4, n_dst = per * B, n_patch = (size_t)B * planes * cw * ch * 4, n_p = (size_t)W * H * 4;
    if ((dst != orig || n_orig != B) && overlap(dst, n_dst, orig, per * n_orig)) return mlsd_set_error(-1, "mlsd_composite: dst overlaps orig (in place needs dst == orig and n_orig == B)");
    if (overlap(dst, n_dst, patch, n_patch) || overlap(dst, n_dst, p, n_p)) return mlsd_set_error(-1, "mlsd_composite: dst overlaps patch or p");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("composite");
    const long total = (long)B * planes * H * W;
    hipLaunchKernelGGL(composite_kernel, dim3(nblk(total)), dim3(256), 0, (hipStream_t)stream, dst, orig, n_orig, patch, p, W, H, planes, total, x0, y0, cw, ch);
    return mlsd_check_launch("composite");
}
