// Antialiased resampling of NCHW fp32 planes (mlsd_resample2d_aa, include/mlsd_kernels.h): a filter whose support grows with the shrink factor, what
// PIL's resize and torch's interpolate(antialias=True) do.  Separable: the host builds one tap table per axis (mlsd_resample_aa_taps: first tap, tap count and
// normalised fp32 weights of every output index), a horizontal pass makes [planes][sh][dw], a vertical pass makes dst.  An axis whose extents are equal
// is skipped.  Every sum is fp32 in ascending tap order, products and additions rounded one by one: the result is a function of the tables alone.
//
// Horizontal pass: neighbouring lanes read addresses `scale` floats apart and each walks 2 sup max(scale, 1) taps, so a block stages the source span of
// its 64 output columns x 4 to 16 rows in LDS (coalesced reads, every source float fetched once per block) together with the tile's weights, stored tap-major
// (lane x reads bank x: no conflicts; the source reads are scale-way conflicted at most).  A block may use 32 KiB: five blocks per CU of the 160 KiB.
// A shape whose widest tile needs more (a 40x lanczos shrink: 240 taps per output) reads global memory directly in that launch.
// Vertical pass: a block owns 256 columns of one output row; the row's first tap, count and weights are uniform over the block, the tap loop walks source
// rows, every load and store is coalesced.  No LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

// ---------------------------------------------------------------- tap tables (host)
const int k_two_sup[4] = { 1, 2, 4, 6 };      // 2 x support of box, triangle, cubic, lanczos3

long floor_div(long a, long b) { long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

double sinc_pi(double x) { if (x == 0.0) return 1.0; const double t = M_PI * x; return sin(t) / t; }

double aa_filter(int filter, double x)
{
    switch (filter) {
    case MLSD_AA_BOX: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case MLSD_AA_TRIANGLE: { const double a = fabs(x); return a < 1.0 ? 1.0 - a : 0.0; }
    case MLSD_AA_CUBIC: {      // Keys, a = -0.5
        const double a = -0.5, t = fabs(x);
        if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
        if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
        return 0.0;
    }
    default: { const double t = fabs(x); return t < 3.0 ? sinc_pi(x) * sinc_pi(x / 3.0) : 0.0; }
    }
}

// taps [lo, hi) of output index d: exact integer floors of c -+ sup fs + 0.5; clipped to the plane unless the axis wraps
void tap_range(int s_in, int s_out, int filter, int wrap_axis, int d, long* lo, long* hi)
{
    const long mid = (long)s_in * (2L * d + 1) + s_out, half = (long)k_two_sup[filter] * (s_in > s_out ? s_in : s_out), den = 2L * s_out;
    long a = floor_div(mid - half, den), b = floor_div(mid + half, den);
    if (!wrap_axis) { if (a < 0) a = 0; if (b > s_in) b = s_in; }
    *lo = a; *hi = b;
}

bool taps_args_ok(int s_in, int s_out, int filter)
{
    return s_in >= 1 && s_out >= 1 && s_in <= MLSD_RESAMPLE_MAX_EXTENT && s_out <= MLSD_RESAMPLE_MAX_EXTENT && filter >= MLSD_AA_BOX && filter <= MLSD_AA_LANCZOS3;
}

// ---------------------------------------------------------------- kernels
enum { H_TX = 64, H_WAVES = 4, H_TY_MAX = 16, H_LDS_BYTES = 32 * 1024, V_TX = 256, MAX_BLOCKS = 65536 };

__device__ __forceinline__ int wrap_index(long j, int n) { j %= n; return (int)(j < 0 ? j + n : j); }

// Horizontal pass from LDS.  rows = planes * sh source rows of sw floats -> rows of dw floats.  Tile t covers output columns [64 tx, 64 tx + 64) of rows
// [ty r, ty r + ty), ty a multiple of 4 chosen by the host; its source span starts at the first column's first tap and is `span` floats per row at most.
// A wave stages and computes the rows ly, ly + 4, ...: one row of the span per pass of its 64 lanes, one output column per lane.
__global__ void __launch_bounds__(256) aa_rows_lds(const float* __restrict__ src, int sw, float* __restrict__ dst, int dw, long rows, const int* __restrict__ start,
                                                   const int* __restrict__ count, const float* __restrict__ w, int K, int span, int ty, int wrap, long n_tiles, int tiles_x)
{
    extern __shared__ float lds[];
    float* s_src = lds;                       // [ty][span]
    float* s_w = lds + ty * span;             // [K][H_TX]
    const int lx = threadIdx.x % H_TX, ly = threadIdx.x / H_TX;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int x0 = (int)(t % tiles_x) * H_TX;
        const long r0 = (t / tiles_x) * ty;
        const int nx = dw - x0 < H_TX ? dw - x0 : H_TX;
        const int lo0 = start[x0], len = start[x0 + nx - 1] + count[x0 + nx - 1] - lo0;      // <= span (host: the maximum over the tiles)
        const int first = lx < nx ? start[x0 + lx] - lo0 : 0, n = lx < nx ? count[x0 + lx] : 0;
        __syncthreads();                      // the previous tile's reads are done
        for (int r = ly; r < ty && r0 + r < rows; r += H_WAVES) {
            const float* row = src + (r0 + r) * sw;
            for (int c = lx; c < len; c += H_TX) s_src[r * span + c] = row[wrap ? wrap_index((long)lo0 + c, sw) : lo0 + c];
        }
        if (lx < nx) for (int k = ly; k < K; k += H_WAVES) s_w[k * H_TX + lx] = w[(long)(x0 + lx) * K + k];
        __syncthreads();
        if (lx < nx) for (int r = ly; r < ty && r0 + r < rows; r += H_WAVES) {
            const float* p = s_src + r * span + first;
            float acc = __fmul_rn(s_w[lx], p[0]);
            for (int k = 1; k < n; ++k) acc = __fadd_rn(acc, __fmul_rn(s_w[k * H_TX + lx], p[k]));
            dst[(r0 + r) * dw + x0 + lx] = acc;
        }
    }
}

// Horizontal pass reading global memory: one thread per output, x fastest
__global__ void __launch_bounds__(256) aa_rows_direct(const float* __restrict__ src, int sw, float* __restrict__ dst, int dw, long rows, const int* __restrict__ start,
                                                      const int* __restrict__ count, const float* __restrict__ w, int K, int wrap)
{
    const long total = rows * dw;
    GRID_LOOP(i, total) {
        const int x = (int)(i % dw);
        const float* p = src + (i / dw) * sw;
        const float* wx = w + (long)x * K;
        const int lo = start[x], n = count[x];
        float acc = __fmul_rn(wx[0], p[wrap ? wrap_index(lo, sw) : lo]);
        for (int k = 1; k < n; ++k) acc = __fadd_rn(acc, __fmul_rn(wx[k], p[wrap ? wrap_index((long)lo + k, sw) : lo + k]));
        dst[i] = acc;
    }
}

// Vertical pass: planes of sh rows of `width` floats -> planes of dh rows.  Tile t covers columns [256 tx, 256 tx + 256) of output row t / tiles_x.
__global__ void __launch_bounds__(256) aa_cols(const float* __restrict__ src, int sh, float* __restrict__ dst, int dh, int width, const int* __restrict__ start,
                                               const int* __restrict__ count, const float* __restrict__ w, int K, int wrap, long n_tiles, int tiles_x)
{
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int x = (int)(t % tiles_x) * V_TX + threadIdx.x;
        const long r = t / tiles_x;           // output row over all planes
        const int y = (int)(r % dh);
        const float* p = src + (r / dh) * ((long)sh * width);
        const float* wy = w + (long)y * K;
        const int lo = start[y], n = count[y];
        if (x < width) {
            float acc = __fmul_rn(wy[0], p[(long)(wrap ? wrap_index(lo, sh) : lo) * width + x]);
            for (int k = 1; k < n; ++k) acc = __fadd_rn(acc, __fmul_rn(wy[k], p[(long)(wrap ? wrap_index((long)lo + k, sh) : lo + k) * width + x]));
            dst[r * width + x] = acc;
        }
    }
}

// ---------------------------------------------------------------- workspace layout
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct AxisTable { int s_in, s_out, K; size_t off_start, off_count, off_w, end; };      // offsets in bytes from the workspace's start

// the table of one axis behind byte offset `at`; K = 0 and nothing reserved when the axis is skipped
AxisTable axis_table(int s_in, int s_out, int filter, size_t at)
{
    AxisTable a = { s_in, s_out, 0, at, at, at, at };
    if (s_in == s_out) return a;
    a.K = mlsd_resample_aa_max_taps(s_in, s_out, filter);
    a.off_count = a.off_start + align256(sizeof(int) * (size_t)s_out);
    a.off_w = a.off_count + align256(sizeof(int) * (size_t)s_out);
    a.end = a.off_w + align256(sizeof(float) * (size_t)s_out * a.K);
    return a;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

int g_lds_limit = H_LDS_BYTES;      // mlsd_resample2d_aa_lds_limit

unsigned grid_for(long n_tiles) { return (unsigned)(n_tiles < 1 ? 1 : (n_tiles > MAX_BLOCKS ? MAX_BLOCKS : n_tiles)); }

}  // namespace

extern "C" MLSD_API int mlsd_resample_aa_max_taps(int s_in, int s_out, int filter)
{
    if (!taps_args_ok(s_in, s_out, filter)) return -1;
    // without wrap the widest window is an unclipped one if there is any; the loop is s_out integer divisions
    long k = 0;
    for (int d = 0; d < s_out; ++d) { long lo, hi; tap_range(s_in, s_out, filter, 1, d, &lo, &hi); if (hi - lo > k) k = hi - lo; }
    return (int)k;
}

extern "C" MLSD_API int mlsd_resample_aa_taps(int s_in, int s_out, int filter, int wrap_axis, int* start, int* count, float* w, int k_max)
{
    if (!taps_args_ok(s_in, s_out, filter) || !start || !count || !w || (wrap_axis & ~1)) return -1;
    const double scale = (double)s_in / (double)s_out, fs = scale > 1.0 ? scale : 1.0;
    int k_used = 0;
    for (int d = 0; d < s_out; ++d) { long lo, hi; tap_range(s_in, s_out, filter, wrap_axis, d, &lo, &hi); if (hi - lo > k_used) k_used = (int)(hi - lo); }
    if (k_used > k_max || k_used < 1) return -1;
    double* tmp = (double*)malloc(sizeof(double) * (size_t)k_used);
    if (!tmp) return -1;
    for (int d = 0; d < s_out; ++d) {
        long lo, hi;
        tap_range(s_in, s_out, filter, wrap_axis, d, &lo, &hi);
        const int n = (int)(hi - lo);
        const double c = scale * ((double)d + 0.5);
        double sum = 0.0;
        for (int k = 0; k < n; ++k) { tmp[k] = aa_filter(filter, ((double)(lo + k) - c + 0.5) / fs); sum += tmp[k]; }
        float* wd = w + (size_t)d * k_max;
        for (int k = 0; k < n; ++k) wd[k] = (float)(tmp[k] / sum);
        for (int k = n; k < k_max; ++k) wd[k] = 0.f;
        start[d] = (int)lo; count[d] = n;
    }
    free(tmp);
    return k_used;
}

extern "C" MLSD_API int mlsd_resample2d_aa_lds_limit(int bytes)
{
    const int was = g_lds_limit;
    if (bytes >= 0) g_lds_limit = bytes < H_LDS_BYTES ? bytes : H_LDS_BYTES;
    return was;
}

extern "C" MLSD_API size_t mlsd_resample2d_aa_ws_bytes(int sw, int sh, int dw, int dh, int planes, int filter)
{
    if (!taps_args_ok(sw, dw, filter) || !taps_args_ok(sh, dh, filter) || planes < 1) return 0;
    const AxisTable ax = axis_table(sw, dw, filter, 0), ay = axis_table(sh, dh, filter, ax.end);
    size_t n = ay.end;
    if (ax.K && ay.K) n += align256(sizeof(float) * (size_t)planes * sh * dw);
    return n ? n : 256;
}

extern "C" MLSD_API int mlsd_resample2d_aa(const float* src, int sw, int sh, float* dst, int dw, int dh, int planes, int filter, int wrap, void* ws, void* stream)
{
    if (!src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1 || planes < 1) return mlsd_set_error(-1, "mlsd_resample2d_aa: bad size %dx%d -> %dx%d, %d planes", sw, sh, dw, dh, planes);
    if (sw > MLSD_RESAMPLE_MAX_EXTENT || sh > MLSD_RESAMPLE_MAX_EXTENT || dw > MLSD_RESAMPLE_MAX_EXTENT || dh > MLSD_RESAMPLE_MAX_EXTENT)
        return mlsd_set_error(-1, "mlsd_resample2d_aa: extent above %d in %dx%d -> %dx%d", MLSD_RESAMPLE_MAX_EXTENT, sw, sh, dw, dh);
    if (filter < MLSD_AA_BOX || filter > MLSD_AA_LANCZOS3 || (wrap & ~3)) return mlsd_set_error(-1, "mlsd_resample2d_aa: bad filter %d / wrap %d", filter, wrap);
    const long n_src = (long)planes * sh * sw, n_dst = (long)planes * dh * dw, n_mid = (long)planes * sh * dw;
    if (n_src >= (1L << 31) || n_dst >= (1L << 31) || n_mid >= (1L << 31)) return mlsd_set_error(-1, "mlsd_resample2d_aa: more than 2^31 elements");
    if (!ws) return mlsd_set_error(-1, "mlsd_resample2d_aa: no workspace");
    const size_t ws_bytes = mlsd_resample2d_aa_ws_bytes(sw, sh, dw, dh, planes, filter);
    if (overlap(src, n_src * 4, dst, n_dst * 4) || overlap(src, n_src * 4, ws, ws_bytes) || overlap(dst, n_dst * 4, ws, ws_bytes))
        return mlsd_set_error(-1, "mlsd_resample2d_aa: src, dst and ws overlap");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("resample2d_aa");      // the dry runtime's buffers are host memory: refuse before the launch
    hipStream_t st = (hipStream_t)stream;
    if (sw == dw && sh == dh) {       // a copy of the bits
        MLSD_HIP_TRY(hipMemcpyAsync(dst, src, (size_t)n_src * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    const AxisTable ax = axis_table(sw, dw, filter, 0), ay = axis_table(sh, dh, filter, ax.end);
    // the tables: built in one host block that mirrors the head of the workspace, uploaded on the stream, which is waited for before the block is freed
    char* host = (char*)calloc(1, ay.end);
    if (!host) return mlsd_set_error(-1, "mlsd_resample2d_aa: out of host memory");
    int span = 0;      // widest source span of a horizontal tile
    if (ax.K) {
        int *h_start = (int*)(host + ax.off_start), *h_count = (int*)(host + ax.off_count);
        if (mlsd_resample_aa_taps(sw, dw, filter, wrap & 1, h_start, h_count, (float*)(host + ax.off_w), ax.K) < 0) { free(host); return mlsd_set_error(-1, "mlsd_resample2d_aa: column taps"); }
        for (int x0 = 0; x0 < dw; x0 += H_TX) {
            const int x1 = (x0 + H_TX < dw ? x0 + H_TX : dw) - 1, len = h_start[x1] + h_count[x1] - h_start[x0];
            if (len > span) span = len;
        }
    }
    if (ax.K && sh == sw && dh == dw && ((wrap >> 1) & 1) == (wrap & 1)) memcpy(host + ay.off_start, host + ax.off_start, ax.end - ax.off_start);      // the same axis twice
    else if (ay.K && mlsd_resample_aa_taps(sh, dh, filter, (wrap >> 1) & 1, (int*)(host + ay.off_start), (int*)(host + ay.off_count), (float*)(host + ay.off_w), ay.K) < 0) {
        free(host); return mlsd_set_error(-1, "mlsd_resample2d_aa: row taps");
    }
    hipError_t e = hipMemcpyAsync(ws, host, ay.end, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    free(host);
    if (e != hipSuccess) { (void)hipGetLastError(); return mlsd_set_error(-(int)e - 1000, "mlsd_resample2d_aa: table upload failed: %s", hipGetErrorString(e)); }

    char* base = (char*)ws;
    const float* vsrc = src;      // what the vertical pass reads
    if (ax.K) {
        float* out = ay.K ? (float*)(base + ay.end) : dst;
        const long rows = (long)planes * sh;
        const int *d_start = (const int*)(base + ax.off_start), *d_count = (const int*)(base + ax.off_count);
        const float* d_w = (const float*)(base + ax.off_w);
        // rows per tile: the most of 16, 8, 4 whose spans fit beside the weights (the weights and two barriers are paid once per tile)
        int ty = H_TY_MAX;
        while (ty > H_WAVES && sizeof(float) * ((size_t)ty * span + (size_t)ax.K * H_TX) > (size_t)g_lds_limit) ty /= 2;
        const size_t lds = sizeof(float) * ((size_t)ty * span + (size_t)ax.K * H_TX);
        if (lds <= (size_t)g_lds_limit) {
            const int tiles_x = (dw + H_TX - 1) / H_TX;
            const long n_tiles = ((rows + ty - 1) / ty) * tiles_x;
            hipLaunchKernelGGL(aa_rows_lds, dim3(grid_for(n_tiles)), dim3(256), lds, st, src, sw, out, dw, rows, d_start, d_count, d_w, ax.K, span, ty, wrap & 1, n_tiles, tiles_x);
        } else {
            hipLaunchKernelGGL(aa_rows_direct, dim3(nblk(rows * dw)), dim3(256), 0, st, src, sw, out, dw, rows, d_start, d_count, d_w, ax.K, wrap & 1);
        }
        { const int r = mlsd_check_launch("resample2d_aa rows"); if (r) return r; }
        vsrc = out;
    }
    if (ay.K) {
        const int tiles_x = (dw + V_TX - 1) / V_TX;
        const long n_tiles = (long)planes * dh * tiles_x;
        hipLaunchKernelGGL(aa_cols, dim3(grid_for(n_tiles)), dim3(256), 0, st, vsrc, sh, dst, dh, dw, (const int*)(base + ay.off_start), (const int*)(base + ay.off_count),
                           (const float*)(base + ay.off_w), ay.K, (wrap >> 1) & 1, n_tiles, tiles_x);
        return mlsd_check_launch("resample2d_aa columns");
    }
    return 0;
}
