// Colour correction of a re-denoised picture against the picture it started from (mlsd_colorfix_*, include/mlsd_kernels.h): wavelet, AdaIN and histogram matching.
// Planes are NCHW fp32, [B][c][h][w]; `content` is the generated picture, `target` the one whose colours are wanted (1 or B images).  None is in the reference; all
// three are as recalled from the front ends' extensions and parity-unpinned.  The rules are stated in full at the prototypes.
//
// WAVELET is the centre.  out = content + Low(target - content), Low = `levels` <= 5 levels of the a-trous low-pass (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4) with taps at
// distance 2^i in level i and indices clamped to the plane at every level.  As a composition of existing calls that is ten launches and ten trips through HBM; here ONE
// launch computes every level in LDS.
//   tile     a workgroup owns a 64 x 64 output tile of one plane (grid: tiles x, tiles y, planes).  Its halo is R = 2^levels - 1, so the patch is P x P, P = 64 + 2 R:
//            126 x 126 floats = 62 KiB at 5 levels.  Two patch buffers (ping-pong between the row and the column pass of a level) are 124 KiB of the CU's 160 KiB: one
//            workgroup per CU at 5 levels, hence 1024 lanes (16 waves) to hide the LDS latency on its own.  A 96- or 128-wide tile does not fit twice, and one buffer
//            is not enough: a pass reads taps other lanes are about to overwrite.  Read amplification of the staging: (P / 64)^2 = 3.88 at 5 levels, 1.06 at 1 level,
//            of reads that mostly hit L2 (the halo is the neighbour tiles' interior); LDS is sized per launch (dynamic), so fewer levels run several workgroups per CU.
//   staging  d = target - content (one fp32 rounding) for the patch slots that lie INSIDE the plane; slots outside are neither written nor ever read.
//   clamping slot (py, px) stands for plane pixel (y0 - R + py, x0 - R + px), so clamping a tap's pixel index to the plane is clamping its slot index to the staged
//            rectangle.  A clamped index lies between the pixel and the unclamped tap, so it is inside the region the previous level computed: an image smaller than
//            the halo (every tap clamps) takes the same path as a tile in the middle of a large image.  No fallback exists.
//   levels   with m_i = R - (2^(i+1) - 1) the margin still valid after level i, level i computes the slots of tile + m_i that lie in the plane: the row pass for the
//            rows of tile + m_(i-1) (the column taps need them), A -> B, then the column pass B -> A.  Valid widths: 124, 120, 112, 96, 64.
//   lanes    128 lanes along x, 8 along y, in BOTH passes: a wave reads 64 consecutive floats of one row at x - s, x, x + s (row pass) or of rows y - s, y, y + s
//            (column pass).  Consecutive floats fall into consecutive banks whatever the pitch, clamped lanes read one address (a broadcast): no bank conflict at any
//            pitch, so the pitch is P, unpadded.
//   order    t = (1/4 l + 1/2 c) + 1/4 r per pass, every product and sum an explicit _rn operation: the products are exact (powers of two), a level is 4 roundings.
//   in place dst may be content (or target): a tile's halo is another tile's output, so the launch then writes the workspace and a device copy follows.
//
// ADAIN has the shape of the guidance statistics: per block double sums of (x - x[0]) and its square through lanes (shuffle), waves (LDS, wave order) and ONE ordinary
// store; a second small launch adds the partials in block order and forms a, b in double.  The map is elementwise with 16-byte accesses where the planes allow.
//
// HISTOGRAM counts 256 bins per plane with LDS integer atomics into per-block partial histograms (ordinary stores), which the LUT launch adds in block order: exact,
// the same bits every run.  A wave whose 64 pixels share a bin serialises on it; at 4 bytes read per atomic that is still far from the memory time (profiles/
// colorfix.md).  The LUT is formed ON THE DEVICE, one 256-lane workgroup per plane in double: the call stays asynchronous on its stream, where a host LUT would wait
// for the counts and upload 1 KiB per plane.  No global atomics anywhere, no block waits on another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

enum { W_T = 64, W_MAXL = 5, W_XL = 128, W_YL = 8, W_THREADS = W_XL * W_YL,
       W_MAXP = W_T + 2 * ((1 << W_MAXL) - 1), W_MAX_LDS = 2 * W_MAXP * W_MAXP * 4,
       ST_THREADS = 256, ST_PER_BLOCK = 16384, ST_MAX_BLOCKS = 64 };

inline bool al16(const void* p) { return !((uintptr_t)p & 15); }
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
bool overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const char *pa = (const char*)a, *pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}
// blocks that share one plane's statistics: about 16 Ki elements each, at most 64
int stat_blocks(long n) { const long b = (n + ST_PER_BLOCK - 1) / ST_PER_BLOCK; return (int)(b < 1 ? 1 : (b > ST_MAX_BLOCKS ? ST_MAX_BLOCKS : b)); }

__device__ __forceinline__ int clampi(int j, int lo, int hi) { return j < lo ? lo : (j > hi ? hi : j); }
__device__ __forceinline__ int mini(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ float tap3(float l, float c, float r) { return __fadd_rn(__fadd_rn(__fmul_rn(0.25f, l), __fmul_rn(0.5f, c)), __fmul_rn(0.25f, r)); }
__device__ __forceinline__ int quantise(float v)      // rule (a) of mlsd_canny
{
    const float t = floorf(__fadd_rn(__fmul_rn(v, 255.0f), 0.5f));
    return (int)fminf(fmaxf(t, 0.0f), 255.0f);
}

// ------------------------------------------------------------------ wavelet
__global__ void __launch_bounds__(W_THREADS) wavelet_kernel(const float* __restrict__ content, const float* __restrict__ target, float* __restrict__ out, int w, int h,
                                                            int c, int nt, int levels)
{
    extern __shared__ float lds[];
    const int R = (1 << levels) - 1, P = W_T + 2 * R;
    float* A = lds;
    float* Bf = lds + P * P;
    const int x0 = blockIdx.x * W_T, y0 = blockIdx.y * W_T, plane = blockIdx.z;
    const long np = (long)w * h;
    const float* cp = content + plane * np;
    const float* tp = target + (nt == 1 ? plane % c : plane) * np;
    const int xl = threadIdx.x & (W_XL - 1), yl = threadIdx.x / W_XL;
    const int ox = x0 - R, oy = y0 - R;                      // plane pixel of slot (0, 0)
    // slots of tile + margin m that lie in the plane: [R - min(m, x0), R + min(64 + m, w - x0)) and likewise in y
    const int cx0 = R - mini(R, x0), cx1 = R + mini(W_T + R, w - x0), cy0 = R - mini(R, y0), cy1 = R + mini(W_T + R, h - y0);      // the staged rectangle

    for (int py = cy0 + yl; py < cy1; py += W_YL) {
        const int px = cx0 + xl;
        if (px < cx1) { const long at = (long)(oy + py) * w + (ox + px); A[py * P + px] = __fsub_rn(tp[at], cp[at]); }
    }
    __syncthreads();
    int m_prev = R;
    for (int i = 0; i < levels; ++i) {
        const int s = 1 << i, m = m_prev - s;
        const int xa = R - mini(m, x0), xb = R + mini(W_T + m, w - x0), ya = R - mini(m, y0), yb = R + mini(W_T + m, h - y0);
        const int ra = R - mini(m_prev, y0), rb = R + mini(W_T + m_prev, h - y0);
        const int px = xa + xl;
        if (px < xb) {
            const int pl = clampi(px - s, cx0, cx1 - 1), pr = clampi(px + s, cx0, cx1 - 1);
            for (int py = ra + yl; py < rb; py += W_YL) Bf[py * P + px] = tap3(A[py * P + pl], A[py * P + px], A[py * P + pr]);
        }
        __syncthreads();
        if (px < xb)
            for (int py = ya + yl; py < yb; py += W_YL) {
                const int pu = clampi(py - s, cy0, cy1 - 1), pd = clampi(py + s, cy0, cy1 - 1);
                A[py * P + px] = tap3(Bf[pu * P + px], Bf[py * P + px], Bf[pd * P + px]);
            }
        __syncthreads();
        m_prev = m;
    }
    const int tw = mini(W_T, w - x0), th = mini(W_T, h - y0);
    if (xl < tw)
        for (int ty = yl; ty < th; ty += W_YL) {
            const long at = (long)(y0 + ty) * w + (x0 + xl);
            out[plane * np + at] = __fadd_rn(cp[at], A[(R + ty) * P + R + xl]);
        }
}

// ------------------------------------------------------------------ sums
// lanes (shuffle tree), waves (LDS, wave order), then thread 0 stores the block's two doubles
__device__ __forceinline__ void block_sum_store2(double s0, double s1, double* dst)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_down(s0, o, 64); s1 += __shfl_down(s1, o, 64); }
    __shared__ double sh[ST_THREADS / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[wave][0] = s0; sh[wave][1] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        dst[0] = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
        dst[1] = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
    }
}

// the run of elements [i0, i1) of a plane of n that block blockIdx.x of gridDim.x owns; whole quads but for the plane's end
__device__ __forceinline__ void block_run(long n, long* i0, long* i1)
{
    const long chunk = (((n + gridDim.x - 1) / gridDim.x) + 3) & ~3L;
    *i0 = (long)blockIdx.x * chunk;
    *i1 = *i0 + chunk < n ? *i0 + chunk : n;
}

// part[plane][block][2] = sum of (x - x[0]) and of its square over the block's run, in double.  V4: n % 4 == 0 and 16-byte aligned planes.  grid (blocks, planes)
template <bool V4>
__global__ void __launch_bounds__(ST_THREADS) adain_sums_kernel(const float* __restrict__ x, long n, double* __restrict__ part)
{
    const float* p = x + (long)blockIdx.y * n;
    const double K = (double)p[0];
    long i0, i1; block_run(n, &i0, &i1);
    double s0 = 0.0, s1 = 0.0;
    const auto acc = [&](float v) { const double d = (double)v - K; s0 += d; s1 += d * d; };
    if constexpr (V4) {
        for (long i = i0 + 4 * (long)threadIdx.x; i < i1; i += 4 * ST_THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(p + i);
            acc(v.x); acc(v.y); acc(v.z); acc(v.w);
        }
    } else
        for (long i = i0 + threadIdx.x; i < i1; i += ST_THREADS) acc(p[i]);
    block_sum_store2(s0, s1, part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2);
}

// coef[plane] = (a, b): thread per content plane, the partials added in block order
__global__ void adain_coef_kernel(const float* __restrict__ content, long n_c, const double* __restrict__ part_c, int nb_c, const float* __restrict__ target, long n_t,
                                  const double* __restrict__ part_t, int nb_t, int planes, int c, int nt, float* __restrict__ coef)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= planes) return;
    float a = 1.0f, b = 0.0f;
    if (n_c >= 2 && n_t >= 2) {
        const int q = nt == 1 ? p % c : p;
        double sc[2] = { 0.0, 0.0 }, stt[2] = { 0.0, 0.0 };
        for (int j = 0; j < nb_c; ++j) { sc[0] += part_c[((long)p * nb_c + j) * 2]; sc[1] += part_c[((long)p * nb_c + j) * 2 + 1]; }
        for (int j = 0; j < nb_t; ++j) { stt[0] += part_t[((long)q * nb_t + j) * 2]; stt[1] += part_t[((long)q * nb_t + j) * 2 + 1]; }
        const double mean_c = (double)content[(long)p * n_c] + sc[0] / (double)n_c, mean_t = (double)target[(long)q * n_t] + stt[0] / (double)n_t;
        double var_c = (sc[1] - sc[0] * sc[0] / (double)n_c) / (double)(n_c - 1), var_t = (stt[1] - stt[0] * stt[0] / (double)n_t) / (double)(n_t - 1);
        if (var_c < 0.0) var_c = 0.0;
        if (var_t < 0.0) var_t = 0.0;
        const double ad = sqrt(var_t + 1e-5) / sqrt(var_c + 1e-5);
        a = (float)ad; b = (float)(mean_t - mean_c * ad);
    }
    coef[2 * p] = a; coef[2 * p + 1] = b;
}

// ------------------------------------------------------------------ histogram
// part[plane][block][256]: the block's run counted in LDS, stored with ordinary stores.  grid (blocks, planes)
template <bool V4>
__global__ void __launch_bounds__(ST_THREADS) hist_count_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ part)
{
    __shared__ unsigned bins[256];
    const float* p = x + (long)blockIdx.y * n;
    long i0, i1; block_run(n, &i0, &i1);
    bins[threadIdx.x] = 0u;
    __syncthreads();
    if constexpr (V4) {
        for (long i = i0 + 4 * (long)threadIdx.x; i < i1; i += 4 * ST_THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(p + i);
            atomicAdd(&bins[quantise(v.x)], 1u); atomicAdd(&bins[quantise(v.y)], 1u); atomicAdd(&bins[quantise(v.z)], 1u); atomicAdd(&bins[quantise(v.w)], 1u);
        }
    } else
        for (long i = i0 + threadIdx.x; i < i1; i += ST_THREADS) atomicAdd(&bins[quantise(p[i])], 1u);
    __syncthreads();
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x] = bins[threadIdx.x];
}

// one workgroup of 256 lanes per content plane, lane v = level v: counts (partials in block order), cumulative shares, the present target levels, the interpolation
__global__ void __launch_bounds__(256) hist_lut_kernel(const unsigned* __restrict__ part_c, int nb_c, long n_c, const unsigned* __restrict__ part_t, int nb_t, long n_t,
                                                       int c, int nt, unsigned* __restrict__ counts_c, unsigned* __restrict__ counts_t, float* __restrict__ lut)
{
    __shared__ unsigned cc[256], ct[256];
    __shared__ double qv[256];
    __shared__ int lv[256], n_lv;
    const int p = blockIdx.x, q = nt == 1 ? p % c : p, v = threadIdx.x;
    unsigned kc = 0u, kt = 0u;
    for (int j = 0; j < nb_c; ++j) kc += part_c[((long)p * nb_c + j) * 256 + v];
    for (int j = 0; j < nb_t; ++j) kt += part_t[((long)q * nb_t + j) * 256 + v];
    cc[v] = kc; ct[v] = kt;
    counts_c[(long)p * 256 + v] = kc;
    if (nt != 1 || p < c) counts_t[(long)q * 256 + v] = kt;      // a shared target plane is written by one workgroup
    __syncthreads();
    // lane v: the cumulative counts up to v, and its rank among the levels present in the target (V, ascending, with their cumulative shares)
    unsigned long long cum_c = 0ull, cum_t = 0ull;
    int rank = 0;
    for (int j = 0; j <= v; ++j) { cum_c += cc[j]; cum_t += ct[j]; rank += (j < v && ct[j]) ? 1 : 0; }
    if (kt) { lv[rank] = v; qv[rank] = (double)cum_t / (double)n_t; }
    if (v == 255) n_lv = rank + (kt ? 1 : 0);
    __syncthreads();
    const double xq = (double)cum_c / (double)n_c;
    const int k = n_lv;
    double r;
    if (xq <= qv[0]) r = (double)lv[0];
    else if (xq >= qv[k - 1]) r = (double)lv[k - 1];
    else {
        int j = 0;
        while (j + 2 < k && qv[j + 1] <= xq) ++j;
        const double slope = (double)(lv[j + 1] - lv[j]) / (qv[j + 1] - qv[j]);
        r = slope * (xq - qv[j]) + (double)lv[j];
    }
    lut[(long)p * 256 + v] = (float)(r / 255.0);
}

// ------------------------------------------------------------------ the two maps.  grid (blocks, planes); V4 as above, for x and out
// MODE 0: out = x a + b (a == 1 and b == 0: a copy of the bits);  MODE 1: out = lut[quantise(x)], the plane's LUT in LDS
template <int MODE, bool V4>
__global__ void __launch_bounds__(256) map_kernel(const float* __restrict__ x, float* __restrict__ out, long n, const float* __restrict__ tab)
{
    __shared__ float s_lut[256];
    const int plane = blockIdx.y;
    float a = 1.0f, b = 0.0f;
    if constexpr (MODE == 1) { s_lut[threadIdx.x] = tab[(long)plane * 256 + threadIdx.x]; __syncthreads(); }
    else { a = tab[2 * plane]; b = tab[2 * plane + 1]; }
    const bool copy = MODE == 0 && a == 1.0f && b == 0.0f;
    const auto f = [&](float v) -> float {
        if constexpr (MODE == 1) return s_lut[quantise(v)];
        else return copy ? v : __fadd_rn(__fmul_rn(v, a), b);
    };
    const float* xp = x + (long)plane * n;
    float* op = out + (long)plane * n;
    const long step = (long)gridDim.x * blockDim.x;
    if constexpr (V4) {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n / 4; i += step) {
            const float4 v = reinterpret_cast<const float4*>(xp)[i];
            reinterpret_cast<float4*>(op)[i] = make_float4(f(v.x), f(v.y), f(v.z), f(v.w));
        }
    } else
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) op[i] = f(xp[i]);
}

// ------------------------------------------------------------------ launching
struct Shape { int w, h, tw, th, c, B, nt; long n_c, n_t; int planes_c, planes_t, nb_c, nb_t; };

// what every entry refuses: 0 and *s filled when the arguments are good
int shape_check(const char* what, int w, int h, int tw, int th, int c, int B, int nt, Shape* s)
{
    if (w < 1 || h < 1 || tw < 1 || th < 1 || c < 1 || B < 1 || (nt != 1 && nt != B)) return mlsd_set_error(-1, "%s: bad shape (%dx%d, target %dx%d, c %d, B %d, %d target images)", what, w, h, tw, th, c, B, nt);
    if ((long)w * h >= (1L << 29) || (long)tw * th >= (1L << 29)) return mlsd_set_error(-1, "%s: a plane of 2^31 bytes or more", what);
    if ((long)c * B > 65535) return mlsd_set_error(-1, "%s: more than 65535 planes", what);
    s->w = w; s->h = h; s->tw = tw; s->th = th; s->c = c; s->B = B; s->nt = nt;
    s->n_c = (long)w * h; s->n_t = (long)tw * th; s->planes_c = c * B; s->planes_t = c * nt;
    s->nb_c = stat_blocks(s->n_c); s->nb_t = stat_blocks(s->n_t);
    return 0;
}

size_t ws_need(int mode, const Shape& s)
{
    const size_t parts = (size_t)s.planes_c * s.nb_c + (size_t)s.planes_t * s.nb_t;
    if (mode == MLSD_COLORFIX_WAVELET) return align256((size_t)s.planes_c * s.n_c * 4);
    if (mode == MLSD_COLORFIX_ADAIN) return align256(parts * 2 * sizeof(double)) + align256((size_t)s.planes_c * 2 * sizeof(float));
    return align256(parts * 256 * 4) + align256((size_t)(s.planes_c + s.planes_t) * 256 * 4) + align256((size_t)s.planes_c * 256 * 4);
}

// content, target, dst and ws as the elementwise modes allow them: dst may be content itself, nothing else may overlap
int buffers_check(const char* what, const Shape& s, int mode, const float* content, const float* target, const float* dst, const void* ws)
{
    if (!content || !target || !dst || !ws) return mlsd_set_error(-1, "%s: NULL buffer", what);
    const size_t nc = (size_t)s.planes_c * s.n_c * 4, ntb = (size_t)s.planes_t * s.n_t * 4, nw = ws_need(mode, s);
    if (((uintptr_t)ws & 7) || overlap(ws, nw, content, nc) || overlap(ws, nw, target, ntb) || overlap(ws, nw, dst, nc) || overlap(dst, nc, target, ntb)
            || (dst != content && overlap(dst, nc, content, nc)))
        return mlsd_set_error(-1, "%s: buffers overlap (dst may be content, nothing else), or a workspace that is not 8-byte aligned", what);
    return 0;
}

// an optional output of `bytes` bytes (coef, counts, lut; NULL = kept in ws): 4-byte aligned and apart from content, target, dst, ws and the other output
int output_check(const char* what, const Shape& s, int mode, const void* out, size_t bytes, const float* content, const float* target, const float* dst, const void* ws,
                 const void* other, size_t other_bytes)
{
    if (!out) return 0;
    const size_t nc = (size_t)s.planes_c * s.n_c * 4, ntb = (size_t)s.planes_t * s.n_t * 4;
    if (((uintptr_t)out & 3) || overlap(out, bytes, content, nc) || overlap(out, bytes, target, ntb) || overlap(out, bytes, dst, nc) || overlap(out, bytes, ws, ws_need(mode, s))
            || (other && overlap(out, bytes, other, other_bytes)))
        return mlsd_set_error(-1, "%s: an output (coef, counts, lut) that overlaps another buffer or is not 4-byte aligned", what);
    return 0;
}

bool plane_v4(const void* p, long n) { return !(n & 3) && al16(p); }
unsigned map_blocks(long n, int planes) { const long want = 16384 / (planes < 1 ? 1 : planes) + 1; const unsigned b = nblk(n / 4 + 1); return (unsigned)(b < want ? b : want); }

template <int MODE>
int launch_map(const char* what, const float* x, float* out, long n, int planes, const float* tab, hipStream_t st)
{
    const dim3 grid(map_blocks(n, planes), (unsigned)planes);
    if (plane_v4(x, n) && plane_v4(out, n)) hipLaunchKernelGGL((map_kernel<MODE, true>), grid, dim3(256), 0, st, x, out, n, tab);
    else hipLaunchKernelGGL((map_kernel<MODE, false>), grid, dim3(256), 0, st, x, out, n, tab);
    return mlsd_check_launch(what);
}

}  // namespace

extern "C" {

MLSD_API int mlsd_colorfix_tile(int which)
{
    switch (which) { case 0: return W_T; case 1: return W_MAXL; case 2: return W_THREADS; case 3: return W_MAX_LDS; case 4: return ST_MAX_BLOCKS; }
    return -1;
}

MLSD_API size_t mlsd_colorfix_ws_bytes(int mode, int w, int h, int tw, int th, int c, int B, int nt)
{
    Shape s;
    if (mode < MLSD_COLORFIX_WAVELET || mode > MLSD_COLORFIX_HISTOGRAM || shape_check("mlsd_colorfix_ws_bytes", w, h, tw, th, c, B, nt, &s)) return 0;
    if (mode == MLSD_COLORFIX_WAVELET && (tw != w || th != h)) return 0;
    return ws_need(mode, s);
}

MLSD_API int mlsd_colorfix_wavelet(const float* content, const float* target, float* dst, int w, int h, int c, int B, int nt, int levels, void* ws, void* stream)
{
    const char* what = "mlsd_colorfix_wavelet";
    Shape s;
    if (shape_check(what, w, h, w, h, c, B, nt, &s)) return -1;
    if (levels < 1 || levels > W_MAXL) return mlsd_set_error(-1, "%s: %d levels (1 .. %d)", what, levels, (int)W_MAXL);
    if (!content || !target || !dst) return mlsd_set_error(-1, "%s: NULL buffer", what);
    const size_t nc = (size_t)s.planes_c * s.n_c * 4, ntb = (size_t)s.planes_t * s.n_t * 4;
    // a tile's halo is another tile's output: a dst that is content or target goes through the workspace
    const bool in_place = overlap(dst, nc, content, nc) || overlap(dst, nc, target, ntb);
    if (in_place) {
        if (dst != content && dst != target) return mlsd_set_error(-1, "%s: dst overlaps an input without being it", what);
        if (!ws || overlap(ws, nc, content, nc) || overlap(ws, nc, target, ntb)) return mlsd_set_error(-1, "%s: in place needs a workspace of its own", what);
    }
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    const int P = W_T + 2 * ((1 << levels) - 1);
    const size_t lds = (size_t)2 * P * P * 4;
    if (lds > 64 * 1024) {
        static bool lds_set[64];      // per device, as mlsd_guidance_plane_select does (two host threads racing here set the same attribute twice at worst)
        int dev = 0;
        MLSD_HIP_TRY(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !lds_set[dev]) {
            MLSD_HIP_TRY(hipFuncSetAttribute((const void*)wavelet_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, W_MAX_LDS));
            if (dev >= 0 && dev < 64) lds_set[dev] = true;
        }
    }
    float* out = in_place ? (float*)ws : dst;
    const dim3 grid((unsigned)((w + W_T - 1) / W_T), (unsigned)((h + W_T - 1) / W_T), (unsigned)s.planes_c);
    if (grid.y > 65535) return mlsd_set_error(-1, "%s: more than 65535 tile rows", what);
    hipLaunchKernelGGL(wavelet_kernel, grid, dim3(W_THREADS), lds, st, content, target, out, w, h, c, nt, levels);
    if (mlsd_check_launch(what)) return -1;
    if (in_place) MLSD_HIP_TRY(hipMemcpyAsync(dst, ws, nc, hipMemcpyDeviceToDevice, st));
    return 0;
}

MLSD_API int mlsd_colorfix_adain(const float* content, int w, int h, const float* target, int tw, int th, float* dst, int c, int B, int nt, void* ws, float* coef,
                                 void* stream)
{
    const char* what = "mlsd_colorfix_adain";
    Shape s;
    if (shape_check(what, w, h, tw, th, c, B, nt, &s) || buffers_check(what, s, MLSD_COLORFIX_ADAIN, content, target, dst, ws)
            || output_check(what, s, MLSD_COLORFIX_ADAIN, coef, (size_t)s.planes_c * 2 * sizeof(float), content, target, dst, ws, nullptr, 0)) return -1;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    double* part_c = (double*)ws;
    double* part_t = part_c + (size_t)s.planes_c * s.nb_c * 2;
    if (!coef) coef = (float*)((char*)ws + align256(((size_t)s.planes_c * s.nb_c + (size_t)s.planes_t * s.nb_t) * 2 * sizeof(double)));
    if (plane_v4(content, s.n_c)) hipLaunchKernelGGL((adain_sums_kernel<true>), dim3(s.nb_c, s.planes_c), dim3(ST_THREADS), 0, st, content, s.n_c, part_c);
    else hipLaunchKernelGGL((adain_sums_kernel<false>), dim3(s.nb_c, s.planes_c), dim3(ST_THREADS), 0, st, content, s.n_c, part_c);
    if (mlsd_check_launch(what)) return -1;
    if (plane_v4(target, s.n_t)) hipLaunchKernelGGL((adain_sums_kernel<true>), dim3(s.nb_t, s.planes_t), dim3(ST_THREADS), 0, st, target, s.n_t, part_t);
    else hipLaunchKernelGGL((adain_sums_kernel<false>), dim3(s.nb_t, s.planes_t), dim3(ST_THREADS), 0, st, target, s.n_t, part_t);
    if (mlsd_check_launch(what)) return -1;
    hipLaunchKernelGGL(adain_coef_kernel, dim3((s.planes_c + 63) / 64), dim3(64), 0, st, content, s.n_c, (const double*)part_c, s.nb_c, target, s.n_t, (const double*)part_t,
                       s.nb_t, s.planes_c, c, nt, coef);
    if (mlsd_check_launch(what)) return -1;
    return launch_map<0>(what, content, dst, s.n_c, s.planes_c, coef, st);
}

MLSD_API int mlsd_colorfix_histogram(const float* content, int w, int h, const float* target, int tw, int th, float* dst, int c, int B, int nt, void* ws,
                                     unsigned* counts, float* lut, void* stream)
{
    const char* what = "mlsd_colorfix_histogram";
    Shape s;
    if (shape_check(what, w, h, tw, th, c, B, nt, &s) || buffers_check(what, s, MLSD_COLORFIX_HISTOGRAM, content, target, dst, ws)) return -1;
    const size_t n_counts = (size_t)(s.planes_c + s.planes_t) * 256 * 4, n_lut = (size_t)s.planes_c * 256 * 4;
    if (output_check(what, s, MLSD_COLORFIX_HISTOGRAM, counts, n_counts, content, target, dst, ws, lut, n_lut)
            || output_check(what, s, MLSD_COLORFIX_HISTOGRAM, lut, n_lut, content, target, dst, ws, nullptr, 0)) return -1;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    const size_t parts = (size_t)s.planes_c * s.nb_c + (size_t)s.planes_t * s.nb_t;
    unsigned* part_c = (unsigned*)ws;
    unsigned* part_t = part_c + (size_t)s.planes_c * s.nb_c * 256;
    if (!counts) counts = (unsigned*)((char*)ws + align256(parts * 256 * 4));
    if (!lut) lut = (float*)((char*)ws + align256(parts * 256 * 4) + align256((size_t)(s.planes_c + s.planes_t) * 256 * 4));
    if (plane_v4(content, s.n_c)) hipLaunchKernelGGL((hist_count_kernel<true>), dim3(s.nb_c, s.planes_c), dim3(ST_THREADS), 0, st, content, s.n_c, part_c);
    else hipLaunchKernelGGL((hist_count_kernel<false>), dim3(s.nb_c, s.planes_c), dim3(ST_THREADS), 0, st, content, s.n_c, part_c);
    if (mlsd_check_launch(what)) return -1;
    if (plane_v4(target, s.n_t)) hipLaunchKernelGGL((hist_count_kernel<true>), dim3(s.nb_t, s.planes_t), dim3(ST_THREADS), 0, st, target, s.n_t, part_t);
    else hipLaunchKernelGGL((hist_count_kernel<false>), dim3(s.nb_t, s.planes_t), dim3(ST_THREADS), 0, st, target, s.n_t, part_t);
    if (mlsd_check_launch(what)) return -1;
    hipLaunchKernelGGL(hist_lut_kernel, dim3(s.planes_c), dim3(256), 0, st, (const unsigned*)part_c, s.nb_c, s.n_c, (const unsigned*)part_t, s.nb_t, s.n_t, c, nt, counts,
                       counts + (size_t)s.planes_c * 256, lut);
    if (mlsd_check_launch(what)) return -1;
    return launch_map<1>(what, content, dst, s.n_c, s.planes_c, lut, st);
}

}  // extern "C"
