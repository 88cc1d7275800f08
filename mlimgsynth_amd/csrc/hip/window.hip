// Tiled diffusion (MultiDiffusion): the canvas latent is denoised in overlapping windows of the UNet plan's size and the windows' predictions are
// blended by a weighted average (mlsd_window_gather / _blend / _wsum, include/mlsd_kernels.h; the window loop is unet_eval of host/engine.c).
// All three are elementwise over a few hundred KB and launch-bound.  One thread per pixel, x fastest:
//   gather  reads a canvas row segment and writes a window row, both contiguous along the wave (a wrapped window splits the read in two);
//   blend   reads the window's first four channels (NHWC with the plan's row stride: 16 bytes of every ld_win * 4) and updates one float4 of the dense canvas;
//   wsum    walks the window lists of both axes per canvas pixel (a handful of windows: registers and the constant arguments only).
// The packed pair (mlsd_window_gather_packed / _blend_packed) serves the P windows of one batched plan evaluation per launch; it is what the engine calls, P = 1
// included, and the single-window pair stays exported as the statement the packed blend is tested against.  The windows of a group overlap, so
// the packed blend runs one thread per CANVAS pixel that walks the group's windows in slot order: no two threads touch the same float4, the summation order is
// the one of successive single-window launches, and the canvas is read and written once per group.  The gather takes its slot from blockIdx.y, so that the
// index into the by-value start lists is uniform over a wave (scalar loads of the kernel arguments, no private copy of the lists).
// The blend weight is a product of two integer ramps divided in fp32; blend and wsum compute it with the same function, so that where one window
// covers a pixel w / wsum is exactly 1.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

// r(i) = min(i + 1, T - i, O + 1) / (O + 1): linear over the overlap, 1 inside
__device__ __forceinline__ float ramp(int i, int T, int O)
{
    int m = i + 1 < T - i ? i + 1 : T - i;
    if (m > O + 1) m = O + 1;
    return __fdiv_rn((float)m, (float)(O + 1));
}
__device__ __forceinline__ float window_weight(int u, int v, int ww, int wh, int ox, int oy) { return __fmul_rn(ramp(v, wh, oy), ramp(u, ww, ox)); }

// position k of a window starting at s on an axis of extent L (s < L, k <= L): (s + k) mod L
__device__ __forceinline__ int wrap_at(int s, int k, int L) { const int p = s + k; return p >= L ? p - L : p; }

__global__ void window_gather_kernel(const uint32_t* __restrict__ canvas, int W, int H, uint32_t* __restrict__ win, int ww, int wh, int x0, int y0, int planes)
{
    const long total = (long)planes * wh * ww;
    GRID_LOOP(i, total) {
        const int u = (int)(i % ww);
        const long r = i / ww;
        const int v = (int)(r % wh);
        const long p = r / wh;
        win[i] = canvas[(p * H + wrap_at(y0, v, H)) * W + wrap_at(x0, u, W)];      // bits, not values: NaN payloads and -0 survive
    }
}

template <bool VEC>
__global__ void window_blend_kernel(const float* __restrict__ eps_win, long ld_win, float4* __restrict__ eps_canvas, const float* __restrict__ wsum,
                                    int W, int H, int ww, int wh, int x0, int y0, int ox, int oy, int N)
{
    const long total = (long)N * wh * ww;
    GRID_LOOP(i, total) {
        const int u = (int)(i % ww);
        const long r = i / ww;
        const int v = (int)(r % wh);
        const long n = r / wh;
        const long q = (long)wrap_at(y0, v, H) * W + wrap_at(x0, u, W);
        const float* src = eps_win + i * ld_win;
        float4 e;
        if (VEC) e = *reinterpret_cast<const float4*>(src);
        else e = make_float4(src[0], src[1], src[2], src[3]);
        const float f = __fdiv_rn(window_weight(u, v, ww, wh, ox, oy), wsum[q]);   // a division, not a stored reciprocal: exactly 1 under a single window
        float4 c = eps_canvas[n * ((long)H * W) + q];
        c.x = __fadd_rn(c.x, __fmul_rn(f, e.x)); c.y = __fadd_rn(c.y, __fmul_rn(f, e.y));
        c.z = __fadd_rn(c.z, __fmul_rn(f, e.z)); c.w = __fadd_rn(c.w, __fmul_rn(f, e.w));
        eps_canvas[n * ((long)H * W) + q] = c;
    }
}

struct WindowLists { int xs[MLSD_WINDOW_MAX_AXIS], ys[MLSD_WINDOW_MAX_AXIS]; };

// offset of canvas position p inside the window starting at s (extent T) on an axis of extent L, or -1: (p - s) mod L < T
__device__ __forceinline__ int window_offset(int p, int s, int T, int L) { int k = p - s; if (k < 0) k += L; return k < T ? k : -1; }

__global__ void window_wsum_kernel(float* __restrict__ wsum, int W, int H, int ww, int wh, WindowLists L, int nx, int ny, int ox, int oy)
{
    const long total = (long)H * W;
    GRID_LOOP(i, total) {
        const int x = (int)(i % W), y = (int)(i / W);
        float s = 0.f;
        for (int j = 0; j < ny; ++j) {           // the order of the blend launches: y outer, x inner
            const int v = window_offset(y, L.ys[j], wh, H);
            if (v < 0) continue;
            for (int k = 0; k < nx; ++k) {
                const int u = window_offset(x, L.xs[k], ww, W);
                if (u >= 0) s = __fadd_rn(s, window_weight(u, v, ww, wh, ox, oy));
            }
        }
        wsum[i] = s;
    }
}

struct WindowSlots { int xs[MLSD_WINDOW_MAX_PACK], ys[MLSD_WINDOW_MAX_PACK]; };

// win [n_slots][planes][wh][ww]: blockIdx.y is the slot, the x grid loops over one slot's planes * wh * ww elements
__global__ void window_gather_packed_kernel(const uint32_t* __restrict__ canvas, int W, int H, uint32_t* __restrict__ win, int ww, int wh, WindowSlots L, int planes)
{
    const int s = (int)blockIdx.y;
    const int x0 = L.xs[s], y0 = L.ys[s];
    const long total = (long)planes * wh * ww;
    uint32_t* __restrict__ dst = win + (long)s * total;
    GRID_LOOP(i, total) {
        const int u = (int)(i % ww);
        const long r = i / ww;
        const int v = (int)(r % wh);
        const long p = r / wh;
        dst[i] = canvas[(p * H + wrap_at(y0, v, H)) * W + wrap_at(x0, u, W)];      // bits, not values
    }
}

// eps_win NHWC [G][n_slots][B][wh ww][ld_win], eps_canvas [G B][H W] float4.  Thread (n, q): for every slot whose window covers q, in slot order, exactly the
// update of window_blend_kernel; the float4 is loaded at the first covering window and stored once after the last.
template <bool VEC>
__global__ void window_blend_packed_kernel(const float* __restrict__ eps_win, long ld_win, float4* __restrict__ eps_canvas, const float* __restrict__ wsum,
                                           int W, int H, int ww, int wh, WindowSlots L, int n_used, int n_slots, int ox, int oy, int B, int GB)
{
    const long hw = (long)H * W, whw = (long)wh * ww, total = (long)GB * hw;
    GRID_LOOP(i, total) {
        const long q = i % hw;
        const int n = (int)(i / hw), g = n / B, b = n - g * B;
        const int x = (int)(q % W), y = (int)(q / W);
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        float ws = 0.f;
        bool covered = false;
        for (int s = 0; s < n_used; ++s) {
            const int v = window_offset(y, L.ys[s], wh, H);
            if (v < 0) continue;
            const int u = window_offset(x, L.xs[s], ww, W);
            if (u < 0) continue;
            if (!covered) { c = eps_canvas[i]; ws = wsum[q]; covered = true; }
            const float* src = eps_win + ((((long)g * n_slots + s) * B + b) * whw + (long)v * ww + u) * ld_win;
            float4 e;
            if (VEC) e = *reinterpret_cast<const float4*>(src);
            else e = make_float4(src[0], src[1], src[2], src[3]);
            const float f = __fdiv_rn(window_weight(u, v, ww, wh, ox, oy), ws);
            c.x = __fadd_rn(c.x, __fmul_rn(f, e.x)); c.y = __fadd_rn(c.y, __fmul_rn(f, e.y));
            c.z = __fadd_rn(c.z, __fmul_rn(f, e.z)); c.w = __fadd_rn(c.w, __fmul_rn(f, e.w));
        }
        if (covered) eps_canvas[i] = c;
    }
}

int window_args_ok(const char* what, int W, int H, int ww, int wh, int x0, int y0)
{
    if (W < 1 || H < 1 || ww < 1 || wh < 1 || ww > W || wh > H || x0 < 0 || x0 >= W || y0 < 0 || y0 >= H)
        return mlsd_set_error(-1, "%s: window %dx%d at (%d, %d) of a %dx%d canvas", what, ww, wh, x0, y0, W, H);
    return 0;
}

}  // namespace

extern "C" MLSD_API int mlsd_window_gather(const float* canvas, int W, int H, float* win, int ww, int wh, int x0, int y0, int planes, void* stream)
{
    if (!canvas || !win || planes < 1) return mlsd_set_error(-1, "mlsd_window_gather: bad argument (%d planes)", planes);
    if (window_args_ok("mlsd_window_gather", W, H, ww, wh, x0, y0)) return -1;
    const long n_src = (long)planes * H * W, n_dst = (long)planes * wh * ww;
    if (n_src >= (1L << 31) || n_dst >= (1L << 31)) return mlsd_set_error(-1, "mlsd_window_gather: more than 2^31 elements");
    if (canvas < win + n_dst && win < canvas + n_src) return mlsd_set_error(-1, "mlsd_window_gather: canvas and window overlap");
    hipLaunchKernelGGL(window_gather_kernel, dim3(nblk(n_dst)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)canvas, W, H, (uint32_t*)win, ww, wh, x0, y0, planes);
    return mlsd_check_launch("window_gather");
}

extern "C" MLSD_API int mlsd_window_blend(const float* eps_win, int64_t ld_win, float* eps_canvas, const float* wsum, int W, int H, int ww, int wh,
                                          int x0, int y0, int ox, int oy, int N, int C, void* stream)
{
    if (!eps_win || !eps_canvas || !wsum || N < 1 || C != 4 || ld_win < C || ox < 0 || oy < 0 || ((uintptr_t)eps_canvas & 15))
        return mlsd_set_error(-1, "mlsd_window_blend: bad argument (N %d, C %d, ld %lld, overlap %d %d)", N, C, (long long)ld_win, ox, oy);
    if (window_args_ok("mlsd_window_blend", W, H, ww, wh, x0, y0)) return -1;
    const long n_win = (long)N * wh * ww, n_can = (long)N * H * W * C;
    if (n_can >= (1L << 31) || n_win * ld_win >= (1L << 31)) return mlsd_set_error(-1, "mlsd_window_blend: more than 2^31 elements");
    if (eps_win < eps_canvas + n_can && eps_canvas < eps_win + n_win * ld_win) return mlsd_set_error(-1, "mlsd_window_blend: window and canvas overlap");
    const bool vec = !(ld_win & 3) && !((uintptr_t)eps_win & 15);
    const dim3 grid(nblk(n_win)), block(256);
    if (vec) hipLaunchKernelGGL(window_blend_kernel<true>, grid, block, 0, (hipStream_t)stream, eps_win, (long)ld_win, (float4*)eps_canvas, wsum, W, H, ww, wh, x0, y0, ox, oy, N);
    else hipLaunchKernelGGL(window_blend_kernel<false>, grid, block, 0, (hipStream_t)stream, eps_win, (long)ld_win, (float4*)eps_canvas, wsum, W, H, ww, wh, x0, y0, ox, oy, N);
    return mlsd_check_launch("window_blend");
}

extern "C" MLSD_API int mlsd_window_wsum(float* wsum, int W, int H, int ww, int wh, const int* xs, int nx, const int* ys, int ny, int ox, int oy, void* stream)
{
    if (!wsum || !xs || !ys || nx < 1 || ny < 1 || nx > MLSD_WINDOW_MAX_AXIS || ny > MLSD_WINDOW_MAX_AXIS || ox < 0 || oy < 0)
        return mlsd_set_error(-1, "mlsd_window_wsum: bad argument (%d x %d windows, at most %d per axis; overlap %d %d)", nx, ny, MLSD_WINDOW_MAX_AXIS, ox, oy);
    if ((long)H * W >= (1L << 31)) return mlsd_set_error(-1, "mlsd_window_wsum: more than 2^31 elements");
    WindowLists L;
    for (int k = 0; k < nx; ++k) { if (window_args_ok("mlsd_window_wsum", W, H, ww, wh, xs[k], 0)) return -1; L.xs[k] = xs[k]; }
    for (int j = 0; j < ny; ++j) { if (window_args_ok("mlsd_window_wsum", W, H, ww, wh, 0, ys[j])) return -1; L.ys[j] = ys[j]; }
    for (int k = nx; k < MLSD_WINDOW_MAX_AXIS; ++k) L.xs[k] = 0;
    for (int j = ny; j < MLSD_WINDOW_MAX_AXIS; ++j) L.ys[j] = 0;
    hipLaunchKernelGGL(window_wsum_kernel, dim3(nblk((long)H * W)), dim3(256), 0, (hipStream_t)stream, wsum, W, H, ww, wh, L, nx, ny, ox, oy);
    return mlsd_check_launch("window_wsum");
}

// the starts of n_slots windows, checked and copied into the by-value lists (unused entries 0)
static int window_slots_get(const char* what, WindowSlots* L, int W, int H, int ww, int wh, const int* xs, const int* ys, int n_slots)
{
    if (!xs || !ys || n_slots < 1 || n_slots > MLSD_WINDOW_MAX_PACK)
        return mlsd_set_error(-1, "%s: bad argument (%d slots, 1 .. %d)", what, n_slots, MLSD_WINDOW_MAX_PACK);
    for (int s = 0; s < MLSD_WINDOW_MAX_PACK; ++s) {
        if (s < n_slots && window_args_ok(what, W, H, ww, wh, xs[s], ys[s])) return -1;
        L->xs[s] = s < n_slots ? xs[s] : 0; L->ys[s] = s < n_slots ? ys[s] : 0;
    }
    return 0;
}

extern "C" MLSD_API int mlsd_window_gather_packed(const float* canvas, int W, int H, float* win, int ww, int wh, const int* xs, const int* ys, int n_slots,
                                                  int planes, void* stream)
{
    if (!canvas || !win || planes < 1) return mlsd_set_error(-1, "mlsd_window_gather_packed: bad argument (%d planes)", planes);
    if (window_args_ok("mlsd_window_gather_packed", W, H, ww, wh, 0, 0)) return -1;
    WindowSlots L;
    if (window_slots_get("mlsd_window_gather_packed", &L, W, H, ww, wh, xs, ys, n_slots)) return -1;
    const long n_src = (long)planes * H * W, n_one = (long)planes * wh * ww, n_dst = n_one * n_slots;
    if (n_src >= (1L << 31) || n_dst >= (1L << 31)) return mlsd_set_error(-1, "mlsd_window_gather_packed: more than 2^31 elements");
    if (canvas < win + n_dst && win < canvas + n_src) return mlsd_set_error(-1, "mlsd_window_gather_packed: canvas and window overlap");
    hipLaunchKernelGGL(window_gather_packed_kernel, dim3(nblk(n_one), (unsigned)n_slots), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)canvas, W, H, (uint32_t*)win,
                       ww, wh, L, planes);
    return mlsd_check_launch("window_gather_packed");
}

extern "C" MLSD_API int mlsd_window_blend_packed(const float* eps_win, int64_t ld_win, float* eps_canvas, const float* wsum, int W, int H, int ww, int wh,
                                                 const int* xs, const int* ys, int n_used, int n_slots, int ox, int oy, int B, int G, int C, void* stream)
{
    if (!eps_win || !eps_canvas || !wsum || B < 1 || (G != 1 && G != 2) || C != 4 || ld_win < C || ox < 0 || oy < 0 || ((uintptr_t)eps_canvas & 15))
        return mlsd_set_error(-1, "mlsd_window_blend_packed: bad argument (B %d, G %d, C %d, ld %lld, overlap %d %d)", B, G, C, (long long)ld_win, ox, oy);
    if (window_args_ok("mlsd_window_blend_packed", W, H, ww, wh, 0, 0)) return -1;
    WindowSlots L;
    if (window_slots_get("mlsd_window_blend_packed", &L, W, H, ww, wh, xs, ys, n_slots)) return -1;
    if (n_used < 1 || n_used > n_slots) return mlsd_set_error(-1, "mlsd_window_blend_packed: %d used of %d slots", n_used, n_slots);
    const long n_pix = (long)G * B * H * W, n_can = n_pix * C, n_win = (long)G * n_slots * B * wh * ww;
    if (n_can >= (1L << 31) || n_win >= (1L << 31) || n_win * ld_win >= (1L << 31)) return mlsd_set_error(-1, "mlsd_window_blend_packed: more than 2^31 elements");
    if (eps_win < eps_canvas + n_can && eps_canvas < eps_win + n_win * ld_win) return mlsd_set_error(-1, "mlsd_window_blend_packed: window and canvas overlap");
    if (wsum < eps_canvas + n_can && eps_canvas < wsum + (long)H * W) return mlsd_set_error(-1, "mlsd_window_blend_packed: weight sum and canvas overlap");
    const bool vec = !(ld_win & 3) && !((uintptr_t)eps_win & 15);
    const dim3 grid(nblk(n_pix)), block(256);
    if (vec) hipLaunchKernelGGL(window_blend_packed_kernel<true>, grid, block, 0, (hipStream_t)stream, eps_win, (long)ld_win, (float4*)eps_canvas, wsum, W, H, ww, wh, L,
                                n_used, n_slots, ox, oy, B, G * B);
    else hipLaunchKernelGGL(window_blend_packed_kernel<false>, grid, block, 0, (hipStream_t)stream, eps_win, (long)ld_win, (float4*)eps_canvas, wsum, W, H, ww, wh, L,
                            n_used, n_slots, ox, oy, B, G * B);
    return mlsd_check_launch("window_blend_packed");
}
