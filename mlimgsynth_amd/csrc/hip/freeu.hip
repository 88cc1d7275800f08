// FreeU ("Free Lunch in Diffusion U-Net", version 2; the FreeU inputs of mlb_unet_denoise_freeu, host/unet.c): the two passes the feature runs in front of a decoder
// concatenation, both on channels-last fp32 maps with row strides, both a reduction followed by an apply.
//   mlsd_freeu_backbone   m[n,p] = mean over the C channels of x[n,p,:], mh = (m - min_p m) / (max_p m - min_p m) per image, and
//                         x'[n,p,c] = x[n,p,c] ((b - 1) mh[n,p] + 1) for c < C / 2; the other half keeps its bits.  max == min: the factor is 1.
//   mlsd_freeu_skip       the published Fourier filter (the four centred DFT bins {0,-1} x {0,-1} times s, real part of the inverse) in its closed form
//                         h'[y,x] = h[y,x] + (s - 1) / (H W) sum_{y',x'} h[y',x'] (1 + cos t + cos f + cos(t + f)),  t = 2 pi (y' - y) / H, f = 2 pi (x' - x) / W,
//                         per image and channel: seven plane sums (v, v cos a', v sin a', v cos b', v sin b', v cos(a'+b'), v sin(a'+b'); a' = 2 pi y' / H,
//                         b' = 2 pi x' / W) and a seven-term apply with the target pixel's angles.  Holds for H, W >= 2 only.
// b and s are ONE float in device memory each, read by every lane through the kernel's pointer argument (a uniform load): they change between launches, and
// under a captured graph, without touching the plan.  A value of exactly 1 makes the launch a bit copy of src: the reduction kernels return at once and the apply
// kernel never reads the workspace.
//
// Summation order (both kernels; no atomics, the same bits every run).  The n terms of a sum (the C channels of a pixel; the H W pixels of a plane) go to 256
// slots, every slot adds its ceil(n / 256) terms one after the other, then the 256 slot sums meet in a balanced binary tree of 8 levels:
//   backbone: a wave per pixel; slot = (lane, component of its float4), the lane's vectors are c4 = lane, lane + 64, ..; tree: (x + y) + (z + w), then 6 butterfly
//             levels across the wave (lane ^ 32, 16, .., 1).
//   skip:     a block per (image, 64 channels, part k of 16); slot = (part k, pixel lane pl of 16), its pixels are k L + pl + 16 i with L = 16 ceil(H W / 256); tree: two
//             butterfly levels inside the wave (pixel lanes pl ^ 1, pl ^ 2), the block's four waves as (w0 + w1) + (w2 + w3) through LDS, the 16 parts from the
//             workspace in a 4-level tree (freeu_skip_combine_kernel).  The products v cos, v sin enter through a fused multiply-add: one rounding per term.
// mlsd_freeu_depth(n) = ceil(n / 256) - 1 + 8 is therefore the largest number of fp32 additions between a term and its finished sum, for either kernel.
//
// Trig values: sincospif of an exact rational.  The angle 2 pi k / L (k < L integers) is cut into its quarter q = 4 k / L and the rest r = 4 k - q L in integers;
// sincospif(r / (2 L)) sees an argument in [0, 1/2) with ONE rounding and the quarter turn is a swap and a sign.  A block keeps the H + W pairs in LDS; the pair of
// a' + b' comes from the angle-addition formulas.
//
// Shapes: both passes move bytes, so lanes run along C (16 bytes each, a wave covers whole 256-byte row segments) and the grid follows the data, not the planes:
// 8 images of 128 x 128 x 640 are 8 x 10 x 16 = 1280 blocks in the skip kernels and 8 x 256 in the backbone's; 2 x 2 x 8 is one wave's worth of work in one block per
// image, the idle lanes masked.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

constexpr int kMaxSide = 1024;      // H, W of the skip filter: the LDS table holds H + W (cos, sin) pairs
constexpr int kParts = 16;          // pixel parts of a plane in the skip reduction
constexpr int kRowBlocks = 256;     // at most this many blocks per image in the backbone's mean pass (each leaves one (min, max) pair)

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }

// (cos, sin) of 2 pi k / L, 0 <= k < L
__device__ __forceinline__ float2 unit_root(int k, int L)
{
    const int q = (int)(4L * k / L), r = (int)(4L * k - (long)q * L);      // angle = (pi / 2) (q + r / L)
    float s, c;
    sincospif((float)r / (float)(2 * L), &s, &c);
    switch (q) {
    case 0: return make_float2(c, s);
    case 1: return make_float2(-s, c);
    case 2: return make_float2(-c, -s);
    default: return make_float2(s, -c);
    }
}

// ------------------------------------------------------------------ backbone
// grid (blocks, images), 4 waves per block, a wave per pixel: mean[n][p], and per block the (min, max) of the means its waves produced -> mm[n][block][2]
__global__ void freeu_mean_kernel(const float* __restrict__ src, long ld_src, int rows, int C4, float* __restrict__ mean, float* __restrict__ mm,
                                  const float* __restrict__ b_dev)
{
    if (*b_dev == 1.f) return;
    __shared__ float s_mn[4], s_mx[4];
    const int n = (int)blockIdx.y, lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const float* __restrict__ img = src + (long)n * rows * ld_src;
    float mn = INFINITY, mx = -INFINITY;
    for (int r = (int)blockIdx.x * 4 + wave; r < rows; r += (int)gridDim.x * 4) {
        const float4* __restrict__ row = reinterpret_cast<const float4*>(img + (long)r * ld_src);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int v = lane; v < C4; v += 64) { const float4 t = row[v]; a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w; }
        float s = (a.x + a.y) + (a.z + a.w);
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);      // a + b == b + a: every lane ends with the same bits
        const float m = s / (float)(4 * C4);
        if (lane == 0) mean[(long)n * rows + r] = m;
        mn = fminf(mn, m); mx = fmaxf(mx, m);
    }
    if (lane == 0) { s_mn[wave] = mn; s_mx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = mm + ((long)n * gridDim.x + blockIdx.x) * 2;
        o[0] = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
        o[1] = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    }
}

// grid (blocks, images): the image's (min, max) from the n_mm pairs (min and max are exact in any order), then one float4 per thread step over [rows][C / 4]
__global__ void freeu_backbone_apply_kernel(float* __restrict__ dst, long ld_dst, const float* __restrict__ src, long ld_src, int rows, int C4,
                                            const float* __restrict__ mean, const float* __restrict__ mm, int n_mm, const float* __restrict__ b_dev)
{
    const float b = *b_dev;
    const int n = (int)blockIdx.y;
    const long total = (long)rows * C4;
    float* __restrict__ out = dst + (long)n * rows * ld_dst;
    const float* __restrict__ in = src + (long)n * rows * ld_src;
    if (b == 1.f) {                                     // (uniform over the grid)
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
            const long r = i / C4; const int c = (int)(i - r * C4) * 4;
            *reinterpret_cast<u32x4*>(out + r * ld_dst + c) = *reinterpret_cast<const u32x4*>(in + r * ld_src + c);      // bits, not values
        }
        return;
    }
    __shared__ float s_mn[4], s_mx[4];
    float mn = INFINITY, mx = -INFINITY;
    if ((int)threadIdx.x < n_mm) { mn = mm[((long)n * n_mm + threadIdx.x) * 2]; mx = mm[((long)n * n_mm + threadIdx.x) * 2 + 1]; }      // n_mm <= 256 = blockDim.x
    mn = wave_min(mn); mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) { s_mn[threadIdx.x >> 6] = mn; s_mx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    mn = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    const float span = mx - mn, bm1 = b - 1.f;
    const bool flat = !(span > 0.f);                    // max == min (one pixel, a constant map), or NaN: the published code divides by zero; here the factor is 1
    const int half = C4 * 2;                            // C / 2 in floats: C % 8 == 0 puts it on a vector boundary
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / C4; const int c = (int)(i - r * C4) * 4;
        if (c >= half || flat) {
            *reinterpret_cast<u32x4*>(out + r * ld_dst + c) = *reinterpret_cast<const u32x4*>(in + r * ld_src + c);
            continue;
        }
        const float f = bm1 * ((mean[(long)n * rows + r] - mn) / span) + 1.f;
        const float4 v = *reinterpret_cast<const float4*>(in + r * ld_src + c);
        *reinterpret_cast<float4*>(out + r * ld_dst + c) = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
    }
}

// ------------------------------------------------------------------ skip
// the block's table: tab[y] = (cos, sin)(2 pi y / H) for y < H, tab[H + x] = (cos, sin)(2 pi x / W) for x < W
__device__ __forceinline__ void trig_table(float2* tab, int H, int W)
{
    for (int i = (int)threadIdx.x; i < H + W; i += (int)blockDim.x) tab[i] = i < H ? unit_root(i, H) : unit_root(i - H, W);
    __syncthreads();
}

struct Trig { float ca, sa, cb, sb, cab, sab; };
__device__ __forceinline__ Trig trig_at(const float2* tab, int p, int H, int W)
{
    const int y = p / W, x = p - y * W;
    const float2 a = tab[y], b = tab[H + x];
    Trig t;
    t.ca = a.x; t.sa = a.y; t.cb = b.x; t.sb = b.y;
    t.cab = a.x * b.x - a.y * b.y; t.sab = a.y * b.x + a.x * b.y;
    return t;
}

#define FMA4(acc, v, t) do { acc.x = __fmaf_rn(v.x, t, acc.x); acc.y = __fmaf_rn(v.y, t, acc.y); acc.z = __fmaf_rn(v.z, t, acc.z); acc.w = __fmaf_rn(v.w, t, acc.w); } while (0)
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 shfl4(float4 a, int o) { return make_float4(__shfl_xor(a.x, o, 64), __shfl_xor(a.y, o, 64), __shfl_xor(a.z, o, 64), __shfl_xor(a.w, o, 64)); }

// grid (ceil(C4 / 16), kParts, images), 256 threads = 16 channel lanes (cl, fastest) x 16 pixel lanes (pl): part[n][k][j][C], j < 7.  Every entry of its slice is
// written, zeros where a part holds no pixel or a channel lane lies past C.
__global__ void freeu_skip_partial_kernel(const float* __restrict__ src, long ld_src, int H, int W, int C4, int part_len, float* __restrict__ part,
                                          const float* __restrict__ s_dev)
{
    if (*s_dev == 1.f) return;
    __shared__ float2 tab[2 * kMaxSide];
    __shared__ float4 red[4][7][16];
    trig_table(tab, H, W);
    const int cl = (int)threadIdx.x & 15, pl = (int)threadIdx.x >> 4, wave = (int)threadIdx.x >> 6;
    const int c4 = (int)blockIdx.x * 16 + cl, k = (int)blockIdx.y, n = (int)blockIdx.z, HW = H * W;
    const float* __restrict__ img = src + (long)n * HW * ld_src;
    float4 a[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) a[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c4 < C4) {
        const int p_end = min(HW, (k + 1) * part_len);
        for (int p = k * part_len + pl; p < p_end; p += 16) {
            const float4 v = *reinterpret_cast<const float4*>(img + (long)p * ld_src + c4 * 4);
            const Trig t = trig_at(tab, p, H, W);
            a[0] = add4(a[0], v);
            FMA4(a[1], v, t.ca); FMA4(a[2], v, t.sa); FMA4(a[3], v, t.cb); FMA4(a[4], v, t.sb); FMA4(a[5], v, t.cab); FMA4(a[6], v, t.sab);
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {                       // pixel lanes pl ^ 1 and pl ^ 2 sit 16 and 32 lanes away
        a[j] = add4(a[j], shfl4(a[j], 16));
        a[j] = add4(a[j], shfl4(a[j], 32));
    }
    if (((int)threadIdx.x & 63) < 16) {
#pragma unroll
        for (int j = 0; j < 7; ++j) red[wave][j][cl] = a[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < 7 * 16) {
        const int j = (int)threadIdx.x >> 4, oc4 = (int)blockIdx.x * 16 + cl;      // (cl = threadIdx.x & 15)
        if (oc4 < C4) {
            const float4 s = add4(add4(red[0][j][cl], red[1][j][cl]), add4(red[2][j][cl], red[3][j][cl]));
            *reinterpret_cast<float4*>(part + (((long)n * kParts + k) * 7 + j) * (C4 * 4L) + oc4 * 4) = s;
        }
    }
}

// one thread per (image, sum j, channel vector): sums[n][j][C] = the 16 parts in a 4-level tree
__global__ void freeu_skip_combine_kernel(const float* __restrict__ part, float* __restrict__ sums, int n_img, int C4, const float* __restrict__ s_dev)
{
    if (*s_dev == 1.f) return;
    const long total = (long)n_img * 7 * C4, slice = 7L * C4 * 4;
    GRID_LOOP(i, total) {
        const long n = i / (7 * C4), jc = i - n * (7 * C4);
        const float* __restrict__ p0 = part + n * kParts * slice + jc * 4;
        float4 a[kParts];
#pragma unroll
        for (int k = 0; k < kParts; ++k) a[k] = *reinterpret_cast<const float4*>(p0 + k * slice);
#pragma unroll
        for (int s = 1; s < kParts; s *= 2)
#pragma unroll
            for (int k = 0; k < kParts; k += 2 * s) a[k] = add4(a[k], a[k + s]);
        *reinterpret_cast<float4*>(sums + n * slice + jc * 4) = a[0];
    }
}

// grid as the partial kernel's: the thread keeps the seven sums of its four channels and walks its pixels
__global__ void freeu_skip_apply_kernel(float* __restrict__ dst, long ld_dst, const float* __restrict__ src, long ld_src, int H, int W, int C4, int part_len,
                                        const float* __restrict__ sums, const float* __restrict__ s_dev)
{
    const float s = *s_dev;
    const int cl = (int)threadIdx.x & 15, pl = (int)threadIdx.x >> 4;
    const int c4 = (int)blockIdx.x * 16 + cl, k = (int)blockIdx.y, n = (int)blockIdx.z, HW = H * W;
    const int p_end = min(HW, (k + 1) * part_len);
    const float* __restrict__ in = src + (long)n * HW * ld_src;
    float* __restrict__ out = dst + (long)n * HW * ld_dst;
    if (s == 1.f) {                                     // (uniform over the grid)
        if (c4 < C4)
            for (int p = k * part_len + pl; p < p_end; p += 16)
                *reinterpret_cast<u32x4*>(out + (long)p * ld_dst + c4 * 4) = *reinterpret_cast<const u32x4*>(in + (long)p * ld_src + c4 * 4);      // bits, not values
        return;
    }
    __shared__ float2 tab[2 * kMaxSide];
    trig_table(tab, H, W);
    if (c4 >= C4) return;
    const float g = (s - 1.f) / (float)HW;
    float4 S[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) S[j] = *reinterpret_cast<const float4*>(sums + ((long)n * 7 + j) * (C4 * 4L) + c4 * 4);
    for (int p = k * part_len + pl; p < p_end; p += 16) {
        const float4 v = *reinterpret_cast<const float4*>(in + (long)p * ld_src + c4 * 4);
        const Trig t = trig_at(tab, p, H, W);
        float4 e = S[0];
        FMA4(e, S[1], t.ca); FMA4(e, S[2], t.sa); FMA4(e, S[3], t.cb); FMA4(e, S[4], t.sb); FMA4(e, S[5], t.cab); FMA4(e, S[6], t.sab);
        float4 o;
        o.x = __fmaf_rn(g, e.x, v.x); o.y = __fmaf_rn(g, e.y, v.y); o.z = __fmaf_rn(g, e.z, v.z); o.w = __fmaf_rn(g, e.w, v.w);
        *reinterpret_cast<float4*>(out + (long)p * ld_dst + c4 * 4) = o;
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) { return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; }

size_t backbone_ws_floats(long n_img, long rows) { return (size_t)(n_img * rows + n_img * kRowBlocks * 2); }
size_t skip_ws_floats(long n_img, long C) { return (size_t)(n_img * (kParts + 1) * 7 * C); }

// what both entry points check alike; rows = rows per image
int check_maps(const char* who, const float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int n_img, long rows, int C, const float* ws, size_t ws_floats,
               const float* f_dev)
{
    if (!dst || !src || !ws || !f_dev || n_img < 1 || rows < 1 || C < 8) return mlsd_set_error(-1, "%s: bad argument (%d images of %ld rows x %d)", who, n_img, rows, C);
    if ((C & 7) || ld_dst < C || ld_src < C || (ld_dst & 3) || (ld_src & 3))
        return mlsd_set_error(-1, "%s: C %d must be a multiple of 8, the row strides %lld %lld multiples of 4 and >= C", who, C, (long long)ld_dst, (long long)ld_src);
    if (((uintptr_t)dst | (uintptr_t)src | (uintptr_t)ws) & 15) return mlsd_set_error(-1, "%s: pointers must be 16-byte aligned", who);
    if ((uintptr_t)f_dev & 3) return mlsd_set_error(-1, "%s: misaligned factor", who);
    if ((long)n_img * rows >= (1L << 31) / 4 || (long)n_img * rows * (ld_dst > ld_src ? ld_dst : ld_src) >= (1L << 40)) return mlsd_set_error(-1, "%s: map too large", who);
    const size_t nd = (size_t)n_img * rows * ld_dst * 4, ns = (size_t)n_img * rows * ld_src * 4, nw = ws_floats * 4;
    if (overlap(dst, nd, src, ns) || overlap(dst, nd, ws, nw) || overlap(src, ns, ws, nw) || overlap(f_dev, 4, dst, nd) || overlap(f_dev, 4, ws, nw))
        return mlsd_set_error(-1, "%s: dst, src, the workspace and the factor must not overlap", who);
    return 0;
}

}  // namespace

extern "C" MLSD_API int mlsd_freeu_depth(int n_terms) { return n_terms < 1 ? 0 : (n_terms + 255) / 256 - 1 + 8; }

extern "C" MLSD_API size_t mlsd_freeu_ws_bytes(int n_img, int H, int W, int C)
{
    if (n_img < 1 || H < 1 || W < 1 || C < 1) return 0;
    const size_t a = backbone_ws_floats(n_img, (long)H * W), b = skip_ws_floats(n_img, C);
    return (((a > b ? a : b) * 4) + 255) & ~(size_t)255;
}

extern "C" MLSD_API int mlsd_freeu_backbone(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int n_img, int rows_per_img, int C, float* ws,
                                            const float* b_dev, void* stream)
{
    if (n_img > 65535) return mlsd_set_error(-1, "mlsd_freeu_backbone: %d images (at most 65535)", n_img);
    const int r = check_maps("mlsd_freeu_backbone", dst, ld_dst, src, ld_src, n_img, rows_per_img, C, ws, backbone_ws_floats(n_img > 0 ? n_img : 1, rows_per_img > 0 ? rows_per_img : 1), b_dev);
    if (r) return r;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("freeu_backbone");      // the dry runtime's buffers are host memory: refuse before the launch
    const int rows = rows_per_img, C4 = C / 4;
    const int n_mm = (rows + 3) / 4 < kRowBlocks ? (rows + 3) / 4 : kRowBlocks;
    float *mean = ws, *mm = ws + (size_t)n_img * rows;
    hipLaunchKernelGGL(freeu_mean_kernel, dim3((unsigned)n_mm, (unsigned)n_img), dim3(256), 0, (hipStream_t)stream, src, (long)ld_src, rows, C4, mean, mm, b_dev);
    long nb = ((long)rows * C4 + 255) / 256;
    const long cap = (4096 + n_img - 1) / n_img;        // about 4096 blocks in all, as nblk
    if (nb > cap) nb = cap;
    hipLaunchKernelGGL(freeu_backbone_apply_kernel, dim3((unsigned)nb, (unsigned)n_img), dim3(256), 0, (hipStream_t)stream, dst, (long)ld_dst, src, (long)ld_src, rows, C4,
                       mean, mm, n_mm, b_dev);
    return mlsd_check_launch("freeu_backbone");
}

extern "C" MLSD_API int mlsd_freeu_skip(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int n_img, int H, int W, int C, float* ws, const float* s_dev,
                                        void* stream)
{
    if (H < 2 || W < 2 || H > kMaxSide || W > kMaxSide)
        return mlsd_set_error(-1, "mlsd_freeu_skip: a %d x %d plane (the closed form of the filter holds for 2 .. %d per side)", H, W, kMaxSide);
    if (n_img > 65535) return mlsd_set_error(-1, "mlsd_freeu_skip: %d images (at most 65535)", n_img);
    const int r = check_maps("mlsd_freeu_skip", dst, ld_dst, src, ld_src, n_img, (long)H * W, C, ws, skip_ws_floats(n_img > 0 ? n_img : 1, C > 0 ? C : 1), s_dev);
    if (r) return r;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("freeu_skip");
    const int C4 = C / 4, HW = H * W, part_len = 16 * ((HW + 255) / 256);
    float *part = ws, *sums = ws + (size_t)n_img * kParts * 7 * C;
    const dim3 grid((unsigned)((C4 + 15) / 16), kParts, (unsigned)n_img);
    hipLaunchKernelGGL(freeu_skip_partial_kernel, grid, dim3(256), 0, (hipStream_t)stream, src, (long)ld_src, H, W, C4, part_len, part, s_dev);
    hipLaunchKernelGGL(freeu_skip_combine_kernel, dim3(nblk((long)n_img * 7 * C4)), dim3(256), 0, (hipStream_t)stream, part, sums, n_img, C4, s_dev);
    hipLaunchKernelGGL(freeu_skip_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, dst, (long)ld_dst, src, (long)ld_src, H, W, C4, part_len, sums, s_dev);
    return mlsd_check_launch("freeu_skip");
}
