// 3x3 convolution (stride 1, zero padding 1) of the Real-ESRGAN COMPACT nets (SRVGGNetCompact; host/upscaler.c is the network, include/mlsd_kernels.h states it): 16 to 32
// identical 64 -> 64 layers with a PReLU each, a 3 -> 64 head and a 64 -> 3 s^2 tail that ends in a pixel shuffle.  Every layer runs at the INPUT resolution.
//
// Why not mlsd_conv3x3_dense (upscale.hip): it restages its weights per 32-channel chunk for every pixel tile, which suits a dense block whose Cin grows; it has no PReLU,
// no pixel-shuffle ending and no 64 -> 3 s^2 shape.  Here the layer's WHOLE weight tensor, [64][3][3][64] halfs = 73 728 bytes, fits in a CU's LDS and stays there:
//
//   * workgroups of 4 waves are PERSISTENT: grid = min(tiles, CUs) (mlsd_cconv_args.grid overrides it).  Each stages the complete weight tensor, the bias and the slopes into
//     LDS once, then walks the tiles b, b + grid, b + 2 grid, ... of the launch: a fixed assignment, no atomics, no block waits on another.
//   * a tile is 12 rows x 16 columns of output pixels of one image and ALL output channels; wave w owns rows 3w .. 3w + 2 = three groups of 16 pixels.  Its 14 x 18 halo
//     patch (128 bytes per pixel at Cin = 64) is staged in LDS; there are TWO patch buffers: the next tile's patch is loaded from memory into registers before the current
//     tile's MFMAs, and written to the other buffer after them, one barrier per tile.  Padding and the ragged image edges stage zeros.
//     LDS: 73 728 (weights) + 2 x 32 768 (patches) + 512 (bias, slopes) = 139 776 bytes, within the 140 800 that attention_wide.hip uses: one workgroup per CU.
//   * LDS images are PLANE-major as in upscale.hip: the 16-byte k-pieces (8 channels) of a pixel or of a weight row live in Cin / 8 planes whose size is a multiple of 256
//     bytes, a row's piece at 16 * row inside its plane; fragment reads (lane = k-piece x 16 consecutive rows) and staging writes use the same lane pattern.
//   * v_mfma_f32_16x16x32_f16, the WEIGHTS as the A operand (16 output channels), 16 pixels as the B operand.  Per (k-step, kw) a wave reads the 5 patch-row fragments
//     its three rows share between the three kh, and per kh the 4 weight fragments: 17 LDS reads for 36 MFMAs.
//   * D[cout][pixel] leaves a lane with 4 consecutive MFMA rows of one pixel.  The weight rows are staged PERMUTED, MFMA row j of channel group n = channel
//     32 (n >> 1) + 8 (j >> 2) + 4 (n & 1) + (j & 3), so that the two groups of a pair give a lane 8 consecutive channels: one 16-byte fp16 store.
//   * the tail form (64 -> 3 s^2, the channels padded to a multiple of 16 whose products are dropped) ends in the pixel shuffle: channel c s^2 + dy s + dx of pixel (y, x) plus
//     the fp32 input pixel x[c][y][x] (= its nearest upsample at that place) goes to channel c of pixel (s y + dy, s x + dx) of the planar fp32 result.  No 64 -> 3 s^2
//     tensor reaches memory.  The head form (3 -> 64) is the body kernel on the input packed to 32 channels.
//
// Arithmetic: fp16 operands, fp32 accumulation on MFMA over (k-step of 32 channels, kw, kh) in that order, nothing else rounded; the ending in fp32, each operation rounded
// once (the build has no contraction):  z = acc + bias[n];  body / head: y = z >= 0 ? z : slope[n] z, fp16(y) to nearest even;  tail: y = z + x, fp32.
// The same input gives the same bits, whatever the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

struct CCP {
    const _Float16* A; long lda;
    const _Float16* Wt;                 // [16 NG][3][3][CIN]
    const float* bias;                  // [cout]
    const float* slope;                 // [cout] or NULL
    _Float16* C16; long ldc16;          // body / head
    const float* X32; float* Y32;       // tail
    int H, W, tiles_x, tiles_y, n_tiles, cout;
};

constexpr int TH = 12, TW = 16;                      // output tile
constexpr int PH = TH + 2, PW = TW + 2;              // its halo patch: 14 x 18 pixels
constexpr int NPX = PH * PW;                         // 252
constexpr int PXPL = 256 * 16;                       // bytes of a k-piece plane of the patch: 256 pixel slots (the last four hold zeros)
constexpr int LDS_BUDGET = 140800;                   // what attention_wide.hip occupies as built

// S = 0: head (CIN 32) and body (CIN 64), NG = 4;  S = 1 .. 4: the tail of scale S, NG = ceil(3 S S / 16)
template <int CIN, int NG, int S>
__global__ __launch_bounds__(256) void cconv3x3_kernel(const CCP p)
{
    constexpr int N = NG * 16;                       // MFMA rows of output channels
    constexpr int KS = CIN / 32;                     // k-steps of one MFMA
    constexpr int KQ = CIN / 8;                      // k-piece planes
    constexpr int WROWS = 9 * N;                     // weight rows (tap, n)
    constexpr int WPL = WROWS * 16;                  // bytes of a plane of the weights
    constexpr int WPIECES = WROWS * KQ;
    static_assert(CIN == 32 || CIN == 64, "input channels");
    static_assert(S == 0 ? NG == 4 : NG == (3 * S * S + 15) / 16, "output channel groups");
    static_assert(WPL % 256 == 0 && PXPL % 256 == 0, "plane sizes keep the bank pattern");
    static_assert(KQ * WPL + 2 * KQ * PXPL + 512 <= LDS_BUDGET, "LDS budget");
    __shared__ __attribute__((aligned(256))) unsigned char s_wt[KQ * WPL];
    __shared__ __attribute__((aligned(256))) unsigned char s_px[2][KQ * PXPL];
    __shared__ float s_bias[64], s_slope[64];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 15, kq = lane >> 4;
    const int tiles_img = p.tiles_x * p.tiles_y;

    // ---- the patch of tile t -> registers: piece i of this thread = unit u = wave + 4 i of (16 pixels x 4 k-pieces), pixel group u / KS, k-step u % KS
    f16x8 px_reg[KQ];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int t) {
        const int img = t / tiles_img, r = t - img * tiles_img;
        const int y0 = (r / p.tiles_x) * TH, x0 = (r % p.tiles_x) * TW;
        const _Float16* Aimg = p.A + (long)img * p.H * p.W * p.lda;
#pragma unroll
        for (int i = 0; i < KQ; ++i) {
            const int u = wave + 4 * i, pix = (u / KS) * 16 + j, plane = (u % KS) * 4 + kq;
            const int gy = y0 - 1 + pix / PW, gx = x0 - 1 + pix % PW;
            const bool ok = pix < NPX && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            px_reg[i] = ok ? *reinterpret_cast<const f16x8*>(Aimg + ((long)gy * p.W + gx) * p.lda + plane * 8) : zero8;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < KQ; ++i) {
            const int u = wave + 4 * i, pix = (u / KS) * 16 + j, plane = (u % KS) * 4 + kq;
            *reinterpret_cast<f16x8*>(s_px[buf] + plane * PXPL + pix * 16) = px_reg[i];
        }
    };

    int t = blockIdx.x;                              // grid <= n_tiles: every workgroup has a first tile
    fetch(t);
    // ---- once per launch: the whole weight tensor, the bias and the slopes
    for (int idx = tid; idx < WPIECES; idx += 256) {
        const int u = idx >> 6, r = (u / KS) * 16 + j, plane = (u % KS) * 4 + kq;
        const int tap = r / N, nn = r % N;
        const int ch = S ? nn : 32 * (nn >> 5) + 8 * ((nn & 15) >> 2) + 4 * ((nn >> 4) & 1) + (nn & 3);
        *reinterpret_cast<f16x8*>(s_wt + plane * WPL + r * 16) = *reinterpret_cast<const f16x8*>(p.Wt + ((long)ch * 9 + tap) * CIN + plane * 8);
    }
    if (tid < 64) {
        s_bias[tid] = tid < p.cout ? p.bias[tid] : 0.f;
        s_slope[tid] = (p.slope && tid < p.cout) ? p.slope[tid] : 1.f;
    }
    stage(0);
    __syncthreads();

    const int wfo = kq * WPL + j * 16;
    const int pfo = kq * PXPL + (3 * wave * PW + j) * 16;
    int cur = 0;
    for (; t < p.n_tiles; t += gridDim.x) {
        const int tn = t + (int)gridDim.x;
        const bool more = tn < p.n_tiles;            // the same for the whole workgroup
        if (more) fetch(tn);                         // in flight during this tile's MFMAs

        f32x4 acc[3][NG];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int n = 0; n < NG; ++n) acc[r][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char* px = s_px[cur];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                f16x8 pf[5];                         // patch rows 3 wave .. 3 wave + 4, shifted by kw
#pragma unroll
                for (int rr = 0; rr < 5; ++rr) pf[rr] = *reinterpret_cast<const f16x8*>(px + pfo + ks * 4 * PXPL + (rr * PW + kw) * 16);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    f16x8 wf[NG];
#pragma unroll
                    for (int n = 0; n < NG; ++n) wf[n] = *reinterpret_cast<const f16x8*>(s_wt + wfo + ks * 4 * WPL + ((kh * 3 + kw) * N + 16 * n) * 16);
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int n = 0; n < NG; ++n) acc[r][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[n], pf[r + kh], acc[r][n], 0, 0, 0);
                }
            }
        }

        // ---- the ending, straight from the accumulators
        const int img = t / tiles_img, rt = t - img * tiles_img;
        const int y0 = (rt / p.tiles_x) * TH, x0 = (rt % p.tiles_x) * TW;
        const int ox = x0 + j;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int oy = y0 + 3 * wave + r;
            if (oy >= p.H || ox >= p.W) continue;
            if constexpr (S == 0) {                  // this lane: channels 32 q + 8 kq .. + 7 of pixel j
                const long m = ((long)img * p.H + oy) * p.W + ox;
#pragma unroll
                for (int q = 0; q < NG / 2; ++q) {
                    const int c0 = 32 * q + 8 * kq;
                    f16x8 y;
#pragma unroll
                    for (int v = 0; v < 8; ++v) {
                        float z = acc[r][2 * q + (v >> 2)][v & 3];
                        z = z + s_bias[c0 + v];
                        z = z >= 0.f ? z : s_slope[c0 + v] * z;
                        y[v] = (_Float16)z;
                    }
                    *reinterpret_cast<f16x8*>(p.C16 + m * p.ldc16 + c0) = y;
                }
            } else {                                 // this lane: channels 16 n + 4 kq .. + 3 of pixel j; pixel shuffle + the input pixel
                const long SH = (long)S * p.H, SW = (long)S * p.W;
#pragma unroll
                for (int n = 0; n < NG; ++n)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int ch = 16 * n + 4 * kq + v;
                        if (ch >= 3 * S * S) continue;
                        const int c = ch / (S * S), dy = (ch % (S * S)) / S, dx = ch % S;
                        const float z = acc[r][n][v] + s_bias[ch];
                        const float x = p.X32[(((long)img * 3 + c) * p.H + oy) * p.W + ox];
                        p.Y32[(((long)img * 3 + c) * SH + (long)S * oy + dy) * SW + (long)S * ox + dx] = z + x;
                    }
            }
        }

        if (more) stage(cur ^ 1);
        __syncthreads();                             // the next patch is whole, and every wave has read this one
        cur ^= 1;
    }
}

// byte ranges [a, a + na) and [b, b + nb)
bool cc_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// the form of a launch: 0 head, 1 body, 2 tail; < 0 and the error text in *why when the kernel does not take it
int cc_check(const mlsd_cconv_args* a, const char** why)
{
#define CC_FAIL(text) do { *why = text; return -1; } while (0)
    if (!a) CC_FAIL("NULL arguments");
    const int tail = a->scale != 0;
    if (a->scale < 0 || a->scale > 4) CC_FAIL("scale must be 0 (head, body) or 1 .. 4 (tail)");
    if (tail ? (a->Cin != 64 || a->Cout != 3 * a->scale * a->scale) : ((a->Cin != 32 && a->Cin != 64) || a->Cout != 64))
        CC_FAIL("Cin -> Cout must be 32 -> 64 (head), 64 -> 64 (body) or, with scale s, 64 -> 3 s s (tail)");
    if (a->n_img < 1 || a->H < 1 || a->W < 1) CC_FAIL("n_img, H and W must be positive");
    if (a->grid < 0) CC_FAIL("grid must not be negative");
    if (!a->A || !a->W_ || !a->bias) CC_FAIL("A, W and bias must be set");
    if (((uintptr_t)a->A & 15) || (a->lda & 7) || a->lda < a->Cin) CC_FAIL("A must be 16-byte aligned with lda a multiple of 8 and >= Cin");
    if ((uintptr_t)a->W_ & 15) CC_FAIL("W must be 16-byte aligned");
    if (((uintptr_t)a->bias & 3) || ((uintptr_t)a->slope & 3)) CC_FAIL("bias and slope must be 4-byte aligned");
    const long M = (long)a->n_img * a->H * a->W;
    if (M > (1L << 36)) CC_FAIL("image too large");
    const size_t a_bytes = ((size_t)(M - 1) * a->lda + a->Cin) * 2;
    if (!tail) {
        if (a->X32 || a->Y32) CC_FAIL("X32 and Y32 belong to the tail form");
        if (!a->C16) CC_FAIL("no output");
        if (((uintptr_t)a->C16 & 15) || (a->ldc16 & 7) || a->ldc16 < a->Cout) CC_FAIL("C16 must be 16-byte aligned with ldc16 a multiple of 8 and >= Cout");
        // an output that aliases A: a tap reads neighbours that another wave may already have overwritten
        if (cc_overlap(a->C16, ((size_t)(M - 1) * a->ldc16 + a->Cout) * 2, a->A, a_bytes)) CC_FAIL("C16 aliases A");
    } else {
        if (a->C16 || a->slope) CC_FAIL("C16 and slope belong to the head and body forms");
        if (!a->X32 || !a->Y32) CC_FAIL("the tail form needs X32 and Y32");
        if (((uintptr_t)a->X32 & 3) || ((uintptr_t)a->Y32 & 3)) CC_FAIL("X32 and Y32 must be 4-byte aligned");
        const size_t x_bytes = (size_t)M * 3 * 4, y_bytes = x_bytes * a->scale * a->scale;
        if (cc_overlap(a->Y32, y_bytes, a->A, a_bytes)) CC_FAIL("Y32 aliases A");
        if (cc_overlap(a->Y32, y_bytes, a->X32, x_bytes)) CC_FAIL("Y32 aliases X32");
    }
#undef CC_FAIL
    return tail ? 2 : (a->Cin == 64 ? 1 : 0);
}

int cc_device_cus()
{
    static thread_local int cached_dev = -1, cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (dev != cached_dev) {
        int n = 0;
        cached = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess ? n : 0;
        (void)hipGetLastError();
        cached_dev = dev;
    }
    return cached;
}

}  // namespace

extern "C" MLSD_API const char* mlsd_cconv_variant(const mlsd_cconv_args* a)
{
    static thread_local char buf[64];
    const char* why;
    const int form = cc_check(a, &why);
    if (form < 0) return "cconv3x3<refused>";
    if (form == 2) snprintf(buf, sizeof buf, "cconv3x3<tail,s%d>", a->scale);
    else snprintf(buf, sizeof buf, "cconv3x3<%s>", form ? "body" : "head");
    return buf;
}

extern "C" MLSD_API int mlsd_conv3x3_compact(const mlsd_cconv_args* a, void* stream)
{
    const char* why = 0;
    const int form = cc_check(a, &why);
    if (form < 0) return mlsd_set_error(-1, "mlsd_conv3x3_compact: %s", why);
    CCP p;
    p.A = (const _Float16*)a->A; p.lda = a->lda; p.Wt = (const _Float16*)a->W_; p.bias = a->bias; p.slope = a->slope;
    p.C16 = (_Float16*)a->C16; p.ldc16 = a->ldc16; p.X32 = a->X32; p.Y32 = a->Y32;
    p.H = a->H; p.W = a->W; p.cout = a->Cout;
    p.tiles_x = (a->W + TW - 1) / TW; p.tiles_y = (a->H + TH - 1) / TH;
    const long tiles = (long)p.tiles_x * p.tiles_y * a->n_img;
    if (tiles > 0x7fffffffL / 2) return mlsd_set_error(-1, "mlsd_conv3x3_compact: too many tiles");
    p.n_tiles = (int)tiles;
    long grid = a->grid > 0 ? a->grid : cc_device_cus();
    if (grid < 1) grid = 1;
    if (grid > tiles) grid = tiles;
    const dim3 g((unsigned)grid), b(256);
    hipStream_t s = (hipStream_t)stream;
    if (form == 0) hipLaunchKernelGGL((cconv3x3_kernel<32, 4, 0>), g, b, 0, s, p);
    else if (form == 1) hipLaunchKernelGGL((cconv3x3_kernel<64, 4, 0>), g, b, 0, s, p);
    else if (a->scale == 1) hipLaunchKernelGGL((cconv3x3_kernel<64, 1, 1>), g, b, 0, s, p);
    else if (a->scale == 2) hipLaunchKernelGGL((cconv3x3_kernel<64, 1, 2>), g, b, 0, s, p);
    else if (a->scale == 3) hipLaunchKernelGGL((cconv3x3_kernel<64, 2, 3>), g, b, 0, s, p);
    else hipLaunchKernelGGL((cconv3x3_kernel<64, 3, 4>), g, b, 0, s, p);
    return mlsd_check_launch("cconv3x3_kernel");
}
