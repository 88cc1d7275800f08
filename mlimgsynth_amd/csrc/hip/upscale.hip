// 3x3 convolution (stride 1, zero padding 1) with a NARROW output, N = 32 or 64 channels, over a full-resolution channels-last fp16 image: the dense-block convolutions of
// RRDBNet (ESRGAN / Real-ESRGAN; not in the reference, host/upscaler.c is the network).  23 blocks x 15 of these are the whole cost of an upscale, ~33 MFLOP per input pixel.
//
// Why not mlsd_gemm: its narrowest tile is 128 columns wide (three quarters of the MFMAs would multiply padding at N = 32), and its epilogue has neither LeakyReLU nor the
// scaled residuals of the dense blocks; conv_smalln.hip keeps ALL weights in registers, which stops at Cout <= 16 (9 x 192 x 32 halfs are 108 KiB).  So:
//
//   * a workgroup of 4 waves owns an 8-row x 32-column tile of output pixels of one image and ALL N output channels; wave w owns rows 2w, 2w + 1 = four groups of 16 pixels.
//     Nothing is shared between workgroups and nothing is handed over inside the launch.
//   * K = 9 Cin is walked in chunks of 32 input channels.  Per chunk the tile's 10 x 34 halo patch (64 bytes per pixel) and the chunk's weights (9 x N x 64 bytes) are staged
//     in LDS -- 22 + 18 KiB at N = 32, 22 + 36 KiB at N = 64: two to three workgroups per CU cover each other's staging -- and the NEXT chunk's global loads are issued into
//     registers before the current chunk's MFMAs, so their latency hides behind 72 (N = 32) or 144 (N = 64) MFMAs per wave.  The nearest-2x upsample is folded into the
//     patch gather (source pixel = output coordinate >> 1), as mlsd_gemm_args.upsample does; padding and the ragged tile edges stage zeros.
//   * LDS images are PLANE-major: the four 16-byte k-quarters of a pixel (of a weight row) live in four planes whose size is a multiple of 256 bytes, a pixel's piece at
//     16 * pixel inside its plane.  A fragment read (lane = k-quarter x 16 consecutive pixels) then touches, in each 16-lane service group of ds_read_b128 -- two k-quarters,
//     eight pixels each, complementary modulo 16 (MI355X_MICROARCH.md, LDS) -- sixteen different bank quads whatever pixel the group starts at; the staging writes use the
//     same lane pattern.
//   * v_mfma_f32_16x16x32_f16 with the WEIGHTS as the A operand (16 output channels) and 16 pixels as the B operand, as conv_smalln.hip: D[cout][pixel] leaves a lane with 4
//     consecutive output channels of one pixel = one 16-byte fp32 / 8-byte fp16 store into a channel slice of a wider buffer.
//
// Arithmetic: fp16 operands, fp32 accumulation on MFMA over (cin chunk, kh, kw, cin in chunk) in that order, NOTHING else rounded; the epilogue is fp32, every multiply and add
// rounded separately (the build has no contraction):  z = acc + bias;  a = lrelu ? (z >= 0 ? z : 0.2f z) : z;  y = a scale + resid;  [y = y scale2 + resid2;]  C32 = y,
// C16 = fp16(y) to nearest even.  The same input gives the same bits: no atomics, a fixed summation order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

struct DCP {
    const _Float16* A; long lda;
    const _Float16* Wt;                 // [N][3][3][Cin]
    const float* bias;
    const float* resid; long ldr;
    const float* resid2; long ldr2;
    float scale, scale2;
    int lrelu;
    float* C32; long ldc32;
    _Float16* C16; long ldc16;
    int H, W, OH, OW, Cin, up, tiles_x, tiles_y;
};

constexpr int TH = 8, TW = 32;                       // output tile
constexpr int PH = TH + 2, PW = TW + 2;              // its halo patch: 10 x 34 pixels
constexpr int NPX = PH * PW;                         // 340
constexpr int PXU = (NPX + 15) / 16;                 // staging units of 16 pixels: 22
constexpr int PXPL = PXU * 16 * 16;                  // bytes of a k-quarter plane of the patch: 5632 = 22 x 256
constexpr int PXI = (PXU * 64 + 255) / 256;          // staging pieces per thread: 6

template <int N>
__global__ __launch_bounds__(256) void dconv3x3_kernel(const DCP p)
{
    constexpr int NG = N / 16;                       // groups of 16 output channels
    constexpr int WROWS = 9 * N;                     // weight rows (tap, n) of a chunk
    constexpr int WPL = WROWS * 16;                  // bytes of a k-quarter plane of the weights: 4608 | 9216 (multiples of 256)
    constexpr int WI = (WROWS * 4 + 255) / 256;      // staging pieces per thread: 5 | 9
    static_assert(N == 32 || N == 64, "output channels");
    static_assert(PXPL % 256 == 0 && WPL % 256 == 0, "plane sizes keep the bank pattern");
    __shared__ __attribute__((aligned(256))) unsigned char s_px[4 * PXPL];
    __shared__ __attribute__((aligned(256))) unsigned char s_wt[4 * WPL];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int j = lane & 15, kq = lane >> 4;
    int b = blockIdx.x;
    const int tx = b % p.tiles_x; b /= p.tiles_x;
    const int ty = b % p.tiles_y;
    const int img = b / p.tiles_y;
    const int x0 = tx * TW, y0 = ty * TH;
    const _Float16* Aimg = p.A + (long)img * p.H * p.W * p.lda;

    // ---- staging: piece i of this thread = unit (tid + 256 i) >> 6 of 16 rows, row (lane & 15) of it, k-quarter lane >> 4
    long px_src[PXI];                                // source offset in halfs of the piece's pixel (k-quarter included), -1: zeros
    int px_dst[PXI];                                 // LDS byte offset, -1: no such piece
#pragma unroll
    for (int i = 0; i < PXI; ++i) {
        const int u = (tid + 256 * i) >> 6, pix = u * 16 + j;
        px_dst[i] = pix < NPX ? kq * PXPL + pix * 16 : -1;
        const int gy = y0 - 1 + pix / PW, gx = x0 - 1 + pix % PW;
        const bool ok = pix < NPX && (unsigned)gy < (unsigned)p.OH && (unsigned)gx < (unsigned)p.OW;
        const int sy = p.up ? gy >> 1 : gy, sx = p.up ? gx >> 1 : gx;
        px_src[i] = ok ? ((long)sy * p.W + sx) * p.lda + kq * 8 : -1;
    }
    int wt_src[WI], wt_dst[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int u = (tid + 256 * i) >> 6, r = u * 16 + j;
        const int tap = r / N, n = r % N;
        wt_dst[i] = r < WROWS ? kq * WPL + r * 16 : -1;
        wt_src[i] = (n * 9 + tap) * p.Cin + kq * 8;
    }
    f16x8 px_reg[PXI], wt_reg[WI];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < PXI; ++i) px_reg[i] = px_src[i] >= 0 ? *reinterpret_cast<const f16x8*>(Aimg + px_src[i] + kc * 32) : zero8;
#pragma unroll
        for (int i = 0; i < WI; ++i) wt_reg[i] = wt_dst[i] >= 0 ? *reinterpret_cast<const f16x8*>(p.Wt + wt_src[i] + kc * 32) : zero8;
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < PXI; ++i) if (px_dst[i] >= 0) *reinterpret_cast<f16x8*>(s_px + px_dst[i]) = px_reg[i];
#pragma unroll
        for (int i = 0; i < WI; ++i) if (wt_dst[i] >= 0) *reinterpret_cast<f16x8*>(s_wt + wt_dst[i]) = wt_reg[i];
    };

    // ---- fragment offsets: pixel group g = (row 2 wave + (g >> 1), columns 16 (g & 1) ..), tap (kh, kw) adds (kh PW + kw) pixels
    int pfo[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) pfo[g] = kq * PXPL + ((2 * wave + (g >> 1)) * PW + 16 * (g & 1) + j) * 16;
    const int wfo = kq * WPL + j * 16;

    f32x4 acc[4][NG];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int n = 0; n < NG; ++n) acc[g][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int KC = p.Cin / 32;
    fetch(0);
    for (int kc = 0; kc < KC; ++kc) {
        __syncthreads();                             // every wave has read the previous chunk's fragments
        stage();
        __syncthreads();
        if (kc + 1 < KC) fetch(kc + 1);              // in flight during this chunk's MFMAs
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int poff = ((tap / 3) * PW + tap % 3) * 16;
            f16x8 wf[NG], pf[4];
#pragma unroll
            for (int n = 0; n < NG; ++n) wf[n] = *reinterpret_cast<const f16x8*>(s_wt + wfo + (tap * N + 16 * n) * 16);
#pragma unroll
            for (int g = 0; g < 4; ++g) pf[g] = *reinterpret_cast<const f16x8*>(s_px + pfo[g] + poff);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int n = 0; n < NG; ++n) acc[g][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[n], pf[g], acc[g][n], 0, 0, 0);
        }
    }

    // ---- epilogue: this lane holds output channels 16 n + 4 kq .. + 3 of pixel j of each group
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int oy = y0 + 2 * wave + (g >> 1), ox = x0 + 16 * (g & 1) + j;
        if (oy >= p.OH || ox >= p.OW) continue;
        const long m = ((long)img * p.OH + oy) * p.OW + ox;
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            const int c0 = 16 * n + 4 * kq;
            float y[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float z = acc[g][n][v];
                if (p.bias) z = z + p.bias[c0 + v];
                if (p.lrelu) z = z >= 0.f ? z : 0.2f * z;
                y[v] = z * p.scale;
            }
            if (p.resid) {
                const float4 r = *reinterpret_cast<const float4*>(p.resid + m * p.ldr + c0);
                y[0] = y[0] + r.x; y[1] = y[1] + r.y; y[2] = y[2] + r.z; y[3] = y[3] + r.w;
            }
            if (p.resid2) {
                const float4 r = *reinterpret_cast<const float4*>(p.resid2 + m * p.ldr2 + c0);
                y[0] = y[0] * p.scale2 + r.x; y[1] = y[1] * p.scale2 + r.y; y[2] = y[2] * p.scale2 + r.z; y[3] = y[3] * p.scale2 + r.w;
            }
            if (p.C32) *reinterpret_cast<float4*>(p.C32 + m * p.ldc32 + c0) = make_float4(y[0], y[1], y[2], y[3]);
            if (p.C16) *reinterpret_cast<f16x4*>(p.C16 + m * p.ldc16 + c0) = f16x4{(_Float16)y[0], (_Float16)y[1], (_Float16)y[2], (_Float16)y[3]};
        }
    }
}

// byte ranges [a, a + na) and [b, b + nb)
bool dc_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// 0 if the launch is one the kernel takes, else the error text in `why`
const char* dc_check(const mlsd_dconv_args* a)
{
    if (!a) return "NULL arguments";
    if (a->Cin != 32 && a->Cin != 64 && a->Cin != 96 && a->Cin != 128 && a->Cin != 160 && a->Cin != 192) return "Cin must be one of 32, 64, 96, 128, 160, 192";
    if (a->N != 32 && a->N != 64) return "N must be 32 or 64";
    if (a->n_img < 1 || a->H < 1 || a->W < 1) return "n_img, H and W must be positive";
    if (a->upsample != 0 && a->upsample != 1) return "upsample must be 0 or 1";
    if (!a->A || !a->W_) return "A and W must be set";
    if (!a->C32 && !a->C16) return "no output";
    if (((uintptr_t)a->A & 15) || (a->lda & 7) || a->lda < a->Cin) return "A must be 16-byte aligned with lda a multiple of 8 and >= Cin";
    if ((uintptr_t)a->W_ & 15) return "W must be 16-byte aligned";
    if (a->bias && ((uintptr_t)a->bias & 3)) return "bias must be 4-byte aligned";
    if (a->resid && (((uintptr_t)a->resid & 15) || (a->ldr & 3) || a->ldr < a->N)) return "resid must be 16-byte aligned with ldr a multiple of 4 and >= N";
    if (a->resid2 && (((uintptr_t)a->resid2 & 15) || (a->ldr2 & 3) || a->ldr2 < a->N)) return "resid2 must be 16-byte aligned with ldr2 a multiple of 4 and >= N";
    if (a->C32 && (((uintptr_t)a->C32 & 15) || (a->ldc32 & 3) || a->ldc32 < a->N)) return "C32 must be 16-byte aligned with ldc32 a multiple of 4 and >= N";
    if (a->C16 && (((uintptr_t)a->C16 & 7) || (a->ldc16 & 3) || a->ldc16 < a->N)) return "C16 must be 8-byte aligned with ldc16 a multiple of 4 and >= N";
    const int f = a->upsample ? 2 : 1;
    const long OH = (long)a->H * f, OW = (long)a->W * f;
    const long Min = (long)a->n_img * a->H * a->W, M = (long)a->n_img * OH * OW;
    if (OH > 0x7fffffffL || OW > 0x7fffffffL || M > (1L << 40)) return "image too large";
    const size_t a_bytes = ((size_t)(Min - 1) * a->lda + a->Cin) * 2;
    // an output that aliases A: a tap reads neighbours that another wave may already have overwritten.  The one overlap that is no alias: an fp16 slice of A's own rows
    // (same pixel stride, same pixels) whose columns lie beyond the Cin columns read.
    if (a->C32 && dc_overlap(a->C32, ((size_t)(M - 1) * a->ldc32 + a->N) * 4, a->A, a_bytes)) return "C32 aliases A";
    if (a->C16 && dc_overlap(a->C16, ((size_t)(M - 1) * a->ldc16 + a->N) * 2, a->A, a_bytes)) {
        const intptr_t d = ((intptr_t)a->C16 - (intptr_t)a->A) / 2;
        if (!(a->ldc16 == a->lda && !a->upsample && d >= a->Cin && d + a->N <= a->lda)) return "C16 aliases A";
    }
    // a residual may be the fp32 output itself (in place: a lane reads its four values before it writes them), nothing in between
    if (a->C32 && a->resid && dc_overlap(a->C32, ((size_t)(M - 1) * a->ldc32 + a->N) * 4, a->resid, ((size_t)(M - 1) * a->ldr + a->N) * 4) &&
        !(a->resid == a->C32 && a->ldr == a->ldc32)) return "C32 overlaps resid";
    if (a->C32 && a->resid2 && dc_overlap(a->C32, ((size_t)(M - 1) * a->ldc32 + a->N) * 4, a->resid2, ((size_t)(M - 1) * a->ldr2 + a->N) * 4) &&
        !(a->resid2 == a->C32 && a->ldr2 == a->ldc32)) return "C32 overlaps resid2";
    return 0;
}

}  // namespace

extern "C" MLSD_API const char* mlsd_dconv_variant(const mlsd_dconv_args* a)
{
    static thread_local char buf[64];
    if (dc_check(a)) return "dconv3x3<refused>";
    snprintf(buf, sizeof buf, "dconv3x3<n%d,c%d%s>", a->N, a->Cin, a->upsample ? ",up" : "");
    return buf;
}

extern "C" MLSD_API int mlsd_conv3x3_dense(const mlsd_dconv_args* a, void* stream)
{
    const char* why = dc_check(a);
    if (why) return mlsd_set_error(-1, "mlsd_conv3x3_dense: %s", why);
    DCP p;
    p.A = (const _Float16*)a->A; p.lda = a->lda; p.Wt = (const _Float16*)a->W_; p.bias = a->bias;
    p.resid = a->resid; p.ldr = a->ldr; p.resid2 = a->resid2; p.ldr2 = a->ldr2; p.scale = a->scale; p.scale2 = a->scale2; p.lrelu = a->lrelu != 0;
    p.C32 = a->C32; p.ldc32 = a->ldc32; p.C16 = (_Float16*)a->C16; p.ldc16 = a->ldc16;
    p.H = a->H; p.W = a->W; p.up = a->upsample; p.OH = a->H << p.up; p.OW = a->W << p.up; p.Cin = a->Cin;
    p.tiles_x = (p.OW + TW - 1) / TW; p.tiles_y = (p.OH + TH - 1) / TH;
    const long nblk = (long)p.tiles_x * p.tiles_y * a->n_img;
    if (nblk > 0x7fffffffL) return mlsd_set_error(-1, "mlsd_conv3x3_dense: grid too large");
    if (a->N == 32) hipLaunchKernelGGL(dconv3x3_kernel<32>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(dconv3x3_kernel<64>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, p);
    return mlsd_check_launch("dconv3x3_kernel");
}
