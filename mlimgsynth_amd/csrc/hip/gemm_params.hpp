// The kernel parameter block of the GEMM / implicit-GEMM kernels of gemm_conv.hip, gemm_pp.hpp and gemm_skinny.hpp, and the small device helpers all three share.
// Every definition lives in the anonymous namespace: the headers and gemm_conv.hip each open their own `namespace {` (the anonymous namespaces of one translation unit
// are one namespace).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

struct GemmP {
    const _Float16* A;
    const _Float16* B;
    long lda, ldb;
    int M, N, K;
    // conv geometry
    int H, W, Cin, OH, OW, KH, KW, stride, pad, ups;
    int korder;   // conv, Cin % 64 == 0: 0 = K runs (kh, kw, cin), 1 = (cin / 64, kh, kw, cin % 64): the KH KW taps of a 64-channel slab are consecutive K tiles (mlsd_gemm_args.conv_korder)
    // epilogue
    const float* bias;
    const float* biasm;
    int act_post;
    int wrap;     // conv: mlsd_gemm_args.wrap of the kernels built with the wrap (in act_post's padding: no other field moves)
    const float* rowbias;
    int rows_per_batch;
    long ldrb;
    const float* resid;
    long ldr;
    int act;
    float* C32;
    long ldc32;
    _Float16* C16;
    long ldc16;
    int nbm, nbn;
    int vec;   // 1: every row stride and N are multiples of 4 -> wide (LDS-transposed) epilogue
    int dbg;   // diagnostics (timing-only builds of the loop): bit0 = no refills in the loop, bit1 = no MFMA/ds_read
    // split-K: blockIdx.y = slice z owns K tiles [z*kt_per, (z+1)*kt_per) and writes its raw fp32 partial sums to
    // C32 + z*ws_stride (the epilogue fields are cleared by the launcher; splitk_reduce applies them)
    int kt_per;
    long ws_stride;
    int gw;    // tile-order panel width (0: row-major)
    unsigned long long* tbuf;   // diagnostics: per-block cycle stamps of the ping-pong kernels (tools/gemm_trace.py), or null
    float* colstats;            // ping-pong kernels built with a *_STATS epilogue: [row block][2][N] column sums / sums of squares
    int cs_shift;               // 1: of (x - K), K = the column's value in the block's first row (mlsd_gemm_args.colstats_shift); 0: of x
    // stream-K (gemm_pp.hpp, SK): K-tile units per block, slabs [block][BM*BN] fp32, one flag per block
    int sk_L;
    float* sk_ws;
    unsigned* sk_flag;
    // LayerNorm at the end of the launch (gemm_pp.hpp *_LN epilogues): gamma, beta, eps, fp16 output, per-(row block, tile column, row) partials, counters
    const float *ln_g, *ln_b;
    float ln_eps;
    _Float16* ln_y;
    long ldln;
    float* ln_ws;
    unsigned* ln_cnt;
    int ln_slot;                // index of this launch's epoch word in ln_cnt (round 6: self-tagged records, no counters)
    int gn_G, gn_hw, gn_silu;   // splitk_reduce_gn: groups, rows per image, SiLU (gamma / beta / eps / output in the ln_* fields)
    // cross attention at the end of its q projection (gemm_pp.hpp PP_EPI_XATTN): K [n_img * Tk][ldk], V^T [n_img][N][96], output, rows per image, keys, log2(e) / sqrt(64)
    const _Float16 *xa_k, *xa_vt;
    _Float16* xa_out;
    long xa_ldk, xa_ldo;
    int xa_Tq, xa_Tk;
    float xa_sc;
    // phase form of an upsampling convolution (mlsd_gemm_args.tap_oy / tap_ox / out_phase; the ping-pong conv kernels): the tap window's origin per axis, and
    // opix = 1 + 2 py + px: row (n, y, x) is stored at pixel (2 y + py, 2 x + px) of a [n][2 OH][2 OW] image (PP_EPI_F32_PIX).  0: none.
    int tap_oy, tap_ox, opix;
};

static_assert(offsetof(GemmP, wrap) + sizeof(int) == offsetof(GemmP, rowbias), "GemmP::wrap must fill act_post's padding");

// wrap (circular padding): a coordinate at most one extent outside [0, e) folded into it
__host__ __device__ __forceinline__ int wrap_fold(int v, int e) { return v < 0 ? v + e : (v >= e ? v - e : v); }

// phase form of an upsampling convolution (GemmP::opix = 1 + 2 py + px): the pixel of the [n][2 OH][2 OW] output that row m = (n, y, x) of the launch is stored at
__host__ __device__ __forceinline__ long ups_out_pixel(int m, int OH, int OW, int opix)
{
    const int hw = OH * OW, ph = opix - 1;
    const int img = m / hw, rem = m - img * hw;
    const int y = rem / OW, x = rem - y * OW;
    return (long)img * 4 * hw + (long)(2 * y + (ph >> 1)) * (2 * OW) + 2 * x + (ph & 1);
}

// LDS tile: rows of BK halfs (128 B at BK=64, 64 B at BK=32); the 16-byte chunk c of row r lives at slot
// c ^ swz(r) so that a ds_read_b128 fragment read (32 lanes = 32 consecutive rows, one logical chunk)
// touches every bank once (64 banks x 4 B; 16-lane service groups).
template <int BK>
__device__ __forceinline__ int row_swz(int row) { return BK == 64 ? ((row >> 1) & 7) : ((row >> 2) & 3); }
template <int BK>
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * (BK * 2) + ((chunk ^ row_swz<BK>(row)) << 4); }

// 16 zero bytes in global memory: the source of every padded / out-of-range 16-byte chunk
// (global_load_lds has no bounds check and no zero-fill)
__device__ uint4 g_zero_page[4];

template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N < 64, "vmcnt immediate range");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

}  // namespace
