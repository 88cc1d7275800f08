// The PHASE FORM of an upsampling convolution: derived weights and the index maps, stated once for the device and the host.
//
// A 3x3 convolution (pad 1) that reads a nearest-2x upsampled H x W image computes, for output pixel (2 y + py, 2 x + px), taps at upsampled rows 2 y + py - 1 + kh,
// i.e. source rows (2 y + py - 1 + kh) >> 1:
//     py = 0:  kh = 0 -> y - 1,   kh = 1, 2 -> y            py = 1:  kh = 0, 1 -> y,   kh = 2 -> y + 1
// and the same along x.  Three taps of an axis meet TWO source pixels, so the 9 taps x Cin products of an output pixel are 4 x Cin products once the weights that meet
// the same pixel are added: each output parity (py, px) is a 2x2 convolution over the SOURCE whose window starts at (y - 1 + py, x - 1 + px) -- 4/9 of the multiply-adds.
// Padding agrees in both forms: upsampled row -1 is source row -1 and upsampled row 2 H is source row H, zero or wrapped alike.
//
// The new rounding point: a derived weight is the sum of 1, 2 or 4 fp16 weights, formed in fp32 in ascending (kh, kw) order (exact but for the last additions' rounding)
// and rounded ONCE to fp16 for the MFMA.  The launches that read them are ordinary ping-pong convolutions with mlsd_gemm_args.tap_oy / tap_ox / out_phase (gemm_pp.hpp).
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "gemm_params.hpp"

namespace {

// the taps k0 .. k1 of one axis that land on source offset a (0, 1) of the 2-wide window of output parity par
__host__ __device__ __forceinline__ void ups_tap_set(int par, int a, int& k0, int& k1)
{
    if (par == 0) { k0 = a ? 1 : 0; k1 = a ? 2 : 0; }
    else { k0 = a ? 2 : 0; k1 = a ? 2 : 1; }
}

// element e of dst [4][cout][2][2][cin] from src [cout][3][3][cin]
__host__ __device__ __forceinline__ _Float16 ups_phase_weight(const _Float16* src, long e, int cout, int cin)
{
    const int c = (int)(e % cin); long t = e / cin;
    const int b = (int)(t & 1), a = (int)((t >> 1) & 1); t >>= 2;
    const int o = (int)(t % cout), phase = (int)(t / cout);
    int kh0, kh1, kw0, kw1;
    ups_tap_set(phase >> 1, a, kh0, kh1);
    ups_tap_set(phase & 1, b, kw0, kw1);
    float s = 0.f;
    bool first = true;
    for (int kh = kh0; kh <= kh1; ++kh)
        for (int kw = kw0; kw <= kw1; ++kw) {
            const float w = (float)src[((long)(o * 3 + kh) * 3 + kw) * cin + c];
            s = first ? w : s + w;      // (a lone weight keeps its bits, a negative zero included)
            first = false;
        }
    return (_Float16)s;                 // round to nearest even
}

__global__ void ups_phase_weights_kernel(const _Float16* __restrict__ src, _Float16* __restrict__ dst, int cout, int cin, long n)
{
    GRID_LOOP(e, n) dst[e] = ups_phase_weight(src, e, cout, cin);
}

}  // namespace

extern "C" {

MLSD_API int mlsd_ups_phase_weights(const void* src, void* dst, int cout, int cin, void* stream)
{
    if (!src || !dst || cout < 1 || cin < 1) return mlsd_set_error(-1, "mlsd_ups_phase_weights: null pointer or empty weight (%d x %d)", cout, cin);
    const long n = 16L * cout * cin;
    if (mlsd_runtime_is_dry()) return mlsd_ups_phase_weights_host(src, dst, cout, cin);      // the dry runtime's buffers are host memory (plans built without a GPU, and the CPU tests of the rule)
    hipLaunchKernelGGL(ups_phase_weights_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)src, (_Float16*)dst, cout, cin, n);
    return mlsd_check_launch("ups_phase_weights");
}

/* the same rule on host memory (the master copy of a weight-streaming plan) */
MLSD_API int mlsd_ups_phase_weights_host(const void* src, void* dst, int cout, int cin)
{
    if (!src || !dst || cout < 1 || cin < 1) return mlsd_set_error(-1, "mlsd_ups_phase_weights_host: null pointer or empty weight (%d x %d)", cout, cin);
    const long n = 16L * cout * cin;
    for (long e = 0; e < n; ++e) ((_Float16*)dst)[e] = ups_phase_weight((const _Float16*)src, e, cout, cin);
    return 0;
}

/* The index maps of a convolution launch as the ping-pong kernels apply them (host restatement for the tests; stride / pad / tap_oy / tap_ox / wrap of a launch WITHOUT
 * the upsample in its gather): the source pixel n H W + ih W + iw that tap (kh, kw) of row m reads, or -1 where it reads a zero ... */
MLSD_API long mlsd_conv_tap_source(const mlsd_gemm_args* a, int m, int kh, int kw)
{
    if (!a || !a->conv || a->upsample || m < 0 || m >= a->M) return -2;
    const int ohw = a->OH * a->OW, img = m / ohw, rem = m - img * ohw, oh = rem / a->OW, ow = rem - oh * a->OW;
    int ih = oh * a->stride - a->pad + a->tap_oy + kh, iw = ow * a->stride - a->pad + a->tap_ox + kw;
    if (a->wrap & 2) ih = wrap_fold(ih, a->H);
    if (a->wrap & 1) iw = wrap_fold(iw, a->W);
    if ((unsigned)ih >= (unsigned)a->H || (unsigned)iw >= (unsigned)a->W) return -1;
    return ((long)img * a->H + ih) * a->W + iw;
}

/* ... and the pixel of the output image that row m is stored at (out_phase: the [n][2 OH][2 OW] image; 0: row m itself) */
MLSD_API long mlsd_conv_out_pixel(const mlsd_gemm_args* a, int m)
{
    if (!a || m < 0 || m >= a->M) return -2;
    return a->out_phase ? ups_out_pixel(m, a->OH, a->OW, a->out_phase) : m;
}

}  // extern "C"
