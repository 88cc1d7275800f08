// ControlNet (mlb_controlnet / the control inputs of mlb_unet_denoise_ctrl, host/unet.c): the two passes the feature adds outside GEMMs.
//   mlsd_ctrl_add            dst = base + gain * ctrl on channels-last fp32 maps; the UNet plan runs it on every skip tensor it pops and on the middle block's output.
//                            The gain is ONE float in device memory, read by every lane through the kernel's pointer argument (a uniform load): strength and the
//                            step window change between evaluations, and under a captured graph, without touching the plan.  gain == 0 is a copy of base's bits
//                            that never reads ctrl (the ControlNet plan did not run: ctrl holds whatever the last controlled evaluation left, or nothing).
//   mlsd_window_gather_nhwc  windows of the canvas's hint embedding for the slots of a tiled plan's batch, bit copies.
// Both are bandwidth-bound: 16 bytes per lane along the channel axis, one row segment per run of C / 4 lanes, the grid follows the element count (nblk).
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

// one float4 per thread step: element i = (row, c4) of [rows][C / 4], rows = images x rows per image; ctrl holds ctrl_rows of them and is read modulo that
__global__ void ctrl_add_kernel(float* __restrict__ dst, long ld_dst, const float* __restrict__ base, long ld_base, const float* __restrict__ ctrl, long ld_ctrl,
                                long rows, long ctrl_rows, int C4, const float* __restrict__ gain_dev)
{
    const float gain = *gain_dev;
    const long total = rows * C4;
    if (gain == 0.f) {                                  // (uniform over the grid; -0 is 0 too)
        GRID_LOOP(i, total) {
            const long r = i / C4; const int c = (int)(i - r * C4) * 4;
            *reinterpret_cast<u32x4*>(dst + r * ld_dst + c) = *reinterpret_cast<const u32x4*>(base + r * ld_base + c);      // bits, not values
        }
        return;
    }
    GRID_LOOP(i, total) {
        const long r = i / C4; const int c = (int)(i - r * C4) * 4;
        const long rc = r % ctrl_rows;                  // image n of dst reads image n % n_ctrl_img of ctrl: rows are [image][row of the image]
        const float4 b = *reinterpret_cast<const float4*>(base + r * ld_base + c);
        const float4 k = *reinterpret_cast<const float4*>(ctrl + rc * ld_ctrl + c);
        float4 o;
        o.x = __fadd_rn(b.x, __fmul_rn(gain, k.x)); o.y = __fadd_rn(b.y, __fmul_rn(gain, k.y));
        o.z = __fadd_rn(b.z, __fmul_rn(gain, k.z)); o.w = __fadd_rn(b.w, __fmul_rn(gain, k.w));
        *reinterpret_cast<float4*>(dst + r * ld_dst + c) = o;
    }
}

struct NhwcSlots { int xs[MLSD_WINDOW_MAX_PACK], ys[MLSD_WINDOW_MAX_PACK]; };

__device__ __forceinline__ int wrap_at(int s, int k, int L) { const int p = s + k; return p >= L ? p - L : p; }      // s < L, k <= L

// dst [n_slots][n_rep][wh][ww][C]: blockIdx.y is the slot (its start is uniform over the wave), the x grid loops over one slot's n_rep * wh * ww * C / 4 vectors
__global__ void window_gather_nhwc_kernel(const u32x4* __restrict__ src, int W, int H, int C4, u32x4* __restrict__ dst, int ww, int wh, NhwcSlots L, int n_rep)
{
    const int s = (int)blockIdx.y;
    const int x0 = L.xs[s], y0 = L.ys[s];
    const long whw = (long)wh * ww, total = (long)n_rep * whw * C4;
    u32x4* __restrict__ out = dst + (long)s * total;
    GRID_LOOP(i, total) {
        const int c = (int)(i % C4);
        const long p = (i / C4) % whw;                  // pixel of the window; the repeats read the same source
        const int u = (int)(p % ww), v = (int)(p / ww);
        out[i] = src[((long)wrap_at(y0, v, H) * W + wrap_at(x0, u, W)) * C4 + c];
    }
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) { return (const char*)a < (const char*)b + nb && (const char*)b < (const char*)a + na; }

}  // namespace

extern "C" MLSD_API int mlsd_ctrl_add(float* dst, int64_t ld_dst, const float* base, int64_t ld_base, const float* ctrl, int64_t ld_ctrl, int n_img, int rows_per_img,
                                      int C, int n_ctrl_img, const float* gain_dev, void* stream)
{
    if (!dst || !base || !ctrl || !gain_dev || n_img < 1 || rows_per_img < 1 || C < 4 || n_ctrl_img < 1 || n_ctrl_img > n_img)
        return mlsd_set_error(-1, "mlsd_ctrl_add: bad argument (%d images of %d rows x %d, %d control images)", n_img, rows_per_img, C, n_ctrl_img);
    if ((C & 3) || ld_dst < C || ld_base < C || ld_ctrl < C || (ld_dst & 3) || (ld_base & 3) || (ld_ctrl & 3))
        return mlsd_set_error(-1, "mlsd_ctrl_add: C %d and the row strides %lld %lld %lld must be multiples of 4, strides >= C", C, (long long)ld_dst, (long long)ld_base, (long long)ld_ctrl);
    if (((uintptr_t)dst | (uintptr_t)base | (uintptr_t)ctrl) & 15) return mlsd_set_error(-1, "mlsd_ctrl_add: pointers must be 16-byte aligned");
    if ((uintptr_t)gain_dev & 3) return mlsd_set_error(-1, "mlsd_ctrl_add: misaligned gain");
    const long rows = (long)n_img * rows_per_img, ctrl_rows = (long)n_ctrl_img * rows_per_img;
    const size_t nd = (size_t)rows * ld_dst * 4, nb = (size_t)rows * ld_base * 4, nc = (size_t)ctrl_rows * ld_ctrl * 4;
    if (overlap(dst, nd, ctrl, nc) || (dst != base && overlap(dst, nd, base, nb)) || (dst == base && ld_dst != ld_base))
        return mlsd_set_error(-1, "mlsd_ctrl_add: dst overlaps an operand");      // (dst == base with equal strides is the in-place form: every lane reads what it writes)
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("ctrl_add");      // the dry runtime's buffers are host memory: refuse before the launch
    hipLaunchKernelGGL(ctrl_add_kernel, dim3(nblk(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, dst, (long)ld_dst, base, (long)ld_base, ctrl, (long)ld_ctrl,
                       rows, ctrl_rows, C / 4, gain_dev);
    return mlsd_check_launch("ctrl_add");
}

extern "C" MLSD_API int mlsd_window_gather_nhwc(const float* src, int W, int H, int C, float* dst, int ww, int wh, const int* xs, const int* ys, int n_slots, int n_rep,
                                                void* stream)
{
    if (!src || !dst || !xs || !ys || n_rep < 1 || n_slots < 1 || n_slots > MLSD_WINDOW_MAX_PACK)
        return mlsd_set_error(-1, "mlsd_window_gather_nhwc: bad argument (%d slots, 1 .. %d; %d repeats)", n_slots, MLSD_WINDOW_MAX_PACK, n_rep);
    if (C < 4 || (C & 3) || (((uintptr_t)src | (uintptr_t)dst) & 15)) return mlsd_set_error(-1, "mlsd_window_gather_nhwc: C %d must be a multiple of 4, pointers 16-byte aligned", C);
    if (W < 1 || H < 1 || ww < 1 || wh < 1 || ww > W || wh > H) return mlsd_set_error(-1, "mlsd_window_gather_nhwc: window %dx%d of a %dx%d canvas", ww, wh, W, H);
    NhwcSlots L;
    for (int s = 0; s < MLSD_WINDOW_MAX_PACK; ++s) {
        if (s < n_slots && (xs[s] < 0 || xs[s] >= W || ys[s] < 0 || ys[s] >= H))
            return mlsd_set_error(-1, "mlsd_window_gather_nhwc: window %d starts at (%d, %d) of a %dx%d canvas", s, xs[s], ys[s], W, H);
        L.xs[s] = s < n_slots ? xs[s] : 0; L.ys[s] = s < n_slots ? ys[s] : 0;
    }
    const long n_src = (long)H * W * C, n_one = (long)n_rep * wh * ww * C, n_dst = n_one * n_slots;
    if (n_src >= (1L << 33) || n_dst >= (1L << 33)) return mlsd_set_error(-1, "mlsd_window_gather_nhwc: more than 2^33 elements");
    if (overlap(src, (size_t)n_src * 4, dst, (size_t)n_dst * 4)) return mlsd_set_error(-1, "mlsd_window_gather_nhwc: source and windows overlap");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("window_gather_nhwc");
    hipLaunchKernelGGL(window_gather_nhwc_kernel, dim3(nblk(n_one / 4), (unsigned)n_slots), dim3(256), 0, (hipStream_t)stream, (const u32x4*)src, W, H, C / 4,
                       (u32x4*)dst, ww, wh, L, n_rep);
    return mlsd_check_launch("window_gather_nhwc");
}
