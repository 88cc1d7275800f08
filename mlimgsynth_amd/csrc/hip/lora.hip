// LoRA update of a weight that is already on the device, in the engine's layout and type:
//   W[dst(o n0 + c)] = round(W[..] + (sum_r up[o][r] down[r][c]) * scale)
// THE ARITHMETIC IS THE HOST MERGE'S (mlts_lora_apply, host/tstore.c), operation for operation: delta starts at +0, the rank index ascends, every product
// is rounded before it is added (both sides are built with -ffp-contract=off; written with __fmul_rn / __fadd_rn here so that no flag can change it), one
// multiplication by scale, one addition to the weight, one round-to-nearest-even conversion to the device type.  No MFMA and no reordered reduction: a weight
// patched here equals, bit for bit, the weight a cold load would have merged on the host, so an image never depends on what the context generated before.
// The kernel is bound by reading and writing W once (2 r fp32 operations per element moved); up and down are small and stay in L2.
//
// A block owns LT_ROWS output rows x LT_COLS columns and walks the rank in chunks of LT_RK: up rows and down columns of the chunk are staged in LDS (down reads are
// one dword per lane at consecutive addresses: conflict-free; up reads are broadcasts), a thread keeps 4 rows x 4 columns of delta in registers, columns interleaved
// by 64 so that each store instruction of a wave covers 64 consecutive elements of the device layout.  For the conv layout the fastest device dimension is cin, not
// the reference column c = k0 + K0 (k1 + K1 cin): the column POSITIONS q a block walks are then ordered (kk, cin) -- c = q / Cin + K0 K1 (q % Cin) -- and the
// destination comes from the same index rule as everywhere else (param_dst_index of common.hpp), which never produces a padding element.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

constexpr int LT_ROWS = 16, LT_COLS = 256, LT_RK = 16;      // 256 threads: 4 waves x 4 rows each, 64 lanes x 4 interleaved columns

__global__ __launch_bounds__(256) void lora_apply_kernel(void* __restrict__ W, int dtype, long n0, long n1, const float* __restrict__ up,
                                                         const float* __restrict__ down, int r, float scale, int layout, long p0, long p1, long p2, long p4,
                                                         int cin_major, int* __restrict__ flag)
{
    __shared__ float s_up[LT_ROWS][LT_RK];
    __shared__ float s_dn[LT_RK][LT_COLS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long row0 = (long)blockIdx.x * LT_ROWS, col0 = (long)blockIdx.y * LT_COLS;
    const long kk_n = p0 * p1;
    // reference column of a column position
#define LORA_COL(q) (cin_major ? (q) / p2 + kk_n * ((q) % p2) : (q))
    const long q_ld = col0 + tid;                       // the column this thread stages
    const long c_ld = q_ld < n0 ? LORA_COL(q_ld) : -1;
    const int u_row = tid / LT_RK, u_k = tid % LT_RK;   // the up element this thread stages
    long c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const long q = col0 + lane + 64 * j; c[j] = q < n0 ? LORA_COL(q) : -1; }
#undef LORA_COL
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    for (int k0 = 0; k0 < r; k0 += LT_RK) {
        const int kn = r - k0 < LT_RK ? r - k0 : LT_RK;
        __syncthreads();
        s_up[u_row][u_k] = (row0 + u_row < n1 && u_k < kn) ? up[(row0 + u_row) * r + k0 + u_k] : 0.f;
        for (int k = 0; k < kn; ++k) s_dn[k][tid] = c_ld >= 0 ? down[(long)(k0 + k) * n0 + c_ld] : 0.f;
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            float d[4], u[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = s_dn[k][lane + 64 * j];
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = s_up[wave * 4 + i][k];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __fadd_rn(acc[i][j], __fmul_rn(u[i], d[j]));
        }
    }

    int bad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long o = row0 + wave * 4 + i;
        if (o >= n1) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (c[j] < 0) continue;
            const long at = param_dst_index(layout, o * n0 + c[j], p0, p1, p2, p4);
            const float w = dtype == 1 ? (float)((const _Float16*)W)[at] : ((const float*)W)[at];
            const float v = __fadd_rn(w, __fmul_rn(acc[i][j], scale));
            bad |= !(fabsf(v) <= 3.4028234e38f);                // the host checks the fp32 sum, before the conversion
            if (dtype == 1) ((_Float16*)W)[at] = (_Float16)v; else ((float*)W)[at] = v;
        }
    }
    if (bad) atomicOr(flag, 1);
}

}  // namespace

extern "C" {

MLSD_API int mlsd_lora_apply(void* W, int dtype, int64_t n0, int64_t n1, const float* up, const float* down, int r, float scale, int layout,
                             int64_t p0, int64_t p1, int64_t p2, int64_t p3, int64_t p4, int* flag, void* stream)
{
    if (!W || !up || !down || !flag) return mlsd_set_error(-1, "mlsd_lora_apply: null pointer");
    if (dtype != 0 && dtype != 1) return mlsd_set_error(-1, "mlsd_lora_apply: unknown dtype %d (0 fp32, 1 fp16)", dtype);
    if (r < 1 || n0 < 1 || n1 < 1 || n0 >= ((int64_t)1 << 31) || n1 >= ((int64_t)1 << 31))
        return mlsd_set_error(-1, "mlsd_lora_apply: invalid sizes n0 %lld, n1 %lld, rank %d", (long long)n0, (long long)n1, r);
    const int64_t n = n0 * n1;
    // the layout parameters must describe exactly the n0 n1 elements that are updated: every destination index then lies inside the parameter's buffer
    auto fits = [n](int64_t a, int64_t b) { return a >= 1 && b >= 1 && a <= n / b; };        // a b <= n without overflow
    if (layout == 1) {
        if (!fits(p0, p1) || !fits(p0 * p1, p2) || !fits(p0 * p1 * p2, p3) || p0 * p1 * p2 * p3 != n || p4 < p2 || p4 >= ((int64_t)1 << 31))
            return mlsd_set_error(-1, "mlsd_lora_apply: conv layout %lldx%lldx%lldx%lld (pad %lld) does not hold %lld elements", (long long)p0, (long long)p1,
                                  (long long)p2, (long long)p3, (long long)p4, (long long)n);
    } else if (layout == 2) {
        if (p1 < 1 || p1 >= ((int64_t)1 << 31) || (p1 & 31) || !fits(p0, 2 * p1) || p0 * 2 * p1 != n)
            return mlsd_set_error(-1, "mlsd_lora_apply: GEGLU layout [%lld, 2 x %lld] does not hold %lld elements (d a multiple of 32)", (long long)p0, (long long)p1, (long long)n);
    } else if (layout != 0) return mlsd_set_error(-1, "mlsd_lora_apply: unknown layout %d", layout);
    const int64_t gx = (n1 + LT_ROWS - 1) / LT_ROWS, gy = (n0 + LT_COLS - 1) / LT_COLS;
    if (gy > 65535) return mlsd_set_error(-1, "mlsd_lora_apply: %lld columns are too many", (long long)n0);
    // the dry runtime's buffers are host memory: refuse before the launch
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("lora_apply");
    const int cin_major = layout == 1 && p0 * p1 > 1 && n0 == p0 * p1 * p2;
    hipLaunchKernelGGL(lora_apply_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, W, dtype, (long)n0, (long)n1, up, down, r, scale,
                       layout, (long)p0, (long)p1, (long)p2, (long)p4, cin_major, flag);
    return mlsd_check_launch("lora_apply");
}

}  // extern "C"
