// The output epilogue of the general GEMM tiles and of the split-K reduce passes (gemm_conv.hip): "finish four consecutive columns of row m".
//
// THE BIT-IDENTITY PROMISE.  A launch may finish its output in gemm_kernel's wide epilogue, in the PAR tail of the same kernel, or in one of the reduce passes
// (splitk_reduce, _stats, _ln, _gn); the plan builder picks among them by speed alone, and the GPU tests assert that the fp32 output does not depend on the pick.
// That holds because every one of them adds the K slices with sum_slices4's order (slice 0 starts the sum, then 1, 2, ...) and finishes the sum with epilogue4:
// the same operations in the same order, written once, here.  A new epilogue term or activation goes into epilogue4 / act_apply and nowhere else.
#pragma once
#include "gemm_params.hpp"

namespace {

__device__ __forceinline__ float4 add4(float4 a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; return a; }

// v = the raw sums of columns n .. n + 3 of row m.  Order: column bias, per-row bias (biasm), per-image row bias, residual if act_post, activation, residual if not
// act_post.  A caller that loaded the bias of its columns once for many rows passes it as `bv` with bias_pre (it is then added unconditionally: zeros where there is
// none); one that prefetched the residual (gemm_kernel's PRE builds) passes it as `rs_pre` with resid_pre.  Everything else is read here.
__device__ __forceinline__ float4 epilogue4(const GemmP& p, int m, int n, float4 v, bool bias_pre = false, const float4 bv = make_float4(0, 0, 0, 0),
                                            bool resid_pre = false, const float4 rs_pre = make_float4(0, 0, 0, 0))
{
    if (bias_pre) v = add4(v, bv);
    else if (p.bias) v = add4(v, *reinterpret_cast<const float4*>(p.bias + n));
    if (p.biasm) { const float b = p.biasm[m]; v.x += b; v.y += b; v.z += b; v.w += b; }
    if (p.rowbias) v = add4(v, *reinterpret_cast<const float4*>(p.rowbias + (long)(m / p.rows_per_batch) * p.ldrb + n));
    float4 rs = make_float4(0, 0, 0, 0);
    if (resid_pre) rs = rs_pre;
    else if (p.resid) rs = *reinterpret_cast<const float4*>(p.resid + (long)m * p.ldr + n);
    if (p.act_post) v = add4(v, rs);
    v = act_apply(p.act, v);
    if (!p.act_post) v = add4(v, rs);
    return v;
}

// the finished columns to the fp32 and / or the fp16 output (a null pointer: that output is not written)
__device__ __forceinline__ void store4(float* C32, long ldc32, _Float16* C16, long ldc16, int m, int n, const float4 v)
{
    if (C32) *reinterpret_cast<float4*>(C32 + (long)m * ldc32 + n) = v;
    if (C16) {
        f16x4 h = {(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w};
        *reinterpret_cast<f16x4*>(C16 + (long)m * ldc16 + n) = h;
    }
}

// the K slices of a split-K workspace ([slice][M][N] fp32, ws_stride floats apart) at element offset `off`, added in slice order: slice 0 starts the sum
__device__ __forceinline__ float4 sum_slices4(const float* __restrict__ ws, long ws_stride, long off, int nsplit)
{
    float4 v = *reinterpret_cast<const float4*>(ws + off);
    for (int z = 1; z < nsplit; ++z) v = add4(v, *reinterpret_cast<const float4*>(ws + z * ws_stride + off));
    return v;
}

}  // namespace
