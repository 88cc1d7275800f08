// Perturbed-attention guidance (PAG; "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance", 2024; not in the reference): the mix of an evaluation
// whose plan carries a third row group.  eps is the UNet output, NHWC [N][HW][ld] with the groups [cond B | uncond B (only at cfg > 1) | perturbed B]; x, dx and
// noise are NCHW [B][C][HW].  Per element, with c, u, p after the v-prediction rescale of src/unet.c:490-494:
//   g  = c*cfg + u*(1 - cfg)   (cfg > 1; else g = c)       -- the very operations of dxdt_cfg_kernel (sampler.hip)
//   dx = g + pag*(c - p)                                    -- three more, each rounded once
// pag == 0 is dxdt_cfg_kernel's path: the perturbed rows are not read (they may hold anything).
//
// Bandwidth bound on a few hundred KB to a few MB: what matters is that no lane fetches a 4-byte piece of a row another lane fetches again.  An eps row is the C = 4
// channels of one pixel (16 bytes of an ld x 4 byte stride), an x / dx plane is HW consecutive floats.  So a thread owns PIXELS and all four channels of them: one
// 16-byte load per group row, and the NCHW side is either four plane accesses that are consecutive across the lanes (one pixel per thread) or, where HW and the
// pointers allow, four 16-byte accesses of four consecutive pixels (four pixels per thread).  Everything else (C != 4, rows that are not whole 16-byte pieces) takes
// the element-per-thread form of sampler.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

struct PagMix { float cfg, pag, c_out, c_skip; int vparam; };

__device__ __forceinline__ float pag_rescale(float e, float xv, const PagMix& m)
{
    return m.vparam ? __fadd_rn(__fmul_rn(e, m.c_out), __fmul_rn(xv, m.c_skip)) : e;                 // unet.c:493
}

// one element: ec / eu / ep are read through the pointers only where the mix needs them
__device__ __forceinline__ float pag_mix(float c, float u, float p, float xv, const PagMix& m)
{
    const float d = pag_rescale(c, xv, m);
    float g = d;
    if (m.cfg > 1.0f) g = __fadd_rn(__fmul_rn(d, m.cfg), __fmul_rn(pag_rescale(u, xv, m), 1.0f - m.cfg));   // mlimgsynth.c:1583
    if (m.pag != 0.0f) g = __fadd_rn(g, __fmul_rn(m.pag, __fsub_rn(d, pag_rescale(p, xv, m))));
    return g;
}

// solvers.c:86 and sampling.c:115 behind the mix (the fused Euler(-ancestral) step)
__device__ __forceinline__ float euler_step(float x, float d, float dt, const float* noise, long i, float s_up)
{
    float v = __fadd_rn(x, __fmul_rn(d, dt));
    if (noise) v = __fadd_rn(v, __fmul_rn(noise[i], s_up));
    return v;
}

// element per thread: any C, any ld >= C.  EULER: x is updated in place (vparam is 0), else dx = mix
template <bool EULER>
__global__ void pag_scalar_kernel(const float* __restrict__ eps, long ld, const float* x, float* out, const float* __restrict__ noise,
                                  int B, int C, int HW, PagMix m, float dt, float s_up)
{
    const long total = (long)B * C * HW;
    const int gu = B, gp = m.cfg > 1.0f ? 2 * B : B;
    GRID_LOOP(i, total) {
        const int pix = (int)(i % HW);
        const long t = i / HW;
        const int c = (int)(t % C), b = (int)(t / C);
        const float ec = eps[((long)b * HW + pix) * ld + c];
        const float eu = m.cfg > 1.0f ? eps[((long)(b + gu) * HW + pix) * ld + c] : 0.f;
        const float ep = m.pag != 0.0f ? eps[((long)(b + gp) * HW + pix) * ld + c] : 0.f;
        const float xv = (EULER || m.vparam) ? x[i] : 0.f;
        const float d = pag_mix(ec, eu, ep, xv, m);
        out[i] = EULER ? euler_step(xv, d, dt, noise, i, s_up) : d;
    }
}

// C == 4, rows of whole 16-byte pieces: a thread owns PX consecutive pixels of one image (PX 4 needs HW % 4 == 0 and 16-byte aligned planes)
template <int PX, bool EULER>
__global__ void pag_pixel_kernel(const float* __restrict__ eps, long ld, const float* x, float* out, const float* __restrict__ noise,
                                 int B, int HW, PagMix m, float dt, float s_up)
{
    const long per = HW / PX, total = (long)B * per;
    const int gu = B, gp = m.cfg > 1.0f ? 2 * B : B;
    const bool need_x = EULER || m.vparam;
    GRID_LOOP(i, total) {
        const int b = (int)(i / per);
        const long pix0 = (i - (long)b * per) * PX;
        float v[4][PX], xv[4][PX], nz[4][PX];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long o = ((long)b * 4 + c) * HW + pix0;
            if constexpr (PX == 4) {
                const float4 a = need_x ? *reinterpret_cast<const float4*>(x + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                xv[c][0] = a.x; xv[c][1] = a.y; xv[c][2] = a.z; xv[c][3] = a.w;
                if (EULER && noise) {
                    const float4 n = *reinterpret_cast<const float4*>(noise + o);
                    nz[c][0] = n.x; nz[c][1] = n.y; nz[c][2] = n.z; nz[c][3] = n.w;
                }
            } else {
                xv[c][0] = need_x ? x[o] : 0.f;
                if (EULER && noise) nz[c][0] = noise[o];
            }
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 ec = *reinterpret_cast<const float4*>(eps + ((long)b * HW + pix0 + k) * ld);
            const float4 eu = m.cfg > 1.0f ? *reinterpret_cast<const float4*>(eps + ((long)(b + gu) * HW + pix0 + k) * ld) : z;
            const float4 ep = m.pag != 0.0f ? *reinterpret_cast<const float4*>(eps + ((long)(b + gp) * HW + pix0 + k) * ld) : z;
            v[0][k] = pag_mix(ec.x, eu.x, ep.x, xv[0][k], m); v[1][k] = pag_mix(ec.y, eu.y, ep.y, xv[1][k], m);
            v[2][k] = pag_mix(ec.z, eu.z, ep.z, xv[2][k], m); v[3][k] = pag_mix(ec.w, eu.w, ep.w, xv[3][k], m);
        }
        if (EULER) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int k = 0; k < PX; ++k) {
                    float r = __fadd_rn(xv[c][k], __fmul_rn(v[c][k], dt));
                    if (noise) r = __fadd_rn(r, __fmul_rn(nz[c][k], s_up));
                    v[c][k] = r;
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long o = ((long)b * 4 + c) * HW + pix0;
            if constexpr (PX == 4) *reinterpret_cast<float4*>(out + o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            else out[o] = v[c][0];
        }
    }
}

inline bool al16(const void* p) { return !((uintptr_t)p & 15); }

// x: the evaluation point (dxdt; read only with vparam) or the latent updated in place (EULER); out: dx or that latent
template <bool EULER>
int pag_launch(const char* what, const float* eps, int64_t ld, const float* x, float* out, const float* noise, int B, int C, int HW, PagMix m, float dt, float s_up,
               void* stream)
{
    if (!eps || (!x && (EULER || m.vparam)) || !out || B < 1 || C < 1 || HW < 1 || ld < C || !(m.pag >= 0.0f))
        return mlsd_set_error(-1, "%s: bad argument (B %d, C %d, HW %d, ld %lld, pag %g)", what, B, C, HW, (long long)ld, (double)m.pag);
    const long n = (long)B * C * HW, rows = (long)B * HW * (1 + (m.cfg > 1.0f ? 1 : 0) + (m.pag != 0.0f ? 1 : 0));
    if (n >= (1L << 31) || rows * ld >= (1L << 31)) return mlsd_set_error(-1, "%s: more than 2^31 elements", what);
    hipStream_t st = (hipStream_t)stream;
    if (C == 4 && !(ld & 3) && al16(eps)) {
        if (!(HW & 3) && al16(x) && al16(out) && (!noise || al16(noise)))
            hipLaunchKernelGGL((pag_pixel_kernel<4, EULER>), dim3(nblk((long)B * (HW / 4))), dim3(256), 0, st, eps, (long)ld, x, out, noise, B, HW, m, dt, s_up);
        else
            hipLaunchKernelGGL((pag_pixel_kernel<1, EULER>), dim3(nblk((long)B * HW)), dim3(256), 0, st, eps, (long)ld, x, out, noise, B, HW, m, dt, s_up);
    } else
        hipLaunchKernelGGL((pag_scalar_kernel<EULER>), dim3(nblk(n)), dim3(256), 0, st, eps, (long)ld, x, out, noise, B, C, HW, m, dt, s_up);
    return mlsd_check_launch(what);
}

}  // namespace

extern "C" MLSD_API int mlsd_dxdt_pag(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag,
                                      int vparam, float c_out, float c_skip, void* stream)
{
    const PagMix m = { cfg, pag, c_out, c_skip, vparam };
    return pag_launch<false>("mlsd_dxdt_pag", eps, ld, x_eval, dx, nullptr, B, C, HW, m, 0.f, 0.f, stream);
}

extern "C" MLSD_API int mlsd_euler_pag_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, float dt,
                                              const float* noise, float s_up, void* stream)
{
    const PagMix m = { cfg, pag, 1.f, 0.f, 0 };
    return pag_launch<true>("mlsd_euler_pag_update", eps, ld, x, x, noise, B, C, HW, m, dt, s_up, stream);
}
