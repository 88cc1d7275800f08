// The guided prediction every solver stage reads: classifier-free guidance (src/mlimgsynth.c:1565-1587), perturbed-attention guidance (PAG; "Self-Rectifying
// Diffusion Sampling with Perturbed-Attention Guidance", 2024; not in the reference) and guidance rescale ("Common Diffusion Noise Schedules and Sample Steps are
// Flawed", 2023, Algorithm 2; not in the reference), stated ONCE: one mix (guided), one kernel family (guide_*_kernel), one launcher (guide_launch).  The entries,
// the row groups and the two operation orders are described in include/mlsd_kernels.h.  A further guidance term is a field of Guide and a line of guided().
//
// eps is the UNet output, NHWC [N][HW][ld] with the groups [cond B | uncond B (only at cfg > 1) | perturbed B (only read at pag != 0)]; x, dx and noise are NCHW
// [B][C][HW].  Every operation is an explicit _rn intrinsic, rounded once: the bits do not depend on the kernel form.
//
// Bandwidth bound on a few hundred KB to a few MB: what matters is that no lane fetches a 4-byte piece of a row another lane fetches again.  An eps row is the C = 4
// channels of one pixel (16 bytes of an ld x 4 byte stride), an x / dx plane is HW consecutive floats.  So a thread owns PIXELS and all four channels of them: one
// 16-byte load per group row, and the NCHW side is either four plane accesses that are consecutive across the lanes (one pixel per thread) or, where HW and the
// pointers allow, four 16-byte accesses of four consecutive pixels (four pixels per thread).  Everything else (C != 4, rows that are not whole 16-byte pieces) takes
// the element-per-thread form.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

struct Guide { float cfg, pag, c_out, c_skip; int vparam; const float* factor; };      // factor: device, one float per image; NULL: no rescale

// the raw mix of the three groups; u and p are used only where cfg > 1 and pag != 0 (the callers do not load them elsewhere)
__device__ __forceinline__ float guided(float c, float u, float p, float cfg, float pag)
{
    float g = c;
    if (cfg > 1.0f) g = __fadd_rn(__fmul_rn(c, cfg), __fmul_rn(u, 1.0f - cfg));                      // mlimgsynth.c:1583
    if (pag != 0.0f) g = __fadd_rn(g, __fmul_rn(pag, __fsub_rn(c, p)));
    return g;
}

// not rescaled: the v map (unet.c:493) on each group, then the mix.  Rescaled: the mix of the raw outputs, times factor[b], then the v map once.
template <bool RESCALED>
__device__ __forceinline__ float guide_mix(float c, float u, float p, float xv, float f, const Guide& m)
{
    const auto vmap = [&](float e) { return m.vparam ? __fadd_rn(__fmul_rn(e, m.c_out), __fmul_rn(xv, m.c_skip)) : e; };
    if constexpr (RESCALED) return vmap(__fmul_rn(guided(c, u, p, m.cfg, m.pag), f));
    else return guided(vmap(c), vmap(u), vmap(p), m.cfg, m.pag);
}

// solvers.c:86 and sampling.c:115 behind the mix (the fused Euler(-ancestral) step)
__device__ __forceinline__ float euler_tail(float x, float d, float dt, bool noisy, float nz, float s_up)
{
    const float v = __fadd_rn(x, __fmul_rn(d, dt));
    return noisy ? __fadd_rn(v, __fmul_rn(nz, s_up)) : v;
}

// element per thread: any C, any ld >= C.  EULER: x is updated in place (vparam is 0), else dx = mix
template <bool EULER, bool RESCALED>
__global__ void guide_scalar_kernel(const float* __restrict__ eps, long ld, const float* x, float* out, const float* __restrict__ noise,
                                    int B, int C, int HW, Guide m, float dt, float s_up)
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
        const float d = guide_mix<RESCALED>(ec, eu, ep, xv, RESCALED ? m.factor[b] : 1.f, m);
        out[i] = EULER ? euler_tail(xv, d, dt, noise, noise ? noise[i] : 0.f, s_up) : d;
    }
}

// C == 4, rows of whole 16-byte pieces: a thread owns PX consecutive pixels of one image (PX 4 needs HW % 4 == 0 and 16-byte aligned planes)
template <int PX, bool EULER, bool RESCALED>
__global__ void guide_pixel_kernel(const float* __restrict__ eps, long ld, const float* x, float* out, const float* __restrict__ noise,
                                   int B, int HW, Guide m, float dt, float s_up)
{
    const long per = HW / PX, total = (long)B * per;
    const int gu = B, gp = m.cfg > 1.0f ? 2 * B : B;
    const bool need_x = EULER || m.vparam;
    GRID_LOOP(i, total) {
        const int b = (int)(i / per);
        const long pix0 = (i - (long)b * per) * PX;
        const float f = RESCALED ? m.factor[b] : 1.f;
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
            // (the zeros are temporaries, not one named zero: between two lvalues ?: selects an ADDRESS, the zero's in scratch, and the load goes through it)
            const float4 ec = *reinterpret_cast<const float4*>(eps + ((long)b * HW + pix0 + k) * ld);
            const float4 eu = m.cfg > 1.0f ? *reinterpret_cast<const float4*>(eps + ((long)(b + gu) * HW + pix0 + k) * ld) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 ep = m.pag != 0.0f ? *reinterpret_cast<const float4*>(eps + ((long)(b + gp) * HW + pix0 + k) * ld) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0][k] = guide_mix<RESCALED>(ec.x, eu.x, ep.x, xv[0][k], f, m); v[1][k] = guide_mix<RESCALED>(ec.y, eu.y, ep.y, xv[1][k], f, m);
            v[2][k] = guide_mix<RESCALED>(ec.z, eu.z, ep.z, xv[2][k], f, m); v[3][k] = guide_mix<RESCALED>(ec.w, eu.w, ep.w, xv[3][k], f, m);
        }
        if (EULER) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int k = 0; k < PX; ++k) v[c][k] = euler_tail(xv[c][k], v[c][k], dt, noise, noise ? nz[c][k] : 0.f, s_up);
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

// ------------------------------------------------------------------ guidance rescale: the factor
// Per image b, over its n = C*HW elements, with c, u, p the RAW outputs of the three row groups (for a v model: before out*c_out + x*c_skip) and g = guided(c, u, p):
//   f = phi*sqrt(M2(c) / M2(g)) + (1 - phi),  M2 = sum of squared deviations from the mean
// Two launches: statistics, factor.  The mix kernels above then read factor[b] from the device.
//   statistics: grid (blocks per image, B).  The blocks of an image split its pixels into equal contiguous runs, a rule of HW alone (gr_blocks); a thread walks its run
//     in steps of the block size and accumulates, in DOUBLE, sum and sum of squares of (c - c0) and (g - g0), c0 / g0 the image's first element (shifted data: a
//     constant image gives exact zeros, and nothing cancels against a large mean).  Lanes by a shuffle tree, waves through LDS in wave order, then thread 0 stores the
//     block's four doubles to part[b][block][4].  No atomics, no block reads what another block wrote.
//   factor: thread b sums the partials of image b in block order and writes factor[b] as float (f formed in double, rounded once).
constexpr int GR_PIX_PER_BLOCK = 1024;

inline int gr_blocks(int HW)
{
    const int nb = (HW + GR_PIX_PER_BLOCK - 1) / GR_PIX_PER_BLOCK;
    return nb < 1 ? 1 : (nb > MLSD_GUIDANCE_MAX_BLOCKS ? MLSD_GUIDANCE_MAX_BLOCKS : nb);
}

__device__ __forceinline__ void gr_acc(double s[4], float c, float g, float c0, float g0)
{
    const double dc = (double)c - (double)c0, dg = (double)g - (double)g0;
    s[0] += dc; s[1] += dc * dc; s[2] += dg; s[3] += dg * dg;
}

// VEC4: C == 4, ld % 4 == 0 and eps 16-byte aligned (one 16-byte load per group row); else element by element over any C, ld >= C
template <bool VEC4>
__global__ __launch_bounds__(256) void gr_stats_kernel(const float* __restrict__ eps, long ld, int B, int C, int HW, float cfg, float pag, double* __restrict__ part)
{
    const int b = blockIdx.y, nb = gridDim.x;
    const int chunk = (HW + nb - 1) / nb, p0 = blockIdx.x * chunk, p1 = p0 + chunk < HW ? p0 + chunk : HW;
    const bool has_u = cfg > 1.0f, has_p = pag != 0.0f;
    const float* rc = eps + (long)b * HW * ld;
    const float* ru = eps + (long)(b + B) * HW * ld;
    const float* rp = eps + (long)(b + (has_u ? 2 * B : B)) * HW * ld;
    const float c0 = rc[0], g0 = guided(c0, has_u ? ru[0] : 0.f, has_p ? rp[0] : 0.f, cfg, pag);
    double s[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (int pix = p0 + (int)threadIdx.x; pix < p1; pix += 256) {
        const long o = (long)pix * ld;
        if constexpr (VEC4) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 c = *reinterpret_cast<const float4*>(rc + o);
            const float4 u = has_u ? *reinterpret_cast<const float4*>(ru + o) : z;
            const float4 p = has_p ? *reinterpret_cast<const float4*>(rp + o) : z;
            gr_acc(s, c.x, guided(c.x, u.x, p.x, cfg, pag), c0, g0); gr_acc(s, c.y, guided(c.y, u.y, p.y, cfg, pag), c0, g0);
            gr_acc(s, c.z, guided(c.z, u.z, p.z, cfg, pag), c0, g0); gr_acc(s, c.w, guided(c.w, u.w, p.w, cfg, pag), c0, g0);
        } else {
            for (int k = 0; k < C; ++k) {
                const float c = rc[o + k];
                gr_acc(s, c, guided(c, has_u ? ru[o + k] : 0.f, has_p ? rp[o + k] : 0.f, cfg, pag), c0, g0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, 64);
    __shared__ double sh[4][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { sh[wave][0] = s[0]; sh[wave][1] = s[1]; sh[wave][2] = s[2]; sh[wave][3] = s[3]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = part + ((long)b * nb + blockIdx.x) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
    }
}

// identity: g is c (cfg <= 1, pag == 0); the partials are not read and every factor is 1
__global__ void gr_factor_kernel(const double* __restrict__ part, int nb, int B, double n, float phi, int identity, float* __restrict__ factor)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double f = 1.0;
    if (!identity && n > 1.0) {
        double s[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int j = 0; j < nb; ++j)
            for (int k = 0; k < 4; ++k) s[k] += part[((long)b * nb + j) * 4 + k];
        double m2c = s[1] - s[0] * s[0] / n;
        const double m2g = s[3] - s[2] * s[2] / n;
        if (m2c < 0.0) m2c = 0.0;                              // (a rounding residue of a constant-but-for-noise image)
        if (m2g > 0.0 && isfinite(m2g) && isfinite(m2c)) f = (double)phi * sqrt(m2c / m2g) + (1.0 - (double)phi);
        if (!isfinite(f)) f = 1.0;
    }
    factor[b] = (float)f;
}

// ------------------------------------------------------------------ launching
// the arguments every entry of this file shares; 0 when they are good
int gr_check(const char* what, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag)
{
    if (!eps || B < 1 || C < 1 || HW < 1 || ld < C || !(pag >= 0.0f) || cfg != cfg)
        return mlsd_set_error(-1, "%s: bad argument (B %d, C %d, HW %d, ld %lld, cfg %g, pag %g)", what, B, C, HW, (long long)ld, (double)cfg, (double)pag);
    const long n = (long)B * C * HW, rows = (long)B * HW * (1 + (cfg > 1.0f ? 1 : 0) + (pag != 0.0f ? 1 : 0));
    if (n >= (1L << 31) || rows * ld >= (1L << 31)) return mlsd_set_error(-1, "%s: more than 2^31 elements", what);
    return 0;
}

// the form rule.  x: the evaluation point (dxdt; read only with vparam) or the latent updated in place (EULER); out: dx or that latent
template <bool EULER, bool RESCALED>
int guide_launch(const char* what, const float* eps, int64_t ld, const float* x, float* out, const float* noise, int B, int C, int HW, const Guide& m, float dt,
                 float s_up, hipStream_t st)
{
    if (C == 4 && !(ld & 3) && al16(eps)) {
        if (!(HW & 3) && al16(x) && al16(out) && (!noise || al16(noise)))
            hipLaunchKernelGGL((guide_pixel_kernel<4, EULER, RESCALED>), dim3(nblk((long)B * (HW / 4))), dim3(256), 0, st, eps, (long)ld, x, out, noise, B, HW, m, dt, s_up);
        else
            hipLaunchKernelGGL((guide_pixel_kernel<1, EULER, RESCALED>), dim3(nblk((long)B * HW)), dim3(256), 0, st, eps, (long)ld, x, out, noise, B, HW, m, dt, s_up);
    } else
        hipLaunchKernelGGL((guide_scalar_kernel<EULER, RESCALED>), dim3(nblk((long)B * C * HW)), dim3(256), 0, st, eps, (long)ld, x, out, noise, B, C, HW, m, dt, s_up);
    return mlsd_check_launch(what);
}

// every mix entry: the refusals, then the launch; `what` is the entry that was called
template <bool EULER>
int guide(const char* what, const float* eps, int64_t ld, const float* x, float* out, const float* noise, int B, int C, int HW, const Guide& m, float dt, float s_up,
          void* stream)
{
    if ((!x && (EULER || m.vparam)) || !out) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (gr_check(what, eps, ld, B, C, HW, m.cfg, m.pag)) return -1;
    return m.factor ? guide_launch<EULER, true>(what, eps, ld, x, out, noise, B, C, HW, m, dt, s_up, (hipStream_t)stream)
                    : guide_launch<EULER, false>(what, eps, ld, x, out, noise, B, C, HW, m, dt, s_up, (hipStream_t)stream);
}

int no_factor(const char* what) { return mlsd_set_error(-1, "%s: NULL factor", what); }

}  // namespace

extern "C" {

MLSD_API int mlsd_guidance_blocks(int HW) { return HW < 1 ? -1 : gr_blocks(HW); }

MLSD_API size_t mlsd_guidance_scratch_bytes(int B, int HW) { return (B < 1 || HW < 1) ? 0 : (size_t)B * gr_blocks(HW) * 4 * sizeof(double); }

MLSD_API int mlsd_guidance_stats(const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, float phi, double* scratch, size_t scratch_bytes,
                                 float* factor, void* stream)
{
    const char* what = "mlsd_guidance_stats";
    if (!scratch || !factor) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (gr_check(what, eps, ld, B, C, HW, cfg, pag)) return -1;
    if (!(phi >= 0.0f && phi <= 1.0f)) return mlsd_set_error(-1, "%s: phi %g (0 .. 1)", what, (double)phi);
    if (scratch_bytes < mlsd_guidance_scratch_bytes(B, HW) || ((uintptr_t)scratch & 7))
        return mlsd_set_error(-1, "%s: scratch of %zu bytes, %zu needed (8-byte aligned)", what, scratch_bytes, mlsd_guidance_scratch_bytes(B, HW));
    hipStream_t st = (hipStream_t)stream;
    const int nb = gr_blocks(HW), identity = !(cfg > 1.0f) && pag == 0.0f;
    if (!identity) {
        if (C == 4 && !(ld & 3) && al16(eps))
            hipLaunchKernelGGL((gr_stats_kernel<true>), dim3(nb, B), dim3(256), 0, st, eps, (long)ld, B, C, HW, cfg, pag, scratch);
        else
            hipLaunchKernelGGL((gr_stats_kernel<false>), dim3(nb, B), dim3(256), 0, st, eps, (long)ld, B, C, HW, cfg, pag, scratch);
        if (mlsd_check_launch(what)) return -1;
    }
    hipLaunchKernelGGL(gr_factor_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, nb, B, (double)C * HW, phi, identity, factor);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_dxdt_guided(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag, const float* factor,
                              int vparam, float c_out, float c_skip, void* stream)
{
    return guide<false>("mlsd_dxdt_guided", eps, ld, x_eval, dx, nullptr, B, C, HW, Guide{ cfg, pag, c_out, c_skip, vparam, factor }, 0.f, 0.f, stream);
}

MLSD_API int mlsd_euler_guided_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, const float* factor, float dt,
                                      const float* noise, float s_up, void* stream)
{
    return guide<true>("mlsd_euler_guided_update", eps, ld, x, x, noise, B, C, HW, Guide{ cfg, pag, 1.f, 0.f, 0, factor }, dt, s_up, stream);
}

// the narrow names: each fixes arguments of the general entry and keeps its own name in the error texts
MLSD_API int mlsd_dxdt_cfg(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, int vparam, float c_out, float c_skip,
                           void* stream)
{
    return guide<false>("mlsd_dxdt_cfg", eps, ld, x_eval, dx, nullptr, B, C, HW, Guide{ cfg, 0.f, c_out, c_skip, vparam, nullptr }, 0.f, 0.f, stream);
}

MLSD_API int mlsd_euler_cfg_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float dt, const float* noise, float s_up, void* stream)
{
    return guide<true>("mlsd_euler_cfg_update", eps, ld, x, x, noise, B, C, HW, Guide{ cfg, 0.f, 1.f, 0.f, 0, nullptr }, dt, s_up, stream);
}

MLSD_API int mlsd_dxdt_pag(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag, int vparam, float c_out,
                           float c_skip, void* stream)
{
    return guide<false>("mlsd_dxdt_pag", eps, ld, x_eval, dx, nullptr, B, C, HW, Guide{ cfg, pag, c_out, c_skip, vparam, nullptr }, 0.f, 0.f, stream);
}

MLSD_API int mlsd_euler_pag_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, float dt, const float* noise, float s_up,
                                   void* stream)
{
    return guide<true>("mlsd_euler_pag_update", eps, ld, x, x, noise, B, C, HW, Guide{ cfg, pag, 1.f, 0.f, 0, nullptr }, dt, s_up, stream);
}

MLSD_API int mlsd_dxdt_rescaled(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag, const float* factor,
                                int vparam, float c_out, float c_skip, void* stream)
{
    const char* what = "mlsd_dxdt_rescaled";
    return factor ? guide<false>(what, eps, ld, x_eval, dx, nullptr, B, C, HW, Guide{ cfg, pag, c_out, c_skip, vparam, factor }, 0.f, 0.f, stream) : no_factor(what);
}

MLSD_API int mlsd_euler_rescaled_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, const float* factor, float dt,
                                        const float* noise, float s_up, void* stream)
{
    const char* what = "mlsd_euler_rescaled_update";
    return factor ? guide<true>(what, eps, ld, x, x, noise, B, C, HW, Guide{ cfg, pag, 1.f, 0.f, 0, factor }, dt, s_up, stream) : no_factor(what);
}

}  // extern "C"
