// Guidance limiters for high cfg_scale: dynamic thresholding (the "CFG scale fix" extension's default path as recalled: per channel, "AD" measure, "MEAN" start point,
// constant scales, interpolation 1) and APG ("Eliminating Oversaturation and Artifacts of High Guidance Scales", 2024, without its momentum buffer).  Neither is in the
// reference; both are parity-unpinned.  The rules are stated in full in include/mlsd_kernels.h.
//
// eps is the raw UNet output, NHWC [N][HW][ld] with the groups [cond B | uncond B | perturbed B (only read at pag != 0)], as in guidance.hip; dx and x are NCHW
// [B][C][HW].  Every float operation of the mix is an explicit _rn intrinsic, rounded once: the bits do not depend on the kernel form.
//
// What is new here is SELECTION.  Thresholding needs, per (image, channel) plane, the p-quantile of a = |g - mean| over the plane's HW values: an exact order
// statistic, on the device, without a sort.  One workgroup of 1024 lanes owns a plane:
//   gather:  the plane's channel is read ONCE from the 16-byte pixel rows, a is formed, and its bit pattern goes to LDS (non-negative floats order as uint32);
//            the maxima of the cfg and of the mimic plane fall out of the same loop (lane, wave shuffle, one integer LDS atomic per wave)
//   select:  MSB-first radix select, four passes of 8 bits.  Per pass the candidates (keys whose bits above the pass equal the prefix found so far) are counted
//            into a 256-bin LDS histogram with integer atomics -- counts are exact, so every run gives the same bits -- and beside each count the bin's smallest key
//            is kept (integer atomicMin).  A lane combines a run of equal digits before it touches LDS: in the first pass nearly all keys of a plane share two or
//            three exponent bins, and one atomic per element would serialise on them.  Four waves scan the 256 counts (shuffle scan, wave totals through LDS); the
//            lane whose bin holds rank lo publishes the digit and the rank inside the bin.
//   rank hi = lo + 1 rides along: while it lies in lo's bin nothing is to do; in the pass where it does not, it is the smallest key of the bins above, which the
//            minima give without another pass over the data.  After four passes the prefix IS a_(lo), and a_(hi) is that same value (a tie) or the minimum found.
// Planes of more than mlsd_guidance_select_lds_limit() bytes do not fit LDS: the same kernel re-forms the keys from global memory in every pass.
//
// The sums (plane means, APG's three dot products) have the shape of guidance.hip's statistics: double accumulation per lane, a shuffle tree, waves through LDS in
// wave order, one ordinary store per block, a second launch that adds the partials in block order.  No global atomics, no block waits on another.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_LDS_BYTES = 128 * 1024;      // keys of one plane: HW <= 32768 (an SDXL 1024 x 1024 latent is 16384); gfx950 has 160 KiB per workgroup, 3 KiB are the bins'
int g_sel_lds_limit = SEL_LDS_BYTES;           // mlsd_guidance_select_lds_limit

inline bool al16(const void* p) { return !((uintptr_t)p & 15); }

__device__ __forceinline__ float cfg_mix(float c, float u, float s) { return __fadd_rn(__fmul_rn(c, s), __fmul_rn(u, 1.0f - s)); }

// ------------------------------------------------------------------ sums
// lanes (shuffle tree), waves (LDS, wave order), then thread 0 stores the block's N doubles to dst
template <int N>
__device__ __forceinline__ void block_sum_store(double (&s)[N], double* dst)
{
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[k] += __shfl_down(s[k], o, 64);
    __shared__ double sh[4][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) sh[wave][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) dst[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
}

// plane sums of g_cfg and g_mim.  VEC4 (C == 4, ld % 4 == 0, eps 16-byte aligned): grid (blocks, B), a block sums all four channels of its pixel run from one 16-byte
// load per group row.  Else: grid (blocks, B * C), a block sums one channel.  part[b][block][C][2]
template <bool VEC4>
__global__ __launch_bounds__(256) void plane_sums_kernel(const float* __restrict__ eps, long ld, int B, int C, int HW, float cfg, float mimic, double* __restrict__ part)
{
    const int nb = gridDim.x, b = VEC4 ? blockIdx.y : blockIdx.y / C, ch = VEC4 ? 0 : blockIdx.y % C;
    const int chunk = (HW + nb - 1) / nb, p0 = blockIdx.x * chunk, p1 = p0 + chunk < HW ? p0 + chunk : HW;
    const float* rc = eps + (long)b * HW * ld;
    const float* ru = eps + (long)(b + B) * HW * ld;
    double* dst = part + (((long)b * nb + blockIdx.x) * C + ch) * 2;
    if constexpr (VEC4) {
        double s[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
        for (int pix = p0 + (int)threadIdx.x; pix < p1; pix += 256) {
            const float4 c = *reinterpret_cast<const float4*>(rc + (long)pix * ld), u = *reinterpret_cast<const float4*>(ru + (long)pix * ld);
            s[0] += (double)cfg_mix(c.x, u.x, cfg); s[1] += (double)cfg_mix(c.x, u.x, mimic);
            s[2] += (double)cfg_mix(c.y, u.y, cfg); s[3] += (double)cfg_mix(c.y, u.y, mimic);
            s[4] += (double)cfg_mix(c.z, u.z, cfg); s[5] += (double)cfg_mix(c.z, u.z, mimic);
            s[6] += (double)cfg_mix(c.w, u.w, cfg); s[7] += (double)cfg_mix(c.w, u.w, mimic);
        }
        block_sum_store<8>(s, dst);
    } else {
        double s[2] = { 0.0, 0.0 };
        for (int pix = p0 + (int)threadIdx.x; pix < p1; pix += 256) {
            const float c = rc[(long)pix * ld + ch], u = ru[(long)pix * ld + ch];
            s[0] += (double)cfg_mix(c, u, cfg); s[1] += (double)cfg_mix(c, u, mimic);
        }
        block_sum_store<2>(s, dst);
    }
}

// means[b][ch][2]: thread per value, the partials added in block order, divided by HW, rounded once
__global__ void plane_means_kernel(const double* __restrict__ part, int nb, int B, int C, int HW, float* __restrict__ means)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * C * 2) return;
    const int b = i / (2 * C), r = i % (2 * C);
    double s = 0.0;
    for (int j = 0; j < nb; ++j) s += part[((long)b * nb + j) * 2 * C + r];
    means[i] = (float)(s / (double)HW);
}

// APG: per image, S_dd, S_dc, S_cc over its C * HW raw elements, d = c - u formed in double.  grid (blocks, B); part[b][block][3]
template <bool VEC4>
__global__ __launch_bounds__(256) void apg_sums_kernel(const float* __restrict__ eps, long ld, int B, int C, int HW, double* __restrict__ part)
{
    const int nb = gridDim.x, b = blockIdx.y;
    const int chunk = (HW + nb - 1) / nb, p0 = blockIdx.x * chunk, p1 = p0 + chunk < HW ? p0 + chunk : HW;
    const float* rc = eps + (long)b * HW * ld;
    const float* ru = eps + (long)(b + B) * HW * ld;
    double s[3] = { 0.0, 0.0, 0.0 };
    const auto acc = [&](float cf, float uf) { const double c = (double)cf, d = c - (double)uf; s[0] += d * d; s[1] += d * c; s[2] += c * c; };
    for (int pix = p0 + (int)threadIdx.x; pix < p1; pix += 256) {
        if constexpr (VEC4) {
            const float4 c = *reinterpret_cast<const float4*>(rc + (long)pix * ld), u = *reinterpret_cast<const float4*>(ru + (long)pix * ld);
            acc(c.x, u.x); acc(c.y, u.y); acc(c.z, u.z); acc(c.w, u.w);
        } else {
            for (int k = 0; k < C; ++k) acc(rc[(long)pix * ld + k], ru[(long)pix * ld + k]);
        }
    }
    block_sum_store<3>(s, part + ((long)b * nb + blockIdx.x) * 3);
}

// coef[b] = (A_b, B_b): thread per image
__global__ void apg_coef_kernel(const double* __restrict__ part, int nb, int B, float cfg, float eta, float norm, float* __restrict__ coef)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s[3] = { 0.0, 0.0, 0.0 };
    for (int j = 0; j < nb; ++j)
        for (int k = 0; k < 3; ++k) s[k] += part[((long)b * nb + j) * 3 + k];
    float A = cfg, Bc = 1.0f - cfg;                           // a sum that is not finite: the plain mix
    if (isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2])) {
        double sc = 1.0;
        if (norm > 0.0f) { sc = (double)norm / sqrt(s[0]); if (sc > 1.0) sc = 1.0; }
        const double alpha = s[2] > 0.0 ? s[1] / s[2] : 0.0, w = ((double)cfg - 1.0) * sc;
        A = (float)(1.0 + w * (1.0 - (1.0 - (double)eta) * alpha));
        Bc = (float)(-w);
    }
    coef[2 * b] = A; coef[2 * b + 1] = Bc;
}

// ------------------------------------------------------------------ selection
// one workgroup per plane (blockIdx.x = b * C + ch).  lo, hi, frac: the position p (HW - 1) split on the host, in double; want_q 0 (p == 1): the quantile is the
// maximum and no pass runs.  IN_LDS: the keys live in dynamic LDS (HW * 4 bytes); else every pass forms them again from eps.
template <bool IN_LDS>
__global__ __launch_bounds__(SEL_THREADS) void plane_select_kernel(const float* __restrict__ eps, long ld, int B, int C, int HW, float cfg, float mimic, int lo, int hi,
                                                                   double frac, int want_q, const float* __restrict__ means, float* __restrict__ triple)
{
    extern __shared__ uint32_t keys[];
    __shared__ uint32_t hist[256], minkey[256], s_wave[4], s_max[2], s_digit, s_rank, s_same, s_next;
    const int plane = blockIdx.x, b = plane / C, ch = plane % C, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float mean_cfg = means[2 * plane], mean_mim = means[2 * plane + 1];
    const float* rc = eps + (long)b * HW * ld + ch;
    const float* ru = eps + (long)(b + B) * HW * ld + ch;
    const auto key_at = [&](int i) -> uint32_t {
        if constexpr (IN_LDS) return keys[i];
        else return __float_as_uint(fabsf(__fsub_rn(cfg_mix(rc[(long)i * ld], ru[(long)i * ld], cfg), mean_cfg)));
    };

    // ---- gather: keys to LDS, the two maxima
    if (tid < 2) s_max[tid] = 0u;
    __syncthreads();
    uint32_t mx_cfg = 0u, mx_mim = 0u;
    for (int i = tid; i < HW; i += SEL_THREADS) {
        const float c = rc[(long)i * ld], u = ru[(long)i * ld];
        const uint32_t kc = __float_as_uint(fabsf(__fsub_rn(cfg_mix(c, u, cfg), mean_cfg)));
        const uint32_t km = __float_as_uint(fabsf(__fsub_rn(cfg_mix(c, u, mimic), mean_mim)));
        if constexpr (IN_LDS) keys[i] = kc;
        mx_cfg = kc > mx_cfg ? kc : mx_cfg; mx_mim = km > mx_mim ? km : mx_mim;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t a = __shfl_xor(mx_cfg, o, 64), m = __shfl_xor(mx_mim, o, 64);
        mx_cfg = a > mx_cfg ? a : mx_cfg; mx_mim = m > mx_mim ? m : mx_mim;
    }
    if (lane == 0) { atomicMax(&s_max[0], mx_cfg); atomicMax(&s_max[1], mx_mim); }
    __syncthreads();

    // ---- select: prefix / mask / rank are the same in every lane (they are read back from LDS after each pass)
    uint32_t prefix = 0u, mask = 0u, rank = (uint32_t)lo, hi_val = 0u;
    bool hi_found = hi == lo;                                  // (then a_(hi) is a_(lo))
    if (want_q) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) { hist[tid] = 0u; minkey[tid] = 0xFFFFFFFFu; }
            if (tid == 0) s_next = 0xFFFFFFFFu;
            __syncthreads();
            int cur = -1;
            uint32_t cnt = 0u, mn = 0xFFFFFFFFu;
            for (int i = tid; i < HW; i += SEL_THREADS) {
                const uint32_t key = key_at(i);
                if ((key & mask) != prefix) continue;
                const int dgt = (int)((key >> shift) & 255u);
                if (dgt != cur) {
                    if (cnt) { atomicAdd(&hist[cur], cnt); atomicMin(&minkey[cur], mn); }
                    cur = dgt; cnt = 0u; mn = 0xFFFFFFFFu;
                }
                ++cnt; mn = key < mn ? key : mn;
            }
            if (cnt) { atomicAdd(&hist[cur], cnt); atomicMin(&minkey[cur], mn); }
            __syncthreads();
            uint32_t incl = 0u, own = 0u;
            if (tid < 256) {
                own = hist[tid]; incl = own;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                if (lane == 63) s_wave[wave] = incl;
            }
            __syncthreads();
            if (tid < 256) {
                for (int w = 0; w < wave; ++w) incl += s_wave[w];
                const uint32_t excl = incl - own;
                if (excl <= rank && rank < incl) { s_digit = (uint32_t)tid; s_rank = rank - excl; s_same = rank + 1u < incl; }
            }
            __syncthreads();
            const uint32_t digit = s_digit;
            if (!hi_found && !s_same) {                           // rank hi leaves lo's bin here: the smallest key of the bins above
                if (tid < 256 && (uint32_t)tid > digit && hist[tid]) atomicMin(&s_next, minkey[tid]);
                __syncthreads();
                hi_val = s_next; hi_found = true;
            }
            rank = s_rank; prefix |= digit << shift; mask |= 255u << shift;
            __syncthreads();                                      // (the bins are cleared next)
        }
    }
    if (tid != 0) return;
    const float m_ref = __uint_as_float(s_max[1]);
    float q_ref = __uint_as_float(s_max[0]);
    if (want_q) {
        const double a_lo = (double)__uint_as_float(prefix), a_hi = (double)__uint_as_float((hi == lo || !hi_found) ? prefix : hi_val);
        q_ref = (float)(a_lo + frac * (a_hi - a_lo));
    }
    const float t = m_ref > q_ref ? m_ref : q_ref;
    const bool ident = HW == 1 || !isfinite(m_ref) || !isfinite(q_ref) || t == 0.0f;
    triple[3 * plane] = mean_cfg;
    triple[3 * plane + 1] = ident ? INFINITY : t;
    triple[3 * plane + 2] = ident ? 1.0f : (float)((double)m_ref / (double)t);
}

// ------------------------------------------------------------------ the limited mix
struct Limit { float cfg, pag, c_out, c_skip; int vparam, mode; const float* lim; };      // lim: mode 1 triples [B][C][3], mode 2 coefficients [B][2]

// l0, l1, l2: mode 1 the plane's mean, t, r; mode 2 the image's A, B (l2 unused)
__device__ __forceinline__ float limited(float c, float u, float p, float xv, float l0, float l1, float l2, const Limit& m)
{
    float g;
    if (m.mode == 1) g = __fadd_rn(__fmul_rn(fminf(fmaxf(__fsub_rn(cfg_mix(c, u, m.cfg), l0), -l1), l1), l2), l0);
    else g = __fadd_rn(__fmul_rn(c, l0), __fmul_rn(u, l1));
    if (m.pag != 0.0f) g = __fadd_rn(g, __fmul_rn(m.pag, __fsub_rn(c, p)));
    return m.vparam ? __fadd_rn(__fmul_rn(g, m.c_out), __fmul_rn(xv, m.c_skip)) : g;
}

// element per thread: any C, any ld >= C
__global__ void limited_scalar_kernel(const float* __restrict__ eps, long ld, const float* __restrict__ x, float* __restrict__ out, int B, int C, int HW, Limit m)
{
    const long total = (long)B * C * HW;
    GRID_LOOP(i, total) {
        const int pix = (int)(i % HW);
        const long t = i / HW;
        const int c = (int)(t % C), b = (int)(t / C);
        const float ec = eps[((long)b * HW + pix) * ld + c], eu = eps[((long)(b + B) * HW + pix) * ld + c];
        const float ep = m.pag != 0.0f ? eps[((long)(b + 2 * B) * HW + pix) * ld + c] : 0.f;
        const float* l = m.mode == 1 ? m.lim + ((long)b * C + c) * 3 : m.lim + 2 * b;
        out[i] = limited(ec, eu, ep, m.vparam ? x[i] : 0.f, l[0], l[1], m.mode == 1 ? l[2] : 0.f, m);
    }
}

// C == 4, rows of whole 16-byte pieces: a thread owns PX consecutive pixels of one image (PX 4 needs HW % 4 == 0 and 16-byte aligned planes)
template <int PX>
__global__ void limited_pixel_kernel(const float* __restrict__ eps, long ld, const float* __restrict__ x, float* __restrict__ out, int B, int HW, Limit m)
{
    const long per = HW / PX, total = (long)B * per;
    GRID_LOOP(i, total) {
        const int b = (int)(i / per);
        const long pix0 = (i - (long)b * per) * PX;
        float l[4][3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (m.mode == 1) { l[c][0] = m.lim[(b * 4 + c) * 3]; l[c][1] = m.lim[(b * 4 + c) * 3 + 1]; l[c][2] = m.lim[(b * 4 + c) * 3 + 2]; }
            else { l[c][0] = m.lim[2 * b]; l[c][1] = m.lim[2 * b + 1]; l[c][2] = 0.f; }
        }
        float v[4][PX], xv[4][PX];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long o = ((long)b * 4 + c) * HW + pix0;
            if constexpr (PX == 4) {
                const float4 a = m.vparam ? *reinterpret_cast<const float4*>(x + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                xv[c][0] = a.x; xv[c][1] = a.y; xv[c][2] = a.z; xv[c][3] = a.w;
            } else xv[c][0] = m.vparam ? x[o] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const float4 ec = *reinterpret_cast<const float4*>(eps + ((long)b * HW + pix0 + k) * ld);
            const float4 eu = *reinterpret_cast<const float4*>(eps + ((long)(b + B) * HW + pix0 + k) * ld);
            const float4 ep = m.pag != 0.0f ? *reinterpret_cast<const float4*>(eps + ((long)(b + 2 * B) * HW + pix0 + k) * ld) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0][k] = limited(ec.x, eu.x, ep.x, xv[0][k], l[0][0], l[0][1], l[0][2], m); v[1][k] = limited(ec.y, eu.y, ep.y, xv[1][k], l[1][0], l[1][1], l[1][2], m);
            v[2][k] = limited(ec.z, eu.z, ep.z, xv[2][k], l[2][0], l[2][1], l[2][2], m); v[3][k] = limited(ec.w, eu.w, ep.w, xv[3][k], l[3][0], l[3][1], l[3][2], m);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const long o = ((long)b * 4 + c) * HW + pix0;
            if constexpr (PX == 4) *reinterpret_cast<float4*>(out + o) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
            else out[o] = v[c][0];
        }
    }
}

// ------------------------------------------------------------------ launching
// the statistics read the uncond group: it exists only at cfg > 1
int stats_check(const char* what, const float* eps, int64_t ld, int B, int C, int HW, float cfg)
{
    if (guidance_args_check(what, eps, ld, B, C, HW, cfg, 0.0f)) return -1;
    if (!(cfg > 1.0f)) return mlsd_set_error(-1, "%s: cfg %g (the statistics read the uncond rows: cfg > 1)", what, (double)cfg);
    return 0;
}

int scratch_check(const char* what, const void* scratch, size_t bytes, int B, int C, int HW)
{
    const size_t need = mlsd_guidance_limit_scratch_bytes(B, C, HW);
    if (!scratch || bytes < need || ((uintptr_t)scratch & 7)) return mlsd_set_error(-1, "%s: scratch of %zu bytes, %zu needed (8-byte aligned)", what, scratch ? bytes : 0, need);
    return 0;
}

bool mimic_ok(float mimic) { return mimic >= 1.0f && mimic < INFINITY; }

}  // namespace

extern "C" {

MLSD_API int mlsd_guidance_select_lds_limit(int bytes)
{
    const int was = g_sel_lds_limit;
    if (bytes >= 0) g_sel_lds_limit = bytes < SEL_LDS_BYTES ? bytes : SEL_LDS_BYTES;
    return was;
}

MLSD_API size_t mlsd_guidance_limit_scratch_bytes(int B, int C, int HW)
{
    if (B < 1 || C < 1 || HW < 1) return 0;
    return (size_t)B * mlsd_guidance_blocks(HW) * (2 * C > 3 ? 2 * C : 3) * sizeof(double);
}

MLSD_API int mlsd_guidance_plane_means(const float* eps, int64_t ld, int B, int C, int HW, float cfg, float mimic, double* scratch, size_t scratch_bytes, float* means,
                                       void* stream)
{
    const char* what = "mlsd_guidance_plane_means";
    if (!means) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (stats_check(what, eps, ld, B, C, HW, cfg)) return -1;
    if (!mimic_ok(mimic)) return mlsd_set_error(-1, "%s: mimic %g (>= 1)", what, (double)mimic);
    if (scratch_check(what, scratch, scratch_bytes, B, C, HW)) return -1;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    const int nb = mlsd_guidance_blocks(HW);
    if (C == 4 && !(ld & 3) && al16(eps)) hipLaunchKernelGGL((plane_sums_kernel<true>), dim3(nb, B), dim3(256), 0, st, eps, (long)ld, B, C, HW, cfg, mimic, scratch);
    else hipLaunchKernelGGL((plane_sums_kernel<false>), dim3(nb, B * C), dim3(256), 0, st, eps, (long)ld, B, C, HW, cfg, mimic, scratch);
    if (mlsd_check_launch(what)) return -1;
    hipLaunchKernelGGL(plane_means_kernel, dim3((B * C * 2 + 63) / 64), dim3(64), 0, st, scratch, nb, B, C, HW, means);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_guidance_plane_select(const float* eps, int64_t ld, int B, int C, int HW, float cfg, float mimic, float p, const float* means, float* triple,
                                        void* stream)
{
    const char* what = "mlsd_guidance_plane_select";
    if (!means || !triple) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (stats_check(what, eps, ld, B, C, HW, cfg)) return -1;
    if (!mimic_ok(mimic)) return mlsd_set_error(-1, "%s: mimic %g (>= 1)", what, (double)mimic);
    if (!(p >= 0.5f && p <= 1.0f)) return mlsd_set_error(-1, "%s: percentile %g (0.5 .. 1)", what, (double)p);
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    const double pos = (double)p * (double)(HW - 1);
    const int lo = (int)floor(pos), hi = lo + 1 < HW - 1 ? lo + 1 : HW - 1, want_q = p < 1.0f;
    const double frac = pos - (double)lo;
    const size_t lds = (size_t)HW * 4;
    if (lds <= (size_t)g_sel_lds_limit) {
        static bool lds_set[64];      // per device: the attribute belongs to the device's copy of the kernel, and a multi-GPU split runs engines on several
                                      // (written without a lock: two host threads racing here set the same attribute twice at worst)
        int dev = 0;
        MLSD_HIP_TRY(hipGetDevice(&dev));
        if (dev < 0 || dev >= 64 || !lds_set[dev]) {
            MLSD_HIP_TRY(hipFuncSetAttribute((const void*)plane_select_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SEL_LDS_BYTES));
            if (dev >= 0 && dev < 64) lds_set[dev] = true;
        }
        hipLaunchKernelGGL((plane_select_kernel<true>), dim3(B * C), dim3(SEL_THREADS), lds, st, eps, (long)ld, B, C, HW, cfg, mimic, lo, hi, frac, want_q, means, triple);
    } else
        hipLaunchKernelGGL((plane_select_kernel<false>), dim3(B * C), dim3(SEL_THREADS), 0, st, eps, (long)ld, B, C, HW, cfg, mimic, lo, hi, frac, want_q, means, triple);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_guidance_apg_coef(const float* eps, int64_t ld, int B, int C, int HW, float cfg, float eta, float norm, double* scratch, size_t scratch_bytes, float* coef,
                                    void* stream)
{
    const char* what = "mlsd_guidance_apg_coef";
    if (!coef) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (stats_check(what, eps, ld, B, C, HW, cfg)) return -1;
    if (!(eta >= 0.0f && eta <= 1.0f) || !(norm >= 0.0f && norm < INFINITY)) return mlsd_set_error(-1, "%s: eta %g (0 .. 1), norm %g (>= 0)", what, (double)eta, (double)norm);
    if (scratch_check(what, scratch, scratch_bytes, B, C, HW)) return -1;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    const int nb = mlsd_guidance_blocks(HW);
    if (C == 4 && !(ld & 3) && al16(eps)) hipLaunchKernelGGL((apg_sums_kernel<true>), dim3(nb, B), dim3(256), 0, st, eps, (long)ld, B, C, HW, scratch);
    else hipLaunchKernelGGL((apg_sums_kernel<false>), dim3(nb, B), dim3(256), 0, st, eps, (long)ld, B, C, HW, scratch);
    if (mlsd_check_launch(what)) return -1;
    hipLaunchKernelGGL(apg_coef_kernel, dim3((B + 63) / 64), dim3(64), 0, st, scratch, nb, B, cfg, eta, norm, coef);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_dxdt_limited(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, int mode, float cfg, float pag, const float* lim,
                               int vparam, float c_out, float c_skip, void* stream)
{
    const char* what = "mlsd_dxdt_limited";
    if (mode != MLSD_GLIMIT_DYNTHRESH && mode != MLSD_GLIMIT_APG) return mlsd_set_error(-1, "%s: mode %d (1 thresholding, 2 APG)", what, mode);
    if ((!x_eval && vparam) || !dx) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (guidance_args_check(what, eps, ld, B, C, HW, cfg, pag)) return -1;      // what mlsd_dxdt_guided refuses
    // cfg <= 1: the guided prediction is the cond prediction, there is nothing to limit and no uncond group to read: the plain mix, its bytes
    if (!(cfg > 1.0f)) return mlsd_dxdt_guided(eps, ld, x_eval, dx, B, C, HW, cfg, pag, nullptr, vparam, c_out, c_skip, stream);
    if (!lim) return mlsd_set_error(-1, "%s: NULL %s", what, mode == MLSD_GLIMIT_APG ? "coefficients" : "triples");
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    hipStream_t st = (hipStream_t)stream;
    const Limit m{ cfg, pag, c_out, c_skip, vparam, mode, lim };
    if (C == 4 && !(ld & 3) && al16(eps)) {
        if (!(HW & 3) && al16(x_eval) && al16(dx)) hipLaunchKernelGGL((limited_pixel_kernel<4>), dim3(nblk((long)B * (HW / 4))), dim3(256), 0, st, eps, (long)ld, x_eval, dx, B, HW, m);
        else hipLaunchKernelGGL((limited_pixel_kernel<1>), dim3(nblk((long)B * HW)), dim3(256), 0, st, eps, (long)ld, x_eval, dx, B, HW, m);
    } else
        hipLaunchKernelGGL(limited_scalar_kernel, dim3(nblk((long)B * C * HW)), dim3(256), 0, st, eps, (long)ld, x_eval, dx, B, C, HW, m);
    return mlsd_check_launch(what);
}

}  // extern "C"
