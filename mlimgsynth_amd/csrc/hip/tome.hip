// Token merging (ToMe, "Token Merging for Fast Stable Diffusion", 2023) for the UNet's self-attention: the rule AS RECALLED, with the random destination choice
// fixed to the cell's corner (0, 0); not in the reference, parity-unpinned.  The rule is stated in full in include/mlsd_kernels.h; the plan's users are the four
// copy-kind ops mlb_basic_transf records on a merged level (host/mlblock_nn.c).
//
// match   the new design: cosine similarity of every source row against every destination row, reduced on the fly to (row maximum, its index).  No score matrix
//         exists anywhere: per image Ns ints and Ns floats go to global memory.
//           work split   grid (ceil(Ns / 128), n_img), 4 waves.  A workgroup owns 128 source rows, a wave 32 of them: two 16-row B operands of
//                        mfma_f32_16x16x32_f16, so that an accumulator lane holds four destinations of ONE source row and the running (maximum, index) is lane-local.
//           sources      gathered by the partition rule (src_token) and RE-READ FROM L2 per destination tile, 16 bytes per lane straight from the token rows into the
//                        B operand (lane (l15, lg) reads halfs 32 ks + 8 lg .. + 7 of row l15): a block of 128 rows x 1280 halfs is 320 KiB, it fits neither LDS
//                        beside a destination tile nor the registers (40 k-steps x 2 operands x 4 VGPRs = 320 per lane); its second and later reads hit L2, where the
//                        whole map of one image lives (<= 20 MiB at 128 x 128 x 640).  Their inverse norms are formed once, in the same lane layout.
//           destinations walked in tiles of 32 rows staged in LDS at a row stride of C + 8 halfs (an odd number of 16-byte units: the sixteen rows an A operand
//                        read touches fall on distinct bank groups); rows past Nd are zeros and never enter the maximum.  Eight lanes stage one row and sum its
//                        squares on the way; the tile's 32 inverse norms sit behind the rows.
//           budget       LDS 32 (2 C + 16) + 128 bytes: 20.6 KiB at C = 320, 41.1 KiB at 640, 80.6 KiB at 1280 (one workgroup per CU there, three at 640);
//                        registers: 16 accumulators, 4 operand quads, the two running pairs -- under 64 VGPRs, occupancy is set by LDS.
//           ending       per source row the four lanes (lg) that hold it combine by two shuffles, larger score first, lower index on equal scores; lane lg 0
//                        stores best and score once.
// select  one workgroup of 1024 lanes per image: the r-th largest key by an MSB-first radix select (four passes of 8 bits over a 256-bin LDS histogram, integer
//         atomics: exact counts, the same bits in every run), ties resolved by source index through an ordered block scan, then slot / kept / off / members by
//         prefix scans and a stable counting placement (a lane's rank among the equal destinations of its chunk is counted, not raced for).  Keys of more than
//         mlsd_tome_select_lds_limit() bytes are re-formed from global memory in every pass.
// merge   one wave per row of the merged set: a kept source is a row copy, a destination the fp32 sum (itself, then its members in list order) divided by the count,
//         rounded to fp16 once; 16 bytes per lane.
// unmerge y[t] = x[t] + o[slot[t]] in fp32, 16 bytes per lane.
// No floating-point atomics anywhere; all row offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "common.hpp"
#include "mlsd_kernels.h"

namespace {

// ------------------------------------------------------------------ the partition (rule 1)
// Hh, Wh: cells per axis; E: sources of an even row (odd x below 2 Wh, then the leftover column); P: sources of a row pair
struct Geom { int H, W, Hh, Wh, T, Nd, Ns, E, P; };

inline Geom geom_of(int H, int W)
{
    Geom g; g.H = H; g.W = W; g.Hh = H / 2; g.Wh = W / 2; g.T = H * W; g.Nd = g.Hh * g.Wh; g.Ns = g.T - g.Nd; g.E = W - g.Wh; g.P = W + g.E;
    return g;
}
__device__ __forceinline__ int src_token(const Geom& g, int i)
{
    const int pair = i / g.P, rem = i - pair * g.P;
    if (pair >= g.Hh) return 2 * g.Hh * g.W + rem;                                  // the leftover row of an odd map
    if (rem < g.E) return 2 * pair * g.W + (rem < g.Wh ? 2 * rem + 1 : g.Wh + rem);  // (2 Wh + rem - Wh)
    return (2 * pair + 1) * g.W + rem - g.E;
}
__device__ __forceinline__ int dst_token(const Geom& g, int j) { const int cy = j / g.Wh; return 2 * cy * g.W + 2 * (j - cy * g.Wh); }

__device__ __forceinline__ int ld_l2(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }   // (a word other lanes wrote, or counted with atomics)

// ------------------------------------------------------------------ match
constexpr int MT_WAVES = 4, MT_SRC = 32 * MT_WAVES, MT_DT = 32;
constexpr int MT_LDS_MAX = MT_DT * (2 * 1280 + 16) + MT_DT * 4;

__device__ __forceinline__ float sumsq8(const f16x8 v, float q)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) q += (float)v[e] * (float)v[e];
    return q;
}
__device__ __forceinline__ float inv_norm(float q) { return q > 0.0f ? 1.0f / sqrtf(q) : 0.0f; }

__global__ __launch_bounds__(64 * MT_WAVES) void match_kernel(const _Float16* __restrict__ n, long ld, Geom g, int C, int* __restrict__ best, float* __restrict__ score)
{
    extern __shared__ unsigned char tile[];
    const int RS = 2 * C + 16, KS = C / 32, pieces = C / 8;
    float* inv_d = reinterpret_cast<float*>(tile + MT_DT * RS);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4, img = (int)blockIdx.y;
    const _Float16* base = n + (long)img * g.T * ld;
    const int s0 = (int)blockIdx.x * MT_SRC + wave * 32;

    const _Float16* sp[2]; bool sv[2]; float inv_s[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        const int i = s0 + 16 * f + l15;
        sv[f] = i < g.Ns;
        sp[f] = base + (long)src_token(g, sv[f] ? i : 0) * ld + 8 * lg;
        float q = 0.0f;
        if (sv[f]) for (int ks = 0; ks < KS; ++ks) q = sumsq8(*reinterpret_cast<const f16x8*>(sp[f] + 32 * ks), q);
        q += __shfl_xor(q, 16, 64); q += __shfl_xor(q, 32, 64);
        inv_s[f] = inv_norm(q);
    }
    float bs[2] = { -INFINITY, -INFINITY };
    int bi[2] = { 0, 0 };
    const int tr = tid >> 3, sub = tid & 7;
    const unsigned char* a0 = tile + l15 * RS + 16 * lg;
    const unsigned char* a1 = a0 + 16 * RS;
    const f16x8 zero8 = { 0, 0, 0, 0, 0, 0, 0, 0 };

    for (int t0 = 0; t0 < g.Nd; t0 += MT_DT) {
        __syncthreads();                                       // the previous tile is consumed
        {
            const int j = t0 + tr;
            const bool dv = j < g.Nd;
            const _Float16* dp = base + (long)dst_token(g, dv ? j : 0) * ld;
            float q = 0.0f;
            for (int p = sub; p < pieces; p += 8) {
                const f16x8 v = dv ? *reinterpret_cast<const f16x8*>(dp + 8 * p) : zero8;
                *reinterpret_cast<f16x8*>(tile + tr * RS + 16 * p) = v;
                q = sumsq8(v, q);
            }
            q += __shfl_xor(q, 1, 64); q += __shfl_xor(q, 2, 64); q += __shfl_xor(q, 4, 64);
            if (sub == 0) inv_d[tr] = inv_norm(q);
        }
        __syncthreads();
        f32x4 acc[2][2];
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int h = 0; h < 2; ++h) acc[f][h] = f32x4{ 0.f, 0.f, 0.f, 0.f };
        for (int ks = 0; ks < KS; ++ks) {
            const f16x8 b0 = sv[0] ? *reinterpret_cast<const f16x8*>(sp[0] + 32 * ks) : zero8;
            const f16x8 b1 = sv[1] ? *reinterpret_cast<const f16x8*>(sp[1] + 32 * ks) : zero8;
            const f16x8 x0 = *reinterpret_cast<const f16x8*>(a0 + 64 * ks), x1 = *reinterpret_cast<const f16x8*>(a1 + 64 * ks);
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x0, b0, acc[0][0], 0, 0, 0);      // destinations t0 + 4 lg + e of source l15
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, b0, acc[0][1], 0, 0, 0);      // destinations t0 + 16 + 4 lg + e
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x0, b1, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, b1, acc[1][1], 0, 0, 0);
        }
#pragma unroll
        for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int e = 0; e < 4; ++e) {                  // ascending j: the strict comparison keeps the lowest index
                    const int jj = 16 * h + 4 * lg + e, j = t0 + jj;
                    const float s = acc[f][h][e] * inv_s[f] * inv_d[jj];
                    if (j < g.Nd && s > bs[f]) { bs[f] = s; bi[f] = j; }
                }
    }
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const float os = __shfl_xor(bs[f], o, 64);
            const int oi = __shfl_xor(bi[f], o, 64);
            if (os > bs[f] || (os == bs[f] && oi < bi[f])) { bs[f] = os; bi[f] = oi; }
        }
        if (lg == 0 && sv[f]) {
            const long o = (long)img * g.Ns + s0 + 16 * f + l15;
            best[o] = bi[f]; score[o] = bs[f];
        }
    }
}

// ------------------------------------------------------------------ select
constexpr int SEL_THREADS = 1024;
constexpr int SEL_LDS_BYTES = 96 * 1024;       // keys of one image: Ns <= 24576 (an SDXL 1024 x 1024 pass has 12288 at its first transformer level)
int g_sel_lds_limit = SEL_LDS_BYTES;           // mlsd_tome_select_lds_limit

// ascending in this key = descending in the score: positive floats by falling bits, then negative floats by rising bits; a NaN is ordered by its bits like any value
__device__ __forceinline__ uint32_t sel_key(float s)
{
    const uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? u : (~u & 0x7FFFFFFFu);
}

// exclusive prefix of v over the block in thread order, *total = the block's sum; s_w: 16 ints
__device__ __forceinline__ int block_scan(int v, int* s_w, int* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    __syncthreads();                                           // (s_w of the previous scan is read)
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) { const int x = s_w[w]; pre += w < wave ? x : 0; tot += x; }
    *total = tot;
    return pre + incl - v;
}

// lists of one image (ints): slot[T] | kept[Ns - r] | off[Nd + 1] | members[r] | cnt[Nd]
template <bool IN_LDS>
__global__ __launch_bounds__(SEL_THREADS) void select_kernel(const float* __restrict__ score, const int* __restrict__ best, Geom g, int r, int* __restrict__ lists, long per_img)
{
    extern __shared__ uint32_t keys[];
    __shared__ uint32_t hist[256], s_digit, s_rank;
    __shared__ int s_w[SEL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) int s_b[SEL_THREADS];
    const int img = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, nk = g.Ns - r;
    const float* sc = score + (long)img * g.Ns;
    const int* be = best + (long)img * g.Ns;
    int* slot = lists + (long)img * per_img;
    int* kept = slot + g.T;
    int* off = kept + nk;
    int* members = off + g.Nd + 1;
    int* cnt = members + r;
    const auto key_at = [&](int i) -> uint32_t { if constexpr (IN_LDS) return keys[i]; else return sel_key(sc[i]); };

    if constexpr (IN_LDS) for (int i = tid; i < g.Ns; i += SEL_THREADS) keys[i] = sel_key(sc[i]);
    for (int j = tid; j < g.Nd; j += SEL_THREADS) { cnt[j] = 0; slot[dst_token(g, j)] = nk + j; }
    __syncthreads();

    // ---- the key of rank r - 1 and how many of its equals are merged
    uint32_t thr = 0u, need = 0u;
    if (r > 0) {
        uint32_t prefix = 0u, mask = 0u, rank = (uint32_t)(r - 1);
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            int cur = -1;
            uint32_t c = 0u;
            for (int i = tid; i < g.Ns; i += SEL_THREADS) {
                const uint32_t key = key_at(i);
                if ((key & mask) != prefix) continue;
                const int dgt = (int)((key >> shift) & 255u);
                if (dgt != cur) { if (c) atomicAdd(&hist[cur], c); cur = dgt; c = 0u; }
                ++c;
            }
            if (c) atomicAdd(&hist[cur], c);
            __syncthreads();
            uint32_t incl = 0u, own = 0u;
            if (tid < 256) {
                own = hist[tid]; incl = own;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
                if (lane == 63) s_w[wave] = (int)incl;
            }
            __syncthreads();
            if (tid < 256) {
                for (int w = 0; w < wave; ++w) incl += (uint32_t)s_w[w];
                const uint32_t excl = incl - own;
                if (excl <= rank && rank < incl) { s_digit = (uint32_t)tid; s_rank = rank - excl; }
            }
            __syncthreads();
            rank = s_rank; prefix |= s_digit << shift; mask |= 255u << shift;
            __syncthreads();
        }
        thr = prefix; need = rank + 1u;
    }

    // ---- in source order: who is merged (ties by index), the kept sources' rows, the destinations' counts
    int c_tie = 0, c_kept = 0;
    for (int c0 = 0; c0 < g.Ns; c0 += SEL_THREADS) {
        const int i = c0 + tid;
        const bool valid = i < g.Ns;
        const uint32_t key = valid ? key_at(i) : 0u;
        const int tie = valid && r > 0 && key == thr;
        int tot;
        const int tie_x = c_tie + block_scan(tie, s_w, &tot);
        c_tie += tot;
        const bool merged = valid && r > 0 && (key < thr || (tie && (uint32_t)tie_x < need));
        const int kp = valid && !merged;
        const int kept_x = c_kept + block_scan(kp, s_w, &tot);
        c_kept += tot;
        if (valid) {
            const int tok = src_token(g, i);
            if (merged) {
                int b = be[i];
                b = b < 0 ? 0 : b >= g.Nd ? g.Nd - 1 : b;      // (a best outside 0 .. Nd - 1 cannot come from match: kept inside the arrays whatever the caller gave)
                slot[tok] = nk + b;
                atomicAdd(&cnt[b], 1);
            } else if (kept_x < nk) { slot[tok] = kept_x; kept[kept_x] = tok; }
        }
    }
    __syncthreads();

    // ---- off = exclusive prefix of the counts; the counts start again as the placement's cursors
    int carry = 0;
    for (int c0 = 0; c0 < g.Nd; c0 += SEL_THREADS) {
        const int j = c0 + tid;
        const int v = j < g.Nd ? ld_l2(cnt + j) : 0;
        int tot;
        const int x = carry + block_scan(v, s_w, &tot);
        carry += tot;
        if (j < g.Nd) { off[j] = x; cnt[j] = 0; }
    }
    if (tid == 0) off[g.Nd] = r;
    __syncthreads();

    // ---- members: the merged sources of every destination in ascending source order.  Chunks of 1024 sources in order; inside a chunk a lane's place is the number
    // of lower lanes with its destination, counted from LDS
    for (int c0 = 0; c0 < g.Ns && r > 0; c0 += SEL_THREADS) {
        const int i = c0 + tid;
        const int tok = i < g.Ns ? src_token(g, i) : 0;
        const int sl = i < g.Ns ? ld_l2(slot + tok) : 0;
        const int b = (i < g.Ns && sl >= nk) ? sl - nk : -1;
        s_b[tid] = b;
        __syncthreads();
        if (b >= 0) {
            int rank = 0, u = 0;
            for (; u + 4 <= tid; u += 4) { const int4 v = *reinterpret_cast<const int4*>(s_b + u); rank += (v.x == b) + (v.y == b) + (v.z == b) + (v.w == b); }
            for (; u < tid; ++u) rank += s_b[u] == b;
            const int pos = ld_l2(off + b) + ld_l2(cnt + b) + rank;
            if (pos < r) members[pos] = tok;
        }
        __syncthreads();
        if (b >= 0) atomicAdd(&cnt[b], 1);
        __syncthreads();
    }
}

// ------------------------------------------------------------------ merge, unmerge
constexpr int kWaves = 4;

__global__ __launch_bounds__(64 * kWaves) void merge_kernel(const _Float16* __restrict__ n, long ld, Geom g, int C, int r, const int* __restrict__ lists, long per_img,
                                                            _Float16* __restrict__ m, int n_img)
{
    const int lane = (int)(threadIdx.x & 63), pieces = C / 8, nk = g.Ns - r, Tm = g.T - r;
    const long wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long)blockIdx.x * kWaves, n_waves = (long)gridDim.x * kWaves, rows = (long)n_img * Tm;
    for (long row = wave0; row < rows; row += n_waves) {
        const int img = (int)(row / Tm), k = (int)(row - (long)img * Tm);
        const int* slot = lists + (long)img * per_img;
        const int* kept = slot + g.T;
        const int* off = kept + nk;
        const int* members = off + g.Nd + 1;
        const _Float16* src = n + (long)img * g.T * ld;
        _Float16* d = m + row * C;
        if (k < nk) {
            const _Float16* s = src + (long)kept[k] * ld;
            for (int p = lane; p < pieces; p += 64) *reinterpret_cast<u32x4*>(d + 8 * p) = *reinterpret_cast<const u32x4*>(s + 8 * p);
            continue;
        }
        const int j = k - nk, m0 = off[j], m1 = off[j + 1];
        const _Float16* s = src + (long)dst_token(g, j) * ld;
        const float cntf = (float)(1 + m1 - m0);
        for (int p = lane; p < pieces; p += 64) {
            const f16x8 v = *reinterpret_cast<const f16x8*>(s + 8 * p);
            float a[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = (float)v[e];
            for (int q = m0; q < m1; ++q) {
                const f16x8 w = *reinterpret_cast<const f16x8*>(src + (long)members[q] * ld + 8 * p);
#pragma unroll
                for (int e = 0; e < 8; ++e) a[e] += (float)w[e];
            }
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)(a[e] / cntf);
            *reinterpret_cast<f16x8*>(d + 8 * p) = o;
        }
    }
}

__global__ __launch_bounds__(64 * kWaves) void unmerge_add_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ o, long ldo, int T, int Tm, int C,
                                                                  const int* __restrict__ lists, long per_img, float* __restrict__ y, long ldy, int n_img)
{
    const int lane = (int)(threadIdx.x & 63), quads = C / 4;
    const long wave0 = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + (long)blockIdx.x * kWaves, n_waves = (long)gridDim.x * kWaves, rows = (long)n_img * T;
    for (long row = wave0; row < rows; row += n_waves) {
        const int img = (int)(row / T), t = (int)(row - (long)img * T);
        int s = lists[(long)img * per_img + t];
        s = s < 0 ? 0 : s >= Tm ? Tm - 1 : s;
        const float4* xr = reinterpret_cast<const float4*>(x + row * ldx);
        const float4* orow = reinterpret_cast<const float4*>(o + ((long)img * Tm + s) * ldo);
        float4* yr = reinterpret_cast<float4*>(y + row * ldy);
        for (int p = lane; p < quads; p += 64) {
            const float4 a = xr[p], b = orow[p];
            yr[p] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
    }
}

// ------------------------------------------------------------------ launching
inline bool al16(const void* p) { return !((uintptr_t)p & 15); }

int map_check(const char* what, int n_img, int H, int W)
{
    if (n_img < 1 || H < 2 || W < 2) return mlsd_set_error(-1, "%s: %d maps of %d x %d tokens (at least one 2 x 2 cell)", what, n_img, H, W);
    if ((long)H * W > (1L << 24)) return mlsd_set_error(-1, "%s: a map of %d x %d tokens (at most 2^24)", what, H, W);
    return 0;
}
int rows_check(const char* what, int C, int64_t ld)
{
    if (C < 64 || C > 1280 || C % 32) return mlsd_set_error(-1, "%s: rows of %d halfs (a multiple of 32, 64 .. 1280)", what, C);
    if (ld < C || ld % 8) return mlsd_set_error(-1, "%s: row stride of %lld halfs (a multiple of 8, at least %d)", what, (long long)ld, C);
    return 0;
}
int r_check(const char* what, const Geom& g, int r)
{
    if (r < 0 || r > g.Ns || r % 16) return mlsd_set_error(-1, "%s: r %d (a multiple of 16, 0 .. %d sources)", what, r, g.Ns);
    return 0;
}
unsigned row_blocks(long rows) { long b = (rows + kWaves - 1) / kWaves; return (unsigned)(b > 4096 ? 4096 : b); }

// the dynamic LDS a kernel may ask for, once per device (as mlsd_guidance_plane_select does)
int lds_attr(const void* fn, int bytes, bool* set)
{
    int dev = 0;
    MLSD_HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !set[dev]) {
        MLSD_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        if (dev >= 0 && dev < 64) set[dev] = true;
    }
    return 0;
}

}  // namespace

extern "C" {

MLSD_API int mlsd_tome_r(int H, int W, float ratio)
{
    if (H < 2 || W < 2 || !(ratio > 0.0f)) return 0;
    const Geom g = geom_of(H, W);
    long r = (long)floor((double)ratio * (double)g.T);
    if (r > g.Ns) r = g.Ns;
    return (int)(r / 16 * 16);
}

MLSD_API size_t mlsd_tome_lists_ints(int H, int W, int r)
{
    if (H < 2 || W < 2) return 0;
    const Geom g = geom_of(H, W);
    if (r < 0 || r > g.Ns) return 0;
    return (size_t)g.T + (size_t)(g.Ns - r) + (size_t)g.Nd + 1 + (size_t)r + (size_t)g.Nd;
}

MLSD_API int mlsd_tome_select_lds_limit(int bytes)
{
    const int was = g_sel_lds_limit;
    if (bytes >= 0) g_sel_lds_limit = bytes < SEL_LDS_BYTES ? bytes : SEL_LDS_BYTES;
    return was;
}

MLSD_API int mlsd_tome_match(const void* n, int64_t ld, int n_img, int H, int W, int C, int* best, float* score, void* stream)
{
    const char* what = "mlsd_tome_match";
    if (!n || !best || !score) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (map_check(what, n_img, H, W) || rows_check(what, C, ld)) return -1;
    if (!al16(n)) return mlsd_set_error(-1, "%s: rows must be 16-byte aligned", what);
    if (n_img > 65535) return mlsd_set_error(-1, "%s: %d maps (at most 65535)", what, n_img);
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    const Geom g = geom_of(H, W);
    static bool lds_set[64];
    if (lds_attr((const void*)match_kernel, MT_LDS_MAX, lds_set)) return -1;
    const size_t lds = (size_t)MT_DT * (2 * C + 16) + MT_DT * 4;
    hipLaunchKernelGGL(match_kernel, dim3((g.Ns + MT_SRC - 1) / MT_SRC, n_img), dim3(64 * MT_WAVES), lds, (hipStream_t)stream, (const _Float16*)n, (long)ld, g, C, best, score);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_tome_select(const float* score, const int* best, int n_img, int H, int W, int r, int* lists, void* stream)
{
    const char* what = "mlsd_tome_select";
    if (!score || !best || !lists) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (map_check(what, n_img, H, W)) return -1;
    const Geom g = geom_of(H, W);
    if (r_check(what, g, r)) return -1;
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    const long per = (long)mlsd_tome_lists_ints(H, W, r);
    const size_t lds = (size_t)g.Ns * 4;
    if (lds <= (size_t)g_sel_lds_limit) {
        static bool lds_set[64];
        if (lds_attr((const void*)select_kernel<true>, SEL_LDS_BYTES, lds_set)) return -1;
        hipLaunchKernelGGL((select_kernel<true>), dim3(n_img), dim3(SEL_THREADS), lds, (hipStream_t)stream, score, best, g, r, lists, per);
    } else
        hipLaunchKernelGGL((select_kernel<false>), dim3(n_img), dim3(SEL_THREADS), 0, (hipStream_t)stream, score, best, g, r, lists, per);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_tome_merge(const void* n, int64_t ld, int n_img, int H, int W, int C, int r, const int* lists, void* m, void* stream)
{
    const char* what = "mlsd_tome_merge";
    if (!n || !lists || !m) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (map_check(what, n_img, H, W) || rows_check(what, C, ld)) return -1;
    const Geom g = geom_of(H, W);
    if (r_check(what, g, r)) return -1;
    if (!al16(n) || !al16(m)) return mlsd_set_error(-1, "%s: rows must be 16-byte aligned", what);
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    const long rows = (long)n_img * (g.T - r);
    hipLaunchKernelGGL(merge_kernel, dim3(row_blocks(rows)), dim3(64 * kWaves), 0, (hipStream_t)stream, (const _Float16*)n, (long)ld, g, C, r, lists,
                       (long)mlsd_tome_lists_ints(H, W, r), (_Float16*)m, n_img);
    return mlsd_check_launch(what);
}

MLSD_API int mlsd_tome_unmerge_add(const float* x, int64_t ldx, const float* o, int64_t ldo, int n_img, int H, int W, int C, int r, const int* lists, float* y, int64_t ldy,
                                   void* stream)
{
    const char* what = "mlsd_tome_unmerge_add";
    if (!x || !o || !lists || !y) return mlsd_set_error(-1, "%s: NULL buffer", what);
    if (map_check(what, n_img, H, W)) return -1;
    const Geom g = geom_of(H, W);
    if (r_check(what, g, r)) return -1;
    if (C < 4 || C % 4 || ldx < C || ldo < C || ldy < C || (ldx | ldo | ldy) % 4) return mlsd_set_error(-1, "%s: rows of %d floats at strides %lld, %lld, %lld (multiples of 4)", what, C, (long long)ldx, (long long)ldo, (long long)ldy);
    if (!al16(x) || !al16(o) || !al16(y)) return mlsd_set_error(-1, "%s: rows must be 16-byte aligned", what);
    if (mlsd_runtime_is_dry()) return mlsd_check_launch(what);
    const long rows = (long)n_img * g.T;
    hipLaunchKernelGGL(unmerge_add_kernel, dim3(row_blocks(rows)), dim3(64 * kWaves), 0, (hipStream_t)stream, x, (long)ldx, o, (long)ldo, g.T, g.T - r, C, lists,
                       (long)mlsd_tome_lists_ints(H, W, r), y, (long)ldy, n_img);
    return mlsd_check_launch(what);
}

}  // extern "C"
