// Flash attention for ONE head of d = 512 (the KL-VAE's mid-block self attention, reference src/vae.c:46-74), gfx950 (MI355X).
// fp16 operands, fp32 accumulate, online softmax; the [T][T] scores never leave the CU.
//
// d = 512 breaks the layout of the kernels in attention.hip, where one wave owns a block of query rows from the scores to the output: a wave cannot hold its rows' Q
// (512 wide), their 512-wide fp32 output and the score fragment in 256 registers.  Here the two products are split over the waves of a workgroup along DIFFERENT axes:
//
//   workgroup = 8 waves = 128 query rows of one image; key tiles of 32 keys.
//   phase A, scores:   wave w owns query rows 16 w .. 16 w + 15 with their Q in registers for the whole kernel (16 k-steps x 8 halfs = 64 VGPRs).
//                      S^T[key][q] = K . Q^T over the full d on v_mfma_f32_16x16x32_f16 (A = K rows out of LDS, B = Q): a lane ends with 8 scores of ONE query
//                      (l & 15), keys 4 (l >> 4) + e and 16 + 4 (l >> 4) + e, so the row maximum is in-lane plus two exchanges.  Online softmax with the scale folded
//                      into the exp2 argument; the wave writes fp16 P[128][32] and the rows' rescale factors to LDS.
//   phase B, P . V:    wave w owns output COLUMNS 64 w .. 64 w + 63 of all 128 rows: O^T[d][q] += V^T . P on v_mfma_f32_32x32x16_f16 with the V^T fragments read out of
//                      the row-major V tile by ds_read_b64_tr_b16 (as attn_kernel) and P read back from LDS in the key order those fragments have.  128 fp32
//                      accumulator registers per lane, rescaled per row (= per lane) by the factors of phase A.
//   No FLOP is done twice, no accumulator set exceeds 128 registers, and the two phases need 2 barriers per key tile.
//
//   K and V tiles (32 KiB each) are double buffered and filled by LDS-DMA (global_load_lds_dwordx4, one 1 KiB row per wave instruction), issued at the top of a tile for
//   the next one and drained before the barrier that ends phase A: in phase B nothing is in flight.  Rows are unpadded (the DMA image is lane-linear); the bank spread
//   comes from an XOR on the SOURCE chunk:  K slot = chunk ^ (row & 15) (16 rows x one chunk -> 16 different bank quads for ds_read_b128),
//                                            V slot = chunk ^ ((row & 3) << 2) (4 rows x 64 B -> the four quarters of the 64 banks for the transposed read).
//   The four tile buffers are four __shared__ arrays and the tile loop is unrolled by two, so that every LDS read names the array it reads: the compiler then does
//   not wait for the DMA into the OTHER buffer in front of it.
//
// Keys at or past T are clamped duplicates of the last key, masked to -1e30 before the maximum; query rows at or past T are clamped duplicates that are never stored.
// No atomics, nothing waits for another workgroup, every sum has one fixed order: two launches give the same bits.
#include <hip/hip_runtime.h>
#include "common.hpp"
#include "mlsd_kernels.h"
#include <math.h>

namespace {

constexpr int WD = 512;             // d_head
constexpr int WBM = 128;            // query rows per workgroup
constexpr int WBK = 32;             // keys per tile
constexpr int WROWB = WD * 2;       // bytes per K / V row in LDS
constexpr int WPSTR = 72;           // bytes per P row: 32 keys + 8 (18 dwords: 32 rows start on 32 different even banks)

struct WideP {
    const _Float16 *q, *k, *v;
    _Float16* o;
    long ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso;
    int T, nq;          // tokens; query blocks per image
    float sc;           // 1/sqrt(512) * log2(e)
};

__global__ __launch_bounds__(512, 1) void attn_wide_kernel(const WideP p)
{
    __shared__ __attribute__((aligned(1024))) unsigned char Ks0[WBK * WROWB];
    __shared__ __attribute__((aligned(1024))) unsigned char Ks1[WBK * WROWB];
    __shared__ __attribute__((aligned(1024))) unsigned char Vs0[WBK * WROWB];
    __shared__ __attribute__((aligned(1024))) unsigned char Vs1[WBK * WROWB];
    __shared__ __attribute__((aligned(16))) unsigned char Ps[WBM * WPSTR];
    __shared__ float Al[WBM];       // phase A -> B: the rows' rescale factors of this tile; after the loop 1 / l

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;      // 16x16x32 fragments: row / column l15, k group lg
    const int lr = lane & 31, lh = lane >> 5;       // 32x32x16 fragments
    const int b = blockIdx.x / p.nq, q0 = (blockIdx.x - b * p.nq) * WBM;

    const _Float16* Qg = p.q + (long)b * p.bsq;
    const _Float16* Kg = p.k + (long)b * p.bsk;
    const _Float16* Vg = p.v + (long)b * p.bsv;

    // Q fragments (B operand of S^T = K . Q^T): lane (l15 = query, lg) holds Q[q][32 ks + 8 lg + j]
    f16x8 qf[16];
    {
        const _Float16* qr = Qg + (long)min(q0 + 16 * wave + l15, p.T - 1) * p.ldq + 8 * lg;
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) qf[ks] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(qr + 32 * ks));
    }

    // LDS-DMA staging: wave w fills rows 4 w .. 4 w + 3 of the K and the V tile, one row (64 lanes x 16 bytes) per instruction
    auto stage = [&](int t, unsigned char* Kd, unsigned char* Vd) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = 4 * wave + i;
            const long key = min(t * WBK + row, p.T - 1);
            int ln = lane;
            asm volatile("" : "+v"(ln));             // the source chunks are recomputed per piece (two VALU instructions): kept across the loop as 16 address registers they were spilled
            const int ck = ln ^ (row & 15), cv = ln ^ ((row & 3) << 2);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Kg + key * p.ldk + ck * 8),
                                             (__attribute__((address_space(3))) void*)(Kd + row * WROWB), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Vg + key * p.ldv + cv * 8),
                                             (__attribute__((address_space(3))) void*)(Vd + row * WROWB), 16, 0, 0);
        }
    };

    f32x16 oacc[4][2];                               // O^T of [32-row query block][32-column block of this wave's 64 columns]
#pragma unroll
    for (int qb = 0; qb < 4; ++qb)
#pragma unroll
        for (int d = 0; d < 2; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[qb][d][e] = 0.f;
    float m_run = -1.0e30f, l_run = 0.f;             // of query 16 wave + l15 (l_run: this lane's 8 keys of every tile)

    // transposed-read lane address pattern (attn_kernel): 4 key rows x 16 columns per 16 lanes
    const int tg = lane >> 4, ti = lane & 15;
    const int tr_row = 4 * (tg >> 1) + (ti >> 2);                    // + 16 s (+ 8): row & 3 == ti >> 2
    const int vswz = (ti >> 2) << 2;
    const int tr_c = 2 * (tg & 1) + ((ti & 3) >> 1), tr_b = 8 * (ti & 1);

    int kx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kx[j] = (((4 * j) ^ (l15 & 12)) + (lg ^ (l15 & 3))) << 4;

    const int nt = (p.T + WBK - 1) / WBK;

    // one key tile: K / V in Kc / Vc, the next tile's DMA into Kn / Vn
    auto tile = [&](int t, const unsigned char* Kc, const unsigned char* Vc, unsigned char* Kn, unsigned char* Vn) __attribute__((always_inline)) {
        const int kv0 = t * WBK;
        if (t + 1 < nt) stage(t + 1, Kn, Vn);       // the buffers tile t - 1 used: every wave passed the barrier that ended its phase B

        // ---- phase A: S^T = K . Q^T for this wave's 16 query rows (two 16-key blocks, two interleaved chains each)
        f32x4 s0, s1;
        {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            f32x4 a0 = zero, a1 = zero, c0 = zero, c1 = zero;
            const unsigned char* kr0 = Kc + l15 * WROWB;
            const unsigned char* kr1 = Kc + (16 + l15) * WROWB;
#pragma unroll
            for (int ks = 0; ks < 16; ks += 2) {
                // chunk (4 ks + lg) ^ l15 = 16 (ks >> 2) + ((4 (ks & 3)) ^ (l15 & 12)) + (lg ^ (l15 & 3)): four per-lane offsets and a constant
                const int o0 = kx[ks & 3] + 256 * (ks >> 2), o1 = kx[(ks + 1) & 3] + 256 * ((ks + 1) >> 2);
                a0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(kr0 + o0), qf[ks], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(kr1 + o0), qf[ks], a1, 0, 0, 0);
                c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(kr0 + o1), qf[ks + 1], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8*>(kr1 + o1), qf[ks + 1], c1, 0, 0, 0);
            }
            s0 = a0 + c0; s1 = a1 + c1;             // keys kv0 + 4 lg + e and kv0 + 16 + 4 lg + e of query l15
        }
        if (kv0 + WBK > p.T) {                       // ragged last tile (wave-uniform): the clamped duplicates
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (kv0 + 4 * lg + e >= p.T) s0[e] = -1.0e30f;
                if (kv0 + 16 + 4 * lg + e >= p.T) s1[e] = -1.0e30f;
            }
        }
        float mx = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);       // (key kv0 is never masked: m_new is a real score from the first tile on)
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * p.sc);
        m_run = m_new;
        const float msc = -m_new * p.sc;
        float pr[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pr[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[e], p.sc, msc));        // arguments <= 0; a masked key gives 0
            pr[4 + e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[e], p.sc, msc));
        }
        l_run = l_run * alpha + (((pr[0] + pr[1]) + (pr[2] + pr[3])) + ((pr[4] + pr[5]) + (pr[6] + pr[7])));
        {
            unsigned char* pw = Ps + (16 * wave + l15) * WPSTR + 8 * lg;
            const f16x4 h0 = {(_Float16)pr[0], (_Float16)pr[1], (_Float16)pr[2], (_Float16)pr[3]};
            const f16x4 h1 = {(_Float16)pr[4], (_Float16)pr[5], (_Float16)pr[6], (_Float16)pr[7]};
            *reinterpret_cast<f16x4*>(pw) = h0;
            *reinterpret_cast<f16x4*>(pw + 32) = h1;
            if (lg == 0) Al[16 * wave + l15] = alpha;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's rows of tile t + 1 have landed
        __syncthreads();                                       // P, the factors and tile t + 1 visible; every wave is done reading K(t)

        // ---- phase B: O^T += V^T . P for all 128 rows, this wave's 64 columns
        float al[4];
#pragma unroll
        for (int qb = 0; qb < 4; ++qb) al[qb] = Al[32 * qb + lr];
        if (__any(al[0] != 1.0f || al[1] != 1.0f || al[2] != 1.0f || al[3] != 1.0f)) {
#pragma unroll
            for (int qb = 0; qb < 4; ++qb)
#pragma unroll
                for (int d = 0; d < 2; ++d)
#pragma unroll
                    for (int e = 0; e < 16; ++e) oacc[qb][d][e] *= al[qb];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // P as the B operand in the key order of the transposed V fragments: j < 4: key 16 s + 4 lh + j, j >= 4: key 16 s + 8 + 4 lh + j - 4
            union { f16x4 h[2]; f16x8 f; } pf[4];
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) {
                const unsigned char* pr_ = Ps + (32 * qb + lr) * WPSTR + (16 * s + 4 * lh) * 2;
                pf[qb].h[0] = *reinterpret_cast<const f16x4*>(pr_);
                pf[qb].h[1] = *reinterpret_cast<const f16x4*>(pr_ + 16);
            }
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const unsigned char* a0 = Vc + (16 * s + tr_row) * WROWB + (((8 * wave + 4 * d + tr_c) ^ vswz) << 4) + tr_b;
                union { h16x4 h[2]; f16x8 f; } vf;
                vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h16x4*)a0);
                vf.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h16x4*)(a0 + 8 * WROWB));
#pragma unroll
                for (int qb = 0; qb < 4; ++qb) oacc[qb][d] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf.f, pf[qb].f, oacc[qb][d], 0, 0, 0);
            }
        }
        __syncthreads();                                       // every wave is done reading P, the factors and V(t)
    };

    stage(0, Ks0, Vs0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nt; t += 2) {
        tile(t, Ks0, Vs0, Ks1, Vs1);
        if (t + 1 < nt) tile(t + 1, Ks1, Vs1, Ks0, Vs0);
    }

    // ---- epilogue: O = O^T / l.  A query's sum is spread over the four lanes l15 + 16 lg; oacc[qb][d][e]: column 64 wave + 32 d + (e & 3) + 8 (e >> 2) + 4 lh, query 32 qb + lr
    {
        float l = l_run + __shfl_xor(l_run, 16, 64);
        l = l + __shfl_xor(l, 32, 64);
        if (lg == 0) Al[16 * wave + l15] = 1.0f / l;
    }
    __syncthreads();
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
        const int row = q0 + 32 * qb + lr;
        const float inv = Al[32 * qb + lr];
        if (row < p.T) {
            _Float16* og = p.o + (long)b * p.bso + (long)row * p.ldo + 64 * wave + 4 * lh;
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int eg = 0; eg < 4; ++eg) {
                    const f16x4 h = {(_Float16)(oacc[qb][d][4 * eg + 0] * inv), (_Float16)(oacc[qb][d][4 * eg + 1] * inv),
                                     (_Float16)(oacc[qb][d][4 * eg + 2] * inv), (_Float16)(oacc[qb][d][4 * eg + 3] * inv)};
                    *reinterpret_cast<u32x2*>(og + 32 * d + 8 * eg) = __builtin_bit_cast(u32x2, h);
                }
        }
    }
}

// the one rule of what the kernel takes: NULL, or the reason of the refusal
const char* wide_refusal(const mlsd_attn_args* a, char* why, size_t n)
{
    if (!a || !a->q || !a->k || !a->v || !a->out) { snprintf(why, n, "mlsd_attention_wide: null operand"); return why; }
    if (a->n_head != 1 || a->d_head != WD) { snprintf(why, n, "mlsd_attention_wide: %d head(s) of d_head %d (takes one head of %d)", a->n_head, a->d_head, WD); return why; }
    if (a->causal) { snprintf(why, n, "mlsd_attention_wide: no causal mask"); return why; }
    if (a->Tq < 1 || a->Tq != a->Tk || a->n_batch < 1) { snprintf(why, n, "mlsd_attention_wide: Tq %d, Tk %d, n_batch %d (self attention: Tq == Tk >= 1)", a->Tq, a->Tk, a->n_batch); return why; }
    if ((a->ldq & 7) || (a->ldk & 7) || (a->ldv & 7) || (a->ldo & 3) || a->ldq < WD || a->ldk < WD || a->ldv < WD || a->ldo < WD) {
        snprintf(why, n, "mlsd_attention_wide: strides must be multiples of 8 and at least %d", WD); return why;
    }
    if ((a->bsq & 7) || (a->bsk & 7) || (a->bsv & 7) || (a->bso & 3) || (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v) & 15) || ((uintptr_t)a->out & 7)) {
        snprintf(why, n, "mlsd_attention_wide: misaligned operand"); return why;
    }
    if ((long)a->n_batch * ((a->Tq + WBM - 1) / WBM) > 0x7fffffffL) { snprintf(why, n, "mlsd_attention_wide: too many query blocks"); return why; }
    return nullptr;
}

}  // namespace

extern "C" {

/* the label of the launch (as mlsd_attention_variant), NULL where mlsd_attention_wide would refuse */
MLSD_API const char* mlsd_attention_wide_variant(const mlsd_attn_args* a)
{
    char why[160];
    return wide_refusal(a, why, sizeof(why)) ? nullptr : "attn<wide,d512>";
}

MLSD_API int mlsd_attention_wide(const mlsd_attn_args* a, void* stream)
{
    char why[160];
    if (wide_refusal(a, why, sizeof(why))) return mlsd_set_error(-1, "%s", why);
    if (mlsd_runtime_is_dry()) return mlsd_check_launch("attn<wide,d512>");      // the dry runtime's buffers are host memory: refuse before the launch
    WideP p;
    p.q = (const _Float16*)a->q; p.k = (const _Float16*)a->k; p.v = (const _Float16*)a->v; p.o = (_Float16*)a->out;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.bsq = a->bsq; p.bsk = a->bsk; p.bsv = a->bsv; p.bso = a->bso;
    p.T = a->Tq; p.nq = (a->Tq + WBM - 1) / WBM;
    p.sc = (float)(1.4426950408889634 / sqrt((double)WD));
    hipLaunchKernelGGL(attn_wide_kernel, dim3((unsigned)(a->n_batch * p.nq)), dim3(512), 0, (hipStream_t)stream, p);
    return mlsd_check_launch("attn_wide_kernel");
}

}  // extern "C"
