"""Float64 references of the normalisation and attention kernels, and the per-group / per-row error bounds they are held to
(tests/test_conditioning_gpu.py).

Every reference takes the exact values the kernel reads -- the fp32 maps downloaded from the device, the fp16-rounded Q / K / V --
so that the only differences left are the kernel's own roundings.  The bounds are stated per group or per row (never one global
norm): a wrong group, row or key tile cannot hide behind good ones.

Bounds (u32 = 2^-24, u16 = 2^-11):
  half_ulp16(y)     half an fp16 ulp of each output element (the final rounding of every fp16 output);
  GroupNorm / LayerNorm, per group or row:
                    eps_norm = C_NORM * u32 * ((1 + r + max|x^|) * max|gamma| + max|beta|),
                    r = |mean| / sqrt(var + eps) and x^ = (x - mean) / sqrt(var + eps) from the float64 statistics.  This is what an
                    algorithm that centres before it squares achieves on fp32 data: the centring x - mean loses u32 |mean|, i.e. u32 r in
                    units of the spread; the variance is then good to a few u32 relative (u32 |x^| per element); the fp32 affine adds
                    u32 (r + |x^|) |gamma| + u32 |beta|.  A single pass of unshifted fp32 sums loses u32 r^2 (times the block length) in
                    the variance instead: at r = 300 that is percents.
  attention, per output element of a row:
                    eps_attn = C_ATTN * u16 * (sum_j p_j |v_j| + |o|)                   (P rounded to fp16; everything else fp32 on fp16
                                                                                         operands)
                    + C_ATTN * sum_j p_j dq_j (|v_j| + |o|),  dq_j = u16 * scale * sum_i |q_i k_ji|
                                                              (kernels that round the scaled Q to fp16 before the QK product: an error of
                                                              dq_j in score j moves o by p_j dq_j (v_j - o))
"""
import numpy as np

U32 = 2.0 ** -24
U16 = 2.0 ** -11

# The constants are fixed here for every case; they are never widened per case.
# 64 = 2^6 roundings' worth: the fp32 mean (a sum of up to 128 sequential terms before the exact or double combination: ~sqrt(128) = 11
# u32 typical), the centring, the variance sum, rstd, the affine and SiLU.  An unshifted single-pass variance exceeds it by a factor ~r.
C_NORM = 64.0
# 4: P rounded once (u16), the row sum l and O / l in fp32, the fp32 accumulation of fp16 products; the Q term is a first-order estimate.
C_ATTN = 4.0


def half_ulp16(y):
    """Half an fp16 ulp of each element of y (subnormals included: the ulp never goes below 2^-24)."""
    a = np.abs(np.asarray(y, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


def silu(y):
    return y / (1.0 + np.exp(-y))


# ------------------------------------------------------------------ GroupNorm
def group_stats(x, G, eps):
    """x [n_img][HW][C] (any float): float64 mean, var, r, max|x^| per (image, group), each [n_img][G]."""
    x = np.asarray(x, np.float64)
    n, hw, C = x.shape
    xg = x.reshape(n, hw, G, C // G)
    mu = xg.mean(axis=(1, 3))
    var = ((xg - mu[:, None, :, None]) ** 2).mean(axis=(1, 3))
    sd = np.sqrt(var + eps)
    r = np.abs(mu) / sd
    xh = (np.abs(xg - mu[:, None, :, None]) / sd[:, None, :, None]).max(axis=(1, 3))
    return mu, var, r, xh


def groupnorm64(x1, x2, G, eps, gamma, beta, silu_on):
    """GroupNorm over the virtual concat [x1 | x2] along channels ([n_img][HW][C_i] each, x2 may be None), affine, optional SiLU."""
    x = np.asarray(x1, np.float64) if x2 is None else np.concatenate([np.asarray(x1, np.float64), np.asarray(x2, np.float64)], axis=2)
    n, hw, C = x.shape
    mu, var, _, _ = group_stats(x, G, eps)
    xg = x.reshape(n, hw, G, C // G)
    y = ((xg - mu[:, None, :, None]) / np.sqrt(var + eps)[:, None, :, None]).reshape(n, hw, C)
    y = y * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return silu(y) if silu_on else y


def groupnorm_bound(x, G, eps, gamma, beta):
    """eps_norm per (image, group) [n_img][G], and r per (image, group)."""
    _, _, r, xh = group_stats(x, G, eps)
    C = np.asarray(x).shape[2]
    gm = np.abs(np.asarray(gamma, np.float64)).reshape(G, C // G).max(1)
    bm = np.abs(np.asarray(beta, np.float64)).reshape(G, C // G).max(1)
    return C_NORM * U32 * ((1 + r + xh) * gm + bm), r


def groupnorm_worst(got, want, x, G, eps, gamma, beta):
    """max over (image, group) of max|got - want| / (half_ulp16(want) + eps_norm): [n_img][G] ratios and r.  <= 1 passes."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    n, hw, C = want.shape
    eb, r = groupnorm_bound(x, G, eps, gamma, beta)
    tol = half_ulp16(want).reshape(n, hw, G, C // G) + eb[:, None, :, None]
    err = np.abs(got - want).reshape(n, hw, G, C // G)
    ratio = (err / tol).max(axis=(1, 3))
    ratio[~np.isfinite(got.reshape(n, hw, G, C // G)).all(axis=(1, 3))] = np.inf
    return ratio, r


# ------------------------------------------------------------------ LayerNorm
def layernorm64(x, eps, gamma, beta):
    x = np.asarray(x, np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + (0 if beta is None else np.asarray(beta, np.float64))


def layernorm_worst(got, want, x, eps, gamma, beta, half=True):
    """Per-row ratio max|got - want| / ([half_ulp16(want)] + eps_norm) [rows], and r per row."""
    x = np.asarray(x, np.float64)
    mu = x.mean(1)
    sd = np.sqrt(((x - mu[:, None]) ** 2).mean(1) + eps)
    r = np.abs(mu) / sd
    xh = (np.abs(x - mu[:, None]) / sd[:, None]).max(1)
    gm, bm = np.abs(np.asarray(gamma, np.float64)).max(), (0.0 if beta is None else np.abs(np.asarray(beta, np.float64)).max())
    tol = C_NORM * U32 * ((1 + r + xh) * gm + bm)[:, None] + (half_ulp16(want) if half else 0.0)
    got = np.asarray(got, np.float64)
    ratio = (np.abs(got - want) / tol).max(1)
    ratio[~np.isfinite(got).all(1)] = np.inf
    return ratio, r


# ------------------------------------------------------------------ attention
def attention64(q, k, v, heads, causal=False):
    """q [Tq][H*d], k / v [Tk][H*d] (the fp16 values the kernel reads): float64 o [Tq][H*d] and p [H][Tq][Tk]."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Tq, D = q.shape
    Tk, d = k.shape[0], D // heads
    qh, kh, vh = (a.reshape(a.shape[0], heads, d).transpose(1, 0, 2) for a in (q, k, v))
    s = qh @ kh.transpose(0, 2, 1) / np.sqrt(d)
    if causal:
        s = np.where(np.arange(Tk)[None, None, :] > np.arange(Tq)[None, :, None], -np.inf, s)
    p = softmax64(s)
    o = (p @ vh).transpose(1, 0, 2).reshape(Tq, D)
    return o, p


def softmax64(s, scale=1.0):
    s = np.asarray(s, np.float64) * scale
    e = np.exp(s - s.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def attention_bound(q, k, v, heads, o, p, q_scaled_f16):
    """eps_attn per output element [Tq][H*d]; q_scaled_f16 adds the documented term of the kernels that round Q * log2(e) / sqrt(d)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    Tq, D = q.shape
    d = D // heads
    vh = np.abs(v.reshape(-1, heads, d).transpose(1, 0, 2))                     # [H][Tk][d]
    oh = np.abs(np.asarray(o, np.float64).reshape(Tq, heads, d).transpose(1, 0, 2))   # [H][Tq][d]
    pv = p @ vh                                                                   # sum_j p_j |v_j|
    b = C_ATTN * U16 * (pv + oh)
    if q_scaled_f16:
        qh = np.abs(q.reshape(Tq, heads, d).transpose(1, 0, 2))
        kh = np.abs(k.reshape(-1, heads, d).transpose(1, 0, 2))
        dq = U16 / np.sqrt(d) * (qh @ kh.transpose(0, 2, 1))                      # [H][Tq][Tk]
        w = p * dq
        b = b + C_ATTN * (w @ vh + w.sum(-1, keepdims=True) * oh)
    return b.transpose(1, 0, 2).reshape(Tq, D)


def attention_worst(got, want, bound):
    """Per-row ratio max|got - want| / (half_ulp16(want) + bound) [Tq]."""
    got = np.asarray(got, np.float64)
    ratio = (np.abs(got - want) / (half_ulp16(want) + bound)).max(1)
    ratio[~np.isfinite(got).all(1)] = np.inf
    return ratio
