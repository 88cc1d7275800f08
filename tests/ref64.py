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
                    A cross attention that ends its q projection (tests/plan_audit.py) takes q = fp16(the launch's fp32 projection), the reference
                    q = fp16_rne(float64 projection): where the float64 value lies within the projection's fp32 bound of an fp16 tie the two may be
                    neighbours, one fp16 ulp apart (fp16_tie_ulp); attention_dq_term adds what that moves o by, in the same first-order form.
  GEMM / implicit-GEMM convolution, per output element (tests/test_gemm_float64_gpu.py, tests/test_ref64_gemm_cpu.py):
                    acc:  C_GEMM * u32 * D * S,   S = sum_k |a_k w_k| in float64 (|A| @ |W|^T).
                          The products of fp16 operands are exact in fp32 (11 + 11 significant bits).  Every kernel sums them in MFMA steps of
                          k_step = 16 (v_mfma_f32_32x32x16_f16: gemm_kernel, the general tiles) or 32 (v_mfma_f32_16x16x32_f16: the ping-pong,
                          stream-K, two-tiles-per-CU, skinny and small-Cout kernels), each added to ONE fp32 accumulator in K order; split-K and
                          stream-K add their nsplit slice sums one after another.  A sequential fp32 sum of n terms is off by at most
                          (n - 1) u32 sum|terms| to first order, so  D = ceil(K / k_step) + nsplit + 5,  the 5 covering the MFMA's own sum
                          of 16 / 32 products (a tree of depth <= 5).
                    epilogue adds (bias, rowbias, bias_m, residual): C_EPI * u32 * (|bias| + |rowbias| + |bias_m| + |resid| + |y|)
                          (four fp32 adds at most, each rounding a partial sum; the |acc| part of those partial sums is in the acc term);
                    activation of an argument z known to +-e_z:
                          |act'(z)| e_z + C_ACT * u32 * (1 + |eta(z)|) |act(z)| + min(|act(z)|, ACT_TINY),
                          eta = the argument of the exponential the kernel evaluates (common.hpp: v_exp_f32 on an fp32 argument, whose rounding
                          moves the exponential by u32 |eta| relative): silu z, quick-GELU 1.702 z, tanh-GELU 2 sqrt(2/pi) (z + 0.044715 z^3).
                          The last term: where the exponential overflows fp32 (eta < -88.7) the kernels return 0 for a value below 2^-120;
                          ACT_TINY = 2^-100 bounds that without touching any value a test can see.
                          GEGLU y = a gelu(g): |gelu(g)| e_a + |a| |gelu'(g)| e_g + C_ACT u32 (1 + |eta(g)|) |y| + u32 |y| + min(|y|, ACT_TINY).
                    fp16 outputs: the fp32 bound b32 + half_ulp16(|y| + b32); where a launch writes both C32 and C16, C16 must also be
                          fp16_rne(C32) bit for bit (the epilogues round the one fp32 value).  An fp16 output is +-inf exactly where fp16(C32) is.
  Small ops of the plans (tests/plan_audit.py), each from the kernel's own rounding steps (elementwise.hip, norm.hip) and the ulp errors the HIP math API
  documents for the functions it calls (expf, logf, sinf, cosf, tanhf: 1 ulp each; __expf: 2 + floor(|1.16 x|) ulp); one ulp is at most 2 u32 relative:
                    act_f32_to_f16 (silu_f16): y = fp16(act(x)) with the epilogues' act_apply on an exact fp32 argument: act_bound(x, 0, act) above, then
                          the fp16 rounding.  With MLSD_ACT_NONE (f32_to_f16) the op is exact: fp16_rne(x) bit for bit.
                    timestep_embedding: e = -logf(P) j / half (logf 1 ulp, one multiply, one divide: 4 u32 relative), f = expf(e) (its argument's error
                          moves it by 4 u32 |e|, expf adds 1 ulp), arg = t f (one multiply): arg is good to (4 |e| + 3) u32 relative; cosf / sinf move by
                          at most |arg| times that and add 1 ulp of their own:
                          b32 = u32 ((4 |e| + 3) |arg| + 2 |y|),  e = -ln(P) j / half, arg = t exp(e) in float64; then the fp16 rounding.
                    softmax_rows: z_j = (x_j - max) scale (two roundings: 2 u32 |z_j| absolute), e_j = __expf(z_j): relative error
                          d_j = u32 (2 |z_j| + 2 (2 + 1.16 |z_j|)) = u32 (4 + 4.32 |z_j|); the row sum (strided per lane, then a tree: at most cols / 256 + 10
                          sequential fp32 adds) carries sum_k p_k d_k + (cols / 256 + 10) u32 relative, its reciprocal and the product 2 u32 each:
                          b32_j = p_j (d_j + sum_k p_k d_k + (cols / 256 + 14) u32) + min(p_j, ACT_TINY) (v_exp_f32 may flush an fp32 subnormal); then the fp16 rounding.
                    nchw_to_nhwc_f16, mode 1 (TAE clamp): y = fp16(3 tanhf(x / 3) s): m = x (1/3) (the constant and the product: 2 u32 relative, which moves
                          tanh by (1 - t^2) |m| 2 u32), tanhf 1 ulp, the multiplies by 3 and by s one rounding each:
                          b32 = |s| 3 u32 (2 (1 - t^2) |x / 3| + 4 |t|),  t = tanh(x / 3) in float64; then the fp16 rounding.
                          Modes 0 and 2 are exact: fp16_rne of the fp32 products (x [* 2 - 1]) s.
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


def fp16_tie_ulp(y, b):
    """One fp16 ulp of y where a value known only to +- b may round to the other neighbour (y within b of the midpoint of two fp16 values), else 0:
    how far fp16(kernel's fp32 value) can lie from fp16_rne(y) when the kernel's value is within b of y."""
    y, b = np.asarray(y, np.float64), np.asarray(b, np.float64)
    ulp = 2.0 * half_ulp16(y)
    frac = np.abs(y) / ulp
    dist = np.abs(frac - np.floor(frac) - 0.5) * ulp
    return np.where(dist <= b, ulp, 0.0)


def attention_dq_term(dq, k, v, heads, o, p):
    """Bound term [Tq][H*d] for a Q whose elements may be off by dq [Tq][H*d] (absolute): score j of a row moves by at most
    ds_j = sum_i dq_i |k_ji| / sqrt(d), and o by sum_j p_j ds_j (|v_j| + |o|) to first order (as the q_scaled_f16 term of attention_bound)."""
    dq, k, v = (np.asarray(a, np.float64) for a in (dq, k, v))
    Tq, D = dq.shape
    d = D // heads
    dh = dq.reshape(Tq, heads, d).transpose(1, 0, 2)
    kh = np.abs(k.reshape(-1, heads, d).transpose(1, 0, 2))
    vh = np.abs(v.reshape(-1, heads, d).transpose(1, 0, 2))
    oh = np.abs(np.asarray(o, np.float64).reshape(Tq, heads, d).transpose(1, 0, 2))
    w = p * (dh @ kh.transpose(0, 2, 1) / np.sqrt(d))
    return (C_ATTN * (w @ vh + w.sum(-1, keepdims=True) * oh)).transpose(1, 0, 2).reshape(Tq, D)


def attention_worst(got, want, bound):
    """Per-row ratio max|got - want| / (half_ulp16(want) + bound) [Tq]."""
    got = np.asarray(got, np.float64)
    ratio = (np.abs(got - want) / (half_ulp16(want) + bound)).max(1)
    ratio[~np.isfinite(got).all(1)] = np.inf
    return ratio


# ------------------------------------------------------------------ GEMM / implicit-GEMM convolution
# 2: twice the first-order worst case of a sequential sum.  Typical errors are ~sqrt(D) times smaller than D u32 S; a 64-wide K tile dropped,
# a slice added twice, an fp16 partial sum or a flushed subnormal operand are > 2^-12 S-relative and fail by orders of magnitude.
C_GEMM = 2.0
# 4: bias, row bias, per-row bias and residual, one fp32 add each (see the docstring).
C_EPI = 4.0
# 8: v_exp_f32 and v_rcp_f32 (~1 ulp each), the add and multiplies of the sigmoid form, and the rounding of the argument eta itself.
C_ACT = 8.0
ACT_TINY = 2.0 ** -100
K_STEP_GENERAL, K_STEP_MFMA16 = 16, 32


def fp16_rne(x):
    """fp32 -> fp16 with round-to-nearest-even, overflow to +-inf and fp16 subnormals (numpy's conversion)."""
    return np.asarray(x, np.float32).astype(np.float16)


def gemm_depth(K, k_step, nsplit=1):
    """D of the accumulation bound (module docstring)."""
    return -(-K // k_step) + nsplit + 5


def im2col64(x, n_img, H, W, Cin, KH, KW, stride, pad, ups, OH, OW, rows=None, wrap=0):
    """Implicit-GEMM A operand in float64: x is the NHWC image [n_img * H * W][Cin] (the fp16 values the kernel reads, Cin already padded
    to the kernel's multiple of 8); row m = (image, oy, ox), column k = (kh, kw, cin) with cin fastest; zero outside the (nearest-2x upsampled
    when ups) image, or with wrap (bit 0 columns, bit 1 rows: mlsd_gemm_args.wrap) the pixel modulo the extent.  rows: the output rows wanted
    (default all)."""
    x = np.asarray(x, np.float64).reshape(n_img, H, W, Cin)
    if ups:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
        H, W = 2 * H, 2 * W
    m = np.arange(n_img * OH * OW) if rows is None else np.asarray(rows)
    b, oy, ox = m // (OH * OW), (m // OW) % OH, m % OW
    out = np.zeros((len(m), KH, KW, Cin))
    for kh in range(KH):
        iy = oy * stride - pad + kh
        if wrap & 2:
            iy = iy % H
        for kw in range(KW):
            ix = ox * stride - pad + kw
            if wrap & 1:
                ix = ix % W
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            out[ok, kh, kw] = x[b[ok], iy[ok], ix[ok]]
    return out.reshape(len(m), KH * KW * Cin)


def phase_A(x, py, px, wrap):
    """float64 A operand [n H W][2][2][Cin] of phase (py, px) of an upsampling convolution's phase form (mlsd_gemm_args.tap_oy / tap_ox = py / px): x is the
    NHWC source [n][H][W][Cin]; source pixel (y - 1 + py + a, x - 1 + px + b), zero or wrapped outside"""
    n, H, W, C = x.shape
    out = np.zeros((n, H, W, 2, 2, C))
    for a in range(2):
        for b in range(2):
            iy, ix = np.arange(H) - 1 + py + a, np.arange(W) - 1 + px + b
            if wrap & 2:
                iy = iy % H
            if wrap & 1:
                ix = ix % W
            oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            g = x[:, np.clip(iy, 0, H - 1)][:, :, np.clip(ix, 0, W - 1)].astype(np.float64)
            out[:, :, :, a, b, :] = g * oky[None, :, None, None] * okx[None, None, :, None]
    return out.reshape(n * H * W, 4 * C)


def gemm64(A, Wt):
    """C = A . W^T and S = |A| . |W|^T in float64, from the fp16 operand values."""
    A, Wt = np.asarray(A, np.float64), np.asarray(Wt, np.float64)
    return A @ Wt.T, np.abs(A) @ np.abs(Wt).T


def sigmoid64(x):
    """1 / (1 + e^-x) without cancellation: tiny values for very negative x stay tiny (not 0)"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act_eta(z, act):
    """argument of the exponential of the kernels' fast activation (0 where there is none)"""
    z = np.asarray(z, np.float64)
    if act == 1:
        return z
    if act in (2, 5):
        return 2.0 * np.sqrt(2.0 / np.pi) * (z + 0.044715 * z ** 3)
    if act == 3:
        return 1.702 * z
    return np.zeros_like(z)


def act64(z, act):
    """the epilogue activations in float64: SiLU, tanh-GELU (ggml_gelu; also the GEGLU gate), quick-GELU, ReLU"""
    z = np.asarray(z, np.float64)
    if act == 0:
        return z
    if act == 4:
        return np.maximum(z, 0.0)
    return z * sigmoid64(act_eta(z, act))


def dact64(z, act):
    """|act'(z)|"""
    z = np.asarray(z, np.float64)
    if act == 0:
        return np.ones_like(z)
    if act == 4:
        return (z > 0).astype(np.float64)
    e = act_eta(z, act)
    s = sigmoid64(e)
    de = {1: np.ones_like(z), 3: np.full_like(z, 1.702)}.get(act)
    if de is None:
        de = 2.0 * np.sqrt(2.0 / np.pi) * (1.0 + 3 * 0.044715 * z ** 2)
    return np.abs(s + z * s * (1.0 - s) * de)


def act_bound(z, ez, act):
    """bound of act(z) computed in fp32 from an argument known to +-ez (module docstring)"""
    y = np.abs(act64(z, act))
    return dact64(z, act) * ez + C_ACT * U32 * (1.0 + np.abs(act_eta(z, act))) * y + np.minimum(y, ACT_TINY)


def geglu_cols(nout):
    """GEMM columns of the value and the gate of GEGLU output column j: W rows interleaved in blocks of 32 (value, gate)"""
    j = np.arange(nout)
    v = (j >> 5) * 64 + (j & 31)
    return v, v + 32


def gemm_epilogue64(acc, S, D, rows, cols, bias=None, rowbias=None, rows_per_batch=1, bias_m=None, act=0, resid=None, act_after_resid=False):
    """y and its fp32 bound for the output elements [rows][cols] (global indices into the output) of a launch whose float64 accumulators are
    acc [len(rows)][GEMM columns] and S alike (for GEGLU every GEMM column of the rows, in the interleaved order; otherwise the columns
    `cols`).  The epilogue terms in the order of include/mlsd_kernels.h: bias [N], rowbias [batch][N] (row m uses batch m // rows_per_batch),
    bias_m [M], activation, resid [M][Nout] (or before the activation with act_after_resid)."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    f = lambda a: np.asarray(a, np.float64)
    z, ez = f(acc).copy(), C_GEMM * U32 * D * f(S)
    gcols = np.arange(z.shape[1]) if act == 5 else cols
    mag = np.zeros_like(z)
    for t in ([] if bias is None else [f(bias)[gcols][None, :]]) + \
             ([] if rowbias is None else [f(rowbias)[rows // max(rows_per_batch, 1)][:, gcols]]) + \
             ([] if bias_m is None else [f(bias_m)[rows][:, None]]):
        z = z + t
        mag = mag + np.abs(t)
    r = None if resid is None else f(resid)[rows][:, cols]
    if act == 5:
        vc, gc = geglu_cols(z.shape[1] // 2)
        vc, gc = vc[cols], gc[cols]
        a, g = z[:, vc], z[:, gc]
        ea = ez[:, vc] + C_EPI * U32 * (mag[:, vc] + np.abs(a))
        eg = ez[:, gc] + C_EPI * U32 * (mag[:, gc] + np.abs(g))
        gel = act64(g, 2)
        y = a * gel
        b = np.abs(gel) * ea + np.abs(a) * dact64(g, 2) * eg + C_ACT * U32 * (1.0 + np.abs(act_eta(g, 2))) * np.abs(y) + U32 * np.abs(y) \
            + np.minimum(np.abs(y), ACT_TINY)
    else:
        if r is not None and act_after_resid:
            z = z + r
            mag = mag + np.abs(r)
        ez = ez + C_EPI * U32 * (mag + np.abs(z))
        y, b = act64(z, act), (act_bound(z, ez, act) if act else ez)
    if r is not None and not (act_after_resid and act != 5):
        y = y + r
        b = b + C_EPI * U32 * (np.abs(r) + np.abs(y))
    return y, b


def gemm_ratio32(got, want, b32):
    """per-element |got - want| / b32 (inf where got is not finite)"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / b32)
    r[~np.isfinite(got)] = np.inf
    return r


def gemm_ratio16(got16, want, b32):
    """per-element ratio of an fp16 output to half_ulp16 + b32.  An infinite output passes (ratio 0) where want +- b32 reaches the fp16
    overflow threshold 65520 with the same sign; a finite output that should have overflowed fails through its distance to want."""
    g = np.asarray(got16, np.float64)
    b = b32 + half_ulp16(np.abs(want) + b32)
    fin = np.isfinite(g)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(g - want)
        r = np.where(fin & (err > 0), err / b, 0.0)
    inf_ok = (np.sign(g) == np.sign(want)) & (np.abs(want) + b32 >= 65520.0)
    r[~fin & ~inf_ok] = np.inf
    return r


# ------------------------------------------------------------------ column statistics of a producer (mlsd_gemm_args.colstats)
def colstats_ratios(c32, st, rows, shifted=True):
    """The statistics a launch wrote beside its fp32 output c32 [M][N]: st [M / rows][2][N] = per block and column sum (x - K) and sum (x - K)^2 with
    K = the block's first row (shifted), or the plain sums of x and x^2.  Ratio of each to C_NORM u32 of the sum of the magnitudes of its terms,
    in float64 on the stored output: (ratios of the sums, ratios of the sums of squares), each [M / rows][N]."""
    blk = np.asarray(c32, np.float64).reshape(-1, rows, np.asarray(c32).shape[1])
    d = blk - blk[:, :1] if shifted else blk
    st = np.asarray(st, np.float64)
    es = np.abs(st[:, 0] - d.sum(1)) / (C_NORM * U32 * np.abs(d).sum(1) + 1e-30)
    eq = np.abs(st[:, 1] - (d * d).sum(1)) / (C_NORM * U32 * (d * d).sum(1) + 1e-30)
    return es, eq


# ------------------------------------------------------------------ small ops of the plans (module docstring)
ULP = 2.0 * U32          # one fp32 ulp, relative, at most
ULP_EXPF = ULP_LOGF = ULP_SINCOSF = ULP_TANHF = 1.0      # HIP math API, maximum ulp error of the single-precision functions


def act16_bound(x, act):
    """(y64, b32) of y = act(x) computed in fp32 from an exact fp32 x (act_apply of common.hpp)"""
    x = np.asarray(x, np.float64)
    return act64(x, act), act_bound(x, 0.0, act)


def timestep_embedding64(t, dim, max_period):
    """(y64 [n][dim] = cos | sin, b32) of mlsd_timestep_embedding"""
    t = np.asarray(t, np.float64).reshape(-1)
    half = dim // 2
    e = -np.log(float(max_period)) * np.arange(half) / half
    arg = t[:, None] * np.exp(e)[None, :]
    rel = ((2 * ULP_LOGF + 2) * np.abs(e) + 2 * ULP_EXPF + 1)[None, :]            # (4 |e| + 3) at 1 ulp each
    y = np.concatenate([np.cos(arg), np.sin(arg)], axis=1)
    b = U32 * (np.concatenate([rel * np.abs(arg)] * 2, axis=1) + 2 * ULP_SINCOSF * np.abs(y))
    return y, b


def softmax_rows64(x, scale):
    """(p64, b32) of mlsd_softmax_rows on fp32 scores x [rows][cols]"""
    x = np.asarray(x, np.float64)
    z = (x - x.max(1, keepdims=True)) * float(scale)
    e = np.exp(z)
    p = e / e.sum(1, keepdims=True)
    d = U32 * (2 * np.abs(z) + 2 * (2 + 1.16 * np.abs(z)))
    b = p * (d + (p * d).sum(1, keepdims=True) + (x.shape[1] / 256.0 + 14) * U32) + np.minimum(p, ACT_TINY)      # (fp32 subnormals may be flushed: far below any fp16 value)
    return p, b


def tae_clamp64(x, s):
    """(y64, b32) of the tanh mode of mlsd_nchw_to_nhwc_f16: 3 tanh(x / 3) s"""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    t = np.tanh(x / 3.0)
    return 3.0 * t * s, np.abs(s) * 3.0 * U32 * (2 * (1 - t * t) * np.abs(x / 3.0) + (2 * ULP_TANHF + 2) * np.abs(t))
