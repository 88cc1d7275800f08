"""numpy restatements of the guidance limiters' rules (include/mlsd_kernels.h); float32 arithmetic rounds every operation once, like the kernels' _rn intrinsics"""
import numpy as np

F32 = np.float32
KINDS = ("gauss", "equal", "ties", "lowbyte", "negzero")
mix32 = lambda c, u, s: (c * F32(s) + u * (F32(1) - F32(s))).astype(F32)


def plane_inputs(B, HW):
    """rows [2 B][4][HW] float32 (cond, then uncond); plane b * 4 + ch has kind KINDS[(b * 4 + ch) % 5].  The structured kinds have uncond = 0, so that
    g = fmul(c, cfg) keeps the structure: `equal` a constant plane (t = 0: identity); `ties` 90 % of the plane one value; `lowbyte` +-(1.5 + j 2^-23) / 8, j < 128, a zero
    mean and keys that differ in their last byte only; `negzero` half the plane -0.0.  (sym: v, -v and a zero where HW is odd, shuffled: an exactly zero sum.)"""
    rng = np.random.default_rng(B * 1000003 + HW)
    sym = lambda v: rng.permutation(np.concatenate([v[:HW // 2], -v[:HW // 2], np.zeros(HW % 2)])).astype(F32)
    rows = np.zeros((2 * B, 4, HW), F32)
    for i in range(B * 4):
        b, ch, kind = i // 4, i % 4, KINDS[i % len(KINDS)]
        if kind == "gauss":
            rows[b, ch], rows[B + b, ch] = rng.standard_normal(HW) * 2 + 1, rng.standard_normal(HW) * 2 - 1
        elif kind == "equal":
            rows[b, ch], rows[B + b, ch] = 1.25, -0.5
        elif kind == "ties":
            rows[b, ch] = np.where(rng.random(HW) < 0.9, 0.75, rng.standard_normal(HW))
        elif kind == "lowbyte":
            rows[b, ch] = sym((1.5 + rng.integers(0, 128, HW) * 2.0 ** -23) / 8)
        else:
            rows[b, ch] = sym(np.where(rng.random(HW) < 0.5, -0.0, np.abs(rng.standard_normal(HW))))
    return rows


def quantile_np(a, p):      # over the last axis; the two order statistics by np.partition, interpolated in double, rounded once
    pos = float(F32(p)) * (a.shape[-1] - 1)
    lo, hi = int(pos), min(int(pos) + 1, a.shape[-1] - 1)
    part = np.partition(a, (lo, hi), axis=-1).astype(np.float64)
    return (part[..., lo] + (pos - lo) * (part[..., hi] - part[..., lo])).astype(F32)


def triples32(rows, B, HW, cfg, mimic, p, means):      # (mean_cfg, t, r) [B][4][3] from the library's own plane means [B][4][2]
    c, u = rows[:B], rows[B:2 * B]
    a = np.abs(mix32(c, u, cfg) - means[..., 0:1])
    m = np.abs(mix32(c, u, mimic) - means[..., 1:2]).max(-1)
    t = np.maximum(m, a.max(-1) if F32(p) == 1 else quantile_np(a, p))
    ident = (t == 0) | ~np.isfinite(t) | (HW == 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (m.astype(np.float64) / t.astype(np.float64)).astype(F32)
    return np.stack([means[..., 0], np.where(ident, F32(np.inf), t), np.where(ident, F32(1), r)], -1).astype(F32)


def limited(rows, x, B, mode, cfg, pag, lim, vparam, c_out, c_skip, dtype):      # rule (d) per element in `dtype` arithmetic; lim: triples (mode 1) or coefficients
    c, u, p = (rows[k * B:(k + 1) * B].astype(dtype) for k in range(3))
    s = dtype(F32(cfg))
    g = c * s + u * (dtype(1) - s)
    if mode == 1:
        mean, t, r = (lim[..., k:k + 1].astype(dtype) for k in range(3))
        g = np.clip(g - mean, -t, t) * r + mean
    else:
        g = c * lim[:, 0].astype(dtype).reshape(B, 1, 1) + u * lim[:, 1].astype(dtype).reshape(B, 1, 1)
    if pag:
        g = g + dtype(pag) * (c - p)
    return g * dtype(c_out) + x.astype(dtype) * dtype(c_skip) if vparam else g
