"""The colour-fix rules of include/mlsd_kernels.h (mlsd_colorfix_*) restated in numpy float64 on arrays [B][c][h][w]; a target has 1 or B images."""
import numpy as np


def low(x, levels):      # Low = L_(levels-1)(... L_0(x)): nine taps per level at distance 2^i, indices clamped to the plane
    x = np.asarray(x, np.float64)
    h, w = x.shape[-2:]
    k = (0.25, 0.5, 0.25)
    for i in range(levels):
        ys = [np.clip(np.arange(h) + (d << i), 0, h - 1) for d in (-1, 0, 1)]
        xs = [np.clip(np.arange(w) + (d << i), 0, w - 1) for d in (-1, 0, 1)]
        x = sum(k[a] * k[b] * x[..., ys[a][:, None], xs[b][None, :]] for a in range(3) for b in range(3))
    return x


def wavelet(content, target, levels=5):
    c, t = np.asarray(content, np.float64), np.asarray(target, np.float64)
    return c + low(t - c, levels)


def wavelet_two_filters(content, target, levels=5):      # the published form
    c, t = np.asarray(content, np.float64), np.asarray(target, np.float64)
    return c - low(c, levels) + low(t, levels)


def adain_coef(content, target):      # a, b per plane, [B][c]
    c, t = np.asarray(content, np.float64), np.asarray(target, np.float64)
    if c.shape[-2] * c.shape[-1] < 2 or t.shape[-2] * t.shape[-1] < 2:
        return np.ones(c.shape[:2]), np.zeros(c.shape[:2])
    a = np.sqrt(t.var((-2, -1), ddof=1) + 1e-5) / np.sqrt(c.var((-2, -1), ddof=1) + 1e-5)
    return a, t.mean((-2, -1)) - c.mean((-2, -1)) * a


def quant(x):      # rule (a) of mlsd_canny, in float32
    x = np.asarray(x, np.float32)
    return np.clip(np.floor(x * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.int64)


def hist_lut(content_plane, target_plane):      # counts of both planes and the float64 LUT
    kc, kt = np.bincount(quant(content_plane).ravel(), minlength=256), np.bincount(quant(target_plane).ravel(), minlength=256)
    qc, qt = np.cumsum(kc) / content_plane.size, np.cumsum(kt) / target_plane.size
    V = np.nonzero(kt)[0]
    return kc, kt, np.interp(qc, qt[V], V) / 255.0
