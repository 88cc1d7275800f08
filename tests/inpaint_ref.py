"""numpy restatements of the region-inpainting rules of include/mlsd_kernels.h and include/mlis_abi.h: the repaint weight, the grow (twice: by hand and on scipy's
rank filters), the Gaussian taps and blur matrices, the bounding box, the composite and the region rule in Python integers.  wrap: bit 0 the x axis, bit 1 the y axis;
a non-wrapped axis replicates its border pixel, a wrapped one takes indices modulo the extent."""
import numpy as np


def mask_weight(m, invert):
    m = np.asarray(m, np.float32)
    v = m if invert else np.float32(1) - m
    return np.where(np.isnan(v), np.float32(0), np.minimum(np.maximum(v, np.float32(0)), np.float32(1))).astype(np.float32)


def axis_indices(n, r, wrap):
    """[n][2 r + 1] source indices of every output index along one axis"""
    j = np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :]
    return j % n if wrap else np.clip(j, 0, n - 1)


def grow(x, radius, wrap):
    """[h][w]: maximum (radius > 0) or minimum (radius < 0) over the (2 |radius| + 1)^2 square, rows then columns"""
    x = np.asarray(x, np.float32)
    if radius == 0:
        return x.copy()
    r, red = abs(radius), (np.max if radius > 0 else np.min)
    h, w = x.shape
    rows = red(x[:, axis_indices(w, r, wrap & 1)], axis=2)
    return red(rows[axis_indices(h, r, (wrap >> 1) & 1), :], axis=1).astype(np.float32)


def grow_scipy(x, radius, wrap):
    """the same on scipy.ndimage's maximum_filter / minimum_filter with a per-axis border mode"""
    from scipy import ndimage
    x = np.asarray(x, np.float32)
    if radius == 0:
        return x.copy()
    size, f = 2 * abs(radius) + 1, (ndimage.maximum_filter if radius > 0 else ndimage.minimum_filter)
    mode = ("wrap" if wrap & 2 else "nearest", "wrap" if wrap & 1 else "nearest")      # axis 0 is y; 'wrap' is periodic over any number of periods
    return f(x, size=size, mode=mode).astype(np.float32)


def gauss_radius(sigma):
    return int(2.5 * float(np.float32(sigma)) + 0.5)


def gauss_taps(sigma):
    """float32 taps: exp(-k^2 / (2 sigma^2)), k = -r .. r, normalised in double, then rounded"""
    r = gauss_radius(sigma)
    if r == 0:
        return np.ones(1, np.float32)
    s = float(np.float32(sigma))
    k = np.arange(-r, r + 1, dtype=np.float64)
    t = np.exp(-(k * k) / (2.0 * s * s))
    return (t / t.sum()).astype(np.float32)


def blur_matrix(n, taps, wrap):
    """float64 [n][n]: A[d][s] = the sum of the taps that output d takes from source s (replicated border or modulo)"""
    r = len(taps) // 2
    A = np.zeros((n, n), np.float64)
    idx = axis_indices(n, r, wrap)
    for k, t in enumerate(np.asarray(taps, np.float64)):
        np.add.at(A, (np.arange(n), idx[:, k]), t)
    return A


def blur_matrix_abs(n, taps, wrap):
    return blur_matrix(n, np.abs(np.asarray(taps, np.float64)), wrap)


def bbox(p):
    ys, xs = np.nonzero(np.asarray(p) > 0)
    return (0, 0, 0, 0) if xs.size == 0 else (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)


def composite(orig, patch, p, x0, y0):
    """orig [1 or B][c][H][W], patch [B][c][ch][cw], p [H][W] -> [B][c][H][W], numpy's fp32 expression inside the rectangle"""
    orig, patch, p = np.asarray(orig, np.float32), np.asarray(patch, np.float32), np.asarray(p, np.float32)
    B, c, ch, cw = patch.shape
    out = np.broadcast_to(orig, (B,) + orig.shape[1:]).copy()
    o, pv = out[:, :, y0:y0 + ch, x0:x0 + cw], p[None, None, y0:y0 + ch, x0:x0 + cw]
    out[:, :, y0:y0 + ch, x0:x0 + cw] = o * (np.float32(1) - pv) + patch * pv
    return out


def ceil_div(a, b):
    return -((-a) // b)


def region(W, H, box, padding, tw, th):
    """the region rule of mlis_abi.h in Python integers; None where the library returns -1"""
    bx0, by0, bx1, by1 = box
    if W < 1 or H < 1 or tw < 1 or th < 1 or padding < 0 or bx0 < 0 or by0 < 0 or bx1 > W or by1 > H or bx0 >= bx1 or by0 >= by1:
        return None
    x0, y0, x1, y1 = max(0, bx0 - padding), max(0, by0 - padding), min(W, bx1 + padding), min(H, by1 + padding)
    cw, ch = x1 - x0, y1 - y0
    if cw * th < ch * tw:
        n = min(W, ceil_div(ch * tw, th))
        x0 -= (n - cw) // 2
        cw = n
        x0 = min(max(x0, 0), W - cw)
    else:
        n = min(H, ceil_div(cw * th, tw))
        y0 -= (n - ch) // 2
        ch = n
        y0 = min(max(y0, 0), H - ch)
    return (x0, y0, x0 + cw, y0 + ch)


def control_rect(reg, W, H, Wc, Hc):
    """the region scaled to a control image of Wc x Hc: floor of the near edges, ceil of the far ones"""
    x0, y0, x1, y1 = reg
    return (x0 * Wc // W, y0 * Hc // H, ceil_div(x1 * Wc, W), ceil_div(y1 * Hc, H))
