"""The Canny rules of include/mlsd_kernels.h (mlsd_canny, (a) - (f)) restated twice, and the inputs the Canny tests share.

canny() is the reference: numpy int64 written from the rules, padded arrays for the neighbours, hysteresis by a plain flood fill from the strong pixels.
canny_scipy() is a second statement that shares no code with it (it takes the same integer thresholds; it quantises for itself, in float64 from the float32
product and sum): Sobel as two scipy.ndimage.correlate1d passes per derivative (mode "nearest" or "wrap" per axis), neighbours by np.roll with the rolled-in border zeroed, hysteresis by scipy.ndimage.label with a 3 x 3 structure keeping the components that hold a
strong pixel -- on wrapped axes a 3 x 3 tiling of the class map is labelled and the centre read back, repeated with the kept pixels made strong until nothing
is added (one labelling reaches one turn around the image).  tests/test_canny_cpu.py holds the two to each other on every input below."""
import numpy as np


# ------------------------------------------------------------------ (a), (b)
def quantise(x):
    """(a): float32 planes -> int64 in 0 .. 255, product and sum rounded to float32 one by one"""
    x = np.asarray(x, np.float32)
    v = np.floor((x * np.float32(255.0)).astype(np.float32) + np.float32(0.5))
    return np.clip(v, 0, 255).astype(np.int64)


def thresholds(low, high, l2):
    """(b): the integers mlsd_canny compares magnitudes with"""
    if low > high:
        low, high = high, low
    if l2:
        lo, hi = (int(np.floor(max(0.0, min(32767.0, v)))) for v in (low, high))
        return lo * lo, hi * hi
    return int(np.floor(low)), int(np.floor(high))


# ------------------------------------------------------------------ the reference
def _pad(a, wrap, fill):
    """one pixel around the last two axes: wrapped on a wrapped axis, else the border pixel (fill None) or a constant"""
    for axis, bit in ((a.ndim - 1, 1), (a.ndim - 2, 2)):
        width = [(0, 0)] * a.ndim
        width[axis] = (1, 1)
        if wrap & bit:
            a = np.pad(a, width, mode="wrap")
        elif fill is None:
            a = np.pad(a, width, mode="edge")
        else:
            a = np.pad(a, width, mode="constant", constant_values=fill)
    return a


def gradient(q, wrap, l2):
    """(c), (d): q int64 [planes][h][w] -> dx, dy, m [h][w] of the plane with the largest m (the lowest index on ties)"""
    p = _pad(q, wrap, None)
    dx = (p[:, :-2, 2:] + 2 * p[:, 1:-1, 2:] + p[:, 2:, 2:]) - (p[:, :-2, :-2] + 2 * p[:, 1:-1, :-2] + p[:, 2:, :-2])
    dy = (p[:, 2:, :-2] + 2 * p[:, 2:, 1:-1] + p[:, 2:, 2:]) - (p[:, :-2, :-2] + 2 * p[:, :-2, 1:-1] + p[:, :-2, 2:])
    m = dx * dx + dy * dy if l2 else np.abs(dx) + np.abs(dy)
    k = np.argmax(m, axis=0)[None]           # the first of equal maxima
    return tuple(np.take_along_axis(v, k, 0)[0] for v in (dx, dy, m))


def classes(dx, dy, m, lo, hi, wrap):
    """(e): 0 none, 1 weak, 2 strong"""
    p = _pad(m, wrap, 0)
    c = p[1:-1, 1:-1]
    left, right, up, down = p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]
    ul, ur, dl, dr = p[:-2, :-2], p[:-2, 2:], p[2:, :-2], p[2:, 2:]
    x, y = np.abs(dx), np.abs(dy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    neg = (dx ^ dy) < 0
    keep = np.where(y < t22, (c > left) & (c >= right),
                    np.where(y > t67, (c > up) & (c >= down),
                             np.where(neg, (c > ur) & (c > dl), (c > ul) & (c > dr))))
    keep &= c > lo
    return np.where(keep, np.where(c > hi, 2, 1), 0).astype(np.uint8)


def hysteresis(cls, wrap):
    """(f): flood fill from the strong pixels through weak ones, 8-connected, around wrapped axes"""
    h, w = cls.shape
    out = cls == 2
    stack = [(int(y), int(x)) for y, x in zip(*np.nonzero(out))]
    while stack:
        y, x = stack.pop()
        for ny in (y - 1, y, y + 1):
            if wrap & 2:
                ny %= h
            elif not 0 <= ny < h:
                continue
            for nx in (x - 1, x, x + 1):
                if wrap & 1:
                    nx %= w
                elif not 0 <= nx < w:
                    continue
                if cls[ny, nx] == 1 and not out[ny, nx]:
                    out[ny, nx] = True
                    stack.append((ny, nx))
    return out


def canny(x, lo, hi, l2, wrap, parts=False):
    """x float32 [planes][h][w], lo / hi as thresholds() gives them -> bool [h][w]; parts: (edges, classes, m) instead"""
    dx, dy, m = gradient(quantise(x), wrap, l2)
    cls = classes(dx, dy, m, lo, hi, wrap)
    e = hysteresis(cls, wrap)
    return (e, cls, m) if parts else e


# ------------------------------------------------------------------ the second statement
def _shift(m, sy, sx, wrap):
    """m at (y + sy, x + sx); 0 outside the image on an axis that does not wrap"""
    r = np.roll(m, (-sy, -sx), (0, 1))
    h, w = m.shape
    if sy and not wrap & 2:
        r[(h - 1) if sy > 0 else 0, :] = 0
    if sx and not wrap & 1:
        r[:, (w - 1) if sx > 0 else 0] = 0
    return r


def canny_scipy(x, lo, hi, l2, wrap):
    from scipy import ndimage as ndi
    # (a) for itself: the float32 product, the float32 sum, then floor and clamp as integers
    v = np.float32(255.0) * np.asarray(x, np.float32)
    v = v + np.float32(0.5)
    assert v.dtype == np.float32
    q = np.minimum(255, np.maximum(0, np.floor(v.astype(np.float64)).astype(np.int64)))
    mode_x, mode_y = ("wrap" if wrap & 1 else "nearest"), ("wrap" if wrap & 2 else "nearest")
    best = None
    for plane in q:
        dx = ndi.correlate1d(ndi.correlate1d(plane, [1, 2, 1], axis=0, mode=mode_y), [-1, 0, 1], axis=1, mode=mode_x)
        dy = ndi.correlate1d(ndi.correlate1d(plane, [1, 2, 1], axis=1, mode=mode_x), [-1, 0, 1], axis=0, mode=mode_y)
        m = dx ** 2 + dy ** 2 if l2 else np.abs(dx) + np.abs(dy)
        if best is None:
            best = [dx, dy, m]
        else:
            win = m > best[2]
            best = [np.where(win, a, b) for a, b in zip((dx, dy, m), best)]
    dx, dy, m = best
    # the sector from the exact comparisons of |dy| 2^15 with |dx| 13573 and |dx| (13573 + 2^16)
    ax, ay = np.abs(dx), np.abs(dy) * 32768
    horizontal, vertical = ay < ax * 13573, ay > ax * (13573 + 65536)
    s = np.where((dx < 0) != (dy < 0), -1, 1)
    keep = np.zeros(m.shape, bool)
    keep |= horizontal & (m > _shift(m, 0, -1, wrap)) & (m >= _shift(m, 0, 1, wrap))
    keep |= ~horizontal & vertical & (m > _shift(m, -1, 0, wrap)) & (m >= _shift(m, 1, 0, wrap))
    diag = ~horizontal & ~vertical
    keep |= diag & (s == 1) & (m > _shift(m, -1, -1, wrap)) & (m > _shift(m, 1, 1, wrap))
    keep |= diag & (s == -1) & (m > _shift(m, -1, 1, wrap)) & (m > _shift(m, 1, -1, wrap))
    keep &= m > lo
    strong = keep & (m > hi)
    h, w = m.shape
    ry, rx = (3 if wrap & 2 else 1), (3 if wrap & 1 else 1)
    while True:
        lab, _ = ndi.label(np.tile(keep, (ry, rx)), structure=np.ones((3, 3), int))
        held = np.unique(lab[np.tile(strong, (ry, rx))])
        big = np.isin(lab, held[held > 0])
        y0, x0 = (h if ry == 3 else 0), (w if rx == 3 else 0)
        edges = big[y0:y0 + h, x0:x0 + w]
        if not wrap or np.array_equal(edges, strong):
            return edges
        strong = edges


# ------------------------------------------------------------------ inputs
def _smoothstep_ramp(h, w, ax, ay):
    """0 .. 255 along the direction (ax, ay) through a smoothstep: the gradient magnitude rises and falls, rounding to 8 bits leaves plateaus"""
    yy, xx = np.mgrid[0:h, 0:w]
    t = (ax * xx + ay * yy).astype(np.float64)
    t = (t - t.min()) / (t.max() - t.min())
    return np.rint(255 * t * t * (3 - 2 * t)).astype(np.uint8)


def _staircase(h, w, step, runs, axis):
    """steps of equal height whose treads are runs[i % len] pixels: equal neighbouring magnitudes across the risers"""
    line, v, i = [], 0, 0
    n = w if axis == 1 else h
    while len(line) < n:
        line += [v] * runs[i % len(runs)]
        v, i = min(255, v + step), i + 1
    line = np.array(line[:n], np.uint8)
    return np.tile(line[None, :], (h, 1)) if axis == 1 else np.tile(line[:, None], (1, w))


def _comb(h, w, band, base, lift, strong_at=None):
    """a region of value base + lift hanging from the top in fingers of alternating length: its boundary is one serpentine step edge"""
    a = np.full((h, w), base, np.uint8)
    for b in range((w + band - 1) // band):
        a[:(h - 10) if b % 2 == 0 else 10, b * band:(b + 1) * band] = base + lift
    if strong_at is not None:
        y, x = strong_at
        a[y - 1:y + 2, x - 1:x + 2] = 255
    return a


def _seam(h, w, base, lift, strong):
    """a horizontal step edge over the whole width, interrupted around the middle columns; the strong spot sits right of the gap, so the part left of it is lit
    only around the seam of a wrapped x axis"""
    a = np.full((h, w), base, np.uint8)
    a[h // 2:, :] = base + lift
    a[:, w // 2 - 10:w // 2 + 10] = base
    if strong:
        a[h // 2 - 1:h // 2 + 2, 3 * w // 4 - 1:3 * w // 4 + 2] = 255
    return a


def _three(a):
    return np.stack([a, np.roll(a, 3, 1) // 2, 255 - np.roll(a, 5, 0)])


def cases(tile):
    """name -> (uint8 [3][h][w], thresholds): (low, high) in the units of the canny_* options, or "pct" for the 60th / 85th percentile of the reference's own
    magnitude map.  tile = the kernels' (classify x, classify y, sweep x, sweep y) from mlsd_canny_tile.  The one-plane runs take plane 0."""
    rng = np.random.default_rng(2024)
    out = {}
    for h, w in ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (29, 37)):
        out[f"rand_{w}x{h}"] = (rng.integers(0, 256, (3, h, w), dtype=np.uint8), (100, 200))
    cx, cy, sx, sy = tile
    for name, (tx, ty) in (("classify", (cx, cy)), ("sweep", (sx, sy))):
        for d in (-1, 1):
            out[f"{name}_tile{d:+d}"] = (rng.integers(0, 256, (3, ty + d, tx + d), dtype=np.uint8), (300, 700))
    out["rand_300x200"] = (rng.integers(0, 256, (3, 200, 300), dtype=np.uint8), "pct")
    for ax, ay in ((3, 1), (-3, 1), (1, 3), (1, -3), (2, 2), (2, -2), (-2, -2)):
        out[f"ramp_{ax}_{ay}"] = (_three(_smoothstep_ramp(40, 44, ax, ay)), (20, 60))
    out["stairs_x"] = (_three(_staircase(20, 48, 40, (2, 2, 1, 3), 1)), (50, 150))
    out["stairs_y"] = (_three(_staircase(48, 20, 40, (2, 2, 1, 3), 0)), (50, 150))
    # plane 0 a vertical step, plane 1 a horizontal one of the same height (they tie where they cross: plane 0 wins), plane 2 a weaker diagonal one
    p = np.zeros((3, 32, 32), np.uint8)
    p[0, :, 15:] = 100
    p[1, 15:, :] = 100
    p[2][np.add.outer(np.arange(32), np.arange(32)) > 40] = 60
    out["planes_differ"] = (p, (50, 150))
    t = np.zeros((3, 32, 32), np.uint8)
    t[0, :, 15:] = 100
    t[1] = t[0].T
    t[2] = t[0]
    out["planes_tie"] = (t, (50, 150))
    # hysteresis across tiles: a weak serpentine edge about 200 x 200 with one strong spot at its first finger, and the same without the spot
    out["serpentine_lit"] = (np.repeat(_comb(200, 200, 8, 60, 20, strong_at=(100, 8))[None], 3, 0), (50, 300))
    out["serpentine_dark"] = (np.repeat(_comb(200, 200, 8, 60, 20)[None], 3, 0), (50, 300))
    out["seam_x"] = (np.repeat(_seam(60, 200, 60, 20, True)[None], 3, 0), (50, 300))
    out["seam_y"] = (np.repeat(_seam(60, 200, 60, 20, True).T[None], 3, 0), (50, 300))
    for v in out.values():
        v[0].setflags(write=False)
    return out


def overshoot_input():
    """values a bicubic or lanczos resample leaves outside [0, 1], among ones inside: float32 [3][41][67], thresholds (100, 200)"""
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([-0.2, 1.3, 0.0, 1.0, 0.25, 0.75], np.float32), (3, 41, 67)).astype(np.float32)
    x.setflags(write=False)
    return x


def as_float(u8):
    """uint8 / 255 in float32: (a) returns the integer whatever the evaluation order"""
    return (u8.astype(np.float32) / np.float32(255)).astype(np.float32)


_memo = {}


def expected(name, u8, thr, planes, l2, wrap):
    """(edges bool [h][w], classes, m, lo, hi) of the reference for one configuration, computed once"""
    key = (name, planes, l2, wrap)
    if key not in _memo:
        x = as_float(u8[:planes])
        if thr == "pct":
            m = gradient(quantise(x), wrap, l2)[2]
            lo, hi = int(np.percentile(m, 60)), int(np.percentile(m, 85))
        else:
            lo, hi = thresholds(thr[0], thr[1], l2)
        e, cls, m = canny(x, lo, hi, l2, wrap, parts=True)
        _memo[key] = (e, cls, m, lo, hi)
    return _memo[key]
