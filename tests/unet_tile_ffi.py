"""What the tiled-diffusion tests share: the option ids and prototypes on top of mlis_ffi's table, and a numpy restatement of the window
geometry and of the blend -- window starts per axis, the ramp weight, and the float64 weighted average sum_j w_j e_j / sum_j w_j."""
import ctypes as C

import numpy as np

import mlis_ffi as F

UNET_TILE, UNET_TILE_OVERLAP = 111, 112
OPTION_NAMES = {UNET_TILE: "unet_tile", UNET_TILE_OVERLAP: "unet_tile_overlap"}
pi = C.POINTER(C.c_int)
pf = C.POINTER(C.c_float)
PROTOTYPES = [
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
    ("mlis_amd_window_starts", F.ci, [F.ci, F.ci, F.ci, F.ci, pi, F.ci]),
    ("mlsd_window_gather", F.ci, [F.vp, F.ci, F.ci, F.vp, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp]),
    ("mlsd_window_blend", F.ci, [F.vp, C.c_int64, F.vp, F.vp, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp]),
    ("mlsd_window_wsum", F.ci, [F.vp, F.ci, F.ci, F.ci, F.ci, pi, F.ci, pi, F.ci, F.ci, F.ci, F.vp]),
]
EXPORTS = [p[0] for p in PROTOTYPES] + ["mlis_amd_create_tiled", "mlis_amd_dxdt", "mlis_amd_tile_info", "mlis_amd_tile_windows"]


def bind(path):
    lib = F.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def get(lib, m, opt):
    v = C.c_int(-7)
    assert lib.mlis_option_get(m.ctx, opt, C.byref(v)) == 1, m.err()
    return v.value


def c_starts(lib, L, T, O, wrap, cap=64):
    out = (C.c_int * max(cap, 1))()
    n = lib.mlis_amd_window_starts(L, T, O, int(wrap), out, cap)
    return None if n < 0 else [out[i] for i in range(n)]


# ------------------------------------------------------------------ numpy restatement
def starts(L, T, O, wrap):
    """the rule of the issue, in Python integers"""
    if T >= L:
        return [0]
    if wrap:
        n = -(-L // (T - O))
        return [i * L // n for i in range(n)]
    n = -(-(L - O) // (T - O))
    return [i * (L - T) // (n - 1) for i in range(n)]


def ramp(T, O):
    i = np.arange(T)
    return np.minimum(np.minimum(i + 1, T - i), O + 1) / (O + 1)


def weight(wh, ww, oy, ox):
    """[wh, ww] float64"""
    return np.outer(ramp(wh, oy), ramp(ww, ox))


def windows(W, H, tw, th, O, tiling=0):
    """((x0, y0) row-major with y outer, window width, window height)"""
    xs, ys = starts(W, tw, O, tiling & 1), starts(H, th, O, tiling & 2)
    return [(x, y) for y in ys for x in xs], min(tw, W), min(th, H)


def crop(x, x0, y0, ww, wh):
    """x [..., H, W] -> the window at (x0, y0), wrapped"""
    H, W = x.shape[-2:]
    return np.take(np.take(x, np.arange(y0, y0 + wh), axis=-2, mode="wrap"), np.arange(x0, x0 + ww), axis=-1, mode="wrap")


def blend64(parts, wins, ww, wh, O, H, W):
    """parts[j] [..., wh, ww] of window wins[j] -> (float64 weighted average [..., H, W], cover count [H, W])"""
    w = weight(wh, ww, O, O)
    num = np.zeros(parts[0].shape[:-2] + (H, W))
    den = np.zeros((H, W))
    cnt = np.zeros((H, W), int)
    for p, (x0, y0) in zip(parts, wins):
        iy, ix = np.ix_((np.arange(wh) + y0) % H, (np.arange(ww) + x0) % W)
        num[..., iy, ix] += w * np.asarray(p, np.float64)
        den[iy, ix] += w
        cnt[iy, ix] += 1
    return num / den, cnt
