"""What the hires tests share: the prototypes and option ids of the hires fix on top of mlis_ffi's table, and the float64 references of the
resampling kernel -- torch's F.interpolate(align_corners=False) and a numpy restatement of the same definitions that also knows the
wrap (tests/test_hires_cpu.py pins the one to the other)."""
import ctypes as C

import numpy as np

import mlis_ffi as F

HIRES_SCALE, HIRES_DENOISE, HIRES_STEPS, HIRES_UPSCALER = 102, 103, 104, 105
OPTION_NAMES = {HIRES_SCALE: "hires_scale", HIRES_DENOISE: "hires_denoise", HIRES_STEPS: "hires_steps", HIRES_UPSCALER: "hires_upscaler"}
MODES = ["nearest", "bilinear", "bicubic"]                # MLSD_RESAMPLE_* / MLIS_AMD_RESAMPLE_* 0..2
TORCH_MODES = ["nearest-exact", "bilinear", "bicubic"]
PROTOTYPES = [
    ("mlis_amd_tensor_resample", F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor), F.ci, F.ci, F.ci]),
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
]
PAD = 4         # source pixels of padding in the wrap reference


def bind(path):
    lib = F.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def get(lib, m, opt):
    v = (C.c_float if opt in (HIRES_SCALE, HIRES_DENOISE) else C.c_int)(-7)
    assert lib.mlis_option_get(m.ctx, opt, C.byref(v)) == 1, m.err()
    return v.value


# ------------------------------------------------------------------ float64 references
def _axis_matrix(n_in, n_out, mode, wrap):
    """[n_out, n_in] float64 weights of one axis: pixel centres, taps clamped or (wrap) modulo the extent"""
    d = np.arange(n_out, dtype=np.int64)
    W = np.zeros((n_out, n_in))
    fold = (lambda i: i % n_in) if wrap else (lambda i: np.clip(i, 0, n_in - 1))
    if mode == 0:
        np.add.at(W, (d, fold(((2 * d + 1) * n_in) // (2 * n_out))), 1.0)          # floor((d + 0.5) n_in / n_out)
        return W
    src = (d + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(src).astype(np.int64)
    t = src - i0
    if mode == 1:
        taps = [(0, 1 - t), (1, t)]
    else:
        a = -0.75
        c1 = lambda x: ((a + 2) * x - (a + 3)) * x * x + 1
        c2 = lambda x: ((a * x - 5 * a) * x + 8 * a) * x - 4 * a
        taps = [(-1, c2(t + 1)), (0, c1(t)), (1, c1(1 - t)), (2, c2(2 - t))]
    for k, w in taps:
        np.add.at(W, (d, fold(i0 + k)), w)
    return W


def resample64(x, dh, dw, mode, wrap=0):
    """numpy float64 restatement: x [..., sh, sw] -> [..., dh, dw]; wrap bit 0 columns, bit 1 rows"""
    x = np.asarray(x, np.float64)
    Wy = _axis_matrix(x.shape[-2], dh, mode, wrap & 2)
    Wx = _axis_matrix(x.shape[-1], dw, mode, wrap & 1)
    return Wy @ x @ Wx.T


def torch64(x, dh, dw, mode, wrap=0):
    """F.interpolate in float64; with a wrap, of the input padded by PAD source pixels -- circularly along the wrapped axes, with the border
    value along the others -- and cropped by PAD * scale (the sizes of the tests make that an integer)"""
    import torch
    import torch.nn.functional as TF
    x = np.asarray(x, np.float64)
    x = x.reshape((-1, 1) + x.shape[-2:])
    kw = {} if mode == 0 else dict(align_corners=False)
    if not wrap:
        return TF.interpolate(torch.from_numpy(x), size=(dh, dw), mode=TORCH_MODES[mode], **kw).numpy()[:, 0]
    sh, sw = x.shape[-2:]
    assert (PAD * dh) % sh == 0 and (PAD * dw) % sw == 0, "PAD * scale must be an integer"
    py, px = PAD * dh // sh, PAD * dw // sw
    xp = np.pad(x, ((0, 0), (0, 0), (PAD, PAD), (0, 0)), mode="wrap" if wrap & 2 else "edge")
    xp = np.pad(xp, ((0, 0), (0, 0), (0, 0), (PAD, PAD)), mode="wrap" if wrap & 1 else "edge")
    y = TF.interpolate(torch.from_numpy(xp), size=(dh + 2 * py, dw + 2 * px), mode=TORCH_MODES[mode], **kw).numpy()
    return y[:, 0, py:py + dh, px:px + dw]
