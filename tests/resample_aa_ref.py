"""What the antialiased-resampling tests share: the float64 restatement of the tap tables (include/mlsd_kernels.h, mlsd_resample_aa_taps) in numpy and the
resample as dense matrices, My @ x @ Mx.T -- another formulation than the kernel's two tap loops --, the prototypes on top of mlis_ffi's table, and the
references the restatement is pinned to (tests/test_resample_aa_cpu.py): torch's interpolate(antialias=True) in float64, with a wrap the middle copy of a
circular tiling."""
import ctypes as C
import math

import numpy as np

import mlis_ffi as F

DOWNSCALE_FILTER = 161
DOWNSCALE_VALUES = ["none", "box", "bilinear", "bicubic", "lanczos"]       # 0 = none, else MLIS_AMD_AA_* + 1
FILTERS = ["box", "triangle", "cubic", "lanczos3"]                         # MLSD_AA_* / MLIS_AMD_AA_* 0..3
TWO_SUP = [1, 2, 4, 6]                                                     # 2 x support
TORCH_MODES = {1: "bilinear", 2: "bicubic"}
U32 = 2.0 ** -24
PROTOTYPES = [
    ("mlis_amd_tensor_resample_aa", F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor), F.ci, F.ci, F.ci]),
    ("mlis_amd_tensor_resample", F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor), F.ci, F.ci, F.ci]),
    ("mlis_amd_tensor_upscale", F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor)]),
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
]


def bind(path):
    lib = F.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def get_filter(lib, m):
    v = C.c_int(-7)
    assert lib.mlis_option_get(m.ctx, DOWNSCALE_FILTER, C.byref(v)) == 1, m.err()
    return v.value


# ------------------------------------------------------------------ the filters, float64
def _sinc(x):
    return np.sinc(x)           # sin(pi x) / (pi x)


def kernel(filter, x):
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    if filter == 0:
        return ((x > -0.5) & (x <= 0.5)).astype(np.float64)
    if filter == 1:
        return np.where(a < 1, 1 - a, 0.0)
    if filter == 2:
        A = -0.5
        return np.where(a < 1, ((A + 2) * a - (A + 3)) * a * a + 1, np.where(a < 2, (((a - 5) * a + 8) * a - 4) * A, 0.0))
    return np.where(a < 3, _sinc(x) * _sinc(x / 3), 0.0)


def taps(s_in, s_out, filter, wrap=0):
    """(start [s_out], count [s_out], list of float64 weight vectors) of one axis, from the formulas: integer floor divisions for the window, weights normalised
    in float64 (not rounded to fp32)"""
    start, count, ws = [], [], []
    scale = s_in / s_out
    fs = max(scale, 1.0)
    for d in range(s_out):
        mid, half = s_in * (2 * d + 1) + s_out, TWO_SUP[filter] * max(s_in, s_out)
        lo, hi = (mid - half) // (2 * s_out), (mid + half) // (2 * s_out)       # Python's // is the floor
        if not wrap:
            lo, hi = max(lo, 0), min(hi, s_in)
        c = scale * (d + 0.5)
        w = kernel(filter, (np.arange(lo, hi) - c + 0.5) / fs)
        start.append(lo), count.append(hi - lo), ws.append(w / w.sum())
    return np.array(start), np.array(count), ws


def axis_matrix(s_in, s_out, filter, wrap=0):
    """[s_out, s_in] float64: the taps folded into the plane (a wrapped window may pass a source pixel several times)"""
    start, count, ws = taps(s_in, s_out, filter, wrap)
    M = np.zeros((s_out, s_in))
    for d in range(s_out):
        np.add.at(M[d], np.arange(start[d], start[d] + count[d]) % s_in, ws[d])
    return M


def table_matrix(s_in, start, count, w):
    """the same from a table as the library hands it out (start, count, w [s_out][K] fp32), in float64: (M, A), the taps' weights and their magnitudes folded
    into the plane.  A = |M| unless a wrapped window passes a source pixel twice with weights of both signs: the kernel adds those products one by one, so the
    magnitudes its rounding errors scale with are the sum of the |w|, not |sum of the w|."""
    M, A = np.zeros((len(start), s_in)), np.zeros((len(start), s_in))
    for d in range(len(start)):
        j, wd = np.arange(start[d], start[d] + count[d]) % s_in, w[d, :count[d]].astype(np.float64)
        np.add.at(M[d], j, wd)
        np.add.at(A[d], j, np.abs(wd))
    return M, A


def resample64(x, dh, dw, filter, wrap=0):
    """x [..., sh, sw] -> [..., dh, dw] in float64; wrap bit 0 columns, bit 1 rows"""
    x = np.asarray(x, np.float64)
    return axis_matrix(x.shape[-2], dh, filter, wrap & 2) @ x @ axis_matrix(x.shape[-1], dw, filter, wrap & 1).T


# ------------------------------------------------------------------ torch
def torch64(x, dh, dw, filter):
    import torch
    import torch.nn.functional as TF
    x = np.asarray(x, np.float64)
    y = TF.interpolate(torch.from_numpy(x.reshape((-1, 1) + x.shape[-2:])), size=(dh, dw), mode=TORCH_MODES[filter], align_corners=False, antialias=True)
    return y.numpy()[:, 0].reshape(x.shape[:-2] + (dh, dw))


def copies_needed(s_in, s_out, filter):
    """the odd number n of copies of a circular tiling whose (n - 1) / 2 copies on either side cover the widest window's reach beyond the plane"""
    reach = TWO_SUP[filter] / 2 * max(s_in / s_out, 1.0) + 1
    return 2 * max(1, math.ceil(reach / s_in)) + 1


def torch64_wrapped(x, dh, dw, filter, wrap):
    """the middle copy of an n x n circular tiling (along the wrapped axes; an axis that does not wrap is left alone) resampled to n times the size: the same
    scale, and the windows of the middle copy see the plane's periodic continuation.  One axis per call (the filter is separable, torch applies it so itself):
    a single call that shrinks a 10 x 3 plane to 5 x 1 returns its first row in every row with the torch this was written against (2.x, CPU, float64)"""
    x = np.asarray(x, np.float64)
    sh, sw = x.shape[-2:]
    ny = copies_needed(sh, dh, filter) if wrap & 2 else 1
    nx = copies_needed(sw, dw, filter) if wrap & 1 else 1
    y = torch64(torch64(np.tile(x, (ny, nx)), ny * dh, nx * sw, filter), ny * dh, nx * dw, filter)
    return y[..., (ny // 2) * dh:(ny // 2 + 1) * dh, (nx // 2) * dw:(nx // 2 + 1) * dw]
