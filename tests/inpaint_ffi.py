"""What the inpainting tests share: option ids and prototypes on top of canny_ffi's table."""
import ctypes as C

import numpy as np

import canny_ffi as CN
import controlnet_ffi as CF
import mlis_ffi as F

INPAINT_AREA, INPAINT_PADDING, MASK_BLUR, MASK_GROW, MASK_INVERT, INPAINT_COMPOSITE = 181, 182, 183, 184, 185, 186
OPTION_NAMES = {INPAINT_AREA: "inpaint_area", INPAINT_PADDING: "inpaint_padding", MASK_BLUR: "mask_blur", MASK_GROW: "mask_grow", MASK_INVERT: "mask_invert",
                INPAINT_COMPOSITE: "inpaint_composite"}
GAUSS_MAX_TAPS = 321
TP = C.POINTER(F.Tensor)

PROTOTYPES = [
    ("mlsd_mask_weight", F.ci, [F.vp, F.vp, C.c_int64, F.ci, F.vp]),
    ("mlsd_mask_grow", F.ci, [F.vp, F.vp, F.ci, F.ci, F.ci, F.ci, F.vp, F.vp]),
    ("mlsd_gauss_taps", F.ci, [F.cf, CF.pf, F.ci]),
    ("mlsd_gauss_blur_ws_bytes", C.c_size_t, [F.ci, F.ci, F.ci]),
    ("mlsd_gauss_blur", F.ci, [F.vp, F.vp, F.ci, F.ci, F.ci, F.cf, F.ci, F.vp, F.vp]),
    ("mlsd_gauss_blur_lds_limit", F.ci, [F.ci]),
    ("mlsd_mask_bbox", F.ci, [F.vp, F.ci, F.ci, F.vp, F.vp]),
    ("mlsd_composite", F.ci, [F.vp, F.vp, F.ci, F.vp, F.vp, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp]),
    ("mlis_amd_tensor_mask_weight", F.ci, [F.vp, TP, TP, F.ci]),
    ("mlis_amd_tensor_mask_grow", F.ci, [F.vp, TP, TP, F.ci, F.ci]),
    ("mlis_amd_tensor_gauss_blur", F.ci, [F.vp, TP, TP, F.cf, F.ci]),
    ("mlis_amd_tensor_mask_bbox", F.ci, [F.vp, TP, CF.pi]),
    ("mlis_amd_tensor_composite", F.ci, [F.vp, TP, TP, TP, TP, F.ci, F.ci]),
    ("mlis_amd_inpaint_region", F.ci, [F.ci, F.ci, CF.pi, F.ci, F.ci, F.ci, CF.pi]),
    ("mlis_amd_inpaint_info", F.ci, [F.vp, CF.pi, CF.pi]),
]
EXPORTS = [p[0] for p in PROTOTYPES]


def bind(path):
    lib = CN.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def taps(lib, sigma, k_max=GAUSS_MAX_TAPS):
    """the library's float taps of sigma as a float32 array, or None when refused"""
    w = np.zeros(max(k_max, 1), np.float32)
    n = lib.mlsd_gauss_taps(sigma, w.ctypes.data_as(CF.pf), k_max)
    return None if n < 0 else w[:n].copy()


def region(lib, W, H, box, padding, tw, th):
    b, out = (C.c_int * 4)(*box), (C.c_int * 4)()
    r = lib.mlis_amd_inpaint_region(W, H, b, padding, tw, th, out)
    return None if r < 0 else tuple(out)


def as_tensor(x):
    """float32 [b][c][h][w], C-contiguous, as an MLIS_Tensor over the same memory"""
    b, c, h, w = x.shape
    return F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, b), 0)


def call_tensor(lib, m, fn, x, *args):
    """fn(ctx, src, dst, *args) on a float32 [b][c][h][w] array; the result as an array"""
    x = np.ascontiguousarray(x, np.float32)
    out = F.Tensor()
    assert fn(m.ctx, C.byref(as_tensor(x)), C.byref(out), *args) == 1, m.err()
    got = F.tensor_np(out)
    lib.mlis_tensor_free(C.byref(out))
    return got


def bbox(lib, m, p):
    p = np.ascontiguousarray(p, np.float32)
    box = (C.c_int * 4)()
    assert lib.mlis_amd_tensor_mask_bbox(m.ctx, C.byref(as_tensor(p)), box) == 1, m.err()
    return tuple(box)


def composite(lib, m, orig, patch, p, x0, y0):
    orig, patch, p = (np.ascontiguousarray(a, np.float32) for a in (orig, patch, p))
    out = F.Tensor()
    assert lib.mlis_amd_tensor_composite(m.ctx, C.byref(out), C.byref(as_tensor(orig)), C.byref(as_tensor(patch)), C.byref(as_tensor(p)), x0, y0) == 1, m.err()
    got = F.tensor_np(out)
    lib.mlis_tensor_free(C.byref(out))
    return got
