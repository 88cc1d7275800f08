"""What the upscaler tests share: the prototypes and option ids of the ESRGAN upscaler on top of mlis_ffi's table, and the driver (mlis_amd_upscaler_*) behind it."""
import ctypes as C

import numpy as np

import mlis_ffi as F

UPSCALE_MODEL, HIRES_USE_MODEL = 151, 152
OPTION_NAMES = {UPSCALE_MODEL: "upscale_model", HIRES_USE_MODEL: "hires_use_model"}
PROTOTYPES = [
    ("mlis_amd_tensor_upscale", F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor)]),
    ("mlis_amd_upscaler_builds", F.ci, [F.vp, C.POINTER(F.ci)]),
    ("mlis_amd_tensor_resample", F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor), F.ci, F.ci, F.ci]),
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
    ("mlis_amd_upscaler_create", F.vp, [F.cs]),
    ("mlis_amd_upscaler_destroy", None, [F.vp]),
    ("mlis_amd_upscaler_info", F.ci, [F.vp, C.POINTER(F.ci), C.POINTER(F.ci)]),
    ("mlis_amd_upscaler_run", F.ci, [F.vp, C.POINTER(F.cf), F.ci, F.ci, F.ci, C.POINTER(F.cf)]),
    ("mlsd_last_error", F.cs, []),
    ("mlsd_runtime_dry", None, [F.ci]),
]


def bind(path):
    lib = F.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def as_tensor(x):
    """planar float32 [n, c, h, w] -> MLIS_Tensor view (the array must stay alive)"""
    n, c, h, w = x.shape
    return F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, n), 0)


class Upscaler:
    """the driver, outside any context"""

    def __init__(self, lib, spec):
        self.lib = lib
        self.h = lib.mlis_amd_upscaler_create(spec.encode())
        if not self.h:
            raise RuntimeError(lib.mlsd_last_error().decode())

    def n_block(self):
        nb, sc = F.ci(), F.ci()
        assert self.lib.mlis_amd_upscaler_info(self.h, C.byref(nb), C.byref(sc)) == 1 and sc.value == 4
        return nb.value

    def run(self, x):
        x = np.ascontiguousarray(x, np.float32)
        n, c, h, w = x.shape
        assert c == 3
        out = np.empty((n, 3, 4 * h, 4 * w), np.float32)
        r = self.lib.mlis_amd_upscaler_run(self.h, x.ctypes.data_as(C.POINTER(C.c_float)), w, h, n, out.ctypes.data_as(C.POINTER(C.c_float)))
        if r < 0:
            raise RuntimeError(self.lib.mlsd_last_error().decode())
        return out

    def close(self):
        if self.h:
            self.lib.mlis_amd_upscaler_destroy(self.h)
            self.h = None
