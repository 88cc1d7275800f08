"""What the Canny tests share: option ids and prototypes on top of controlnet_ffi's table."""
import ctypes as C

import controlnet_ffi as CF
import mlis_ffi as F

CONTROL_PREPROCESS, CANNY_LOW, CANNY_HIGH, CANNY_L2 = 171, 172, 173, 174
OPTION_NAMES = {CONTROL_PREPROCESS: "control_preprocess", CANNY_LOW: "canny_low", CANNY_HIGH: "canny_high", CANNY_L2: "canny_l2"}
PREPROCESS_NONE, PREPROCESS_CANNY, PREPROCESS_INVERT = 0, 1, 2
TP = C.POINTER(F.Tensor)

PROTOTYPES = [
    ("mlsd_canny_ws_bytes", C.c_size_t, [F.ci, F.ci]),
    ("mlsd_canny", F.ci, [F.vp, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp, F.ci, F.vp, CF.pi, F.vp]),
    ("mlsd_canny_thresholds", F.ci, [C.c_double, C.c_double, F.ci, CF.pi, CF.pi]),
    ("mlsd_canny_tile", F.ci, [F.ci]),
    ("mlsd_invert", F.ci, [F.vp, F.vp, C.c_int64, F.vp]),
    ("mlis_amd_tensor_canny", F.ci, [F.vp, TP, TP, F.cf, F.cf, F.ci, F.ci]),
    ("mlis_amd_tensor_resample", F.ci, [F.vp, TP, TP, F.ci, F.ci, F.ci]),
    ("mlis_amd_tensor_resample_aa", F.ci, [F.vp, TP, TP, F.ci, F.ci, F.ci]),
    ("mlis_amd_control_image_get", F.ci, [F.vp, CF.pf, CF.pi, CF.pi]),
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
]
EXPORTS = [p[0] for p in PROTOTYPES]


def bind(path):
    lib = CF.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def tile(lib):
    """the kernels' tiles: (classify x, classify y, sweep x, sweep y)"""
    return tuple(lib.mlsd_canny_tile(i) for i in range(4))
