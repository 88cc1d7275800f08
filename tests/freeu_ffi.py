"""What the FreeU tests share: option ids and prototypes on top of controlnet_ffi's table."""
import ctypes as C

import controlnet_ffi as CF
import mlis_ffi as F

FREEU, FREEU_B1, FREEU_B2, FREEU_S1, FREEU_S2 = 141, 142, 143, 144, 145
OPTION_NAMES = {FREEU: "freeu", FREEU_B1: "freeu_b1", FREEU_B2: "freeu_b2", FREEU_S1: "freeu_s1", FREEU_S2: "freeu_s2"}
DEFAULTS = {FREEU_B1: 1.3, FREEU_B2: 1.4, FREEU_S1: 0.9, FREEU_S2: 0.2}
CONTROL_NET, CONTROL_FREEU = 1, 2
c64 = C.c_int64

PROTOTYPES = [
    ("mlsd_freeu_backbone", F.ci, [F.vp, c64, F.vp, c64, F.ci, F.ci, F.ci, F.vp, F.vp, F.vp]),
    ("mlsd_freeu_skip", F.ci, [F.vp, c64, F.vp, c64, F.ci, F.ci, F.ci, F.ci, F.vp, F.vp, F.vp]),
    ("mlsd_freeu_ws_bytes", C.c_size_t, [F.ci, F.ci, F.ci, F.ci]),
    ("mlsd_freeu_depth", F.ci, [F.ci]),
    ("mlis_amd_set_freeu", F.ci, [F.vp, F.cf, F.cf, F.cf, F.cf]),
    ("mlis_amd_freeu_info", F.ci, [F.vp, CF.pi, CF.pi]),
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
]
EXPORTS = [p[0] for p in PROTOTYPES] + ["mlb_unet_denoise_freeu", "unet_denoise_build_freeu"]


def bind(path):
    lib = CF.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib
