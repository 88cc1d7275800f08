"""What the packed tiled-diffusion tests share: the option id and the prototypes on top of unet_tile_ffi's, and a numpy restatement of the pack
rule -- how many windows one plan evaluation takes, how many evaluations that makes, and which windows each group holds."""
import ctypes as C

import mlis_ffi as F
import unet_tile_ffi as U

UNET_TILE_BATCH = 121
OPTION_NAMES = {UNET_TILE_BATCH: "unet_tile_batch"}
MAX_PACK, MAX_BATCH = 16, 64
pi = C.POINTER(C.c_int)
PROTOTYPES = [
    ("mlis_amd_tile_pack", F.ci, [F.ci, F.ci, F.ci, pi]),
    ("mlis_amd_tile_pack_info", F.ci, [F.vp, pi, pi]),
    ("mlsd_window_gather_packed", F.ci, [F.vp, F.ci, F.ci, F.vp, F.ci, F.ci, pi, pi, F.ci, F.ci, F.vp]),
    ("mlsd_window_blend_packed", F.ci, [F.vp, C.c_int64, F.vp, F.vp, F.ci, F.ci, F.ci, F.ci, pi, pi, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp]),
]
EXPORTS = [p[0] for p in PROTOTYPES] + ["mlis_amd_create_tiled_packed", "mlis_amd_create_tiled", "mlsd_window_gather", "mlsd_window_blend", "mlsd_window_wsum"]


def bind(path):
    lib = U.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def ints(v):
    return (C.c_int * max(len(v), 1))(*v)


def c_pack(lib, n_win, B, pack):
    """(P, n_eval) of the library, or None where it refuses"""
    n_eval = C.c_int(-7)
    p = lib.mlis_amd_tile_pack(n_win, B, pack, C.byref(n_eval))
    return None if p < 0 else (p, n_eval.value)


# ------------------------------------------------------------------ numpy restatement
def pack_rule(n_win, B, pack):
    """the rule of the issue, in Python integers: (P, n_eval, P0)"""
    p0 = min(pack, n_win, MAX_PACK, MAX_BATCH // B)
    n_eval = -(-n_win // p0)
    return -(-n_win // n_eval), n_eval, p0


def groups(n_win, B, pack):
    """[(slots, n_used)] per plan evaluation: slots are window indices in evaluation order, P of them; the unused slots of the short last group repeat
    its last window"""
    P, n_eval, _ = pack_rule(n_win, B, pack)
    out = []
    for g in range(n_eval):
        used = list(range(g * P, min((g + 1) * P, n_win)))
        out.append((used + [used[-1]] * (P - len(used)), len(used)))
    return out
