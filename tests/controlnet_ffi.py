"""What the ControlNet tests share: option ids, prototypes on top of mlis_ffi's table, mirrors of the builder structures, the control-window rule and the
original-layout (cldm.py) tensor names of a ControlNet file."""
import ctypes as C

import mlis_ffi as F

CONTROL_MODEL, CONTROL_IMAGE, CONTROL_STRENGTH, CONTROL_START, CONTROL_END = 131, 132, 133, 134, 135
OPTION_NAMES = {CONTROL_MODEL: "control_model", CONTROL_IMAGE: "control_image", CONTROL_STRENGTH: "control_strength", CONTROL_START: "control_start",
                CONTROL_END: "control_end"}
CONTROL_MAX = 48
pi, pf = C.POINTER(C.c_int), C.POINTER(C.c_float)
c64 = C.c_int64


class ControlState(C.Structure):     # include/mlimgsynth_amd.h
    _fields_ = [("ctx", F.vp), ("par", F.vp), ("lw", F.ci), ("lh", F.ci), ("n_batch", F.ci), ("t_x", F.vp), ("t_t", F.vp), ("t_c", F.vp), ("t_l", F.vp),
                ("t_hint", F.vp), ("n_res", F.ci), ("t_res", F.vp * CONTROL_MAX)]


class UnetControl(C.Structure):      # include/mlimgsynth_amd.h: where a built ControlNet plan leaves its residuals, for unet_denoise_build_ctrl
    _fields_ = [("n", F.ci), ("r", F.vp * CONTROL_MAX), ("ld", c64 * CONTROL_MAX), ("c", F.ci * CONTROL_MAX), ("rows", F.ci * CONTROL_MAX), ("n_img", F.ci), ("gain", F.vp)]


class UnetFreeU(C.Structure):        # the four FreeU factors (device memory) and, out, the concatenations treated per stage
    _fields_ = [("f", F.vp), ("n_stage1", F.ci), ("n_stage2", F.ci)]


PROTOTYPES = [
    ("mlsd_ctrl_add", F.ci, [F.vp, c64, F.vp, c64, F.vp, c64, F.ci, F.ci, F.ci, F.ci, F.vp, F.vp]),
    ("mlsd_window_gather_nhwc", F.ci, [F.vp, F.ci, F.ci, F.ci, F.vp, F.ci, F.ci, pi, pi, F.ci, F.ci, F.vp]),
    ("mlis_amd_control_active", F.ci, [F.ci, F.ci, F.cf, F.cf]),
    ("mlis_amd_set_control", F.ci, [F.vp, F.cf, F.cf, F.cf]),
    ("mlis_amd_set_control_image", F.ci, [F.vp, pf]),
    ("mlis_amd_control_info", F.ci, [F.vp, pi, pi]),
    ("mlis_amd_ctx_at", F.vp, [F.vp, F.ci]),
    ("mlis_amd_engine_get", F.vp, [F.vp]),
    ("mlis_amd_handoff_retries", F.ci, [F.vp]),
    ("mlctx_handoff_ops", F.ci, [F.vp]),
    ("mlis_amd_control_image_device", F.vp, [F.vp]),
    ("mlis_amd_control_tag", C.c_uint64, [F.vp]),
    ("mlis_amd_control_evals", F.ci, [F.vp, F.ci]),
    ("tnconv_controlnet", F.ci, [F.cs, C.c_char_p, C.c_size_t]),
    ("controlnet_init_nc", F.ci, [C.POINTER(ControlState), F.vp, F.vp, C.c_uint, C.c_uint, C.c_uint, F.ci]),
    ("controlnet_build", F.ci, [C.POINTER(ControlState)]),
    ("control_hint_init", F.ci, [F.vp, F.vp, C.c_uint, C.c_uint, C.POINTER(F.vp)]),
    ("control_hint_build", F.ci, [F.vp, F.vp, F.vp]),
]
# what a test needs to drive the three plans at the context level (tests/plan_audit.py)
PLAN_PROTOTYPES = [
    ("controlnet_control", F.ci, [C.POINTER(ControlState), F.vp, C.POINTER(UnetControl)]),
    ("unet_denoise_build_freeu", F.ci, [F.vp, C.POINTER(UnetControl), C.POINTER(UnetFreeU)]),
    ("mlctx_input_set", F.ci, [F.vp, F.vp, F.vp, C.c_size_t]),
    ("mlctx_output_get", F.ci, [F.vp, F.vp, F.vp, C.c_size_t]),
    ("mlctx_result", F.vp, [F.vp]),
    ("mlctx_compute_checked", F.ci, [F.vp]),
    ("mlctx_tensor_device_f32", F.vp, [F.vp, F.vp, C.POINTER(c64)]),
]
EXPORTS = [p[0] for p in PROTOTYPES] + ["mlis_amd_set_control_image_device", "mlb_controlnet", "mlb_unet_denoise_ctrl", "unet_denoise_build_ctrl", "controlnet_control"]


def bind(path):
    lib = F.bind(path)
    for name, res, args in PROTOTYPES + PLAN_PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def active(i_step, n_step, start, end):
    """the rule of mlis_amd_control_active, in Python floats (doubles): the step's midpoint lies in [start n_step, end n_step)"""
    return float(start) * n_step <= i_step + 0.5 < float(end) * n_step


def tnconv(lib, name):
    out = C.create_string_buffer(600)
    r = lib.tnconv_controlnet(name.encode(), out, 600)
    return r, out.value.decode()


# ------------------------------------------------------------------ original-layout names
_BLOCK = {"norm1": "in_layers.0", "conv1": "in_layers.2", "norm2": "out_layers.0", "conv2": "out_layers.3", "emb_proj": "emb_layers.1",
          "skip_conv": "skip_connection"}
_ATTN = {"q_proj": "to_q", "k_proj": "to_k", "v_proj": "to_v", "out_proj": "to_out.0"}


def original_name(key):
    """engine parameter key "control.<...>" -> the name a cldm.py ControlNet file gives the tensor (without "control_model."); the inverse of the loader's
    mapping, written from the published module layout (openaimodel.py ResBlock / SpatialTransformer / Downsample, cldm.py ControlNet)"""
    assert key.startswith("control.")
    p = key[len("control."):].split(".")
    if p[0] == "hint":
        return "input_hint_block." + ".".join(p[1:])
    if p[0] == "zero":
        return f"zero_convs.{p[1]}.0." + ".".join(p[2:])
    if p[0] == "mid_out":
        return "middle_block_out.0." + ".".join(p[1:])
    if p[0] == "time_embed":
        return ".".join(p)
    if p[0] == "label_embed":
        return "label_emb.0." + ".".join(p[1:])
    if p[0] == "in" and p[1] == "conv":
        return "input_blocks.0.0." + ".".join(p[2:])
    if p[0] == "in":
        head, rest = f"input_blocks.{p[1]}.{p[2]}", p[3:]
    else:
        assert p[0] == "mid", key
        head, rest = f"middle_block.{p[1]}", p[2:]
    if rest[0] in _BLOCK:
        return ".".join([head, _BLOCK[rest[0]]] + rest[1:])
    if rest[0] == "conv":                                   # Downsample
        return ".".join([head, "op"] + rest[1:])
    if rest[0] == "transf":
        q = ["transformer_blocks", rest[1]] + rest[2:]
        if q[2] in ("attn1", "attn2"):
            q[3] = _ATTN[q[3]]
        return ".".join([head] + q)
    return ".".join([head] + rest)                          # norm, proj_in, proj_out
