"""Python interface of libmlimgsynth on MI355X -- the counterpart of the reference's python/mlimgsynth.py.

Same surface: the MLIS_* constants, MLIS_Image / MLIS_Tensor (with .similarity) and the class MLImgSynth with
option_set / setup / generate / image_get / infotext_get / errstr_get / clip_text_encode (python/mlimgsynth.py:213-296),
so a script written against the reference imports this module instead and runs unchanged:

    from mlimgsynth_amd.mlimgsynth import *        # was: from mlimgsynth import *

plus the functions the reference wrapper lists as "TODO: all functions": tensor_get, option_get, text_tokenize,
image_encode / image_decode / mask_encode, callbacks, and numpy views of images and tensors.

The library is found like the reference does (environment MLIS_LIB_PATH first), falling back to the in-tree build
mlimgsynth_amd/lib/libmlimgsynth_amd.so.  It is loaded on first use, not at import, and there is no CPU fallback.
"""
import ctypes
import math
import os
import sys

MLIS_VERSION = 0x000402
MLIS_VERSION_STR = "0.4.2"


def _define(prefix, names, start=0, explicit=None):
    g = globals()
    for i, n in enumerate(names):
        g[prefix + n] = start + i
    for n, v in (explicit or {}).items():
        g[prefix + n] = v


# enumerations of include/mlimgsynth.h (values are ABI)
_define("MLIS_E_", [], explicit=dict(UNKNOWN=-1, VERSION=-2, UNK_OPT=-3, OPT_VALUE=-4, PROMPT_PARSE=-5, FILE_NOT_FOUND=-6, NAN=-7, IMAGE=-8))
_define("MLIS_STAGE_", ["IDLE", "COND_ENCODE", "IMAGE_ENCODE", "IMAGE_DECODE", "DENOISE"])
_define("MLIS_METHOD_", ["NONE", "EULER", "HEUN", "TAYLOR3", "DPMPP2M", "DPMPP2S"], explicit=dict(_LAST=5))
_define("MLIS_SCHED_", ["NONE", "UNIFORM", "KARRAS"], explicit=dict(_LAST=2))
_define("MLIS_LOGLVL_", [], explicit=dict(NONE=0, ERROR=10, WARNING=20, INFO=30, VERBOSE=40, DEBUG=50, MAX=255, _INCREASE=0x100 | 10, _DECREASE=0x200 | 10))
_define("MLIS_TENSOR_", ["IMAGE", "MASK", "LATENT", "LMASK", "COND", "LABEL", "NCOND", "NLABEL"], start=1, explicit=dict(TMP=0x100))
_define("MLIS_TUF_", [], explicit=dict(IMAGE=1, MASK=2, LATENT=4, LMASK=8, CONDITIONING=16))
_define("MLIS_MODEL_TYPE_", ["NONE", "SD1", "SD2", "SDXL"], explicit=dict(_LAST=3))
_define("MLIS_MODEL_", ["NONE", "UNET", "VAE", "TAE", "CLIP", "CLIP2"])
_define("MLIS_OPT_", ["NONE", "BACKEND", "MODEL", "TAE", "LORA_DIR", "LORA", "LORA_CLEAR", "PROMPT", "NPROMPT", "IMAGE_DIM", "BATCH_SIZE",
                      "CLIP_SKIP", "CFG_SCALE", "METHOD", "SCHEDULER", "STEPS", "F_T_INI", "F_T_END", "S_NOISE", "S_ANCESTRAL", "IMAGE",
                      "IMAGE_MASK", "NO_DECODE", "TENSOR_USE_FLAGS", "SEED", "VAE_TILE", "UNET_SPLIT", "THREADS", "DUMP_FLAGS", "AUX_DIR",
                      "CALLBACK", "ERROR_HANDLER", "LOG_LEVEL", "MODEL_TYPE", "WEIGHT_TYPE", "NO_PROMPT_PARSE"], explicit=dict(_LAST=35, AMD_TILING=101, AMD_HIRES_SCALE=102, AMD_HIRES_DENOISE=103,
                                                                            AMD_HIRES_STEPS=104, AMD_HIRES_UPSCALER=105, AMD_UNET_TILE=111,
                                                                           AMD_UNET_TILE_OVERLAP=112, AMD_UNET_TILE_BATCH=121, AMD_CONTROL_MODEL=131, AMD_CONTROL_IMAGE=132,
                                                                           AMD_CONTROL_STRENGTH=133, AMD_CONTROL_START=134, AMD_CONTROL_END=135, AMD_FREEU=141,
                                                                           AMD_FREEU_B1=142, AMD_FREEU_B2=143, AMD_FREEU_S1=144, AMD_FREEU_S2=145,
                                                                           AMD_UPSCALE_MODEL=151, AMD_HIRES_USE_MODEL=152, AMD_DOWNSCALE_FILTER=161,
                                                                           AMD_CONTROL_PREPROCESS=171, AMD_CANNY_LOW=172, AMD_CANNY_HIGH=173, AMD_CANNY_L2=174,
                                                                           AMD_INPAINT_AREA=181, AMD_INPAINT_PADDING=182, AMD_MASK_BLUR=183, AMD_MASK_GROW=184,
                                                                           AMD_MASK_INVERT=185, AMD_INPAINT_COMPOSITE=186, AMD_HYPERTILE=191, AMD_HYPERTILE_DEPTH=192, AMD_PAG_SCALE=201,
                                                                           AMD_CFG_RESCALE=211, AMD_PREDICTION=212, AMD_ZSNR=213))
_define("MLIS_AMD_RESAMPLE_", ["NEAREST", "BILINEAR", "BICUBIC"])
_define("MLIS_AMD_AA_", ["BOX", "TRIANGLE", "CUBIC", "LANCZOS"])
_define("MLIS_AMD_PREPROCESS_", ["NONE", "CANNY", "INVERT"])
_define("MLIS_AMD_INPAINT_", ["WHOLE", "MASKED"])
MLIS_CTEF_NO_NORM = 1


class MLIS_Image_C(ctypes.Structure):          # MLIS_Image, include/mlimgsynth.h:366-373
    _fields_ = [("d", ctypes.POINTER(ctypes.c_uint8)), ("sz", ctypes.c_size_t), ("w", ctypes.c_int), ("h", ctypes.c_int),
                ("c", ctypes.c_int), ("flags", ctypes.c_int)]


class MLIS_Tensor_C(ctypes.Structure):         # MLIS_Tensor, include/mlimgsynth.h:409-413
    _fields_ = [("d", ctypes.POINTER(ctypes.c_float)), ("n", ctypes.c_int * 4), ("flags", ctypes.c_int)]


class MLIS_Progress_C(ctypes.Structure):       # MLIS_Progress, include/mlimgsynth.h:377-384
    _fields_ = [("stage", ctypes.c_int), ("step", ctypes.c_int), ("step_end", ctypes.c_int), ("nfe", ctypes.c_int),
                ("step_time", ctypes.c_double), ("time", ctypes.c_double)]


MLIS_Callback = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(MLIS_Progress_C))

_V, _I, _F, _S = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_char_p
_TP, _IP = ctypes.POINTER(MLIS_Tensor_C), ctypes.POINTER(MLIS_Image_C)
_PROTOTYPES = {
    "mlis_ctx_create_i": (_V, [_I]), "mlis_ctx_destroy": (None, [ctypes.POINTER(_V)]), "mlis_errstr_get": (_S, [_V]),
    "mlis_option_set": (_I, [_V, _I]), "mlis_option_set_str": (_I, [_V, _S, _S]), "mlis_option_get": (_I, [_V, _I]),
    "mlis_setup": (_I, [_V]), "mlis_generate": (_I, [_V]), "mlis_image_get": (_IP, [_V, _I]), "mlis_infotext_get": (_S, [_V, _I]),
    "mlis_tensor_get": (_TP, [_V, _I]), "mlis_clip_text_encode": (_I, [_V, _S, _TP, _TP, _I, _I]),
    "mlis_tensor_similarity": (_F, [_TP, _TP]), "mlis_image_encode": (_I, [_V, _TP, _TP, _I]), "mlis_image_decode": (_I, [_V, _TP, _TP, _I]),
    "mlis_mask_encode": (_I, [_V, _TP, _TP, _I]), "mlis_text_tokenize": (_I, [_V, _S, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), _I]),
    "mlis_tensor_resize": (None, [_TP, _I, _I, _I, _I]), "mlis_tensor_free": (None, [_TP]),
    "mlis_amd_tensor_resample": (_I, [_V, _TP, _TP, _I, _I, _I]), "mlis_amd_engine_builds": (_I, [_V]),
    "mlis_amd_tensor_resample_aa": (_I, [_V, _TP, _TP, _I, _I, _I]),
    "mlis_amd_lora_stats": (_I, [_V, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "mlis_amd_tensor_canny": (_I, [_V, _TP, _TP, _F, _F, _I, _I]),
    "mlis_amd_tensor_mask_weight": (_I, [_V, _TP, _TP, _I]), "mlis_amd_tensor_mask_grow": (_I, [_V, _TP, _TP, _I, _I]),
    "mlis_amd_tensor_gauss_blur": (_I, [_V, _TP, _TP, _F, _I]), "mlis_amd_tensor_mask_bbox": (_I, [_V, _TP, ctypes.POINTER(_I)]),
    "mlis_amd_tensor_composite": (_I, [_V, _TP, _TP, _TP, _TP, _I, _I]),
    "mlis_amd_inpaint_region": (_I, [_I, _I, ctypes.POINTER(_I), _I, _I, _I, ctypes.POINTER(_I)]),
    "mlis_amd_inpaint_info": (_I, [_V, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "mlis_amd_prompt_tokens_set": (_I, [_V, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_F), _I, _I]),
    "mlis_amd_engine_get": (_V, [_V]), "mlis_amd_hypertile_info": (_I, [_V, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "mlis_amd_pag_info": (_I, [_V, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "mlis_amd_tensor_upscale": (_I, [_V, _TP, _TP]), "mlis_amd_upscaler_builds": (_I, [_V, ctypes.POINTER(_I)]),
}

mlis_lib = None
mlis_lib_path = None


def _find_library():
    p = os.getenv("MLIS_LIB_PATH", None)
    if p:
        return p
    here = os.path.dirname(os.path.abspath(__file__))
    for cand in (os.path.join(here, "lib", "libmlimgsynth_amd.so"), "libmlimgsynth_amd.so", os.path.join("lib", "libmlimgsynth_amd.so")):
        if os.path.exists(cand):
            return cand
    raise RuntimeError("libmlimgsynth_amd.so not found: build it (python -c 'import __graft_entry__ as g; g.build()') or set MLIS_LIB_PATH")


def load_library(path=None):
    """Load the shared library (once).  Raises instead of falling back to anything else."""
    global mlis_lib, mlis_lib_path
    if mlis_lib is not None and path in (None, mlis_lib_path):
        return mlis_lib
    mlis_lib_path = path or _find_library()
    lib = ctypes.CDLL(mlis_lib_path, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _PROTOTYPES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    mlis_lib = lib
    return lib


class MLIS_Image:
    def __init__(self, cimg):
        self.data = ctypes.string_at(cimg.d, cimg.sz)  # bytes, RGB
        self.w, self.h, self.c = int(cimg.w), int(cimg.h), int(cimg.c)

    def numpy(self):
        import numpy as np
        return np.frombuffer(self.data, np.uint8).reshape(self.h, self.w, self.c)


class MLIS_Tensor:
    def __init__(self, cten):
        self.n = tuple(int(x) for x in cten.n)
        self.data = ctypes.string_at(cten.d, self.n[0] * self.n[1] * self.n[2] * self.n[3] * 4)  # bytes, float32

    def _c(self):
        buf = ctypes.cast(ctypes.c_char_p(self.data), ctypes.POINTER(ctypes.c_float))
        return MLIS_Tensor_C(buf, (ctypes.c_int * 4)(*self.n), 0)

    def similarity(self, other):
        a, b = self._c(), other._c()
        return float(load_library().mlis_tensor_similarity(ctypes.byref(a), ctypes.byref(b)))

    def numpy(self):
        import numpy as np
        return np.frombuffer(self.data, np.float32).reshape(self.n[3], self.n[2], self.n[1], self.n[0])


class MLImgSynth:
    def __init__(self, lib_path=None):
        self._lib = load_library(lib_path)
        self._ctx = self._lib.mlis_ctx_create_i(MLIS_VERSION)
        if not self._ctx:
            raise RuntimeError("Failed to create MLIS context")
        self._keep = []          # callback thunks must outlive the context

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.mlis_ctx_destroy(ctypes.byref(ctypes.c_void_p(self._ctx)))
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- options
    def option_set(self, option, *args):
        if isinstance(option, str):
            r = self._lib.mlis_option_set_str(self._ctx, option.encode("utf8"), ",".join(str(x) for x in args).encode("utf8"))
        elif isinstance(option, int):
            conv = []
            for a in args:             # C default argument promotions of the variadic mlis_option_set
                conv.append(ctypes.c_double(a) if isinstance(a, float) else ctypes.c_char_p(a.encode("utf8")) if isinstance(a, str) else a)
            self._keep.extend(c for c in conv if isinstance(c, ctypes.c_char_p))
            r = self._lib.mlis_option_set(self._ctx, option, *conv)
        else:
            raise RuntimeError("'option' must be str or int")
        if r < 0:
            raise RuntimeError("Failed to set option '%s': %s" % (option, self.errstr_get()))
        return r

    def option_get(self, option, out):
        """out: a ctypes object receiving the value: c_int for int, bool and enum options, c_float for float options, c_char_p for
        string options.  mlis_option_get serves MODEL, MODEL_TYPE, PROMPT and NPROMPT, as in the reference, and every MLIS_OPT_AMD_* option
        (AMD_CONTROL_IMAGE gives a c_int: whether an image is set)."""
        r = self._lib.mlis_option_get(self._ctx, option, ctypes.byref(out))
        if r < 0:
            raise RuntimeError("Failed to get option %s: %s" % (option, self.errstr_get()))
        return r

    def callback_set(self, fn, user=None):
        """fn(progress) -> int (>= 0 continue, < 0 abort with that code); progress has stage / step / step_end / nfe / step_time / time."""
        thunk = MLIS_Callback(lambda ud, ctx, p: int(fn(p.contents) or 0))
        self._keep.append(thunk)
        if self._lib.mlis_option_set(self._ctx, MLIS_OPT_CALLBACK, thunk, ctypes.c_void_p(user)) < 0:   # noqa: F821
            raise RuntimeError("Failed to set the callback: %s" % self.errstr_get())

    # ---- life cycle
    def setup(self):
        "Set up the backend and model. Optional."
        if self._lib.mlis_setup(self._ctx) < 0:
            raise RuntimeError("Failed to setup: %s" % (self.errstr_get()))

    def generate(self):
        "Generate images."
        r = self._lib.mlis_generate(self._ctx)
        if r < 0:
            raise RuntimeError("Failed to generate image: %s" % (self.errstr_get()))
        return r

    def image_get(self, idx=0):
        "Get generated images data."
        p = self._lib.mlis_image_get(self._ctx, idx)
        if not p:
            raise RuntimeError("Failed to get image %d" % idx)
        return MLIS_Image(p.contents)

    def tensor_get(self, tensor_id):
        "Copy of one of the library's tensors (MLIS_TENSOR_*)."
        p = self._lib.mlis_tensor_get(self._ctx, tensor_id)
        if not p or not p.contents.d:
            raise RuntimeError("Failed to get tensor %d" % tensor_id)
        return MLIS_Tensor(p.contents)

    def infotext_get(self, idx=0):
        "Get text describing the generation parameters."
        info = self._lib.mlis_infotext_get(self._ctx, idx)
        if info is None:
            raise RuntimeError("Failed to get infotext %d" % idx)
        return info.decode("utf8")

    def errstr_get(self):
        "Return an string describing the last error."
        e = self._lib.mlis_errstr_get(self._ctx)
        return e.decode("utf8") if e is not None else None

    # ---- direct use of the sub-models
    def clip_text_encode(self, text, features=False, no_norm=True, model_idx=4):
        t_embed = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP)               # noqa: F821
        t_feat = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 1) if features else None   # noqa: F821
        r = self._lib.mlis_clip_text_encode(self._ctx, text.encode("utf8"), t_embed, t_feat, model_idx, MLIS_CTEF_NO_NORM if no_norm else 0)
        if r < 0:
            raise RuntimeError("Failed to encode text with CLIP: %s" % (self.errstr_get()))
        embed = MLIS_Tensor(t_embed.contents)
        return (embed, MLIS_Tensor(t_feat.contents)) if features else embed

    def text_tokenize(self, text, model_idx=4):
        ptr = ctypes.POINTER(ctypes.c_int32)()
        n = self._lib.mlis_text_tokenize(self._ctx, text.encode("utf8"), ctypes.byref(ptr), model_idx)
        if n < 0:
            raise RuntimeError("Failed to tokenize: %s" % self.errstr_get())
        return [int(ptr[i]) for i in range(n)]

    def _transform(self, fn, what, src, flags):
        tin = src._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if fn(self._ctx, ctypes.byref(tin), tout, flags) < 0:
            raise RuntimeError("Failed to %s: %s" % (what, self.errstr_get()))
        return MLIS_Tensor(tout.contents)

    def image_encode(self, image, flags=0):
        "VAE-encode an image tensor [1,3,H,W] in [0,1] into a latent."
        return self._transform(self._lib.mlis_image_encode, "encode the image", image, flags)

    def image_decode(self, latent, flags=0):
        "VAE-decode a latent into an image tensor in [0,1]."
        return self._transform(self._lib.mlis_image_decode, "decode the latent", latent, flags)

    def mask_encode(self, mask, flags=0):
        "Reduce a pixel mask to latent resolution."
        return self._transform(self._lib.mlis_mask_encode, "encode the mask", mask, flags)

    # ---- hires fix
    def hires_set(self, scale, denoise=None, steps=None, upscaler=None, use_model=None):
        """Two-pass generation: scale 0 or 1 switches it off, else 1 < scale <= 4; denoise in (0, 1] is the second pass's strength,
        steps its step count (0 = the STEPS value), upscaler 'nearest' | 'bilinear' | 'bicubic'; use_model True: the first pass is decoded and
        upscaled 4x by the "upscale_model" option's ESRGAN model, then resampled to the target size in the `upscaler` mode.  The options persist."""
        self.option_set("hires_scale", scale)
        if denoise is not None:
            self.option_set("hires_denoise", denoise)
        if steps is not None:
            self.option_set("hires_steps", steps)
        if upscaler is not None:
            self.option_set("hires_upscaler", upscaler)
        if use_model is not None:
            self.option_set("hires_use_model", 1 if use_model else 0)

    # ---- tiled diffusion
    def unet_tile_set(self, tile, overlap=None, batch=None):
        """Tiled diffusion: a pass larger than `tile` pixels on an axis evaluates the UNet in overlapping windows of that size and blends them
        (0 = off).  overlap: minimum overlap of neighbouring windows in pixels, a multiple of 8 with 2 x overlap <= tile; None keeps the
        current setting (auto = a quarter of the tile unless set), -1 goes back to auto.  batch: at most this many windows (1 .. 16) run as one
        batched UNet evaluation, at the activation memory of a plan for that many windows; None keeps the current setting.  The options persist."""
        self.option_set("unet_tile", tile)
        if overlap is not None:
            self.option_set("unet_tile_overlap", overlap)
        if batch is not None:
            self.option_set("unet_tile_batch", batch)

    # ---- ControlNet
    def control_set(self, model=None, image=None, strength=None, start=None, end=None, preprocess=None, canny_low=None, canny_high=None, canny_l2=None):
        """ControlNet: model = path of a safetensors ControlNet for the base model ("synth[:seed]" with a synth: model, "" = off); image = the control
        map, a uint8 array [h][w][3] of any size (it is resampled to each pass's size) or False to clear it; strength in [0, 2]; start / end: the share of the
        steps that is controlled; preprocess = 'none' (the image is the finished map) | 'canny' | 'invert', run on the GPU after the resample, at each pass's own
        size; canny_low / canny_high = its thresholds in 0 .. 32767 (100, 200), canny_l2 = True for the Euclidean gradient magnitude.  None keeps a setting.
        The options persist across generations."""
        if model is not None:
            self.option_set("control_model", model)
        if image is False:
            r = self._lib.mlis_option_set(self._ctx, MLIS_OPT_AMD_CONTROL_IMAGE, ctypes.c_void_p(None))     # noqa: F821
            if r < 0:
                raise RuntimeError("Failed to clear the control image: %s" % self.errstr_get())
        elif image is not None:
            import numpy as np
            a = np.ascontiguousarray(image, np.uint8)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("control image must be uint8 [h][w][3]")
            img = MLIS_Image_C(a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), a.size, a.shape[1], a.shape[0], 3, 0)
            if self._lib.mlis_option_set(self._ctx, MLIS_OPT_AMD_CONTROL_IMAGE, ctypes.byref(img)) < 0:     # noqa: F821  (the library copies the pixels)
                raise RuntimeError("Failed to set the control image: %s" % self.errstr_get())
        for name, v in (("control_strength", strength), ("control_start", start), ("control_end", end), ("control_preprocess", preprocess),
                        ("canny_low", canny_low), ("canny_high", canny_high)):
            if v is not None:
                self.option_set(name, v)
        if canny_l2 is not None:
            self.option_set("canny_l2", 1 if canny_l2 else 0)

    def canny(self, image, low=100, high=200, l2=False, wrap=0):
        """Canny edge map on the GPU (OpenCV's Canny(img_u8, low, high) with aperture 3 as recalled; the rules are in mlsd_kernels.h).  image: an MLIS_Tensor
        [1,c,h,w] in [0,1] or a uint8 array [h][w] / [h][w][c], c = 1 or 3.  Returns an MLIS_Tensor [1,3,h,w]: 1 on edges, 0 elsewhere.  wrap: bit 0 columns,
        bit 1 rows wrap around.  Needs no model."""
        if not isinstance(image, MLIS_Tensor):
            import numpy as np
            a = np.asarray(image)
            if a.dtype != np.uint8 or a.ndim not in (2, 3):
                raise ValueError("canny takes an MLIS_Tensor or a uint8 array [h][w] or [h][w][c]")
            a = a[:, :, None] if a.ndim == 2 else a
            image = tensor_from_numpy((a.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None])
        tin = image._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if self._lib.mlis_amd_tensor_canny(self._ctx, ctypes.byref(tin), tout, float(low), float(high), 1 if l2 else 0, int(wrap)) < 0:
            raise RuntimeError("Failed to run canny: %s" % self.errstr_get())
        return MLIS_Tensor(tout.contents)

    # ---- region inpainting
    def inpaint_set(self, area=None, padding=None, mask_blur=None, mask_grow=None, invert=None, composite=None):
        """Region inpainting: area = 'whole' | 'masked' (masked: only the padded, aspect-fitted bounding box of the repainted pixels is cropped, resampled to
        IMAGE_DIM, inpainted and composited back into the untouched image, which may have any size); padding = pixels around the bounding box (0 .. 512, 32);
        mask_blur = Gaussian sigma of the repaint weight (0 .. 64); mask_grow = pixels the repainted area grows (or shrinks, negative) by (-256 .. 256);
        invert = True: the mask says white = repaint; composite = True: with area 'whole', paste the result over the input through the soft mask.  None
        keeps a setting.  The options persist across generations; with all six at their defaults a generation is what it was without them."""
        for name, v in (("inpaint_area", area), ("inpaint_padding", padding), ("mask_blur", mask_blur), ("mask_grow", mask_grow)):
            if v is not None:
                self.option_set(name, v)
        if invert is not None:
            self.option_set("mask_invert", 1 if invert else 0)
        if composite is not None:
            self.option_set("inpaint_composite", 1 if composite else 0)

    def _mask_call(self, fn, what, tensor, *args):
        tin = tensor._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if fn(self._ctx, ctypes.byref(tin), tout, *args) < 0:
            raise RuntimeError("Failed to %s: %s" % (what, self.errstr_get()))
        return MLIS_Tensor(tout.contents)

    def mask_process(self, mask, grow=0, blur=0.0, invert=False, wrap=0):
        """The repaint weight p of a mask on the GPU, as a generation with these options computes it: clamp(invert ? m : 1 - m, 0, 1), grown by `grow` pixels
        (maximum over a square; negative shrinks), blurred with sigma `blur`.  mask: an MLIS_Tensor [1,1,h,w].  wrap: bit 0 columns, bit 1 rows wrap around."""
        p = self._mask_call(self._lib.mlis_amd_tensor_mask_weight, "weigh the mask", mask, 1 if invert else 0)
        if grow:
            p = self._mask_call(self._lib.mlis_amd_tensor_mask_grow, "grow the mask", p, int(grow), int(wrap))
        if blur > 0:
            p = self._mask_call(self._lib.mlis_amd_tensor_gauss_blur, "blur the mask", p, float(blur), int(wrap))
        return p

    def gauss_blur(self, tensor, sigma, wrap=0):
        "Gaussian blur of every plane of a tensor on the GPU (radius int(2.5 sigma + 0.5), border replicated or wrapped)."
        return self._mask_call(self._lib.mlis_amd_tensor_gauss_blur, "blur the tensor", tensor, float(sigma), int(wrap))

    def mask_bbox(self, p):
        "(x0, y0, x1, y1), half open, of the pixels of p [1,1,h,w] with a value > 0; (0, 0, 0, 0) if there are none."
        tin, box = p._c(), (_I * 4)()
        if self._lib.mlis_amd_tensor_mask_bbox(self._ctx, ctypes.byref(tin), box) < 0:
            raise RuntimeError("Failed to find the bounding box: %s" % self.errstr_get())
        return tuple(int(v) for v in box)

    def composite(self, orig, patch, p, x0=0, y0=0):
        """orig [1 or n,c,H,W] with patch [n,c,ch,cw] pasted at (x0, y0) through the weight p [1,1,H,W]: orig (1 - p) + patch p inside the rectangle, orig
        outside, in fp32 on the GPU.  Returns an MLIS_Tensor [n,c,H,W]."""
        to, tp, tw = orig._c(), patch._c(), p._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if self._lib.mlis_amd_tensor_composite(self._ctx, tout, ctypes.byref(to), ctypes.byref(tp), ctypes.byref(tw), int(x0), int(y0)) < 0:
            raise RuntimeError("Failed to composite: %s" % self.errstr_get())
        return MLIS_Tensor(tout.contents)

    def inpaint_info(self):
        "((x0, y0, x1, y1), (w, h)): the rectangle the last generation composited and the size its pass ran at; None if it composited nothing."
        reg, proc = (_I * 4)(), (_I * 2)()
        r = self._lib.mlis_amd_inpaint_info(self._ctx, reg, proc)
        return (tuple(int(v) for v in reg), tuple(int(v) for v in proc)) if r > 0 else None

    # ---- FreeU
    def freeu_set(self, on=None, b1=None, b2=None, s1=None, s2=None):
        """FreeU (version 2): on = True / False; b1, b2 = backbone factors and s1, s2 = skip factors of stages 1 and 2, each in [0, 4] (1 = that part off).
        None keeps a setting.  The options persist across generations; only `on` is built into the engine, a factor change rebuilds nothing."""
        if on is not None:
            self.option_set("freeu", 1 if on else 0)
        for name, v in (("freeu_b1", b1), ("freeu_b2", b2), ("freeu_s1", s1), ("freeu_s2", s2)):
            if v is not None:
                self.option_set(name, float(v))

    # ---- HyperTile
    def hypertile_set(self, tile=None, depth=None):
        """HyperTile: tile = the tile's side in image pixels (0 = off, else 32 .. 8192 and a multiple of 8), depth = the deepest UNet level that is tiled
        (0 .. 3).  None keeps a setting.  Both persist across generations and are built into the engine; the rule is applied per pass size."""
        if tile is not None:
            self.option_set("hypertile", int(tile))
        if depth is not None:
            self.option_set("hypertile_depth", int(depth))

    def hypertile_info(self):
        """(n_tiled, n_untiled, tiles) of the engine used last: its UNet's spatial transformers that are tiled / not, and (th, tw, nh, nw) per depth 0 .. 3
        (zeros where the depth is not tiled); None before the first engine."""
        e = self._lib.mlis_amd_engine_get(self._ctx)
        if not e:
            return None
        a, b, t = _I(), _I(), (_I * 16)()
        if self._lib.mlis_amd_hypertile_info(e, ctypes.byref(a), ctypes.byref(b), t) < 0:
            raise RuntimeError("Failed to read the HyperTile plan: %s" % self.errstr_get())
        return a.value, b.value, [tuple(int(t[4 * i + j]) for j in range(4)) for i in range(4)]

    # ---- perturbed-attention guidance
    def pag_set(self, scale=3.0):
        """Perturbed-attention guidance: scale in [0, 20]; 0 switches it off (the default), 3 is what front ends use.  It persists across generations.  Only
        on / off is built into the engine (a third UNet row group per image); changing the value builds nothing."""
        self.option_set("pag_scale", float(scale))

    def pag_info(self):
        """(perturbed self-attentions of the UNet plan -- 0 for an engine without PAG --, rows of one UNet evaluation) of the engine used last; None before the
        first engine."""
        e = self._lib.mlis_amd_engine_get(self._ctx)
        if not e:
            return None
        a, b = _I(), _I()
        if self._lib.mlis_amd_pag_info(e, ctypes.byref(a), ctypes.byref(b)) < 0:
            raise RuntimeError("Failed to read the PAG plan: %s" % self.errstr_get())
        return a.value, b.value

    # ---- prediction type, zero-terminal-SNR schedule, guidance rescale
    def guidance_set(self, cfg_rescale=None, prediction=None, zsnr=None):
        """cfg_rescale: phi of the guidance rescale in [0, 1], 0 = off (front ends use 0.7).  prediction: "auto" | "eps" | "v".  zsnr: "auto" | "off" | "on" (or a
        bool): the zero-terminal-SNR sigma table.  "auto" is what the model type and the checkpoint's v_pred / ztsnr markers say.  Arguments left None keep their
        value; all persist across generations and none builds an engine."""
        if cfg_rescale is not None:
            self.option_set("cfg_rescale", float(cfg_rescale))
        if prediction is not None:
            self.option_set("prediction", str(prediction))
        if zsnr is not None:
            self.option_set("zsnr", ("on" if zsnr else "off") if isinstance(zsnr, bool) else str(zsnr))

    def guidance_info(self):
        """dict of the engine used last: vparam and zsnr as resolved, sigma_min, sigma_max, cfg_rescale, n_evals (rescaled mixes so far) and factors (the last
        mix's per-image factors); None before the first engine."""
        e = self._lib.mlis_amd_engine_get(self._ctx)
        if not e:
            return None
        from . import engine as E
        return E.guidance_info(e, 64)      # (room for the largest batch; the engine writes its own B factors)

    def tensor_resample(self, tensor, w, h, mode=MLIS_AMD_RESAMPLE_BILINEAR):   # noqa: F821
        "Resample every plane of a tensor to w x h on the GPU (MLIS_AMD_RESAMPLE_*); edges wrap along the axes of the tiling option."
        tin = tensor._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if self._lib.mlis_amd_tensor_resample(self._ctx, ctypes.byref(tin), tout, w, h, mode) < 0:
            raise RuntimeError("Failed to resample the tensor: %s" % self.errstr_get())
        return MLIS_Tensor(tout.contents)

    def tensor_resample_aa(self, tensor, w, h, filter=MLIS_AMD_AA_LANCZOS):   # noqa: F821
        """Resample every plane of a tensor to w x h on the GPU through a filter whose support grows with the shrink factor (MLIS_AMD_AA_*: what PIL's resize and
        torch's interpolate(antialias=True) compute); edges wrap along the axes of the tiling option."""
        tin = tensor._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if self._lib.mlis_amd_tensor_resample_aa(self._ctx, ctypes.byref(tin), tout, w, h, filter) < 0:
            raise RuntimeError("Failed to resample the tensor: %s" % self.errstr_get())
        return MLIS_Tensor(tout.contents)

    def upscale(self, image, outscale=None):
        """Upscale an image tensor [n,3,h,w] in [0,1] 4x with the ESRGAN model of the "upscale_model" option (a safetensors RRDBNet or
        "synth[:seed[:blocks]]"); the result is not clamped.  The upscaler is built on first use and stays resident.
        outscale F in (0, 4]: the x4 output is brought to round(F w) x round(F h) with the "downscale_filter" option's filter, lanczos where that is none
        (Real-ESRGAN's --outscale); None or 4 is the x4 output itself."""
        if outscale is not None and not 0 < outscale <= 4:
            raise ValueError("outscale must be in (0, 4]")
        tin = image._c()
        tout = self._lib.mlis_tensor_get(self._ctx, MLIS_TENSOR_TMP + 2)              # noqa: F821
        if self._lib.mlis_amd_tensor_upscale(self._ctx, ctypes.byref(tin), tout) < 0:
            raise RuntimeError("Failed to upscale the image: %s" % self.errstr_get())
        if outscale is not None and outscale != 4:
            f = _I()
            self.option_get(MLIS_OPT_AMD_DOWNSCALE_FILTER, f)                          # noqa: F821
            w, h = int(math.floor(outscale * image.n[0] + 0.5)), int(math.floor(outscale * image.n[1] + 0.5))
            if self._lib.mlis_amd_tensor_resample_aa(self._ctx, tout, tout, max(w, 1), max(h, 1), f.value - 1 if f.value else MLIS_AMD_AA_LANCZOS) < 0:   # noqa: F821
                raise RuntimeError("Failed to resample the upscaled image: %s" % self.errstr_get())
        return MLIS_Tensor(tout.contents)

    def engine_builds(self):
        "Engines this context has constructed so far (it keeps the two used last)."
        return int(self._lib.mlis_amd_engine_builds(self._ctx))

    def lora_stats(self):
        """(restored, patched, cold_merges), cumulative: weights set back to the checkpoint's and adapter tensors applied in place on the GPU
        (per resident plan) when the LoRA set or a multiplier changed, and adapters merged on the host before anything was resident."""
        a, b, c = _I(), _I(), _I()
        if self._lib.mlis_amd_lora_stats(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) < 0:
            raise RuntimeError("Failed to read the LoRA statistics: %s" % self.errstr_get())
        return a.value, b.value, c.value


def tensor_from_numpy(a):
    """float32 array of up to 4 dimensions -> MLIS_Tensor (n = shape reversed, padded with ones)."""
    import numpy as np
    a = np.ascontiguousarray(a, np.float32)
    t = MLIS_Tensor.__new__(MLIS_Tensor)
    t.n = tuple((list(a.shape[::-1]) + [1, 1, 1, 1])[:4])
    t.data = a.tobytes()
    return t


def inpaint_region(W, H, bbox, padding, tw, th):
    """mlis_amd_inpaint_region: the rectangle (x0, y0, x1, y1) that inpaint_area masked processes for a bounding box in a W x H image, or None if refused."""
    box, out = (_I * 4)(*[int(v) for v in bbox]), (_I * 4)()
    r = load_library().mlis_amd_inpaint_region(int(W), int(H), box, int(padding), int(tw), int(th), out)
    return tuple(int(v) for v in out) if r > 0 else None


__all__ = [n for n in globals() if n.startswith("MLIS_") or n in ("MLImgSynth", "load_library", "tensor_from_numpy", "inpaint_region")]
