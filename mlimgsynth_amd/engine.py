"""Python (ctypes) mirror of the host-side C API (include/mlblock_amd.h, include/mlimgsynth_amd.h).

Thin by design: every call goes straight into libmlimgsynth_amd.so; numpy arrays at the
boundary use the reference's host layout (LocalTensor: NCHW fp32, src/localtensor.h:16-20).
"""
import ctypes

import numpy as np

from ._lib import check1, lib, vp

c_int, c_f, c_i64, c_u64 = ctypes.c_int, ctypes.c_float, ctypes.c_int64, ctypes.c_uint64
FP = ctypes.POINTER(ctypes.c_float)


class UnetParams(ctypes.Structure):
    _fields_ = [("n_ch_in", c_int), ("n_ch_out", c_int), ("n_res_blk", c_int), ("attn_res", c_int * 4),
                ("ch_mult", c_int * 5), ("transf_depth", c_int * 5), ("n_te", c_int), ("n_head", c_int),
                ("d_head", c_int), ("n_ctx", c_int), ("n_ch", c_int), ("ch_adm_in", c_int),
                ("clip_norm", c_int), ("cond_label", c_int), ("uncond_empty_zero", c_int), ("vparam", c_int),
                ("n_step_train", c_int), ("sigma_min", c_f), ("sigma_max", c_f), ("zsnr", c_int)]


class UnetState(ctypes.Structure):
    _fields_ = [("ctx", vp), ("par", ctypes.POINTER(UnetParams)), ("nfe", ctypes.c_uint), ("lw", c_int), ("lh", c_int),
                ("n_batch", c_int), ("t_x", vp), ("t_t", vp), ("t_c", vp), ("t_l", vp), ("t_out", vp)]


class VaeParams(ctypes.Structure):
    _fields_ = [("ch_x", c_int), ("ch_z", c_int), ("ch", c_int), ("n_res", c_int), ("n_res_blk", c_int),
                ("ch_mult", c_int * 5), ("d_embed", c_int), ("f_down", c_int), ("scale_factor", c_f)]


class ClipParams(ctypes.Structure):
    _fields_ = [("n_vocab", c_int), ("n_token", c_int), ("d_embed", c_int), ("n_interm", c_int),
                ("n_head", c_int), ("n_layer", c_int), ("tok_start", c_int), ("tok_end", c_int), ("tok_pad", c_int)]


class CtxInfo(ctypes.Structure):
    _fields_ = [("mem_params", ctypes.c_size_t), ("mem_compute", ctypes.c_size_t), ("mem_total", ctypes.c_size_t),
                ("t_load", ctypes.c_double), ("t_compute", ctypes.c_double), ("n_compute", ctypes.c_uint),
                ("n_conv", ctypes.c_uint), ("n_ops", ctypes.c_uint), ("flops", ctypes.c_double)]


class AmdConfig(ctypes.Structure):
    _fields_ = [("model", ctypes.c_char_p), ("width", c_int), ("height", c_int), ("n_batch", c_int), ("n_step", c_int),
                ("cfg_scale", c_f), ("s_ancestral", c_f), ("sched", c_int), ("use_tae", c_int), ("use_hipgraph", c_int),
                ("weight_seed", c_u64), ("method", c_int), ("s_noise", c_f), ("f_t_ini", c_f), ("f_t_end", c_f),
                ("defer_weights", c_int), ("unet_split", c_int), ("n_ctx_tok", c_int)]


class AmdControlConfig(ctypes.Structure):
    """MLIS_AmdConfig as it stands, with its trailing field `control`.  AmdConfig above is the layout before that field: the field lies in what was the
    structure's tail padding, so a zero-initialised AmdConfig is a valid configuration without a ControlNet."""
    _fields_ = AmdConfig._fields_ + [("control", c_int)]


CONTROL_NET, CONTROL_FREEU, CONTROL_HYPERTILE, CONTROL_PAG = 1, 2, 4, 8       # MLIS_AMD_CONTROL_*: the bits of `control`


def control_hypertile(tile_px, depth=3):
    """MLIS_AMD_CONTROL_HYPERTILE_OF: the bits of `control` for HyperTile with a tile of tile_px pixels (units of 8 px in bits 8..20) down to UNet depth
    `depth` (bits 24..25); 0 for tile_px 0"""
    return (CONTROL_HYPERTILE | (((int(tile_px) // 8) & 0x1FFF) << 8) | ((int(depth) & 3) << 24)) if tile_px else 0


def eval_rows(B, cfg_scale, pag):
    """mlis_amd_eval_rows: rows of one UNet evaluation, [cond B | uncond B (cfg_scale > 1) | perturbed B (pag)]"""
    f = L().mlis_amd_eval_rows
    f.restype, f.argtypes = c_int, [c_int, c_f, c_int]
    return int(f(int(B), float(cfg_scale), int(bool(pag))))


def hypertile_side(side, px_per_token, tile_px):
    """mlis_amd_hypertile_side: the tile's side in tokens on an axis of `side` tokens"""
    return int(L().mlis_amd_hypertile_side(int(side), int(px_per_token), int(tile_px)))


MLB_F_OPSHAPES, MLB_F_SYNTH_PARAMS, MLB_F_KEEP = 16, 32, 64

_op_kinds = None


def op_kinds():
    """[(name, bytes of the argument structure)] of every op kind, in the library's numbering (mlctx_op_kind_info); read once"""
    global _op_kinds
    if _op_kinds is None:
        f = L().mlctx_op_kind_info
        f.argtypes = [c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_size_t)]
        kinds, name, nb = [], ctypes.c_char_p(), ctypes.c_size_t()
        while f(len(kinds), ctypes.byref(name), ctypes.byref(nb)):
            kinds.append((name.value.decode(), nb.value))
        _op_kinds = kinds
    return _op_kinds


def _op_arg_types():
    """the ctypes record of each kind's arguments, for MLCtx.op_records"""
    from . import kernels as K
    return {"gemm": K.GemmArgs, "attn": K.AttnArgs, "attn_ctx": K.AttnArgs, "gn": K.GnArgs, "ln": K.LnArgs, "n2h": K.N2hArgs, "h2n": K.H2nArgs,
            "temb": K.TembArgs, "act": K.ActArgs, "cemb": K.CembArgs, "smax": K.SmaxArgs, "copy": K.CopyArgs, "xavt": K.XavtArgs, "cadd": K.CaddArgs,
            "freeu_backbone": K.FreeuArgs, "freeu_skip": K.FreeuArgs}


class OpRecord(ctypes.Structure):
    """MLOpRecord"""
    _fields_ = [("kind", c_int), ("fused", c_int), ("once", c_int), ("gn_src", c_int * 2), ("label", ctypes.c_char_p), ("args", vp),
                ("args_bytes", ctypes.c_size_t)]


class InputRecord(ctypes.Structure):
    """MLInputRecord"""
    _fields_ = [("name", ctypes.c_char_p), ("stage", vp), ("stage_bytes", ctypes.c_size_t), ("src", vp), ("n_src", c_int), ("scale", vp)]


_proto_done = False


def L():
    global _proto_done
    l = lib()
    if not _proto_done:
        l.mlctx_new.restype = vp
        l.mlctx_new.argtypes = [vp]
        l.mlctx_destroy.argtypes = [vp]
        l.mlctx_set_flags.argtypes = [vp, c_int]
        l.mlctx_params_synth.argtypes = [vp, c_u64]
        l.mlctx_param_set.argtypes = [vp, ctypes.c_char_p, c_int, vp, c_i64]
        l.mlctx_param_count.argtypes = [vp]
        l.mlctx_param_info.argtypes = [vp, c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int), ctypes.POINTER(c_i64 * 4)]
        l.mlctx_info.argtypes = [vp, ctypes.POINTER(CtxInfo)]
        l.mlctx_op_info.argtypes = [vp, c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double)]
        l.mlctx_profile_ops.argtypes = [vp, FP, c_int]
        l.mlctx_op_bytes.argtypes = [vp, c_int]
        l.mlctx_op_bytes.restype = ctypes.c_double
        l.mlctx_compute.argtypes = [vp]
        l.mlctx_sync.argtypes = [vp]
        l.unet_params_get.argtypes = [ctypes.c_char_p, ctypes.POINTER(UnetParams)]
        l.unet_denoise_init_n.argtypes = [ctypes.POINTER(UnetState), vp, ctypes.POINTER(UnetParams), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
        l.unet_denoise_init_nc.argtypes = [ctypes.POINTER(UnetState), vp, ctypes.POINTER(UnetParams), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, c_int]
        l.unet_denoise_build.argtypes = [ctypes.POINTER(UnetState)]
        l.unet_denoise_run_n.argtypes = [ctypes.POINTER(UnetState), FP, FP, FP, FP, FP]
        l.unet_sigma_to_t.restype = c_f
        l.unet_sigma_to_t.argtypes = [ctypes.POINTER(UnetParams), c_f]
        l.unet_t_to_sigma.restype = c_f
        l.unet_t_to_sigma.argtypes = [ctypes.POINTER(UnetParams), c_f]
        l.mlctx_op_record.argtypes = [vp, c_int, ctypes.POINTER(OpRecord)]
        l.mlctx_param_device.argtypes = [vp, c_int, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(c_int)]
        l.mlctx_weight_slab.argtypes = [vp, c_int, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        l.mlctx_input_count.argtypes = [vp]
        l.mlctx_input_record.argtypes = [vp, c_int, ctypes.POINTER(InputRecord)]
        l.mlctx_zeroed_block.argtypes = [vp, c_int, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        l.mlctx_scratch_block.argtypes = [vp, c_int, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        l.mlctx_ln_alias_refused.argtypes = [vp]
        l.mlb_f32_to_f16_bits.restype = ctypes.c_uint16
        l.mlb_f32_to_f16_bits.argtypes = [c_f]
        l.mlb_f16_bits_to_f32.restype = c_f
        l.mlb_f16_bits_to_f32.argtypes = [ctypes.c_uint16]
        _proto_done = True
    return l


def fptr(a):
    return a.ctypes.data_as(FP) if a is not None else None


def set_hypertile(ctx, tile_px, depth=3):
    """mlctx_set_hypertile: HyperTile for the spatial transformers the context builds from now on (tile_px 0: off)."""
    f = L().mlctx_set_hypertile
    f.argtypes = [vp, c_int, c_int]
    f.restype = None
    f(ctx.h, int(tile_px), int(depth))


def set_conv_wrap(ctx, mode):
    """mlctx_set_conv_wrap: circular padding (0 none, 1 x, 2 y, 3 xy) of the convolutions the context builds from now on."""
    f = L().mlctx_set_conv_wrap
    f.argtypes = [vp, c_int]
    f.restype = None
    f(ctx.h if isinstance(ctx, MLCtx) else vp(ctx), int(mode))


class MLCtx:
    """Owns one MLCtx (one model graph + its device-resident parameters)."""

    def __init__(self, stream=None, flags=0):
        self.h = L().mlctx_new(vp(stream))
        if flags:
            L().mlctx_set_flags(self.h, flags)

    def params_synth(self, seed=1234):
        check1(L().mlctx_params_synth(self.h, seed), "mlctx_params_synth")

    def param_set(self, key, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        check1(L().mlctx_param_set(self.h, key.encode(), 0, a.ctypes.data_as(vp), a.size), f"mlctx_param_set({key})")

    def param_list(self):
        out = []
        for i in range(L().mlctx_param_count(self.h)):
            key, typ, ne = ctypes.c_char_p(), c_int(), (c_i64 * 4)()
            L().mlctx_param_info(self.h, i, ctypes.byref(key), ctypes.byref(typ), ctypes.byref(ne))
            out.append((key.value.decode(), typ.value, [int(v) for v in ne]))
        return out

    def info(self):
        i = CtxInfo()
        L().mlctx_info(self.h, ctypes.byref(i))
        return i

    def op_list(self):
        out = []
        n = self.info().n_ops
        for i in range(n):
            lab, fl = ctypes.c_char_p(), ctypes.c_double()
            L().mlctx_op_info(self.h, i, ctypes.byref(lab), ctypes.byref(fl))
            out.append((lab.value.decode(), fl.value))
        return out

    def op_records(self):
        """mlctx_op_record of every op: [(kind name, label, fused, once, (gn_src0, gn_src1), a copy of the kind's argument structure)]"""
        types, kinds, out, r = _op_arg_types(), op_kinds(), [], OpRecord()
        for i in range(self.info().n_ops):
            check1(L().mlctx_op_record(self.h, i, ctypes.byref(r)), "mlctx_op_record")
            kind = kinds[r.kind][0]
            T = types[kind]
            if r.args_bytes != ctypes.sizeof(T):
                raise RuntimeError(f"op {i} ({kind}): the library's argument record has {r.args_bytes} bytes, its ctypes mirror {ctypes.sizeof(T)}")
            a = T()
            ctypes.memmove(ctypes.byref(a), r.args, ctypes.sizeof(T))
            out.append((kind, (r.label or b"").decode(), r.fused, r.once, (r.gn_src[0], r.gn_src[1]), a))
        return out

    def param_devices(self):
        """[(key, device address, bytes)] of the parameter table (mlctx_param_device)"""
        out = []
        for i, (key, _, _) in enumerate(self.param_list()):
            p, n, e = vp(), ctypes.c_size_t(), c_int()
            check1(L().mlctx_param_device(self.h, i, ctypes.byref(p), ctypes.byref(n), ctypes.byref(e)), "mlctx_param_device")
            out.append((key, p.value or 0, n.value * e.value))
        return out

    def _blocks(self, f):
        out, i = [], 0
        while True:
            p, n = vp(), ctypes.c_size_t()
            if not f(self.h, i, ctypes.byref(p), ctypes.byref(n)):
                return out
            out.append((p.value or 0, n.value))
            i += 1

    def weight_slabs(self):
        """[(address, bytes)] of the device slabs of a weight-streaming plan"""
        return self._blocks(L().mlctx_weight_slab)

    def zeroed_blocks(self):
        """[(address, bytes)] of the blocks the plan zeroed once and no launch writes in full (mlctx_zeroed_block)"""
        return self._blocks(L().mlctx_zeroed_block)

    def scratch_blocks(self):
        """{name: (address, bytes)} of the plan's shared scratch (mlctx_scratch_block)"""
        out = {}
        for which, name in enumerate(("splitk_ws", "sk_flags", "ln_cnt", "ln_ws")):
            p, n = vp(), ctypes.c_size_t()
            if L().mlctx_scratch_block(self.h, which, ctypes.byref(p), ctypes.byref(n)):
                out[name] = (p.value or 0, n.value)
        return out

    def input_records(self):
        """[(name, staging address, bytes, bound source address or 0, images of the bound source, scale vector address or 0)]"""
        out, r = [], InputRecord()
        for i in range(L().mlctx_input_count(self.h)):
            check1(L().mlctx_input_record(self.h, i, ctypes.byref(r)), "mlctx_input_record")
            out.append(((r.name or b"").decode(), r.stage or 0, r.stage_bytes, r.src or 0, r.n_src, r.scale or 0))
        return out

    def ln_alias_refused(self):
        return int(L().mlctx_ln_alias_refused(self.h))

    def op_bytes(self):
        f = L().mlctx_op_bytes
        f.restype = ctypes.c_double
        return [f(self.h, i) for i in range(self.info().n_ops)]

    def profile_ops(self):
        n = self.info().n_ops
        ms = np.zeros(n, np.float32)
        check1(L().mlctx_profile_ops(self.h, fptr(ms), n), "mlctx_profile_ops")
        return ms

    def streaming_info(self):
        """(segments, streamed bytes per evaluation, slab bytes, host bytes) of a weight-streaming plan, or None"""
        f = L().mlctx_weight_streaming_info
        f.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
        n, a, b, c = c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        if not f(self.h, ctypes.byref(n), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)):
            return None
        return n.value, a.value, b.value, c.value

    def streaming_copies(self):
        """host -> device copies one evaluation of a weight-streaming plan issues (the host master is laid out in segment order: one per segment at best)"""
        f = L().mlctx_weight_streaming_copies
        f.argtypes = [vp]
        return int(f(self.h))

    def tune_misses(self):
        """GEMM shapes of this plan that the compiled-in tile table does not list (they run on the static rule)."""
        f = L().mlctx_plan_tune_misses
        f.argtypes = [vp]
        return int(f(self.h))

    def tune_nearest(self):
        """... of which a table entry with the nearest row count lent its tile (mlctx_plan_tune_nearest); the others use the static rule."""
        f = L().mlctx_plan_tune_nearest
        f.argtypes = [vp]
        return int(f(self.h))

    def compute(self):
        check1(L().mlctx_compute(self.h), "mlctx_compute")

    def sync(self):
        check1(L().mlctx_sync(self.h), "mlctx_sync")

    def destroy(self):
        if self.h:
            L().mlctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def unet_params(model, zsnr=False):
    """unet_params_get; zsnr: the zero-terminal-SNR sigma table and its sigma range (unet_params_set_zsnr)"""
    u = UnetParams()
    check1(L().unet_params_get(model.encode(), ctypes.byref(u)), "unet_params_get")
    if zsnr:
        f = L().unet_params_set_zsnr
        f.restype, f.argtypes = None, [ctypes.POINTER(UnetParams), c_int]
        f(ctypes.byref(u), 1)
    return u


def log_sigmas(zsnr=False):
    """unet_log_sigmas: the 1000 stored float logs of the plain or of the zero-terminal-SNR sigma table"""
    f = L().unet_log_sigmas
    f.restype, f.argtypes = FP, [c_int]
    return np.ctypeslib.as_array(f(int(bool(zsnr))), (1000,)).copy()


def prediction_resolve(model, ckpt_v_pred=False, ckpt_ztsnr=False, prediction=0, zsnr=0):
    """mlis_amd_prediction_resolve -> (vparam, zsnr): options 0 auto, 1 eps / off, 2 v / on against the model type and the checkpoint's markers"""
    f = L().mlis_amd_prediction_resolve
    f.restype, f.argtypes = c_int, [ctypes.c_char_p, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    v, z = c_int(-1), c_int(-1)
    check1(f(model.encode(), int(bool(ckpt_v_pred)), int(bool(ckpt_ztsnr)), int(prediction), int(zsnr), ctypes.byref(v), ctypes.byref(z)), "mlis_amd_prediction_resolve")
    return v.value, z.value


class Unet:
    """unet_denoise_init_n / unet_denoise_run_n (src/unet.c:336-498) with a batch dimension."""

    def __init__(self, model, lw, lh, n_batch, stream=None, flags=0, seed=1234, synth=True, stream_weights_mib=0, n_ctx_tok=77,
                 hypertile=0, hypertile_depth=3, pag=0, tiling=0):
        self.P = unet_params(model)
        self.ctx = MLCtx(stream, flags)
        if hypertile:                   # HyperTile: self-attention inside tiles of `hypertile` image pixels, UNet levels 0 .. hypertile_depth
            set_hypertile(self.ctx, hypertile, hypertile_depth)
        if pag:                         # perturbed-attention guidance: the plan's last `pag` images are the perturbed group (mlctx_set_pag)
            f = L().mlctx_set_pag
            f.restype, f.argtypes = None, [vp, c_int]
            f(self.ctx.h, int(pag))
        if tiling:                      # seamless tiling: 1 x, 2 y, 3 xy (circular padding of every convolution built below)
            set_conv_wrap(self.ctx, tiling)
        if stream_weights_mib:          # the reference's --unet-split: weights in pinned host memory, three device slabs of this size
            f = L().mlctx_set_weight_streaming
            f.argtypes = [vp, ctypes.c_size_t]
            check1(f(self.ctx.h, int(stream_weights_mib) << 20), "mlctx_set_weight_streaming")
        self.S = UnetState()
        try:
            if n_ctx_tok == 77:
                check1(L().unet_denoise_init_n(ctypes.byref(self.S), self.ctx.h, ctypes.byref(self.P), lw, lh, n_batch), "unet_denoise_init_n")
            else:                       # windowed prompt: cond [N][77 W][n_ctx]
                check1(L().unet_denoise_init_nc(ctypes.byref(self.S), self.ctx.h, ctypes.byref(self.P), lw, lh, n_batch, int(n_ctx_tok)),
                       "unet_denoise_init_nc")
            check1(L().unet_denoise_build(ctypes.byref(self.S)), "unet_denoise_build")
            if synth:
                self.ctx.params_synth(seed)
        except Exception:               # a plan that cannot be built (a latent the levels do not halve evenly, memory) leaves no context behind
            self.ctx.destroy()
            raise
        self.lw, self.lh, self.n, self.n_ctx_tok = lw, lh, n_batch, int(n_ctx_tok)

    def run(self, x, cond, label, sigma):
        x = np.ascontiguousarray(x, np.float32)
        cond = np.ascontiguousarray(cond, np.float32)
        sigma = np.ascontiguousarray(sigma, np.float32)
        lab = np.ascontiguousarray(label, np.float32) if label is not None else None
        if cond.size != self.n * self.n_ctx_tok * self.P.n_ctx:
            raise ValueError(f"conditioning of {cond.size} values, the plan takes {self.n} x {self.n_ctx_tok} x {self.P.n_ctx}")
        dx = np.empty_like(x)
        check1(L().unet_denoise_run_n(ctypes.byref(self.S), fptr(x), fptr(cond), fptr(lab), fptr(sigma), fptr(dx)), "unet_denoise_run_n")
        return dx


def _proto2():
    l = L()
    if getattr(l, "_proto2_done", False):
        return l
    l.vae_params_get.argtypes = [ctypes.c_char_p, ctypes.POINTER(VaeParams)]
    l.sdvae_decode_init.argtypes = [vp, ctypes.POINTER(VaeParams), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(vp)]
    l.sdvae_decode_build.argtypes = [vp, ctypes.POINTER(VaeParams), vp]
    l.sdvae_decode_run.argtypes = [vp, vp, FP, FP]
    l.sdtae_decode_init.argtypes = [vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(vp)]
    l.sdtae_decode_build.argtypes = [vp, vp]
    l.sdtae_decode_run.argtypes = [vp, vp, FP, FP]
    l.clip_params_get.argtypes = [ctypes.c_char_p, ctypes.POINTER(ClipParams)]
    l.clip_text_encode.argtypes = [vp, ctypes.POINTER(ClipParams), ctypes.c_char_p, ctypes.c_uint, ctypes.c_uint,
                                   ctypes.POINTER(ctypes.c_int32), FP, FP, c_int, ctypes.c_bool, c_u64]
    l.rng_philox_randn.argtypes = [vp, ctypes.c_uint, FP]
    l.dnsamp_schedule.argtypes = [ctypes.POINTER(UnetParams), c_int, c_int, c_f, c_f, FP]
    l.dnsamp_ancestral.argtypes = [c_f, c_f, c_f, FP, FP]
    l.mlis_amd_create.restype = vp
    l.mlis_amd_create.argtypes = [vp, vp]               # (MLIS_AmdConfig*: an AmdConfig or an AmdControlConfig by reference)
    l.mlis_amd_create_ex.restype = vp
    l.mlis_amd_create_ex.argtypes = [vp, c_int, vp]
    l.mlis_amd_create_tiled.restype = vp
    l.mlis_amd_create_tiled.argtypes = [vp, c_int, c_int, c_int, c_int, vp]
    l.mlis_amd_create_tiled_packed.restype = vp
    l.mlis_amd_create_tiled_packed.argtypes = [vp, c_int, c_int, c_int, c_int, c_int, vp]
    l.mlis_amd_tile_pack.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_int)]
    l.mlis_amd_tile_pack_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_window_starts.argtypes = [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int]
    l.mlis_amd_tile_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_tile_windows.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int]
    l.mlis_amd_dxdt.argtypes = [vp, FP, c_f, FP]
    l.mlis_amd_tiling.restype = c_int
    l.mlis_amd_tiling.argtypes = [vp]
    l.mlis_amd_destroy.argtypes = [vp]
    l.mlis_amd_set_cond.argtypes = [vp, FP, FP, FP, FP]
    l.mlis_amd_set_cond_device.argtypes = [vp, vp, vp, vp, vp]
    l.mlis_amd_generate.argtypes = [vp, ctypes.POINTER(c_u64), FP, FP]
    l.mlis_amd_denoise.argtypes = [vp, ctypes.POINTER(c_u64)]
    l.mlis_amd_decode.argtypes = [vp]
    l.mlis_amd_latent_device.restype = vp
    l.mlis_amd_latent_device.argtypes = [vp]
    l.mlis_amd_image_device.restype = vp
    l.mlis_amd_image_device.argtypes = [vp]
    l.mlis_amd_info.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int),
                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    l.mlis_amd_unet_ctx.restype = vp
    l.mlis_amd_unet_ctx.argtypes = [vp]
    l.mlis_amd_decoder_ctx.restype = vp
    l.mlis_amd_decoder_ctx.argtypes = [vp]
    l.mlis_amd_last_unet_ms.restype = c_f
    l.mlis_amd_last_unet_ms.argtypes = [vp]
    l.mlis_amd_last_nfe.argtypes = [vp]
    l.mlis_amd_last_n_step.argtypes = [vp]
    l.mlis_amd_sync.argtypes = [vp]
    l.mlis_amd_set_vae_tile.argtypes = [vp, c_int]
    for f in (l.mlis_amd_decoder_tile_prepare, l.mlis_amd_encoder_tile_prepare):
        f.restype, f.argtypes = vp, [vp]
    l.mlis_amd_vae_tile_walk.argtypes = [c_int] * 4 + [ctypes.POINTER(c_int)] * 4 + [c_int]
    l.mlis_amd_vae_tile_info.argtypes = [vp, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t),
                                         ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_seed.argtypes = [vp, ctypes.POINTER(c_u64)]
    l.mlis_amd_set_init_latent.argtypes = [vp, FP]
    l.mlis_amd_set_lmask.argtypes = [vp, FP]
    l.mlis_amd_encode.argtypes = [vp, FP, c_int]
    l.mlis_amd_encoder_ctx.restype = vp
    l.mlis_amd_encoder_ctx.argtypes = [vp]
    l.mlis_amd_set_callback.argtypes = [vp, vp, vp]
    l.mlis_amd_ctx_at.restype = vp
    l.mlis_amd_ctx_at.argtypes = [vp, c_int]
    l.mlis_amd_set_control_image.argtypes = [vp, FP]
    l.mlis_amd_set_control_image_device.argtypes = [vp, vp]
    l.mlis_amd_set_control.argtypes = [vp, c_f, c_f, c_f]
    l.mlis_amd_control_active.argtypes = [c_int, c_int, c_f, c_f]
    l.mlis_amd_control_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_control_image_get.argtypes = [vp, FP, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_set_freeu.argtypes = [vp, c_f, c_f, c_f, c_f]
    l.mlis_amd_freeu_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_hypertile_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_set_pag.argtypes = [vp, c_f]
    l.mlis_amd_pag_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]
    l.mlis_amd_set_prediction.argtypes = [vp, c_int, c_int]
    l.mlis_amd_set_cfg_rescale.argtypes = [vp, c_f]
    l.mlis_amd_guidance_info.argtypes = [vp, ctypes.POINTER(c_int), ctypes.POINTER(c_int), FP, FP, FP, ctypes.POINTER(c_int), FP, c_int]
    l._proto2_done = True
    return l


class Rng(ctypes.Structure):
    _fields_ = [("seed", c_u64), ("offset", ctypes.c_uint32)]


def randn(seed, offset, n):
    """rng_philox_randn of the host library (src/ccommon/rng_philox.c restated)."""
    r = Rng(seed, offset)
    out = np.empty(n, np.float32)
    _proto2().rng_philox_randn(ctypes.byref(r), n, fptr(out))
    return out, r.offset


def control_active(i_step, n_step, start, end):
    """mlis_amd_control_active: whether step i_step of n_step lies in the control window (start n_step <= i_step + 0.5 < end n_step)"""
    return bool(_proto2().mlis_amd_control_active(int(i_step), int(n_step), float(start), float(end)))


def schedule(model, n_step, sched=1, f_t_ini=1.0, f_t_end=0.0, zsnr=False):
    P = unet_params(model, zsnr)
    sig = np.zeros(n_step + 2, np.float32)
    n = _proto2().dnsamp_schedule(ctypes.byref(P), n_step, sched, f_t_ini, f_t_end, fptr(sig))
    check1(n, "dnsamp_schedule")
    return sig[:n + 1]


def guidance_info(engine, n_batch):
    """mlis_amd_guidance_info of an engine handle as a dict (Generator.guidance_info, MLImgSynth.guidance_info)"""
    v, z, n = c_int(), c_int(), c_int()
    smin, smax, phi = c_f(), c_f(), c_f()
    fac = np.zeros(max(int(n_batch), 1), np.float32)
    r = _proto2().mlis_amd_guidance_info(engine, ctypes.byref(v), ctypes.byref(z), ctypes.byref(smin), ctypes.byref(smax), ctypes.byref(phi), ctypes.byref(n),
                                         fptr(fac), fac.size)
    if r < 0:
        check1(r, "mlis_amd_guidance_info")
    return dict(vparam=v.value, zsnr=z.value, sigma_min=smin.value, sigma_max=smax.value, cfg_rescale=phi.value, n_evals=n.value, factors=fac[:r].copy())


def vae_tile_walk(full, tile_px, unit, margin):
    """mlis_amd_vae_tile_walk: the tile walk of one dimension -> (tile length, origins, source offsets, paste widths); lengths in units of `unit` pixels"""
    l = _proto2()
    n = c_int()
    cnt = check1(l.mlis_amd_vae_tile_walk(int(full), int(tile_px), int(unit), int(margin), ctypes.byref(n), None, None, None, 0), "mlis_amd_vae_tile_walk")
    a = [(c_int * cnt)() for _ in range(3)]
    check1(l.mlis_amd_vae_tile_walk(int(full), int(tile_px), int(unit), int(margin), ctypes.byref(n), a[0], a[1], a[2], cnt), "mlis_amd_vae_tile_walk")
    return (n.value,) + tuple(list(x) for x in a)


class Decoder:
    """sdvae_decode / sdtae_decode (src/vae.c:318-411, src/tae.c:117-136), batched, no tiling."""

    def __init__(self, model, lw, lh, n_batch, tae=False, stream=None, seed=1234, flags=0, tiling=0):
        l = _proto2()
        self.ctx = MLCtx(stream, flags)
        if tiling:
            set_conv_wrap(self.ctx, tiling)
        self.tae, self.lw, self.lh, self.n = tae, lw, lh, n_batch
        self.t_lat = vp()
        if tae:
            check1(l.sdtae_decode_init(self.ctx.h, lw, lh, n_batch, ctypes.byref(self.t_lat)), "sdtae_decode_init")
            check1(l.sdtae_decode_build(self.ctx.h, self.t_lat), "sdtae_decode_build")
        else:
            self.P = VaeParams()
            check1(l.vae_params_get(model.encode(), ctypes.byref(self.P)), "vae_params_get")
            check1(l.sdvae_decode_init(self.ctx.h, ctypes.byref(self.P), lw, lh, n_batch, ctypes.byref(self.t_lat)), "sdvae_decode_init")
            check1(l.sdvae_decode_build(self.ctx.h, ctypes.byref(self.P), self.t_lat), "sdvae_decode_build")
        self.ctx.params_synth(seed)

    def run(self, latent):
        latent = np.ascontiguousarray(latent, np.float32)
        img = np.empty((self.n, 3, self.lh * 8, self.lw * 8), np.float32)
        f = _proto2().sdtae_decode_run if self.tae else _proto2().sdvae_decode_run
        check1(f(self.ctx.h, self.t_lat, fptr(latent), fptr(img)), "decode_run")
        return img


def clip_text_encode(model, prefix, toks, want_embed=True, want_feat=False, clip_skip=1, norm=True, seed=1234, stream=None):
    """clip_text_encode (src/clip.c:439-488) for a batch of prompts; toks int32 [n_prompt][n_tok]."""
    l = _proto2()
    P = ClipParams()
    check1(l.clip_params_get(model.encode(), ctypes.byref(P)), "clip_params_get")
    toks = np.ascontiguousarray(toks, np.int32)
    n_prompt, n_tok = toks.shape
    embed = np.empty((n_prompt, P.n_token, P.d_embed), np.float32) if want_embed else None
    feat = np.empty((n_prompt, P.d_embed), np.float32) if want_feat else None
    ctx = MLCtx(stream)
    check1(l.clip_text_encode(ctx.h, ctypes.byref(P), prefix.encode(), n_prompt, n_tok,
                              toks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), fptr(embed), fptr(feat), clip_skip, norm, seed),
           "clip_text_encode")
    ctx.destroy()
    return embed, feat


class Generator:
    """mlis_amd_* generation driver (mlis_generate slice, src/mlimgsynth.c:1634-1773) for one GPU."""

    METHODS = {"euler": 1, "heun": 2, "taylor3": 3, "dpmpp2m": 4, "dpmpp2s": 5}

    def __init__(self, model, width, height, n_batch, n_step=20, cfg_scale=7.0, s_ancestral=1.0, sched=1, use_tae=False,
                 use_hipgraph=False, weight_seed=1234, stream=None, method="euler", s_noise=0.0, f_t_ini=1.0, f_t_end=0.0,
                 defer_weights=False, unet_split=0, n_ctx_tok=77, unet_tile=0, unet_tile_overlap=0, unet_tile_batch=1, control=False, freeu=False,
                 hypertile=0, hypertile_depth=3, pag=False, tiling=0):
        l = _proto2()
        self.cfg = AmdControlConfig(model.encode(), width, height, n_batch, n_step, cfg_scale, s_ancestral, sched, int(use_tae),
                             int(use_hipgraph), weight_seed, self.METHODS.get(method, method), s_noise, f_t_ini, f_t_end,
                             int(defer_weights), int(unet_split), int(n_ctx_tok),     # n_ctx_tok: context rows, 77 x W (windowed prompt)
                             (CONTROL_NET if control else 0) | (CONTROL_FREEU if freeu else 0) |   # control: flags -- a ControlNet (set_control_image / set_control), FreeU (set_freeu),
                             control_hypertile(hypertile, hypertile_depth) |                       # HyperTile with a tile of `hypertile` pixels (hypertile_info),
                             (CONTROL_PAG if pag else 0))                                          # perturbed-attention guidance: a third row group (set_pag, pag_info)
        if unet_tile:       # tiled diffusion: width x height is the canvas, the UNet plan has the size of one window (pixels; a pair gives w, h),
            tw, th = unet_tile if isinstance(unet_tile, (tuple, list)) else (unet_tile, unet_tile)      # times up to unet_tile_batch windows per evaluation
            self.h = l.mlis_amd_create_tiled_packed(ctypes.byref(self.cfg), int(tiling), int(tw), int(th), int(unet_tile_overlap), int(unet_tile_batch), vp(stream))
        else:
            self.h = l.mlis_amd_create_ex(ctypes.byref(self.cfg), int(tiling), vp(stream))    # tiling: 0 none, 1 x, 2 y, 3 xy (seamless)
        if not self.h:
            from ._lib import MlsdError, last_error
            raise MlsdError("mlis_amd_create failed: " + last_error())
        self.model, self.w, self.h_px, self.B = model, width, height, n_batch
        self.P = unet_params(model)

    def set_cond(self, cond, label=None, uncond=None, unlabel=None):
        a = [np.ascontiguousarray(x, np.float32) if x is not None else None for x in (cond, label, uncond, unlabel)]
        for x in (a[0], a[2]):          # [n_ctx_tok][n_ctx]: the C side copies that many floats
            if x is not None and x.size != self.cfg.n_ctx_tok * self.P.n_ctx:
                raise ValueError(f"conditioning of {x.size} values, the plan takes {self.cfg.n_ctx_tok} x {self.P.n_ctx}")
        check1(_proto2().mlis_amd_set_cond(self.h, *[fptr(x) for x in a]), "mlis_amd_set_cond")

    def set_cond_device(self, cond, label=None, uncond=None, unlabel=None):
        check1(_proto2().mlis_amd_set_cond_device(self.h, vp(cond), vp(label), vp(uncond), vp(unlabel)), "mlis_amd_set_cond_device")

    def set_init_latent(self, latent):
        a = np.ascontiguousarray(latent, np.float32) if latent is not None else None
        check1(_proto2().mlis_amd_set_init_latent(self.h, fptr(a)), "mlis_amd_set_init_latent")

    def set_lmask(self, lmask):
        a = np.ascontiguousarray(lmask, np.float32) if lmask is not None else None
        check1(_proto2().mlis_amd_set_lmask(self.h, fptr(a)), "mlis_amd_set_lmask")

    def seed(self, seeds):
        check1(_proto2().mlis_amd_seed(self.h, (c_u64 * self.B)(*[int(s) for s in seeds])), "mlis_amd_seed")

    def encode(self, images, sample=True):
        """mlis_image_encode: images [B][3][H][W] in [0,1] -> the resident latent (returned as numpy too)"""
        a = np.ascontiguousarray(images, np.float32)
        check1(_proto2().mlis_amd_encode(self.h, fptr(a), int(sample)), "mlis_amd_encode")
        from ._lib import lib
        out = np.empty((self.B, 4, self.h_px // 8, self.w // 8), np.float32)
        lib().mlsd_memcpy(out.ctypes.data_as(vp), vp(self.latent_ptr()), ctypes.c_size_t(out.nbytes), 1, None)
        lib().mlsd_device_sync()
        return out

    def last_n_step(self):
        return _proto2().mlis_amd_last_n_step(self.h)

    def dxdt(self, x, sigma):
        """mlis_amd_dxdt: one evaluation at x [B][4][lh][lw], sigma -> dx (UNet + CFG mix, as a solver stage sees it)"""
        x = np.ascontiguousarray(x, np.float32)
        if x.shape != (self.B, 4, self.h_px // 8, self.w // 8):
            raise ValueError(f"latent of shape {x.shape}, the engine takes {(self.B, 4, self.h_px // 8, self.w // 8)}")
        dx = np.empty_like(x)
        check1(_proto2().mlis_amd_dxdt(self.h, fptr(x), float(sigma), fptr(dx)), "mlis_amd_dxdt")
        return dx

    def set_sampler(self, n_step=0, method="euler", sched=1, cfg_scale=7.0, s_ancestral=1.0, s_noise=0.0, f_t_ini=1.0, f_t_end=0.0):
        """mlis_amd_set_sampler: the sampler options of the next generations (plans and weights stay; cfg_scale must stay on its side of 1)"""
        f = _proto2().mlis_amd_set_sampler
        f.argtypes = [vp, c_int, c_int, c_int, c_f, c_f, c_f, c_f, c_f]
        check1(f(self.h, int(n_step), self.METHODS.get(method, method), int(sched), cfg_scale, s_ancestral, s_noise, f_t_ini, f_t_end), "mlis_amd_set_sampler")

    def set_control_image(self, hint):
        """mlis_amd_set_control_image: hint [3][H][W] in [0,1] at the canvas's pixel size (runs the hint plan); None clears it"""
        a = np.ascontiguousarray(hint, np.float32) if hint is not None else None
        if a is not None and a.shape != (3, self.h_px, self.w):
            raise ValueError(f"control image of shape {a.shape}, the engine takes {(3, self.h_px, self.w)}")
        check1(_proto2().mlis_amd_set_control_image(self.h, fptr(a)), "mlis_amd_set_control_image")

    def set_control(self, strength=1.0, start=0.0, end=1.0):
        """mlis_amd_set_control: strength in [0, 2], step window 0 <= start <= end <= 1"""
        check1(_proto2().mlis_amd_set_control(self.h, float(strength), float(start), float(end)), "mlis_amd_set_control")

    def control_image(self):
        """mlis_amd_control_image_get: the control map the engine holds, float32 [3][H][W], or None without one"""
        w, h = c_int(), c_int()
        if check1(_proto2().mlis_amd_control_image_get(self.h, None, ctypes.byref(w), ctypes.byref(h)), "mlis_amd_control_image_get") == 0:
            return None
        a = np.empty((3, h.value, w.value), np.float32)
        check1(_proto2().mlis_amd_control_image_get(self.h, fptr(a), None, None), "mlis_amd_control_image_get")
        return a

    def control_info(self):
        """(residuals of the ControlNet plan -- 0 without one --, evaluations of the last denoise / dxdt in which it ran)"""
        n, e = c_int(), c_int()
        check1(_proto2().mlis_amd_control_info(self.h, ctypes.byref(n), ctypes.byref(e)), "mlis_amd_control_info")
        return n.value, e.value

    def set_freeu(self, b1=1.0, b2=1.0, s1=1.0, s2=1.0):
        """mlis_amd_set_freeu: backbone factors b1, b2 and skip factors s1, s2 of stages 1 and 2, each in [0, 4]; 1 switches that part off"""
        check1(_proto2().mlis_amd_set_freeu(self.h, float(b1), float(b2), float(s1), float(s2)), "mlis_amd_set_freeu")

    def freeu_info(self):
        """(decoder concatenations treated at stage 1, at stage 2); (0, 0) for an engine without FreeU"""
        a, b = c_int(), c_int()
        check1(_proto2().mlis_amd_freeu_info(self.h, ctypes.byref(a), ctypes.byref(b)), "mlis_amd_freeu_info")
        return a.value, b.value

    def set_pag(self, scale=3.0):
        """mlis_amd_set_pag: the scale of the perturbed-attention term, 0 .. 20; engines start at 0 (the plain mix)"""
        check1(_proto2().mlis_amd_set_pag(self.h, float(scale)), "mlis_amd_set_pag")

    def pag_info(self):
        """(perturbed self-attentions of the UNet plan -- 0 for an engine without PAG --, rows of one evaluation)"""
        a, b = c_int(), c_int()
        check1(_proto2().mlis_amd_pag_info(self.h, ctypes.byref(a), ctypes.byref(b)), "mlis_amd_pag_info")
        return a.value, b.value

    def set_prediction(self, vparam=-1, zsnr=-1):
        """mlis_amd_set_prediction: v-prediction (1) or eps (0) mix and the zero-terminal-SNR sigma table (1) or the plain one (0); negative: the model type's"""
        check1(_proto2().mlis_amd_set_prediction(self.h, int(vparam), int(zsnr)), "mlis_amd_set_prediction")

    def set_cfg_rescale(self, phi=0.7):
        """mlis_amd_set_cfg_rescale: phi of the guidance rescale, 0 .. 1; engines start at 0 (the mix without a factor)"""
        check1(_proto2().mlis_amd_set_cfg_rescale(self.h, float(phi)), "mlis_amd_set_cfg_rescale")

    def last_rows(self):
        """mlis_amd_last_rows: the raw UNet outputs the last mix read, [N][4][lh][lw] (cond | uncond at cfg > 1 | perturbed with PAG); a tiled engine's blended canvas"""
        a, b = c_int(), c_int()
        check1(_proto2().mlis_amd_pag_info(self.h, ctypes.byref(a), ctypes.byref(b)), "mlis_amd_pag_info")
        out = np.empty((b.value, 4, self.h_px // 8, self.w // 8), np.float32)
        f = _proto2().mlis_amd_last_rows
        f.argtypes = [vp, FP, ctypes.c_size_t]
        check1(f(self.h, fptr(out), out.nbytes), "mlis_amd_last_rows")
        return out

    def guidance_info(self):
        """dict: vparam, zsnr, sigma_min, sigma_max, cfg_rescale, n_evals (rescaled mixes so far), factors (float32 [B] of the last rescaled mix; empty before one)"""
        return guidance_info(self.h, self.cfg.n_batch)

    def hypertile_info(self):
        """(spatial transformers of the UNet plan that are tiled, that are not, [(th, tw, nh, nw) per depth 0 .. 3, zeros where the depth is not tiled])"""
        a, b, t = c_int(), c_int(), (c_int * 16)()
        check1(_proto2().mlis_amd_hypertile_info(self.h, ctypes.byref(a), ctypes.byref(b), t), "mlis_amd_hypertile_info")
        return a.value, b.value, [tuple(int(t[4 * i + j]) for j in range(4)) for i in range(4)]

    def ctx_at(self, i):
        """plan i of the engine (0 UNet, 1 decoder, 2 encoder, 3 tile decoder, 4 tile encoder, 5 ControlNet, 6 hint block), or None"""
        h = _proto2().mlis_amd_ctx_at(self.h, int(i))
        if not h:
            return None
        c = MLCtx.__new__(MLCtx)
        c.h = h
        c.destroy = lambda: None
        return c

    def tile_info(self):
        """(windows per evaluation -- 0 when not tiled --, window width, window height) in latent pixels"""
        n, w, h = c_int(), c_int(), c_int()
        check1(_proto2().mlis_amd_tile_info(self.h, ctypes.byref(n), ctypes.byref(w), ctypes.byref(h)), "mlis_amd_tile_info")
        return n.value, w.value, h.value

    def tile_pack_info(self):
        """(windows per plan evaluation, plan evaluations per UNet evaluation); (0, 1) when not tiled"""
        p, n = c_int(), c_int()
        check1(_proto2().mlis_amd_tile_pack_info(self.h, ctypes.byref(p), ctypes.byref(n)), "mlis_amd_tile_pack_info")
        return p.value, n.value

    def tile_windows(self):
        """[(x0, y0)] of every window in evaluation order, latent pixels"""
        n = self.tile_info()[0]
        xs, ys = (c_int * max(n, 1))(), (c_int * max(n, 1))()
        check1(_proto2().mlis_amd_tile_windows(self.h, xs, ys, n), "mlis_amd_tile_windows")
        return [(xs[i], ys[i]) for i in range(n)]

    def generate(self, seeds, want_latents=True, want_images=True):
        seeds = (c_u64 * self.B)(*[int(s) for s in seeds]) if seeds is not None else None
        lat = np.empty((self.B, 4, self.h_px // 8, self.w // 8), np.float32) if want_latents else None
        img = np.empty((self.B, 3, self.h_px, self.w), np.float32) if want_images else None
        check1(_proto2().mlis_amd_generate(self.h, seeds, fptr(lat), fptr(img)), "mlis_amd_generate")
        return lat, img

    def denoise(self, seeds):
        seeds = (c_u64 * self.B)(*[int(s) for s in seeds])
        check1(_proto2().mlis_amd_denoise(self.h, seeds), "mlis_amd_denoise")

    def decode(self):
        check1(_proto2().mlis_amd_decode(self.h), "mlis_amd_decode")
        check1(_proto2().mlis_amd_sync(self.h), "mlis_amd_sync")

    def set_vae_tile(self, tile_px):
        check1(_proto2().mlis_amd_set_vae_tile(self.h, int(tile_px)), "mlis_amd_set_vae_tile")

    def vae_tile_prepare(self, encoder=False):
        """mlis_amd_decoder_tile_prepare / mlis_amd_encoder_tile_prepare: builds the tile plan; False when tiling does not apply (one tile covers all, TAE, off)"""
        l = _proto2()
        return bool((l.mlis_amd_encoder_tile_prepare if encoder else l.mlis_amd_decoder_tile_prepare)(self.h))

    def vae_tile_info(self, encoder=False):
        """mlis_amd_vae_tile_info of the decode / encode tile plan, or None without one: dict(tile=(w, h) in latent / image pixels, in_bytes, out_bytes
        (allocated for the tile's input and output buffers), n_tiles (one pass walks), n_evals (plan evaluations of the last tiled pass))"""
        w, h, n, e = c_int(), c_int(), c_int(), c_int()
        ib, ob = ctypes.c_size_t(), ctypes.c_size_t()
        r = _proto2().mlis_amd_vae_tile_info(self.h, int(encoder), *[ctypes.byref(v) for v in (w, h, ib, ob, n, e)])
        if r < 0:
            check1(r, "mlis_amd_vae_tile_info")
        if r == 0:
            return None
        return dict(tile=(w.value, h.value), in_bytes=ib.value, out_bytes=ob.value, n_tiles=n.value, n_evals=e.value)

    def image(self):
        from ._lib import lib
        out = np.empty((self.B, 3, self.h_px, self.w), np.float32)
        lib().mlsd_memcpy(out.ctypes.data_as(vp), vp(self.image_ptr()), ctypes.c_size_t(out.nbytes), 1, None)
        lib().mlsd_device_sync()
        return out

    def latent_ptr(self):
        return _proto2().mlis_amd_latent_device(self.h)

    def image_ptr(self):
        return _proto2().mlis_amd_image_device(self.h)

    def info(self):
        uf, df, ops, mp, mc = ctypes.c_double(), ctypes.c_double(), c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        _proto2().mlis_amd_info(self.h, ctypes.byref(uf), ctypes.byref(df), ctypes.byref(ops), ctypes.byref(mp), ctypes.byref(mc))
        return dict(unet_flops=uf.value, decode_flops=df.value, unet_ops=ops.value, mem_params=mp.value, mem_compute=mc.value)

    def last_unet_ms(self):
        return _proto2().mlis_amd_last_unet_ms(self.h)

    def last_nfe(self):
        return _proto2().mlis_amd_last_nfe(self.h)

    def unet_ctx(self):
        c = MLCtx.__new__(MLCtx)
        c.h = _proto2().mlis_amd_unet_ctx(self.h)
        c.destroy = lambda: None
        return c

    def decoder_ctx(self):
        c = MLCtx.__new__(MLCtx)
        c.h = _proto2().mlis_amd_decoder_ctx(self.h)
        c.destroy = lambda: None
        return c

    def destroy(self):
        if self.h:
            _proto2().mlis_amd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass
