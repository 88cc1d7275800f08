"""ctypes mirror of include/mlsd_kernels.h (the op-level C-ABI shim into the HIP kernels)."""
import ctypes

from . import _lib
from ._lib import check, lib, vp

c_i64, c_int, c_f = ctypes.c_int64, ctypes.c_int, ctypes.c_float

ACT_NONE, ACT_SILU, ACT_GELU, ACT_GELU_QUICK, ACT_RELU, ACT_GEGLU = range(6)
RESAMPLE_NEAREST, RESAMPLE_BILINEAR, RESAMPLE_BICUBIC = range(3)

# tile variants (MLSD_TILE_*) and the labels mlsd_gemm_variant prints for them
TILE_128x128, TILE_64x128, TILE_256x128, TILE_256x128_S3, TILE_256x256, TILE_128x320 = 0, 1, 3, 4, 9, 16
TILE_PP_256x256, TILE_PP_128x320, TILE_PPSK_256x256, TILE_PP2_128x320, TILE_PP2_256x256, TILE_PPB_128x320 = 17, 18, 19, 20, 21, 22
TILE_PP2_256x128, TILE_W4_256x256, TILE_W4_128x320, TILE_PPSK_128x320, TILE_SKINNY, TILE_TT, TILE_CONV_SMALLN = 25, 26, 27, 28, 29, 30, 31
TILE_LABELS = {TILE_128x128: "128x128x64s2", TILE_64x128: "64x128x64s2", TILE_256x128: "256x128x64s2", TILE_256x128_S3: "256x128x32s3",
               TILE_256x256: "256x256x64s2w16", TILE_128x320: "128x320x64s2", TILE_PP_256x256: "256x256x64pp", TILE_PP_128x320: "128x320x64pp",
               TILE_PPSK_256x256: "256x256x64ppsk", TILE_PP2_128x320: "128x320x64pp2", TILE_PP2_256x256: "256x256x64pp2",
               TILE_PPB_128x320: "128x320x64ppb", TILE_PP2_256x128: "256x128x64pp2", TILE_W4_256x256: "256x256x64w4",
               TILE_W4_128x320: "128x320x64w4", TILE_PPSK_128x320: "128x320x64ppsk", TILE_SKINNY: "skinny128x64", TILE_TT: "128x160x64tt",
               TILE_CONV_SMALLN: "conv3x3n16"}


def tile_arg(v):
    """MLSD_TILE_ARG: the mlsd_gemm_args.tile_variant that asks for tile variant v."""
    return v + 1


class GemmArgs(ctypes.Structure):
    _fields_ = [("A", vp), ("lda", c_i64), ("conv", c_int), ("n_img", c_int), ("H", c_int), ("W", c_int),
                ("Cin", c_int), ("OH", c_int), ("OW", c_int), ("KH", c_int), ("KW", c_int), ("stride", c_int),
                ("pad", c_int), ("upsample", c_int), ("W_", vp), ("ldb", c_i64), ("M", c_int), ("N", c_int),
                ("K", c_int), ("bias", vp), ("rowbias", vp), ("rows_per_batch", c_int), ("ldrb", c_i64),
                ("resid", vp), ("ldr", c_i64), ("act", c_int), ("C32", vp), ("ldc32", c_i64), ("C16", vp),
                ("ldc16", c_i64), ("bias_m", vp), ("act_after_resid", c_int), ("tile_variant", c_int),
                ("ksplit", c_int), ("ws", vp), ("ws_bytes", ctypes.c_size_t), ("colstats", vp), ("colstats_rows", c_int), ("sk_flags", vp),
                ("ln_y16", vp), ("ldln", ctypes.c_int64), ("ln_gamma", vp), ("ln_beta", vp), ("ln_eps", ctypes.c_float), ("ln_ws", vp), ("ln_cnt", vp), ("ln_slot", c_int),
                ("gn_y16", vp), ("gn_ldy", ctypes.c_int64), ("gn_gamma", vp), ("gn_beta", vp), ("gn_eps", ctypes.c_float), ("gn_groups", c_int), ("gn_hw", c_int),
                ("gn_silu", c_int),
                ("xa_k", vp), ("xa_ldk", c_i64), ("xa_vt", vp), ("xa_out", vp), ("xa_ldo", c_i64), ("xa_Tq", c_int), ("xa_Tk", c_int),
                ("tap_oy", c_int), ("tap_ox", c_int), ("out_phase", c_int),
                ("colstats_shift", c_int), ("wrap", c_int)]


class GemmRouteInfo(ctypes.Structure):
    _fields_ = [("variant", c_int), ("asked", c_int), ("nsplit", c_int), ("stats_rows", c_int), ("ln", c_int), ("gn", c_int), ("xattn", c_int),
                ("handoff", c_int), ("stats_rows_if", c_int), ("ln_if", c_int), ("ln_ws_bytes_if", ctypes.c_size_t)]


class AttnArgs(ctypes.Structure):
    _fields_ = [("q", vp), ("k", vp), ("v", vp), ("out", vp), ("ldq", c_i64), ("ldk", c_i64), ("ldv", c_i64),
                ("ldo", c_i64), ("bsq", c_i64), ("bsk", c_i64), ("bsv", c_i64), ("bso", c_i64), ("n_batch", c_int),
                ("n_head", c_int), ("d_head", c_int), ("Tq", c_int), ("Tk", c_int), ("causal", c_int)]


class GnArgs(ctypes.Structure):
    _fields_ = [("x1", vp), ("x2", vp), ("ld1", c_i64), ("ld2", c_i64), ("C1", c_int), ("C2", c_int),
                ("n_img", c_int), ("HW", c_int), ("n_grp", c_int), ("eps", c_f), ("gamma", vp), ("beta", vp),
                ("silu", c_int), ("y16", vp), ("raw16", vp), ("ws", vp), ("cs1", vp), ("cs2", vp), ("rb_rows1", c_int), ("rb_rows2", c_int),
                ("cs_shifted", c_int)]


# the argument records of the plan's other op kinds (include/mlblock_amd.h: mlb_*_args), as mlctx_op_record hands them out
class LnArgs(ctypes.Structure):
    _fields_ = [("x", vp), ("ldx", c_i64), ("rows", c_int), ("d", c_int), ("eps", c_f), ("g", vp), ("b", vp), ("y16", vp), ("y32", vp)]


class N2hArgs(ctypes.Structure):
    _fields_ = [("src", vp), ("n_src", c_int), ("C", c_int), ("HW", c_int), ("dst", vp), ("n_dst", c_int), ("Cpad", c_int), ("scale", vp),
                ("scale0", c_f), ("mode", c_int)]


class H2nArgs(ctypes.Structure):
    _fields_ = [("src", vp), ("ld", c_i64), ("n", c_int), ("C", c_int), ("HW", c_int), ("dst", vp), ("mul", c_f), ("add", c_f)]


class TembArgs(ctypes.Structure):
    _fields_ = [("t", vp), ("n", c_int), ("dim", c_int), ("maxp", c_f), ("out", vp)]


class ActArgs(ctypes.Structure):
    _fields_ = [("x", vp), ("y", vp), ("n", ctypes.c_size_t), ("act", c_int)]


class CembArgs(ctypes.Structure):
    _fields_ = [("tok", vp), ("n", c_int), ("T", c_int), ("d", c_int), ("tw", vp), ("pw", vp), ("out", vp)]


class SmaxArgs(ctypes.Structure):
    _fields_ = [("in_", vp), ("ld_in", c_i64), ("out", vp), ("ld_out", c_i64), ("rows", c_int), ("cols", c_int), ("scale", c_f)]


class CopyArgs(ctypes.Structure):
    """mlb_copy_args: a device copy of nbytes; th > 0: the HyperTile row permutation (mlsd_tile_permute) of n_img maps of H x W rows of row_bytes"""
    _fields_ = [("src", vp), ("dst", vp), ("nbytes", ctypes.c_size_t), ("n_img", c_int), ("H", c_int), ("W", c_int), ("th", c_int), ("tw", c_int),
                ("row_bytes", c_int), ("inverse", c_int)]


class CaddArgs(ctypes.Structure):
    _fields_ = [("dst", vp), ("ld_dst", c_i64), ("base", vp), ("ld_base", c_i64), ("ctrl", vp), ("ld_ctrl", c_i64), ("n_img", c_int), ("rows", c_int),
                ("C", c_int), ("n_ctrl", c_int), ("gain", vp)]


class FreeuArgs(ctypes.Structure):
    _fields_ = [("dst", vp), ("ld_dst", c_i64), ("src", vp), ("ld_src", c_i64), ("n_img", c_int), ("H", c_int), ("W", c_int), ("C", c_int), ("ws", vp), ("f", vp)]


class DconvArgs(ctypes.Structure):
    """mlsd_dconv_args: the dense-block convolution of the ESRGAN upscaler (hip/upscale.hip)"""
    _fields_ = [("A", vp), ("lda", c_i64), ("n_img", c_int), ("H", c_int), ("W", c_int), ("Cin", c_int), ("upsample", c_int),
                ("W_", vp), ("N", c_int), ("bias", vp), ("lrelu", c_int), ("scale", c_f), ("resid", vp), ("ldr", c_i64),
                ("scale2", c_f), ("resid2", vp), ("ldr2", c_i64), ("C32", vp), ("ldc32", c_i64), ("C16", vp), ("ldc16", c_i64)]


class XavtArgs(ctypes.Structure):
    _fields_ = [("v", vp), ("ldv", c_i64), ("n_img", c_int), ("Tk", c_int), ("N", c_int), ("vt", vp)]


def gemm(args, stream=None):
    check(lib().mlsd_gemm(ctypes.byref(args), vp(stream)), "mlsd_gemm")


def conv3x3_dense(args, stream=None):
    check(lib().mlsd_conv3x3_dense(ctypes.byref(args), vp(stream)), "mlsd_conv3x3_dense")


def dconv_variant(args):
    f = lib().mlsd_dconv_variant
    f.restype = ctypes.c_char_p
    return f(ctypes.byref(args)).decode()


def gemm_splitk_ws_bytes(m, n, ksplit):
    f = lib().mlsd_gemm_splitk_ws_bytes
    f.restype = ctypes.c_size_t
    return f(m, n, ksplit)


def gemm_variant(args):
    f = lib().mlsd_gemm_variant
    f.restype = ctypes.c_char_p
    return f(ctypes.byref(args)).decode()


def gemm_route(args):
    r = GemmRouteInfo()
    check(lib().mlsd_gemm_route(ctypes.byref(args), ctypes.byref(r)), "mlsd_gemm_route")
    return r


def attention_variant(args, ctx=False):
    """mlsd_attention_variant: the label of the kernel mlsd_attention (or, with ctx, mlsd_attention_ctx) would launch; None where it would refuse."""
    f = lib().mlsd_attention_variant
    f.restype = ctypes.c_char_p
    f.argtypes = [ctypes.POINTER(AttnArgs), c_int]
    lab = f(ctypes.byref(args), int(bool(ctx)))
    return lab.decode() if lab is not None else None


def attention(args, stream=None):
    check(lib().mlsd_attention(ctypes.byref(args), vp(stream)), "mlsd_attention")


def attention_ctx(args, stream=None):
    """mlsd_attention_ctx: cross attention over 96 < Tk <= 320 keys (windowed text context)."""
    check(lib().mlsd_attention_ctx(ctypes.byref(args), vp(stream)), "mlsd_attention_ctx")


def groupnorm(args, stream=None):
    check(lib().mlsd_groupnorm(ctypes.byref(args), vp(stream)), "mlsd_groupnorm")


def groupnorm_ws_bytes(n_img, hw, n_grp):
    f = lib().mlsd_groupnorm_ws_bytes
    f.restype = ctypes.c_size_t
    return f(n_img, hw, n_grp)


def layernorm(x, ldx, rows, d, eps, gamma, beta, y16, y32=None, stream=None):
    check(lib().mlsd_layernorm(vp(x), c_i64(ldx), rows, d, c_f(eps), vp(gamma), vp(beta), vp(y16), vp(y32), vp(stream)),
          "mlsd_layernorm")


def resample2d(src, sw, sh, dst, dw, dh, planes, mode, wrap=0, stream=None):
    """mlsd_resample2d: fp32 planes [planes][sh][sw] -> [planes][dh][dw] (device pointers); wrap bit 0 columns, bit 1 rows."""
    check(lib().mlsd_resample2d(vp(src), sw, sh, vp(dst), dw, dh, planes, mode, wrap, vp(stream)), "mlsd_resample2d")


AA_BOX, AA_TRIANGLE, AA_CUBIC, AA_LANCZOS3 = range(4)


def resample_aa_max_taps(s_in, s_out, filter):
    """mlsd_resample_aa_max_taps: the largest tap count of one axis (of the unclipped windows: an upper bound with or without wrap); -1 if refused."""
    return int(lib().mlsd_resample_aa_max_taps(int(s_in), int(s_out), int(filter)))


def resample_aa_taps(s_in, s_out, filter, wrap_axis=0):
    """mlsd_resample_aa_taps: (start int32 [s_out], count int32 [s_out], w float32 [s_out][K]) of one axis, K the largest count; None if refused.  Host code."""
    import numpy as np
    k = resample_aa_max_taps(s_in, s_out, filter)
    if k < 1:
        return None
    start, count, w = np.zeros(s_out, np.int32), np.zeros(s_out, np.int32), np.zeros((s_out, k), np.float32)
    ip, fp = ctypes.POINTER(c_int), ctypes.POINTER(c_f)
    f = lib().mlsd_resample_aa_taps
    f.restype, f.argtypes = c_int, [c_int, c_int, c_int, c_int, ip, ip, fp, c_int]
    used = f(int(s_in), int(s_out), int(filter), int(wrap_axis), start.ctypes.data_as(ip), count.ctypes.data_as(ip), w.ctypes.data_as(fp), k)
    return None if used < 0 else (start, count, np.ascontiguousarray(w[:, :used]))


def resample2d_aa_ws_bytes(sw, sh, dw, dh, planes, filter):
    """mlsd_resample2d_aa_ws_bytes: device workspace of one resample2d_aa call (tables + the intermediate); 0 for arguments it refuses."""
    f = lib().mlsd_resample2d_aa_ws_bytes
    f.restype = ctypes.c_size_t
    return int(f(int(sw), int(sh), int(dw), int(dh), int(planes), int(filter)))


def resample2d_aa(src, sw, sh, dst, dw, dh, planes, filter, wrap=0, ws=None, stream=None):
    """mlsd_resample2d_aa: fp32 planes [planes][sh][sw] -> [planes][dh][dw] through a filter that widens with the shrink factor (AA_*; device pointers; ws:
    resample2d_aa_ws_bytes of device memory); wrap bit 0 columns, bit 1 rows."""
    check(lib().mlsd_resample2d_aa(vp(src), sw, sh, vp(dst), dw, dh, planes, filter, wrap, vp(ws), vp(stream)), "mlsd_resample2d_aa")


def canny_ws_bytes(w, h):
    """mlsd_canny_ws_bytes: device workspace of one canny call (two class maps and the sweeps' flags); 0 for a size it refuses."""
    f = lib().mlsd_canny_ws_bytes
    f.restype = ctypes.c_size_t
    return int(f(int(w), int(h)))


def canny_thresholds(low, high, l2=False):
    """mlsd_canny_thresholds: (lo, hi) as mlsd_canny takes them -- swapped if low > high, floored, under l2 limited to 32767 and squared.  Host only."""
    lo, hi = c_int(), c_int()
    check(lib().mlsd_canny_thresholds(ctypes.c_double(low), ctypes.c_double(high), 1 if l2 else 0, ctypes.byref(lo), ctypes.byref(hi)), "mlsd_canny_thresholds")
    return lo.value, hi.value


def canny_tile(which):
    """mlsd_canny_tile: 0, 1 the classification kernel's tile (x, y); 2, 3 a hysteresis sweep's tile; 4 the sweeps launched per flag read"""
    return int(lib().mlsd_canny_tile(int(which)))


def canny(src, w, h, planes, lo, hi, l2, wrap, dst, planes_out, ws, stream=None):
    """mlsd_canny: fp32 planes [planes][h][w] in [0,1] -> edge map [planes_out][h][w] of 1.0 / 0.0 (device pointers; lo, hi: canny_thresholds; ws: canny_ws_bytes
    of device memory; wrap bit 0 columns, bit 1 rows).  Returns the hysteresis sweeps up to and including the first that changed nothing."""
    n = c_int()
    check(lib().mlsd_canny(vp(src), int(w), int(h), int(planes), int(lo), int(hi), 1 if l2 else 0, int(wrap), vp(dst), int(planes_out), vp(ws), ctypes.byref(n), vp(stream)),
          "mlsd_canny")
    return n.value


def invert(src, dst, n, stream=None):
    """mlsd_invert: dst[i] = 1 - src[i] for n floats (device pointers)"""
    check(lib().mlsd_invert(vp(src), vp(dst), c_i64(n), vp(stream)), "mlsd_invert")


MASK_GROW_MAX, GAUSS_MAX_SIGMA, GAUSS_MAX_TAPS = 256, 64, 321


def mask_weight(mask, p, n, invert, stream=None):
    """mlsd_mask_weight: p[i] = clamp(invert ? mask[i] : 1 - mask[i], 0, 1) for n floats (device pointers); NaN gives 0"""
    check(lib().mlsd_mask_weight(vp(mask), vp(p), c_i64(n), 1 if invert else 0, vp(stream)), "mlsd_mask_weight")


def mask_grow(src, dst, w, h, radius, wrap, ws, stream=None):
    """mlsd_mask_grow: one plane [h][w]; maximum (radius > 0) or minimum (radius < 0) over the (2 |radius| + 1)^2 square (device pointers; ws: w h floats)"""
    check(lib().mlsd_mask_grow(vp(src), vp(dst), int(w), int(h), int(radius), int(wrap), vp(ws), vp(stream)), "mlsd_mask_grow")


def gauss_taps(sigma, k_max=GAUSS_MAX_TAPS):
    """mlsd_gauss_taps: the normalised float taps of sigma (2 int(2.5 sigma + 0.5) + 1 of them) as a list, or None when refused (host only)"""
    w = (ctypes.c_float * max(int(k_max), 1))()
    n = lib().mlsd_gauss_taps(ctypes.c_float(sigma), w, int(k_max))
    return None if n < 0 else [w[i] for i in range(n)]


def gauss_blur_ws_bytes(w, h, planes):
    """mlsd_gauss_blur_ws_bytes: workspace of gauss_blur"""
    f = lib().mlsd_gauss_blur_ws_bytes
    f.restype = ctypes.c_size_t
    return int(f(int(w), int(h), int(planes)))


def gauss_blur(src, dst, w, h, planes, sigma, wrap, ws, stream=None):
    """mlsd_gauss_blur: planes [planes][h][w] blurred with gauss_taps(sigma), rows then columns, fp32 sums in tap order (device pointers; ws: gauss_blur_ws_bytes)"""
    check(lib().mlsd_gauss_blur(vp(src), vp(dst), int(w), int(h), int(planes), ctypes.c_float(sigma), int(wrap), vp(ws), vp(stream)), "mlsd_gauss_blur")


def gauss_blur_lds_limit(nbytes=-1):
    """mlsd_gauss_blur_lds_limit: set the LDS a row-pass tile may use (0 = always read global memory directly; negative only asks); returns the previous limit"""
    return int(lib().mlsd_gauss_blur_lds_limit(int(nbytes)))


def mask_bbox(p, w, h, out4, stream=None):
    """mlsd_mask_bbox: out4 (4 ints, device) = x0, y0, x1, y1 (half open) of the pixels of p [h][w] with a value > 0; zeros if none"""
    check(lib().mlsd_mask_bbox(vp(p), int(w), int(h), vp(out4), vp(stream)), "mlsd_mask_bbox")


def composite(dst, orig, n_orig, patch, p, W, H, planes, B, x0, y0, cw, ch, stream=None):
    """mlsd_composite: dst [B][planes][H][W] = orig outside the rectangle, orig (1 - p) + patch p inside (device pointers; orig of 1 or B images, patch
    [B][planes][ch][cw], p [H][W]); dst may be orig when n_orig == B"""
    check(lib().mlsd_composite(vp(dst), vp(orig), int(n_orig), vp(patch), vp(p), int(W), int(H), int(planes), int(B), int(x0), int(y0), int(cw), int(ch), vp(stream)),
          "mlsd_composite")


WINDOW_MAX_AXIS = 64


def window_gather(canvas, W, H, win, ww, wh, x0, y0, planes, stream=None):
    """mlsd_window_gather: win [planes][wh][ww] <- canvas [planes][H][W] at ((y0 + v) mod H, (x0 + u) mod W), a copy of the bits (device pointers)."""
    check(lib().mlsd_window_gather(vp(canvas), W, H, vp(win), ww, wh, x0, y0, planes, vp(stream)), "mlsd_window_gather")


def window_blend(eps_win, ld_win, eps_canvas, wsum, W, H, ww, wh, x0, y0, ox, oy, N, C=4, stream=None):
    """mlsd_window_blend: eps_canvas [N][H W][4] += (w / wsum) * eps_win [N][wh ww][ld_win] (first 4 channels) of one window (device pointers)."""
    check(lib().mlsd_window_blend(vp(eps_win), c_i64(ld_win), vp(eps_canvas), vp(wsum), W, H, ww, wh, x0, y0, ox, oy, N, C, vp(stream)), "mlsd_window_blend")


def window_wsum(wsum, W, H, ww, wh, xs, ys, ox, oy, stream=None):
    """mlsd_window_wsum: wsum [H W] (device) = sum of the blend weights of the windows starting at xs x ys (host lists)."""
    ax, ay = (c_int * len(xs))(*xs), (c_int * len(ys))(*ys)
    check(lib().mlsd_window_wsum(vp(wsum), W, H, ww, wh, ax, len(xs), ay, len(ys), ox, oy, vp(stream)), "mlsd_window_wsum")


WINDOW_MAX_PACK = 16


def window_gather_packed(canvas, W, H, win, ww, wh, xs, ys, planes, stream=None):
    """mlsd_window_gather_packed: win [len(xs)][planes][wh][ww] <- for slot s, canvas [planes][H][W] at ((ys[s] + v) mod H, (xs[s] + u) mod W) (xs, ys: host lists)."""
    ax, ay = (c_int * max(len(xs), 1))(*xs), (c_int * max(len(ys), 1))(*ys)
    check(lib().mlsd_window_gather_packed(vp(canvas), W, H, vp(win), ww, wh, ax, ay, len(xs), planes, vp(stream)), "mlsd_window_gather_packed")


def window_blend_packed(eps_win, ld_win, eps_canvas, wsum, W, H, ww, wh, xs, ys, n_used, ox, oy, B, G, C=4, stream=None):
    """mlsd_window_blend_packed: eps_canvas [G][B][H W][4] += (w / wsum) * eps_win [G][len(xs)][B][wh ww][ld_win] (first 4 channels) for slots 0 .. n_used-1 in
    order, one launch; the canvas ends as after n_used window_blend launches (xs, ys: host lists of the slots' starts)."""
    ax, ay = (c_int * max(len(xs), 1))(*xs), (c_int * max(len(ys), 1))(*ys)
    check(lib().mlsd_window_blend_packed(vp(eps_win), c_i64(ld_win), vp(eps_canvas), vp(wsum), W, H, ww, wh, ax, ay, n_used, len(xs), ox, oy, B, G, C, vp(stream)),
          "mlsd_window_blend_packed")


def ctrl_add(dst, ld_dst, base, ld_base, ctrl, ld_ctrl, n_img, rows_per_img, C, n_ctrl_img, gain_dev, stream=None):
    """mlsd_ctrl_add: dst[n][r][c] = base[n][r][c] + gain * ctrl[n % n_ctrl_img][r][c] on channels-last fp32 maps (device pointers; gain_dev: one float in device
    memory).  gain == 0 copies base bit for bit without reading ctrl."""
    check(lib().mlsd_ctrl_add(vp(dst), c_i64(ld_dst), vp(base), c_i64(ld_base), vp(ctrl), c_i64(ld_ctrl), n_img, rows_per_img, C, n_ctrl_img, vp(gain_dev), vp(stream)),
          "mlsd_ctrl_add")


def dxdt_guided(eps, ld, x_eval, dx, B, C, HW, cfg, pag=0.0, factor=None, vparam=0, c_out=1.0, c_skip=0.0, stream=None):
    """mlsd_dxdt_guided: dx [B][C][HW] = the guidance mix of eps NHWC [N][HW][ld] (groups cond | uncond at cfg > 1 | perturbed, read at pag != 0).  factor None:
    the v map on each group with vparam, then the mix; factor (device, [B]): the mix of the raw outputs * factor[b], then the v map (device pointers)."""
    f = lib().mlsd_dxdt_guided
    f.argtypes = [vp, c_i64, vp, vp, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, vp, c_int, ctypes.c_float, ctypes.c_float, vp]
    check(f(vp(eps), ld, vp(x_eval), vp(dx), B, C, HW, cfg, pag, vp(factor), int(vparam), c_out, c_skip, vp(stream)), "mlsd_dxdt_guided")


def euler_guided_update(x, eps, ld, B, C, HW, cfg, pag=0.0, factor=None, dt=0.0, noise=None, s_up=0.0, stream=None):
    """mlsd_euler_guided_update: x += mix * dt (+ noise * s_up), the fused Euler(-ancestral) step with the mix of dxdt_guided (eps models), in place"""
    f = lib().mlsd_euler_guided_update
    f.argtypes = [vp, vp, c_i64, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, vp, ctypes.c_float, vp, ctypes.c_float, vp]
    check(f(vp(x), vp(eps), ld, B, C, HW, cfg, pag, vp(factor), dt, vp(noise), s_up, vp(stream)), "mlsd_euler_guided_update")


def dxdt_pag(eps, ld, x_eval, dx, B, C, HW, cfg, pag, vparam=0, c_out=1.0, c_skip=0.0, stream=None):
    """mlsd_dxdt_pag: dxdt_guided without a factor (device pointers)"""
    f = lib().mlsd_dxdt_pag
    f.argtypes = [vp, c_i64, vp, vp, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, c_int, ctypes.c_float, ctypes.c_float, vp]
    check(f(vp(eps), ld, vp(x_eval), vp(dx), B, C, HW, cfg, pag, int(vparam), c_out, c_skip, vp(stream)), "mlsd_dxdt_pag")


def euler_pag_update(x, eps, ld, B, C, HW, cfg, pag, dt, noise=None, s_up=0.0, stream=None):
    """mlsd_euler_pag_update: x += mix * dt (+ noise * s_up), the fused Euler(-ancestral) step with the mix of dxdt_pag (no rescale), in place"""
    f = lib().mlsd_euler_pag_update
    f.argtypes = [vp, vp, c_i64, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, ctypes.c_float, vp]
    check(f(vp(x), vp(eps), ld, B, C, HW, cfg, pag, dt, vp(noise), s_up, vp(stream)), "mlsd_euler_pag_update")


def guidance_blocks(HW):
    """mlsd_guidance_blocks: blocks per image of the guidance-rescale statistics, a rule of HW alone"""
    return int(lib().mlsd_guidance_blocks(int(HW)))


def guidance_scratch_bytes(B, HW):
    f = lib().mlsd_guidance_scratch_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [c_int, c_int]
    return int(f(int(B), int(HW)))


def guidance_stats(eps, ld, B, C, HW, cfg, pag, phi, scratch, scratch_bytes, factor, stream=None):
    """mlsd_guidance_stats: factor [B] = phi * sqrt(M2(cond) / M2(guided)) + 1 - phi per image of eps NHWC [N][HW][ld] (raw outputs; groups as for dxdt_pag);
    scratch: guidance_scratch_bytes(B, HW) bytes of device memory (device pointers)"""
    f = lib().mlsd_guidance_stats
    f.argtypes = [vp, c_i64, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, vp, ctypes.c_size_t, vp, vp]
    check(f(vp(eps), ld, B, C, HW, cfg, pag, phi, vp(scratch), scratch_bytes, vp(factor), vp(stream)), "mlsd_guidance_stats")


def dxdt_rescaled(eps, ld, x_eval, dx, B, C, HW, cfg, pag, factor, vparam=0, c_out=1.0, c_skip=0.0, stream=None):
    """mlsd_dxdt_rescaled: dx = guided mix of the raw outputs * factor[b], then the v map with vparam (device pointers)"""
    f = lib().mlsd_dxdt_rescaled
    f.argtypes = [vp, c_i64, vp, vp, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, vp, c_int, ctypes.c_float, ctypes.c_float, vp]
    check(f(vp(eps), ld, vp(x_eval), vp(dx), B, C, HW, cfg, pag, vp(factor), int(vparam), c_out, c_skip, vp(stream)), "mlsd_dxdt_rescaled")


def euler_rescaled_update(x, eps, ld, B, C, HW, cfg, pag, factor, dt, noise=None, s_up=0.0, stream=None):
    """mlsd_euler_rescaled_update: x += rescaled mix * dt (+ noise * s_up), in place (eps models)"""
    f = lib().mlsd_euler_rescaled_update
    f.argtypes = [vp, vp, c_i64, c_int, c_int, c_int, ctypes.c_float, ctypes.c_float, vp, ctypes.c_float, vp, ctypes.c_float, vp]
    check(f(vp(x), vp(eps), ld, B, C, HW, cfg, pag, vp(factor), dt, vp(noise), s_up, vp(stream)), "mlsd_euler_rescaled_update")


def tile_permute(src, dst, n_img, H, W, th, tw, row_bytes, inverse=False, stream=None):
    """mlsd_tile_permute: dense [n_img][H W] rows of row_bytes bytes from image order into tile-major order (tiles of th x tw rows), or back with inverse
    (device pointers; 16-byte aligned, row_bytes a multiple of 16, no overlap)"""
    check(lib().mlsd_tile_permute(vp(src), vp(dst), n_img, H, W, th, tw, row_bytes, 1 if inverse else 0, vp(stream)), "mlsd_tile_permute")


def freeu_ws_bytes(n_img, H, W, C):
    """mlsd_freeu_ws_bytes: workspace of either FreeU kernel for n_img maps of H x W x C"""
    f = lib().mlsd_freeu_ws_bytes
    f.restype = ctypes.c_size_t
    return int(f(n_img, H, W, C))


def freeu_depth(n_terms):
    """mlsd_freeu_depth: the largest number of fp32 additions between a term and its finished sum of n_terms in the FreeU kernels"""
    return int(lib().mlsd_freeu_depth(int(n_terms)))


def freeu_backbone(dst, ld_dst, src, ld_src, n_img, rows_per_img, C, ws, b_dev, stream=None):
    """mlsd_freeu_backbone: dst = src with its first C / 2 channels times (b - 1) x the per-image normalised channel-mean map + 1 (device pointers; b_dev: one
    float in device memory; ws: freeu_ws_bytes).  b == 1 copies src bit for bit."""
    check(lib().mlsd_freeu_backbone(vp(dst), c_i64(ld_dst), vp(src), c_i64(ld_src), n_img, rows_per_img, C, vp(ws), vp(b_dev), vp(stream)), "mlsd_freeu_backbone")


def freeu_skip(dst, ld_dst, src, ld_src, n_img, H, W, C, ws, s_dev, stream=None):
    """mlsd_freeu_skip: dst = src with the four lowest spatial frequencies of every H x W plane times s (device pointers; s_dev: one float in device memory).
    s == 1 copies src bit for bit."""
    check(lib().mlsd_freeu_skip(vp(dst), c_i64(ld_dst), vp(src), c_i64(ld_src), n_img, H, W, C, vp(ws), vp(s_dev), vp(stream)), "mlsd_freeu_skip")


def window_gather_nhwc(src, W, H, C, dst, ww, wh, xs, ys, n_rep, stream=None):
    """mlsd_window_gather_nhwc: dst [len(xs)][n_rep][wh][ww][C] <- src [H][W][C] at ((ys[s] + v) mod H, (xs[s] + u) mod W), bit copies (xs, ys: host lists)."""
    ax, ay = (c_int * max(len(xs), 1))(*xs), (c_int * max(len(ys), 1))(*ys)
    check(lib().mlsd_window_gather_nhwc(vp(src), W, H, C, vp(dst), ww, wh, ax, ay, len(xs), n_rep, vp(stream)), "mlsd_window_gather_nhwc")


def tile_pack(n_win, n_batch, pack):
    """mlis_amd_tile_pack: (windows per plan evaluation, plan evaluations) for n_win windows of n_batch images and at most `pack` windows per evaluation; None if refused."""
    n_eval = c_int()
    p = lib().mlis_amd_tile_pack(int(n_win), int(n_batch), int(pack), ctypes.byref(n_eval))
    return None if p < 0 else (p, n_eval.value)


def window_starts(L, T, O, wrap=False, cap=256):
    """mlis_amd_window_starts: the window starts along one axis (canvas extent L, window T, minimum overlap O, in latent pixels), or None if refused."""
    out = (c_int * cap)()
    n = lib().mlis_amd_window_starts(int(L), int(T), int(O), int(bool(wrap)), out, cap)
    return None if n < 0 else [out[i] for i in range(n)]


def sync():
    check(lib().mlsd_device_sync(), "sync")
