"""mlsd_gemm_args for the routing tests: UNet and decoder shapes, each epilogue form, table and forced tile variants.  The operands are
aligned addresses that nothing dereferences: the routing queries look at pointers only for null and alignment, and no test here launches."""
import ctypes
import itertools

from mlimgsynth_amd import kernels as K
from mlimgsynth_amd._lib import lib

LINEAR = [(8192, 320, 320), (8192, 320, 1280), (8192, 1280, 1280), (8192, 1280, 5120), (8192, 2560, 1280), (2048, 640, 640), (2048, 640, 2560),
          (2048, 1280, 5120), (4096, 1280, 1280), (16384, 640, 640), (32768, 640, 640), (1024, 1280, 1280), (512, 1280, 11520), (308, 1280, 2048),
          (128, 1280, 1280), (64, 1280, 320), (16, 1280, 320)]
# (images, H, W, Cin, Cout, kernel, stride, upsample)
CONV = [(1, 64, 64, 320, 320, 3, 1, 0), (2, 32, 32, 640, 640, 3, 1, 0), (1, 16, 16, 1280, 1280, 3, 1, 0), (1, 8, 8, 1280, 1280, 3, 1, 0),
        (1, 32, 32, 320, 320, 3, 2, 0), (1, 32, 32, 1280, 1280, 3, 1, 1), (2, 64, 64, 640, 320, 1, 1, 0), (1, 128, 128, 128, 3, 3, 1, 0),
        (1, 128, 128, 64, 16, 3, 1, 0), (2, 128, 128, 512, 512, 3, 1, 0), (1, 256, 256, 256, 128, 3, 1, 0)]
EPILOGUES = ["f32", "f16", "f32+f16", "bias", "resid", "silu", "gelu16", "geglu16", "rowbias", "bias_m", "colstats", "ln", "resid+ln", "gn", "xattn"]
TILES = [0] + [K.tile_arg(v) for v in sorted(K.TILE_LABELS)] + [K.tile_arg(2), K.tile_arg(5)]

_next = [1 << 36]


def addr():
    _next[0] += 1 << 26
    return _next[0]


def shape_args(shape):
    a = K.GemmArgs()
    a.A, a.W_ = addr(), addr()
    if len(shape) == 3:
        a.M, a.N, a.K = shape
        a.lda = a.ldb = a.K
    else:
        n, H, W, Cin, Cout, k, stride, ups = shape
        a.conv, a.n_img, a.H, a.W, a.Cin, a.KH, a.KW, a.stride, a.upsample = 1, n, H, W, Cin, k, k, stride, ups
        a.pad = k // 2
        a.OH, a.OW = (H * (1 + ups) + 2 * a.pad - k) // stride + 1, (W * (1 + ups) + 2 * a.pad - k) // stride + 1
        a.M, a.N, a.K = n * a.OH * a.OW, Cout, k * k * Cin
        a.lda, a.ldb = Cin, a.K
    return a


def with_epilogue(a, epi):
    """the args with epilogue form `epi`, or None where the form does not apply to the shape"""
    f32 = epi in ("f32", "bias", "resid", "silu", "rowbias", "bias_m", "colstats", "ln", "resid+ln", "gn") or epi == "f32+f16"
    if epi == "geglu16" and a.N % 64:
        return None
    if epi in ("ln", "resid+ln", "xattn") and a.conv:
        return None
    if f32:
        a.C32, a.ldc32 = addr(), a.N
    if epi in ("f16", "f32+f16", "gelu16", "geglu16"):
        a.C16, a.ldc16 = addr(), a.N // 2 if epi == "geglu16" else a.N
    if epi in ("bias", "silu", "gelu16", "xattn"):
        a.bias = addr()
    if epi in ("resid", "resid+ln"):
        a.resid, a.ldr = addr(), a.N
    a.act = {"silu": K.ACT_SILU, "gelu16": K.ACT_GELU, "geglu16": K.ACT_GEGLU}.get(epi, K.ACT_NONE)
    if epi == "rowbias":
        a.rowbias, a.ldrb, a.rows_per_batch = addr(), a.N, max(a.M // 2, 1)
    if epi == "bias_m":
        a.bias_m = addr()
    if epi == "colstats":
        a.colstats, a.colstats_shift = addr(), 1
    if epi in ("ln", "resid+ln"):
        attach_ln(a)
    if epi == "gn":
        if a.N % 32:
            return None
        a.gn_y16, a.gn_ldy, a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_groups, a.gn_hw = addr(), a.N, addr(), addr(), 1e-5, 32, a.M // (a.n_img or 1)
    if epi == "xattn":
        a.xa_k, a.xa_ldk, a.xa_vt, a.xa_out, a.xa_ldo, a.xa_Tq, a.xa_Tk = addr(), a.N, addr(), addr(), a.N, 1024, 77
    return a


def attach_ln(a):
    a.ln_y16, a.ldln, a.ln_gamma, a.ln_beta, a.ln_eps, a.ln_ws, a.ln_cnt = addr(), a.N, addr(), addr(), 1e-5, addr(), addr()


def cases():
    """(description, args) over shapes x epilogues x tile requests x K splits"""
    for shape, epi, tile, ksplit in itertools.product(LINEAR + CONV, EPILOGUES, TILES, (1, 4)):
        a = with_epilogue(shape_args(shape), epi)
        if a is None:
            continue
        a.tile_variant, a.ksplit = tile, ksplit
        a.ws, a.ws_bytes = addr(), 1 << 28
        if ksplit > 1 or tile in (K.tile_arg(K.TILE_PPSK_256x256), K.tile_arg(K.TILE_PPSK_128x320)):
            a.sk_flags = addr()
        yield f"{shape} {epi} tile_variant={tile} ksplit={ksplit}", a


def check_route(desc, a, forced=-1):
    """the route agrees with the six queries, with mlsd_gemm_variant's label, and its what-if answers with the queries on the args that ask"""
    L = lib()
    for f in ("mlsd_gemm_colstats_rows", "mlsd_gemm_ln_fused", "mlsd_gemm_gn_fused", "mlsd_gemm_xattn_fused", "mlsd_gemm_splitk_parallel",
              "mlsd_conv_smalln_eligible"):
        getattr(L, f).argtypes = [ctypes.POINTER(K.GemmArgs)]
    r = K.gemm_route(a)
    label = K.gemm_variant(a)
    got = (r.stats_rows, r.ln, r.gn, r.xattn)
    want = (L.mlsd_gemm_colstats_rows(a), L.mlsd_gemm_ln_fused(a), L.mlsd_gemm_gn_fused(a), L.mlsd_gemm_xattn_fused(a))
    assert got == want, (desc, got, want)
    par = L.mlsd_gemm_splitk_parallel(a)
    assert r.handoff == ("ppsk" in label or r.ln == 1 or par), (desc, label, r.handoff)
    if r.variant in K.TILE_LABELS:
        assert label.startswith(f"gemm<{K.TILE_LABELS[r.variant]},"), (desc, label, r.variant)
    if r.nsplit > 1:
        assert f"k/{r.nsplit}" in label, (desc, label, r.nsplit)
    if forced >= 0:
        pick = forced
    elif r.xattn:
        pick = K.TILE_PP_128x320
    elif L.mlsd_conv_smalln_eligible(a):
        pick = K.TILE_CONV_SMALLN
    else:
        pick = a.tile_variant - 1 if a.tile_variant > 0 else None
    if pick is not None:
        assert r.asked == (r.variant == pick), (desc, label, r.asked, pick)
    w = K.GemmArgs.from_buffer_copy(a)
    if not w.colstats:
        w.colstats = addr()
    assert r.stats_rows_if == L.mlsd_gemm_colstats_rows(w), desc
    w = K.GemmArgs.from_buffer_copy(a)
    if not w.ln_y16:
        attach_ln(w)
    assert r.ln_if == L.mlsd_gemm_ln_fused(w), desc
    if r.ln_if == 1:
        bn = 160 if K.gemm_route(w).variant == K.TILE_TT else 320
        assert r.ln_ws_bytes_if == a.M * (a.N // bn) * 16, desc
    else:
        assert r.ln_ws_bytes_if == 0, desc
    return r


def forced_cases():
    """(description, forced variant, args): every named tile forced on a few shapes and epilogues"""
    for v in sorted(K.TILE_LABELS):
        for shape, epi in itertools.product([(8192, 1280, 1280), (128, 1280, 1280), (1, 128, 128, 128, 3, 3, 1, 0), (2, 32, 32, 640, 640, 3, 1, 0)],
                                            ["f32", "f16", "colstats", "ln"]):
            a = with_epilogue(shape_args(shape), epi)
            if a is None:
                continue
            a.ws, a.ws_bytes, a.sk_flags = addr(), 1 << 28, addr()
            yield f"forced {v} {shape} {epi}", v, a


# a shape each tile takes, for the name test (stream-K: on a device only)
TAKES = {K.TILE_SKINNY: ((128, 1280, 1280), "f32"), K.TILE_CONV_SMALLN: ((1, 128, 128, 128, 3, 3, 1, 0), "f32"),
         K.TILE_PPSK_256x256: ((2048, 1280, 5120), "f32"), K.TILE_PPSK_128x320: ((512, 1280, 11520), "f32")}


def tile_label_when_forced(v):
    shape, epi = TAKES.get(v, ((8192, 1280, 1280), "f32"))
    a = with_epilogue(shape_args(shape), epi)
    a.ws, a.ws_bytes, a.sk_flags = addr(), 1 << 28, addr()
    L = lib()
    L.mlsd_gemm_force_variant(v)
    try:
        return K.gemm_variant(a), K.gemm_route(a)
    finally:
        L.mlsd_gemm_force_variant(-1)
