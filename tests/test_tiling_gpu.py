"""Seamless tiling on the GPU: every convolution path with circular padding against a float64 reference per output element (the fp16
source padded with np.pad(mode="wrap"), then tests/ref64.py's im2col with pad 0 and its bounds), the UNets and codecs equivariant under
circular shifts, and the public option end to end on synthetic models."""
import ctypes as C

import numpy as np
import pytest

import gemm64_cases as GC
import mlis_ffi as F
import ref64 as R
import tolerances as T

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# (id, forced tile, n, H, W, cin, cout, k, s, p, p_end, ups, wrap, options)
WRAP_CASES = [
    ("g0_xy_ragged", 0, 2, 7, 9, 24, 40, 3, 1, 1, 1, 0, 3, dict(bias=True, c16=True)),
    ("g0_x", 0, 2, 6, 5, 64, 72, 3, 1, 1, 1, 0, 1, {}),
    ("g0_y", 0, 2, 5, 6, 64, 72, 3, 1, 1, 1, 0, 2, {}),
    ("g0_extent1", 0, 2, 1, 1, 16, 24, 3, 1, 1, 1, 0, 3, {}),
    ("g0_extent2", 0, 3, 2, 1, 16, 24, 3, 1, 1, 1, 0, 3, {}),
    ("g0_extent3_s2", 0, 2, 3, 3, 16, 24, 3, 2, 1, 1, 0, 3, {}),
    ("g0_end_only", 0, 2, 8, 10, 64, 64, 3, 2, 0, 1, 0, 3, dict(bias=True)),
    ("g1_x", 1, 2, 5, 6, 64, 72, 3, 1, 1, 1, 0, 1, dict(resid=True)),
    ("g3_s2", 3, 2, 16, 16, 64, 128, 3, 2, 1, 1, 0, 2, {}),
    ("g4_ups", 4, 2, 6, 5, 32, 64, 3, 1, 1, 1, 1, 3, {}),
    ("g9_res", 9, 2, 9, 11, 64, 256, 3, 1, 1, 1, 0, 3, dict(resid=True)),
    ("g16", 16, 2, 8, 8, 64, 320, 3, 1, 1, 1, 0, 3, {}),
    ("g0_splitk", 0, 1, 4, 4, 256, 128, 3, 1, 1, 1, 0, 3, dict(ksplit=4)),
    ("g0_splitk_stats", 0, 1, 4, 4, 256, 128, 3, 1, 1, 1, 0, 3, dict(ksplit=4, stats=True)),
    ("p17_xy", 17, 2, 8, 16, 64, 128, 3, 1, 1, 1, 0, 3, {}),
    ("p17_end_only", 17, 2, 32, 32, 64, 128, 3, 2, 0, 1, 0, 3, {}),
    ("p17_stats", 17, 2, 8, 16, 64, 128, 3, 1, 1, 1, 0, 3, dict(stats=True)),
    ("p18_x_res", 18, 2, 8, 8, 64, 160, 3, 1, 1, 1, 0, 1, dict(resid=True)),
    ("p20_ups", 20, 2, 4, 4, 64, 160, 3, 1, 1, 1, 1, 3, {}),
    ("p21_s2_y", 21, 2, 16, 16, 64, 64, 3, 2, 1, 1, 0, 2, {}),
    ("p21_extent2", 21, 32, 2, 2, 64, 64, 3, 1, 1, 1, 0, 3, {}),
    ("k19", 19, 1, 16, 16, 256, 256, 3, 1, 1, 1, 0, 3, {}),
    ("k28_res", 28, 2, 8, 8, 256, 320, 3, 1, 1, 1, 0, 3, dict(resid=True)),
    ("k28", 28, 2, 8, 8, 256, 320, 3, 1, 1, 1, 0, 1, {}),
    # the statistics builds (column sums for a consuming GroupNorm) of the general and ping-pong tiles, and the other epilogue builds the plans use
    ("g0_stats", 0, 2, 7, 9, 64, 128, 3, 1, 1, 1, 0, 3, dict(stats=True)),
    ("g1_stats_ups", 1, 2, 3, 5, 64, 128, 3, 1, 1, 1, 1, 3, dict(stats=True, resid=True)),
    ("g4_stats_res", 4, 2, 9, 8, 64, 128, 3, 1, 1, 1, 0, 3, dict(stats=True, resid=True)),
    ("g9_stats_ups", 9, 2, 5, 6, 64, 256, 3, 1, 1, 1, 1, 3, dict(stats=True, c16=True)),
    ("g16_c16_s2", 16, 2, 16, 14, 64, 320, 3, 2, 1, 1, 0, 3, dict(c16=True, resid=True)),
    ("p17_res_stats", 17, 2, 8, 16, 64, 128, 3, 1, 1, 1, 0, 3, dict(stats=True, resid=True)),
    ("p18_res_stats", 18, 2, 8, 8, 64, 160, 3, 1, 1, 1, 0, 3, dict(stats=True, resid=True)),
    ("p18", 18, 2, 8, 8, 64, 160, 3, 1, 1, 1, 0, 2, {}),
    ("p20_stats", 20, 2, 8, 8, 64, 160, 3, 1, 1, 1, 0, 3, dict(stats=True)),
    ("p20_res", 20, 2, 8, 8, 64, 160, 3, 1, 1, 1, 0, 3, dict(resid=True)),
    ("p20_res_stats", 20, 2, 8, 8, 64, 160, 3, 1, 1, 1, 0, 1, dict(stats=True, resid=True)),
    ("p20_ups_stats", 20, 2, 4, 4, 64, 160, 3, 1, 1, 1, 1, 2, dict(stats=True)),
    ("p21_ups", 21, 2, 4, 8, 64, 64, 3, 1, 1, 1, 1, 3, {}),
    ("p21_ups_stats", 21, 2, 4, 8, 64, 64, 3, 1, 1, 1, 1, 3, dict(stats=True)),
    ("p21_stats", 21, 2, 8, 8, 64, 64, 3, 1, 1, 1, 0, 3, dict(stats=True)),
    ("p21_res_stats", 21, 2, 8, 8, 64, 64, 3, 1, 1, 1, 0, 3, dict(stats=True, resid=True)),
    ("p21_res", 21, 2, 8, 8, 64, 64, 3, 1, 1, 1, 0, 3, dict(resid=True)),
    ("p17_ups_stats", 17, 2, 4, 8, 64, 128, 3, 1, 1, 1, 1, 3, dict(stats=True)),
    ("s29", 29, 2, 4, 6, 64, 128, 3, 1, 1, 1, 0, 3, {}),
    ("s29_extent1", 29, 2, 1, 3, 64, 128, 3, 1, 1, 1, 0, 3, dict(bias=True)),
    ("n31_xy", 31, 2, 96, 91, 64, 16, 3, 1, 1, 1, 0, 3, dict(bias=True)),
    ("n31_x", 31, 2, 65, 130, 128, 3, 3, 1, 1, 1, 0, 1, dict(bias=True)),
]


def make_case(cid, tile, n, H, W, cin, cout, k, s, p, p_end, ups, wrap, opt):
    c = GC.conv(cid, "", "wrap", n, H, W, cin, cout, k, s, p, ups=ups, tv=GC.tv(tile), ws=True, **opt)
    Hs, Ws = (2 * H, 2 * W) if ups else (H, W)
    c["OH"], c["OW"] = (Hs + p + p_end - k) // s + 1, (Ws + p + p_end - k) // s + 1
    c["M"] = n * c["OH"] * c["OW"]
    c.update(tile=tile, p_end=p_end, wrap=wrap, sk=tile in (19, 28))
    return c


def wrap_reference(c, A):
    """the im2col of the circularly padded fp16 source, float64"""
    n, H, W, cp = c["n"], c["H"], c["W"], c["cin_pad"]
    x = np.asarray(A, np.float64).reshape(n, H, W, cp)
    if c["ups"]:
        x = x.repeat(2, axis=1).repeat(2, axis=2)
    py = (c["p"], c["p_end"])
    px = (c["p"], c["p_end"])
    x = np.pad(x, ((0, 0), py if c["wrap"] & 2 else (0, 0), px if c["wrap"] & 1 else (0, 0), (0, 0)), mode="wrap")
    x = np.pad(x, ((0, 0), (0, 0) if c["wrap"] & 2 else py, (0, 0) if c["wrap"] & 1 else px, (0, 0)))
    _, He, We, _ = x.shape
    return R.im2col64(x.reshape(-1, cp), n, He, We, cp, c["k"], c["k"], c["s"], 0, 0, c["OH"], c["OW"])


def case_args(c, ops, keep):
    """the launch of case c on device copies of its operands (kept alive in `keep`), with its outputs; (args, C32, C16)"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    d = lambda v: keep.append(_lib.from_numpy(np.ascontiguousarray(v))) or keep[-1].ptr
    M, N, Kd = c["M"], c["N"], c["K"]
    a = K.GemmArgs(A=d(ops["A"]), lda=c["cin_pad"], W_=d(ops["W"]), ldb=Kd, M=M, N=N, K=Kd, tile_variant=c["tv"], ksplit=c["ksplit"])
    a.conv, a.n_img, a.H, a.W, a.Cin, a.OH, a.OW = 1, c["n"], c["H"], c["W"], c["cin_pad"], c["OH"], c["OW"]
    a.KH = a.KW = c["k"]
    a.stride, a.pad, a.upsample, a.wrap = c["s"], c["p"], c["ups"], c["wrap"]
    if c["bias"]:
        a.bias = d(ops["bias"])
    if c["resid"]:
        a.resid, a.ldr = d(ops["resid"]), N
    L = _lib.lib()
    L.mlsd_gemm_streamk_ws_bytes.restype = C.c_size_t
    nb = max(K.gemm_splitk_ws_bytes(M, N, max(c["ksplit"], 2)), L.mlsd_gemm_streamk_ws_bytes() if c["sk"] else 0)
    a.ws, a.ws_bytes = d(np.zeros(nb // 4, np.float32)), nb
    if c["sk"]:
        a.sk_flags = d(np.zeros(4096, np.uint32))
    if c["stats"]:
        a.colstats, a.colstats_shift = d(np.zeros(2 * N * (M // 32 + 2), np.float32)), 1
    C32 = _lib.DeviceBuffer(M * N * 4)
    a.C32, a.ldc32 = C32.ptr, N
    C16 = _lib.DeviceBuffer(M * N * 2) if c["c16"] else None
    if C16:
        a.C16, a.ldc16 = C16.ptr, N
    keep += [C32, C16]
    return a, C32, C16


def build_key(a, r):
    """the kernel build a wrap launch runs: general tiles (tile, statistics build); ping-pong / stream-K tiles (tile, upsample, residual,
    statistics: the CONV | 4 build and its epilogue); the others (tile)"""
    if r.variant in (0, 1, 3, 4, 9, 16):
        return (r.variant, r.stats_rows > 0 and r.nsplit == 1)
    if r.variant in (17, 18, 19, 20, 21, 28):
        return (r.variant, bool(a.upsample), bool(a.resid), r.stats_rows > 0, bool(a.C16))
    return (r.variant,)


def prepared(spec):
    c = make_case(*spec)
    ops = GC.make_operands(c)
    # distinct images: image b's pixels carry an offset of its own, so a tap that reads the neighbouring image shows
    A = ops["A"].astype(np.float32).reshape(c["n"], -1, c["cin_pad"])
    A[..., :c["cin"]] += np.arange(c["n"], dtype=np.float32)[:, None, None] * 0.5
    ops["A"] = A.reshape(-1, c["cin_pad"]).astype(np.float16)
    return c, ops


@pytest.mark.parametrize("spec", WRAP_CASES, ids=[w[0] for w in WRAP_CASES])
def test_wrap_conv_float64(spec):
    from mlimgsynth_amd import kernels as K
    c, ops = prepared(spec)
    keep = []
    a, C32, C16 = case_args(c, ops, keep)
    M, N, Kd = c["M"], c["N"], c["K"]
    r = K.gemm_route(a)
    label = K.gemm_variant(a)
    assert r.variant == c["tile"] and r.asked, (c["id"], label, r.variant)
    K.gemm(a)
    K.sync()
    got = C32.download((M, N), np.float32)
    general = c["tile"] in (0, 1, 3, 4, 9, 16)
    D = R.gemm_depth(Kd, R.K_STEP_GENERAL if general else R.K_STEP_MFMA16, r.nsplit + (Kd // 64 if c["sk"] else 0))
    acc, S = R.gemm64(wrap_reference(c, ops["A"]), ops["W"])
    y, b = R.gemm_epilogue64(acc, S, D, np.arange(M), np.arange(N), bias=ops.get("bias"), resid=ops.get("resid"))
    ratio = R.gemm_ratio32(got, y, b)
    worst = float(np.nan_to_num(ratio, nan=1e300).max())
    print(f"{c['id']:18s} {label:32s} worst C32 ratio {worst:.3f}")
    assert worst <= 1.0, (c["id"], label, worst, np.argwhere(~(ratio <= 1.0))[:4].tolist())
    if C16:
        assert (R.fp16_rne(got).view(np.uint16) == C16.download((M, N), np.float16).view(np.uint16)).all()
    # the zero-padded launch of the same operands differs on the border (the wrap is not a no-op)
    if c["p"] > 0:
        a.wrap = 0
        K.gemm(a)
        K.sync()
        assert not np.array_equal(C32.download((M, N), np.float32), got), c["id"]


# ------------------------------------------------------------------ census
def taps_leave(g):
    He, We = g.H * (1 + g.upsample), g.W * (1 + g.upsample)
    return g.pad > 0 or (g.OH - 1) * g.stride - g.pad + g.KH > He or (g.OW - 1) * g.stride - g.pad + g.KW > We


def test_every_planned_wrap_launch_has_a_case():
    """every kernel build that the SD1.5 b1 and SDXL b4 UNet plans and the two VAE decode plans run a wrap launch on has a float64 case above"""
    from mlimgsynth_amd import _lib, engine
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    L.mlctx_op_gemm_args.restype = C.POINTER(K.GemmArgs)
    L.mlctx_op_gemm_args.argtypes = [C.c_void_p, C.c_int]
    covered, keep = set(), []
    for spec in WRAP_CASES:
        c, ops = prepared(spec)
        a = case_args(c, ops, keep)[0]
        covered.add(build_key(a, K.gemm_route(a)))
        keep.clear()

    def planned(ctx, what):
        out = {}
        for i in range(ctx.info().n_ops):
            p = L.mlctx_op_gemm_args(ctx.h, i)
            if p and p.contents.conv and taps_leave(p.contents):
                g = K.GemmArgs.from_buffer_copy(p.contents)
                assert g.wrap == 3, what
                out[build_key(g, K.gemm_route(g))] = K.gemm_variant(g)
        return out

    seen = {}
    for model, lat, n in (("sd1", 64, 2), ("sdxl", 128, 8)):
        un = engine.Unet(model, lat, lat, n, synth=False, tiling=3)
        seen.update(planned(un.ctx, model))
        un.ctx.destroy()
    for model in ("sd1", "sdxl"):
        dec = engine.Decoder(model, 128, 128, 4, tiling=3)
        seen.update(planned(dec.ctx, model + " decoder"))
        dec.ctx.destroy()
    assert len(seen) >= 15
    missing = {k: lab for k, lab in seen.items() if k not in covered}
    assert not missing, missing


# ------------------------------------------------------------------ equivariance
def levels(P):
    return sum(1 for m in P.ch_mult if m) - 1


@pytest.mark.parametrize("model,lw,lh", [("sd1", 24, 16), ("sdxl", 20, 12), ("tinyxl", 12, 8)])
def test_unet_is_equivariant_under_circular_shifts(model, lw, lh):
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(7)
    n = 2
    P = engine.unet_params(model)
    q = 2 ** levels(P)
    x = rng.standard_normal((n, 4, lh, lw)).astype(np.float32)
    cond = rng.standard_normal((n, 77, P.n_ctx)).astype(np.float32)
    label = rng.standard_normal((n, P.ch_adm_in)).astype(np.float32) if P.ch_adm_in else None
    sigma = np.array([3.0, 0.7], np.float32)
    shifts = [(q, 2 * q), (-q, q)]          # (dy, dx) per image

    def roll(v, axes=(1, 2)):
        return np.stack([np.roll(v[i], shifts[i], axis=axes) for i in range(n)])

    def err(tiling, rolled=roll):
        un = engine.Unet(model, lw, lh, n, tiling=tiling)
        try:
            e0 = un.run(x, cond, label, sigma)
            e1 = un.run(rolled(x), cond, label, sigma)
        finally:
            un.ctx.destroy()
        return rel(e1, rolled(e0))

    e_xy = err(3)
    # The shifted image's pixels meet in other orders in the sums over pixels and keys (GroupNorm and column statistics, attention softmax), so a
    # few fp32 sums round differently, a few fp16 activations flip by one ulp, and the synthetic UNet amplifies such flips to its own noise level.
    # That level, measured directly: the output change when 1 % of the input's fp16 values move by one ulp.  Measured on MI355X (shift error /
    # floor): sd1 1.48e-3 / 1.51e-3, sdxl 2.21e-3 / 2.22e-3, tinyxl 1.18e-3 / 1.26e-3 -- the shift error IS the floor (adding a third image to
    # the batch moves sdxl's output by the same 2.16e-3).  Bounds: twice the measured shift error, and 1.5x the floor of the same run.
    un = engine.Unet(model, lw, lh, n, tiling=3)
    try:
        x16 = x.astype(np.float16)
        flip = rng.random(x.shape) < 0.01
        xp = np.where(flip, np.nextafter(x16, np.float16(np.inf)), x16).astype(np.float32)
        floor = rel(un.run(xp, cond, label, sigma), un.run(x16.astype(np.float32), cond, label, sigma))
    finally:
        un.ctx.destroy()
    print(model, f"circular-shift equivariance rel-L2: {e_xy:.3e}, one-ulp floor {floor:.3e}")
    bound = {"sd1": 3e-3, "sdxl": 4.5e-3, "tinyxl": 2.5e-3}[model]
    assert e_xy < bound and e_xy < 1.5 * floor
    assert err(0) > 10 * bound                                       # zero padding is not equivariant
    roll_y = lambda v: np.stack([np.roll(v[i], shifts[i][0], axis=1) for i in range(n)])
    assert err(1, roll_y) > 10 * bound                               # x only: a shift along y is not


@pytest.mark.parametrize("model,tae", [("sd1", False), ("sdxl", False), ("sd1", True)])
def test_decoder_is_equivariant_under_circular_shifts(model, tae):
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(3)
    lw, lh, s = 12, 8, (3, -2)
    z = rng.standard_normal((2, 4, lh, lw)).astype(np.float32)
    dec = engine.Decoder(model, lw, lh, 2, tae=tae, tiling=3)
    try:
        y0 = dec.run(z)
        y1 = dec.run(np.roll(z, s, axis=(2, 3)))
    finally:
        dec.ctx.destroy()
    e = rel(y1, np.roll(y0, (8 * s[0], 8 * s[1]), axis=(2, 3)))
    print(model, "tae" if tae else "vae", "decoder circular-shift equivariance rel-L2:", e)
    # measured on MI355X: sd1 / sdxl KL-VAE 3.2e-4 / 3.0e-4, TAESD 0 (no reduction across pixels: every pixel sums the same terms in the same order)
    assert e < T.EVAL_SMALL


ENC_BOUND = T.EVAL_SMALL


@pytest.mark.parametrize("model,tae", [("sd1", False), ("sdxl", False), ("sd1", True)])
def test_encoder_is_equivariant_under_circular_shifts(model, tae):
    """the encoder of a tiling engine (mlis_amd_encoder_prepare: what img2img and in-painting run), the KL-VAE's end-only-padded stride-2
    downsamples included: an image shift by 8 s is a latent shift by s; the same engine without tiling is not equivariant"""
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(5)
    lw, lh, s = 16, 8, (3, -2)        # (a latent the SD1.5 UNet of the engine takes: sides multiple of 8)
    img = rng.random((2, 3, lh * 8, lw * 8)).astype(np.float32)

    def err(tiling):
        g = engine.Generator(model, lw * 8, lh * 8, 2, use_tae=tae, cfg_scale=1.0, tiling=tiling)
        try:
            z0 = g.encode(img, sample=False)
            z1 = g.encode(np.roll(img, (8 * s[0], 8 * s[1]), axis=(2, 3)), sample=False)
        finally:
            g.destroy()
        return rel(z1, np.roll(z0, s, axis=(2, 3)))

    e = err(3)
    print(model, "tae" if tae else "vae", "encoder circular-shift equivariance rel-L2:", e)
    # measured on MI355X: KL-VAE (sd1, sdxl) 9.5e-4, TAESD 0; an encoder plan built without the wrap (the engine's encoder context not given
    # the mode) measures 0.76 / 0.88: this test fails
    assert e < ENC_BOUND
    assert err(0) > 10 * ENC_BOUND


# ------------------------------------------------------------------ public API
@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return F.bind(_lib.LIB_PATH)


TOKS = np.array([5, 17, 300, 42, 7], np.int32)


def has_vae_tile_plan(lib, m):
    """whether the context's engine holds a tile-sized decoder plan (mlis_amd_ctx_at 3): vae_tile only tiles an image larger than one tile + margins"""
    lib.mlis_amd_engine_get.restype, lib.mlis_amd_engine_get.argtypes = C.c_void_p, [C.c_void_p]
    lib.mlis_amd_ctx_at.restype, lib.mlis_amd_ctx_at.argtypes = C.c_void_p, [C.c_void_p, C.c_int]
    eng = lib.mlis_amd_engine_get(m.ctx)
    return bool(eng and lib.mlis_amd_ctx_at(eng, 3))


def generate(lib, tiling=None, tae=False, image=None, vae_tile=0, expect=1, dim=64, tile_plan=False):
    m = F.Mlis(lib)
    try:
        m.set("model", "synth:tiny")
        m.set("image_dim", dim, dim)
        m.set("steps", 3)
        m.set("seed", 42)
        m.tokens(TOKS)
        if tae:
            m.set("tae", "synth")
        if tiling is not None:
            m.set("tiling", tiling)
        if vae_tile:
            m.set("vae_tile", vae_tile)
        if image is not None:
            m.set("f_t_ini", 0.5)
            im = F.Image(image.ctypes.data_as(C.POINTER(C.c_uint8)), image.size, 64, 64, image.shape[2], 0)
            assert lib.mlis_option_set(m.ctx, F.OPT["IMAGE"], C.byref(im)) == 1
        r = lib.mlis_generate(m.ctx)
        assert r == expect, (r, m.err())
        if r < 0:
            return None, m.err(), None
        assert has_vae_tile_plan(lib, m) == tile_plan
        return m.image(0), m.err(), lib.mlis_infotext_get(m.ctx, 0).decode()
    finally:
        m.close()


def test_public_option_end_to_end(lib):
    base, _, info0 = generate(lib)
    none, _, info_none = generate(lib, "none")
    assert np.array_equal(base, none) and "Tiling" not in info0 and info_none == info0
    xy, _, info_xy = generate(lib, "xy")
    xy2, _, _ = generate(lib, "3")
    assert not np.array_equal(xy, base) and np.array_equal(xy, xy2)
    assert ", Tiling: xy" in info_xy and info_xy.replace(", Tiling: xy", "") == info0
    rng = np.random.default_rng(1)
    rgb = (rng.random((64, 64, 3)) * 255).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full((64, 64, 1), 255, np.uint8)], axis=2)
    rgba[:, 32:, 3] = 0
    for img in (rgb, rgba):                                          # img2img, in-painting
        out, _, info = generate(lib, "xy", image=img)
        assert np.isfinite(out).all() and "Tiling: xy" in info
    _, err, _ = generate(lib, "x", vae_tile=32, expect=-4)
    assert "tiling" in err and "vae_tile" in err
    out, _, _ = generate(lib, "xy", tae=True, vae_tile=32)           # TAESD is never tiled: it wraps
    assert out is not None
    # (64 x 64 is one tile for any codec: no tile plan would exist there with the KL-VAE either.)  At 256 x 256 vae_tile 64 tiles the KL-VAE and still not TAESD
    generate(lib, vae_tile=64, dim=256, tile_plan=True)
    _, err, _ = generate(lib, "x", vae_tile=64, dim=256, expect=-4)
    assert "tiling" in err and "vae_tile" in err
    out, _, _ = generate(lib, "xy", tae=True, vae_tile=64, dim=256)
    assert out is not None and out.shape[:2] == (256, 256)
