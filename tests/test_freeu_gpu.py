"""FreeU on the GPU: the two kernels against float64 per element, one evaluation of a FreeU engine against the torch restatement (tests/freeu_ref.py) through
mlis_amd_dxdt, and the compositions: ControlNet, hipGraph replay, weight streaming, tiled engines, mlis_generate with the freeu options and the hires fix.

Per-element bounds of the kernels, u = 2^-24 (half an ulp of fp32, the relative error of one rounding), D = mlsd_freeu_depth(terms of the sum):

  skip      |got - ref| <= u (2 |ref| + |s - 1| (D + 16) A),  A = (4 / HW) sum |v| of the plane.
            The result is v + (s - 1) / (HW) (S0 + cos a Sca + sin a Ssa + ..): the last fused multiply-add rounds once (u |ref|, the other u |ref| is spare).  Each plane
            sum carries at most D roundings of partial sums bounded by sum |v trig|; the cosine and sine sums of one angle enter with |cos a' cos a| + |sin a' sin a| <= 1,
            so the seven sums weigh like the four terms 1, cos t, cos f, cos(t + f): D u (4 / HW) sum |v| = D u A.  The 16 covers the trig values (a rounded argument
            below 1/2, sincospif, the angle-addition products: about 3 u each at source and target), the six accumulations of the apply and the scale (s - 1) / HW.
  backbone  |got - ref| <= 2 u |ref| + |x| |b - 1| (3 d / (max - min) + 4 u),  d = u (D + 2) max_p (1 / C) sum_c |x|.
            d bounds the error of a computed channel mean (D additions, the division by C); the normalised map (m - min) / (max - min) then errs by at most
            (|e_p| + (1 - mh) |e_min| + mh |e_max|) / (max - min) <= 2 d / (max - min) to first order, the third d / (max - min) and the 4 u cover the second order and the
            roundings of the subtraction, the division, b - 1 and the product; the factor's final addition and the product with x are the 2 u |ref|.
            The test first asserts d / (max - min) <= 1e-4 in float64: a condition on its inputs (a constant mean map has no normalised form), not a tolerance.

Bound of an evaluation: per-image rel-L2 <= tolerances.EVAL_SMALL for each of the N = 2B evaluations behind mlis_amd_dxdt, un-mixed from its answers at cfg 2 and
cfg 3 as tests/test_controlnet_gpu.py does.  With the factors (1.4, 1.6, 0.9, 0.2) the reference differs from the FreeU-less reference by more than 10 x that
bound (asserted), so an engine that ignored FreeU would fail; stage 1 alone and stage 2 alone are held to the same margin."""
import ctypes as C

import numpy as np
import pytest

import controlnet_ffi as CF
import freeu_ffi as FF
import mlis_ffi as F
import tolerances as TOL

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return FF.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ the kernels
SHAPES = [(2, 2, 8, 8), (3, 5, 8, 8), (8, 8, 72, 72), (16, 24, 64, 96), (64, 64, 128, 128)]      # H, W, C, destination stride
FACTORS = (0.2, 0.9, 1.4)
POISON = 7e30
_IN = {}


def maps(n, H, W, Cn, ld=None):
    """[n][H W][ld] float32: a smooth spatial ramp + N(0, 1) + 1.5 (the channel-mean map then has a real spread); shared, read-only"""
    key = (n, H, W, Cn, ld or Cn)
    if key not in _IN:
        rng = np.random.default_rng(H * 1000 + W * 10 + Cn + n)
        y, x = np.mgrid[0:H, 0:W]
        ramp = (y / H + 0.5 * x / W)[None, :, :, None] * (1 + 0.25 * np.arange(n))[:, None, None, None]
        v = np.zeros((n, H * W, ld or Cn), np.float32)
        v[:, :, :Cn] = (ramp + rng.standard_normal((n, H, W, Cn)) + 1.5).reshape(n, H * W, Cn).astype(np.float32)
        v.setflags(write=False)
        _IN[key] = v
    return _IN[key]


def run(lib, which, src, n, H, W, Cn, ld_dst, factor, ws_fill=np.nan):
    """src [n][H W][ld_src] -> dst [n][H W][ld_dst] (columns past Cn keep their fill); the workspace starts out poisoned"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    dst = _lib.from_numpy(np.full((n, H * W, ld_dst), POISON, np.float32))
    s, f = _lib.from_numpy(np.ascontiguousarray(src)), _lib.from_numpy(np.array([factor], np.float32))
    ws = _lib.from_numpy(np.full(lib.mlsd_freeu_ws_bytes(n, H, W, Cn) // 4, ws_fill, np.float32))
    if which == "skip":
        r = lib.mlsd_freeu_skip(dst.ptr, ld_dst, s.ptr, src.shape[2], n, H, W, Cn, ws.ptr, f.ptr, None)
    else:
        r = lib.mlsd_freeu_backbone(dst.ptr, ld_dst, s.ptr, src.shape[2], n, H * W, Cn, ws.ptr, f.ptr, None)
    assert r == 0, _lib.last_error()
    K.sync()
    return dst.download((n, H * W, ld_dst), np.float32)


def nchw64(v, n, H, W, Cn):
    return v[:, :, :Cn].astype(np.float64).reshape(n, H, W, Cn).transpose(0, 3, 1, 2)


def nhwc(a, n, H, W, Cn):
    return a.transpose(0, 2, 3, 1).reshape(n, H * W, Cn)


@pytest.mark.parametrize("H,W,Cn,ld", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES])
def test_skip_against_float64(lib, H, W, Cn, ld):
    import freeu_ref as R
    D = lib.mlsd_freeu_depth(H * W)
    for n in (1, 3):
        src = maps(n, H, W, Cn)
        x64 = nchw64(src, n, H, W, Cn)
        A = nhwc(np.broadcast_to(4.0 / (H * W) * np.abs(x64).sum(axis=(2, 3), keepdims=True), x64.shape), n, H, W, Cn)
        for s in FACTORS:
            s32 = float(np.float32(s))
            got = run(lib, "skip", src, n, H, W, Cn, ld, s)
            ref = nhwc(R.fourier_filter64(x64, s32), n, H, W, Cn)
            bound = U24 * (2 * np.abs(ref) + abs(s32 - 1) * (D + 16) * A)
            err = np.abs(got[:, :, :Cn].astype(np.float64) - ref)
            print(f"skip {H}x{W}x{Cn} n {n} s {s}: depth {D}, max err / bound = {(err / bound).max():.3f}")
            assert np.isfinite(got[:, :, :Cn]).all() and (err <= bound).all()
            assert (got[:, :, Cn:] == np.float32(POISON)).all()                                        # the destination's padding is not written
            assert np.abs(ref - src[:, :, :Cn]).max() > 1e3 * bound.max()                              # the filter does something at this factor
    assert run(lib, "skip", src, n, H, W, Cn, ld, s).tobytes() == got.tobytes()                        # the same bits every run


@pytest.mark.parametrize("H,W,Cn,ld", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES])
def test_backbone_against_float64(lib, H, W, Cn, ld):
    import freeu_ref as R
    D = lib.mlsd_freeu_depth(Cn)
    for n in (1, 3):
        src = maps(n, H, W, Cn)
        x64 = nchw64(src, n, H, W, Cn)
        m = x64.mean(axis=1)
        span = m.max(axis=(1, 2)) - m.min(axis=(1, 2))
        delta = U24 * (D + 2) * np.abs(x64).mean(axis=1).max(axis=(1, 2))
        assert (delta / span <= 1e-4).all(), (delta / span)                                           # a condition on the inputs, not a tolerance
        slack = (3 * delta / span + 4 * U24)[:, None, None]
        for b in FACTORS:
            b32 = float(np.float32(b))
            got = run(lib, "backbone", src, n, H, W, Cn, ld, b)
            ref = nhwc(R.backbone64(x64, b32), n, H, W, Cn)
            bound = U24 * 2 * np.abs(ref) + np.abs(src[:, :, :Cn].astype(np.float64)) * abs(b32 - 1) * slack
            err = np.abs(got[:, :, :Cn].astype(np.float64) - ref)
            print(f"backbone {H}x{W}x{Cn} n {n} b {b}: depth {D}, delta / span {(delta / span).max():.2e}, max err / bound = {(err / bound).max():.3f}")
            assert np.isfinite(got[:, :, :Cn]).all() and (err <= bound).all()
            assert got[:, :, Cn // 2:Cn].tobytes() == np.ascontiguousarray(src[:, :, Cn // 2:Cn]).tobytes()      # the second half keeps its bits
            assert (got[:, :, Cn:] == np.float32(POISON)).all()
            assert np.abs(ref - src[:, :, :Cn]).max() > 1e3 * bound.max()
    assert run(lib, "backbone", src, n, H, W, Cn, ld, b).tobytes() == got.tobytes()


@pytest.mark.parametrize("which", ["skip", "backbone"])
def test_factor_one_is_a_bit_copy_that_never_reads_the_workspace(lib, which):
    for H, W, Cn, ld in (SHAPES[1], SHAPES[3]):
        n = 3
        src = maps(n, H, W, Cn, Cn + 8).copy()
        src[1, 2, 3], src[0, 0, 0], src[2, 5, 7] = -0.0, np.inf, np.nan
        src.view(np.uint32)[0, 1, 1] = 0x7fc12345                    # a NaN with a payload
        got = run(lib, which, src, n, H, W, Cn, ld, 1.0, ws_fill=np.nan)
        assert got[:, :, :Cn].tobytes() == np.ascontiguousarray(src[:, :, :Cn]).tobytes()
        assert (got[:, :, Cn:] == np.float32(POISON)).all()


def test_flat_mean_map_has_factor_one(lib):
    """max == min, where the published code divides by zero: every pixel has the same channel mean (exactly: powers of two), the channels differ"""
    n, H, W, Cn = 2, 3, 5, 8
    src = np.tile(np.array([1, 2, 4, 1, -1, -2, -4, -1], np.float32), (n, H * W, 1))
    got = run(lib, "backbone", src, n, H, W, Cn, Cn, 1.4)
    assert got.tobytes() == src.tobytes()


# ------------------------------------------------------------------ one evaluation against the reference
CFG, SIGMA = 2.0, 2.5
ON = (1.4, 1.6, 0.9, 0.2)
STAGE1, STAGE2 = (1.4, 1.0, 0.9, 1.0), (1.0, 1.6, 1.0, 0.2)
CASES = [("tiny", 8, 8, 2), ("tinyxl", 8, 8, 1), ("tiny", 8, 16, 1), ("tinyv", 8, 8, 1)]      # the latent sizes of tests/test_controlnet_gpu.py
_REF = {}


def inputs(model, w, h, B, seed=3):
    import controlnet_ref as R
    P = R.UNET[model]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, 4, h, w)) * np.sqrt(1 + SIGMA * SIGMA)).astype(np.float32)
    c = lambda: (rng.standard_normal((77, P["n_ctx"])) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P["ch_adm_in"]) * 0.5).astype(np.float32)) if P["ch_adm_in"] else (lambda: None)
    cond = (c(), l(), c(), l())
    hint = rng.random((3, 8 * h, 8 * w)).astype(np.float32)
    return x, cond, hint


def reference(model, w, h, B, factors, control=False, x=None):
    """the N = 2B evaluations [2B,4,h,w] of the shared inputs: factors None = the plain UNet; control: with the ControlNet's residuals at gain 1; once per case"""
    import controlnet_ref as CR
    import freeu_ref as R
    key = (model, w, h, B, factors, control, None if x is None else x.tobytes())
    if key not in _REF:
        x0, (c, l, u, ul), hint = inputs(model, w, h, B)
        if x is not None:
            x0 = x
        if "net" not in _REF:
            _REF["net"] = CR.make_net()
        if factors is None:
            _REF[key] = CR.eps_rows(_REF["net"], model, x0, SIGMA, c, l, u, ul, hint=hint[None] if control else None)
        else:
            _REF[key] = R.eps_rows(_REF["net"], model, x0, SIGMA, c, l, u, ul, factors, hint=hint[None] if control else None)
        _REF[key].setflags(write=False)
    return _REF[key]


def engine(model, w, h, B, **kw):
    from mlimgsynth_amd import engine as E
    x, cond, hint = inputs(model, w, h, B)
    g = E.Generator(model, 8 * w, 8 * h, B, cfg_scale=CFG, freeu=True, **kw)
    g.set_cond(*cond)
    return g, x, hint


def rows(g, x):
    """the N = 2B evaluations behind the engine's dxdt, un-mixed from its answers at cfg 2 and cfg 3 (controlnet_ref.unmix); leaves cfg at CFG"""
    import controlnet_ref as R
    g.set_sampler(cfg_scale=3.0)
    d3 = g.dxdt(x, SIGMA)
    g.set_sampler(cfg_scale=CFG)
    d2 = g.dxdt(x, SIGMA)
    assert np.isfinite(d2).all() and np.isfinite(d3).all()
    return R.unmix(d2, d3)


def per_image(got, want):
    import controlnet_ref as R
    return [R.rel_l2(got[b], want[b]) for b in range(len(got))]


@pytest.mark.parametrize("model,w,h,B", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}" for c in CASES])
def test_freeu_evaluation_against_the_reference(model, w, h, B):
    import freeu_ref as R
    want, plain = reference(model, w, h, B, ON), reference(model, w, h, B, None)
    margin = min(per_image(want, plain))
    assert margin > 10 * TOL.EVAL_SMALL, margin               # otherwise an engine that ignored FreeU would pass
    g, x, _ = engine(model, w, h, B)
    try:
        assert g.freeu_info() == R.COUNTS[model]
        err0 = per_image(rows(g, x), plain)                   # the flag and nothing else: all four factors are 1
        g.set_freeu(*ON)
        got = rows(g, x)
        err = per_image(got, want)
        print(f"{model} {w}x{h} b{B}: FreeU rel-L2 {err}, factors of 1 vs the plain reference {err0}, FreeU vs plain reference {margin:.3f}")
        assert len(err) == 2 * B and max(err) <= TOL.EVAL_SMALL
        assert max(err0) <= TOL.EVAL_SMALL
        assert min(per_image(got, plain)) > 10 * TOL.EVAL_SMALL                 # visibly on
        again = g.dxdt(x, SIGMA)
        assert np.array_equal(g.dxdt(x, SIGMA), again)
        g.set_freeu(1, 1, 1, 1)
        assert max(per_image(rows(g, x), plain)) <= TOL.EVAL_SMALL
    finally:
        g.destroy()


def test_both_stages_are_hit():
    model, w, h, B = CASES[1]
    plain, w1, w2 = reference(model, w, h, B, None), reference(model, w, h, B, STAGE1), reference(model, w, h, B, STAGE2)
    margins = [min(per_image(w1, plain)), min(per_image(w2, plain)), min(per_image(w1, w2))]
    assert min(margins) > 10 * TOL.EVAL_SMALL, margins        # each stage alone moves the result, and differently
    g, x, _ = engine(model, w, h, B)
    try:
        g.set_freeu(*STAGE1)
        e1 = per_image(rows(g, x), w1)
        g.set_freeu(*STAGE2)
        e2 = per_image(rows(g, x), w2)
        print(f"stage 1 alone rel-L2 {e1}, stage 2 alone {e2}; references apart by {margins}")
        assert max(e1) <= TOL.EVAL_SMALL and max(e2) <= TOL.EVAL_SMALL
    finally:
        g.destroy()


# ------------------------------------------------------------------ composition
def test_with_a_controlnet_against_the_reference_with_both():
    model, w, h, B = CASES[1]
    want = reference(model, w, h, B, ON, control=True)
    others = [reference(model, w, h, B, ON), reference(model, w, h, B, None, control=True)]
    assert min(min(per_image(want, o)) for o in others) > 10 * TOL.EVAL_SMALL      # neither half alone would pass
    g, x, hint = engine(model, w, h, B, control=True)
    try:
        assert g.cfg.control == 3 and g.control_info()[0] > 0
        g.set_control_image(hint)
        g.set_freeu(*ON)
        err = per_image(rows(g, x), want)
        print(f"FreeU + ControlNet: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL and g.control_info()[1] == 1
    finally:
        g.destroy()


@pytest.mark.parametrize("how", ["use_hipgraph", "unet_split"])
def test_hipgraph_and_streaming_are_bit_identical(lib, how):
    model, w, h, B = "tinyxl", 8, 8, 1
    outs = []
    for kw in ({}, {how: 1}):
        g, x, _ = engine(model, w, h, B, n_step=3, **kw)
        try:
            g.set_freeu(*ON)
            a = g.dxdt(x, SIGMA)
            g.set_freeu(1.2, 1.0, 0.5, 1.0)                   # the factors change between replays of the captured graph, two of them to the copying value
            lat, _ = g.generate([9], want_images=False)
            g.set_freeu(*ON)
            outs.append((a, lat, g.dxdt(x, SIGMA)))
            assert lib.mlis_amd_handoff_retries(g.h) == 0
        finally:
            g.destroy()
    for p, q in zip(*outs):
        assert np.isfinite(p).all() and p.tobytes() == q.tobytes()
    assert outs[0][0].tobytes() == outs[0][2].tobytes() and not np.array_equal(outs[0][0], outs[0][1])


def test_tiled_engine_equals_the_blend_of_freeu_windows():
    """a tiled engine applies FreeU per window plan evaluation: its answer is the weighted average of window-sized FreeU engines on the crops; the bound is that
    of tests/test_unet_tile_gpu.py (same plan, same bytes: only the blend's rounding differs, magnified by the coefficients of the CFG mix)"""
    import unet_tile_ffi as U
    from mlimgsynth_amd import engine as E
    import controlnet_ref as R
    model, cfg, B = "tiny", 7.0, 2
    x, cond, _ = inputs(model, 12, 12, B)
    wins, ww, wh = U.windows(12, 12, 8, 8, 4)
    tiled = E.Generator(model, 96, 96, B, cfg_scale=cfg, unet_tile=64, unet_tile_overlap=32, freeu=True)
    packed = E.Generator(model, 96, 96, B, cfg_scale=cfg, unet_tile=64, unet_tile_overlap=32, unet_tile_batch=2, freeu=True)
    plain = E.Generator(model, 64, 64, B, cfg_scale=cfg, freeu=True)
    try:
        assert tiled.tile_info() == (4, 8, 8) and tiled.freeu_info() == plain.freeu_info() == (3, 1)
        for g in (tiled, packed, plain):
            g.set_cond(*cond)
        off = tiled.dxdt(x, SIGMA)
        for g in (tiled, packed, plain):
            g.set_freeu(*ON)
        got = tiled.dxdt(x, SIGMA)
        parts = [plain.dxdt(U.crop(x, x0, y0, ww, wh), SIGMA) for x0, y0 in wins]
        want, _ = U.blend64(parts, wins, ww, wh, 4, 12, 12)
        scale = max(np.abs(p).max() for p in parts)
        bound = (cfg + abs(1 - cfg)) * 1e-6 * scale
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"tiled FreeU: max|err| = {err:.3e}, bound {bound:.3e}")
        assert np.isfinite(got).all() and err <= bound and not np.array_equal(got, off)
        # packed windows: another batch size of the same plan, within the engine's evaluation tolerance of the unpacked answer (the cfg 7 mix weighs 13 evaluations)
        assert max(per_image(packed.dxdt(x, SIGMA), got)) <= (cfg + abs(1 - cfg)) * TOL.EVAL_SMALL
    finally:
        tiled.destroy(), packed.destroy(), plain.destroy()


# ------------------------------------------------------------------ the public API
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
STEPS = 4


def context(lib, model="tiny", dim=64, freeu=1, opts=()):
    m = F.Mlis(lib)
    m.set("model", f"synth:{model}")
    m.set("image_dim", dim, dim)
    m.set("steps", STEPS), m.set("seed", 42), m.set("cfg_scale", 7.0), m.set("method", "euler_a")
    m.set("freeu", freeu)
    for k, v in opts:
        m.set(k, v)
    return m


def run_generate(lib, m):
    m.tokens(TOKS)
    m.tokens(NTOKS, negative=True)
    m.generate()
    eng = lib.mlis_amd_engine_get(m.ctx)
    n1, n2 = C.c_int(), C.c_int()
    assert lib.mlis_amd_freeu_info(eng, C.byref(n1), C.byref(n2)) == 1
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]), info=lib.mlis_infotext_get(m.ctx, 0).decode(),
                builds=lib.mlis_amd_engine_builds(m.ctx), stages=(n1.value, n2.value), retries=lib.mlis_amd_handoff_retries(eng))


def generate(lib, setup=None, **kw):
    m = context(lib, **kw)
    try:
        if setup:
            setup(m)
        return run_generate(lib, m)
    finally:
        m.close()


def test_public_api_end_to_end(lib):
    """fresh contexts: every generation starts its Philox streams at offset 0, so results compare bit for bit"""
    off, a, again = generate(lib, freeu=0), generate(lib), generate(lib)
    assert off["builds"] == 1 and "FreeU" not in off["info"] and off["stages"] == (0, 0)
    assert a["builds"] == 1 and a["stages"] == (3, 1) and np.isfinite(a["image"]).all() and a["retries"] == 0
    assert not np.array_equal(a["latent"], off["latent"]) and not np.array_equal(a["image"], off["image"])
    assert ", FreeU: 1.3 1.4 0.9 0.2, Version: " in a["info"] and a["info"].replace(", FreeU: 1.3 1.4 0.9 0.2", "") == off["info"]
    assert again["latent"].tobytes() == a["latent"].tobytes() and again["image"].tobytes() == a["image"].tobytes() and again["info"] == a["info"]
    b = generate(lib, opts=(("freeu_b1", 1.1), ("freeu_s2", 0.5)))
    assert ", FreeU: 1.1 1.4 0.9 0.5, " in b["info"] and not np.array_equal(b["latent"], a["latent"])
    ones = generate(lib, opts=(("freeu_b1", 1), ("freeu_b2", 1), ("freeu_s1", 1), ("freeu_s2", 1)))
    assert np.isfinite(ones["latent"]).all() and not np.array_equal(ones["latent"], a["latent"])


def test_factors_rebuild_nothing_and_the_flag_adds_one_engine(lib):
    m = context(lib, freeu=0)
    try:
        first = run_generate(lib, m)
        assert first["builds"] == 1 and first["stages"] == (0, 0)
        m.set("freeu", 1)
        on = run_generate(lib, m)
        assert on["builds"] == 2 and on["stages"] == (3, 1)                      # switched on: one more engine, the plain one stays resident
        m.set("freeu_b1", 1.1), m.set("freeu_s1", 0.6)
        m.set("seed", 42)
        changed = run_generate(lib, m)
        assert changed["builds"] == 2 and ", FreeU: 1.1 1.4 0.6 0.2, " in changed["info"]      # a factor change rebuilds nothing
        m.set("freeu", 0)
        assert run_generate(lib, m)["builds"] == 2                               # back on the resident plain engine
        m.set("freeu", 1)
        assert run_generate(lib, m)["builds"] == 2
    finally:
        m.close()
    # the factors reach the engine: the same two settings in fresh contexts give different images, the first as above
    a, b = generate(lib), generate(lib, opts=(("freeu_b1", 1.1), ("freeu_s1", 0.6)))
    assert not np.array_equal(a["latent"], b["latent"])


def test_hires_runs_both_passes_with_freeu(lib):
    def hires(m):
        m.set("hires_scale", 1.5), m.set("hires_denoise", 0.6), m.set("hires_steps", 3)
    a, off = generate(lib, setup=hires), generate(lib, setup=hires, freeu=0)
    assert a["latent"].shape == (1, 4, 12, 12) and a["image"].shape == (1, 3, 96, 96) and np.isfinite(a["image"]).all()
    assert a["builds"] == 2 and a["stages"] == (3, 1) and a["retries"] == 0 and ", FreeU: 1.3 1.4 0.9 0.2" in a["info"]
    assert not np.array_equal(a["latent"], off["latent"])
    # both engines of the generation hold FreeU: the one used last (the second pass) reports its stages above; the first pass is shown by factors that switch
    # stage 2 off -- at 8 x 8 and at 12 x 12 latents alike the remaining stage 1 still moves the result away from both
    half = generate(lib, setup=hires, opts=(("freeu_b2", 1), ("freeu_s2", 1)))
    assert half["builds"] == 2 and len({x["latent"].tobytes() for x in (a, off, half)}) == 3
    assert generate(lib, setup=hires)["latent"].tobytes() == a["latent"].tobytes()      # deterministic across contexts
