"""HyperTile on the GPU: the row permutation bit for bit against numpy, the existing attention kernels on tile shapes against float64 per row, one evaluation of
a HyperTile engine against the torch restatement (tests/hypertile_ref.py) through mlis_amd_dxdt, and the compositions: ControlNet, FreeU, hipGraph replay,
weight streaming, tiled-diffusion engines, mlis_generate with the options, the engine key and the hires fix.

Bound of an evaluation: per-image rel-L2 <= tolerances.EVAL_SMALL for each of the N = 2B evaluations behind mlis_amd_dxdt, un-mixed from its answers at cfg 2 and
cfg 3 as tests/test_controlnet_gpu.py does.  The tiled reference differs from the plain reference by more than 10 x that bound in every case (asserted), so an
engine that ignored the option would fail.  HyperTile changes which keys a query sees and nothing about the arithmetic of a launch: the bound is the one of a
plain evaluation at these latent sizes.

Bound of an attention launch on a tile shape: tests/ref64.py's attention_bound per output row, exactly as tests/test_attention_float64_gpu.py applies it."""
import ctypes as C

import numpy as np
import pytest

import attn64_cases as AC
import controlnet_ffi as CF
import mlis_ffi as F
import ref64 as R64
import tolerances as TOL

pytestmark = pytest.mark.gpu
PI = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    lib = CF.bind(_lib.LIB_PATH)
    lib.mlsd_tile_permute.restype, lib.mlsd_tile_permute.argtypes = F.ci, [F.vp, F.vp, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp]
    lib.mlis_amd_hypertile_info.restype, lib.mlis_amd_hypertile_info.argtypes = F.ci, [F.vp, PI, PI, PI]
    lib.mlis_amd_engine_builds.restype, lib.mlis_amd_engine_builds.argtypes = F.ci, [F.vp]
    lib.mlis_amd_engine_get.restype, lib.mlis_amd_engine_get.argtypes = F.vp, [F.vp]
    lib.mlis_amd_handoff_retries.restype, lib.mlis_amd_handoff_retries.argtypes = F.ci, [F.vp]
    return lib


# ------------------------------------------------------------------ the kernel
KERNEL_CASES = [(1, 2, 2, 1, 1, 16), (3, 4, 6, 2, 3, 16), (2, 24, 16, 8, 8, 256), (1, 16, 24, 16, 12, 5120), (2, 6, 10, 6, 5, 640), (1, 64, 64, 32, 32, 1280),
                (1, 1, 8, 1, 4, 16)]
GUARD, SENTINEL = 3, 0xA5


def permute_on_device(lib, src, n, H, W, th, tw, rb, inverse):
    """src [n H W][rb] uint8 -> (dst rows, guard rows before, guard rows after): dst lies between GUARD sentinel rows on either side"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    rows = n * H * W
    s = _lib.from_numpy(src)
    d = _lib.from_numpy(np.full((rows + 2 * GUARD, rb), SENTINEL, np.uint8))
    r = lib.mlsd_tile_permute(s.ptr, d.ptr + GUARD * rb, n, H, W, th, tw, rb, inverse, None)
    assert r == 0, _lib.last_error()
    K.sync()
    out = d.download((rows + 2 * GUARD, rb), np.uint8)
    return out[GUARD:GUARD + rows], out[:GUARD], out[GUARD + rows:]


@pytest.mark.parametrize("n,H,W,th,tw,rb", KERNEL_CASES, ids=["x".join(map(str, c)) for c in KERNEL_CASES])
def test_permutation_bit_for_bit(lib, n, H, W, th, tw, rb):
    import hypertile_ref as HR
    rng = np.random.default_rng(n * 1000 + H * 10 + W + rb)
    src = rng.integers(0, 256, (n * H * W, rb), dtype=np.uint8)
    src[0, :4] = (0x45, 0x23, 0xc1, 0x7f)                         # a NaN with a payload, as fp32 and as two fp16 values: bytes, not numbers
    want = HR.permute_rows(src, n, H, W, th, tw)
    fwd, g0, g1 = permute_on_device(lib, src, n, H, W, th, tw, rb, 0)
    assert fwd.tobytes() == want.tobytes()
    assert (g0 == SENTINEL).all() and (g1 == SENTINEL).all()      # nothing before or after the destination
    inv, g0, g1 = permute_on_device(lib, src, n, H, W, th, tw, rb, 1)
    assert inv.tobytes() == HR.permute_rows(src, n, H, W, th, tw, inverse=True).tobytes() and (g0 == SENTINEL).all() and (g1 == SENTINEL).all()
    back, _, _ = permute_on_device(lib, fwd, n, H, W, th, tw, rb, 1)
    assert back.tobytes() == src.tobytes()                         # inverse(forward(x)) == x
    again, _, _ = permute_on_device(lib, src, n, H, W, th, tw, rb, 0)
    assert again.tobytes() == fwd.tobytes()                        # the same bits on a second run


def test_kernel_refusals_write_nothing(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    n, H, W, rb = 1, 4, 6, 32
    rows = n * H * W
    s = _lib.from_numpy(np.full((2 * rows + 8, rb), 0x11, np.uint8))
    d = _lib.from_numpy(np.full((rows + 8, rb), SENTINEL, np.uint8))
    call = lambda src=s.ptr, dst=d.ptr, th=2, tw=3, rb_=rb, inv=0: lib.mlsd_tile_permute(src, dst, n, H, W, th, tw, rb_, inv, None)
    bad = [call(th=3), call(tw=4), call(rb_=24), call(rb_=8), call(src=s.ptr + 8), call(dst=d.ptr + 4), call(src=s.ptr, dst=s.ptr),
           call(dst=s.ptr + 16 * rb), call(src=s.ptr + 16 * rb, dst=s.ptr), call(src=None), call(dst=None), call(th=0)]
    K.sync()
    assert all(r < 0 for r in bad), bad
    assert (d.download((rows + 8, rb), np.uint8) == SENTINEL).all() and (s.download((2 * rows + 8, rb), np.uint8) == 0x11).all()
    assert call() == 0                                             # the same buffers, good arguments
    K.sync()
    out = d.download((rows + 8, rb), np.uint8)
    assert (out[:rows] == 0x11).all() and (out[rows:] == SENTINEL).all()


# ------------------------------------------------------------------ the attention kernels on tile shapes
# many batches of few tokens through the batch strides of one fused q | k | v buffer, as mlb_attn_mhead_ex records a tiled self-attention:
# (d_head, heads, batches = images x tiles, tokens per tile, the route mlsd_attention_variant must give the launch).  Up to 96 keys d_head 64 goes to the one-pass
# kernel, everything else here to the general tile loop; neither rounds a scaled Q to fp16, so the bound is the one without that term (q_scaled False, fixed
# per case as in tests/attn64_cases.py: a launch that drifted to another kernel fails on its label, it does not get that kernel's bound)
TILE_SHAPES = [(64, 2, 32, 16, "attn<tk96,d64>"), (64, 2, 4, 30, "attn<tk96,d64>"), (32, 4, 12, 64, "attn<tile,d32>"), (64, 2, 16, 256, "attn<tile,d64>"),
               (40, 8, 8, 192, "attn<tile,d40>")]


@pytest.mark.parametrize("d,heads,nb,T,variant", TILE_SHAPES, ids=[f"d{s[0]}-nb{s[2]}-t{s[3]}" for s in TILE_SHAPES])
def test_attention_on_tile_shapes_against_float64(d, heads, nb, T, variant):
    from mlimgsynth_amd import _lib, kernels
    L = _lib.lib()
    c = dict(id=f"hypertile_d{d}_nb{nb}_t{T}", variant=variant, sw={}, nb=nb, heads=heads, d=d, Tq=T, Tk=T, causal=0, layout="fused_qkv", family="sigma4",
             late=T - 3, q_scaled=False, path="tile")
    q, k, v = AC.make_operands(c)
    lay = AC.layout(c)
    dev = {n: _lib.from_numpy(a) for n, a in AC.host_buffers(c, q, k, v).items()}
    dev["o"] = _lib.DeviceBuffer(lay["bufs"]["o"] * 2)
    _lib.check(L.mlsd_memset(_lib.vp(dev["o"].ptr), AC.SENTINEL, C.c_size_t(dev["o"].nbytes), None))
    a = AC.attn_args(kernels, c, {n: b.ptr for n, b in dev.items()})
    AC.restore_switches(L)                                         # the plan's routes: the defaults
    label = kernels.attention_variant(a)
    assert label == variant, f"launch label {label}, case written for {variant}"
    kernels.attention(a)
    kernels.sync()
    D = heads * d
    raw = dev["o"].download((nb, T + 2 * AC.GUARD_ROWS, lay["ldo"]), np.float16)
    guard = raw.view(np.uint16) != (AC.SENTINEL << 8 | AC.SENTINEL)
    guard[:, AC.GUARD_ROWS:AC.GUARD_ROWS + T, :D] = False
    assert not guard.any(), f"{label}: stored outside its rows at (batch, buffer row, column) {np.argwhere(guard)[:4].tolist()}"
    got = raw[:, AC.GUARD_ROWS:AC.GUARD_ROWS + T, :D].astype(np.float64)
    worst, at = 0.0, None
    for b in range(nb):
        o, p = R64.attention64(q[b], k[b], v[b], heads, False)
        ratio = R64.attention_worst(got[b], o, R64.attention_bound(q[b], k[b], v[b], heads, o, p, c["q_scaled"]))
        if not ratio.max() <= worst:
            worst, at = float(ratio.max()), (b, int(np.argmax(ratio)))
    print(f"tile shape d{d} heads {heads} nb {nb} T {T}: {label}, worst row ratio {worst:.3f}")
    assert worst <= 1.0, f"{label}: ratio {worst:.3g} > 1 at (batch, row) {at}"


# ------------------------------------------------------------------ one evaluation against the reference
CFG, SIGMA = 2.0, 2.5
# (model, latent w, latent h, batch, tile, depth): the tiling each produces is in test_hypertile_info_equals_the_rule's table
CASES = [("tiny", 16, 16, 1, 64, 3), ("tiny", 16, 16, 1, 64, 0), ("tiny", 16, 24, 2, 64, 3), ("tinyv", 16, 16, 1, 64, 3), ("tiny", 24, 16, 1, 96, 3),
         ("tinyxl", 20, 12, 1, 32, 3)]
TILINGS = {CASES[0]: [(8, 8, 2, 2), (4, 4, 2, 2)], CASES[1]: [(8, 8, 2, 2), (0,) * 4], CASES[2]: [(8, 8, 3, 2), (4, 4, 3, 2)], CASES[3]: [(8, 8, 2, 2), (4, 4, 2, 2)],
           CASES[4]: [(16, 12, 1, 2), (8, 6, 1, 2)], CASES[5]: [(0,) * 4, (6, 5, 1, 2)]}
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


def net_of(tile, depth):
    """one reference network per setting (tile 0: the plain one), all on one weight cache"""
    import controlnet_ref as CR
    import hypertile_ref as HR
    from tools import torch_ref as TR
    if "weights" not in _REF:
        _REF["weights"] = TR.Weights(CR.synth)
    key = ("net", tile, depth if tile else 0)
    if key not in _REF:
        _REF[key] = HR.HyperNet(_REF["weights"], tile, depth, f16_ops=True) if tile else TR.Net(_REF["weights"], f16_ops=True)
    return _REF[key]


def reference(model, w, h, B, tile, depth=3, control=False, freeu=None, x=None):
    """the N = 2B evaluations [2B,4,h,w] of the shared inputs, once per case: tile 0 = the plain UNet; control: with the ControlNet's residuals at gain 1
    (its encoder copy tiled by the same rule); freeu: the four factors"""
    import controlnet_ref as CR
    import freeu_ref as FR
    key = (model, w, h, B, tile, depth if tile else 0, control, freeu, None if x is None else x.tobytes())
    if key not in _REF:
        x0, (c, l, u, ul), hint = inputs(model, w, h, B)
        if x is not None:
            x0 = x
        net = net_of(tile, depth)
        if freeu:
            _REF[key] = FR.eps_rows(net, model, x0, SIGMA, c, l, u, ul, freeu, hint=hint[None] if control else None)
        else:
            _REF[key] = CR.eps_rows(net, model, x0, SIGMA, c, l, u, ul, hint=hint[None] if control else None)
        _REF[key].setflags(write=False)
    return _REF[key]


def engine(model, w, h, B, **kw):
    from mlimgsynth_amd import engine as E
    x, cond, hint = inputs(model, w, h, B)
    g = E.Generator(model, 8 * w, 8 * h, B, cfg_scale=CFG, **kw)
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


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}-t{c[4]}-d{c[5]}" for c in CASES])
def test_hypertile_evaluation_against_the_reference(case):
    import hypertile_ref as HR
    model, w, h, B, tile, depth = case
    want, plain = reference(model, w, h, B, tile, depth), reference(model, w, h, B, 0)
    margin = per_image(want, plain)
    print(f"{case}: tiled vs plain reference {margin}")
    assert min(margin) > 10 * TOL.EVAL_SMALL, margin              # otherwise an engine that ignored HyperTile would pass
    g, x, _ = engine(model, w, h, B, hypertile=tile, hypertile_depth=depth)
    try:
        n_tiled, n_untiled, tiles = g.hypertile_info()
        assert (n_tiled, n_untiled, tiles) == HR.plan_info(model, w, h, tile, depth)      # hypertile_info equals the rule ...
        assert tiles[:2] == TILINGS[case] and tiles[2:] == [(0,) * 4] * 2 and n_tiled > 0      # ... and the rule gives the tiling the case is there for
        got = rows(g, x)
        err = per_image(got, want)
        print(f"{case}: HyperTile rel-L2 {err}")
        assert len(err) == 2 * B and max(err) <= TOL.EVAL_SMALL
        assert min(per_image(got, plain)) > 10 * TOL.EVAL_SMALL                          # visibly on
        again = g.dxdt(x, SIGMA)
        assert g.dxdt(x, SIGMA).tobytes() == again.tobytes()                             # repeated dxdt is bit-identical
    finally:
        g.destroy()


def test_depth_changes_the_result():
    (model, w, h, B, tile, _) = CASES[0]
    d3, d0 = reference(model, w, h, B, tile, 3), reference(model, w, h, B, tile, 0)
    assert min(per_image(d0, d3)) > 10 * TOL.EVAL_SMALL           # depth 0 and depth 3 are different networks: the cases above tell them apart


@pytest.mark.parametrize("model,w,h,kw", [("tinyxl", 20, 12, dict(hypertile=32, hypertile_depth=0)), ("tiny", 16, 16, dict(hypertile=128))],
                         ids=["tinyxl-depth-0", "tiny-tile-covers-the-picture"])
def test_settings_that_cut_nothing_are_bit_for_bit_the_plain_engine(model, w, h, kw):
    outs = []
    for k in ({}, kw):
        g, x, _ = engine(model, w, h, 1, **k)
        try:
            if k:
                assert g.hypertile_info()[0] == 0
            outs.append(g.dxdt(x, SIGMA))
        finally:
            g.destroy()
    assert np.isfinite(outs[0]).all() and outs[0].tobytes() == outs[1].tobytes()


# ------------------------------------------------------------------ composition
def test_with_a_controlnet_against_the_reference_with_both():
    model, w, h, B, tile, depth = CASES[0]
    want = reference(model, w, h, B, tile, depth, control=True)
    others = [reference(model, w, h, B, tile, depth), reference(model, w, h, B, 0, control=True)]
    assert min(min(per_image(want, o)) for o in others) > 10 * TOL.EVAL_SMALL      # neither half alone would pass
    g, x, hint = engine(model, w, h, B, control=True, hypertile=tile, hypertile_depth=depth)
    try:
        assert g.cfg.control & 7 == 5 and g.control_info()[0] > 0 and g.hypertile_info()[0] > 0
        g.set_control_image(hint)
        err = per_image(rows(g, x), want)
        print(f"HyperTile + ControlNet: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL and g.control_info()[1] == 1
    finally:
        g.destroy()


def test_with_freeu_against_the_reference_with_both():
    model, w, h, B, tile, depth = CASES[0]
    ON = (1.4, 1.6, 0.9, 0.2)
    want = reference(model, w, h, B, tile, depth, freeu=ON)
    others = [reference(model, w, h, B, tile, depth), reference(model, w, h, B, 0, freeu=ON)]
    assert min(min(per_image(want, o)) for o in others) > 10 * TOL.EVAL_SMALL
    g, x, _ = engine(model, w, h, B, freeu=True, hypertile=tile, hypertile_depth=depth)
    try:
        g.set_freeu(*ON)
        err = per_image(rows(g, x), want)
        print(f"HyperTile + FreeU: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL and g.freeu_info() != (0, 0)
    finally:
        g.destroy()


@pytest.mark.parametrize("how", ["use_hipgraph", "unet_split"])
def test_hipgraph_and_streaming_are_bit_identical(lib, how):
    model, w, h, B, tile, depth = CASES[5]
    outs = []
    for kw in ({}, {how: 1}):
        g, x, _ = engine(model, w, h, B, n_step=3, hypertile=tile, hypertile_depth=depth, **kw)
        try:
            a = g.dxdt(x, SIGMA)
            lat, _ = g.generate([9], want_images=False)
            outs.append((a, lat, g.dxdt(x, SIGMA)))
            assert lib.mlis_amd_handoff_retries(g.h) == 0
        finally:
            g.destroy()
    for p, q in zip(*outs):
        assert np.isfinite(p).all() and p.tobytes() == q.tobytes()
    assert outs[0][0].tobytes() == outs[0][2].tobytes()


def test_tiled_diffusion_engine_equals_the_blend_of_hypertile_windows():
    """a unet_tile engine's plan is an ordinary UNet plan at window size, and the rule applies to it unchanged: its answer is the weighted average of window-sized
    HyperTile engines on the crops, under the bound of tests/test_unet_tile_gpu.py (same plan, same bytes: only the blend's rounding differs, magnified by the
    coefficients of the CFG mix)"""
    import unet_tile_ffi as U
    from mlimgsynth_amd import engine as E
    model, cfg, B, tile = "tiny", 7.0, 2, 64
    x, cond, _ = inputs(model, 24, 24, B)
    wins, ww, wh = U.windows(24, 24, 16, 16, 4)
    tiled = E.Generator(model, 192, 192, B, cfg_scale=cfg, unet_tile=128, unet_tile_overlap=32, hypertile=tile)
    window = E.Generator(model, 128, 128, B, cfg_scale=cfg, hypertile=tile)
    off = E.Generator(model, 192, 192, B, cfg_scale=cfg, unet_tile=128, unet_tile_overlap=32)
    try:
        assert tiled.tile_info()[1:] == (16, 16)
        assert tiled.hypertile_info() == window.hypertile_info() and tiled.hypertile_info()[2][:2] == [(8, 8, 2, 2), (4, 4, 2, 2)]
        for g in (tiled, window, off):
            g.set_cond(*cond)
        got = tiled.dxdt(x, SIGMA)
        parts = [window.dxdt(U.crop(x, x0, y0, ww, wh), SIGMA) for x0, y0 in wins]
        want, _ = U.blend64(parts, wins, ww, wh, 4, 24, 24)
        scale = max(np.abs(p).max() for p in parts)
        bound = (cfg + abs(1 - cfg)) * 1e-6 * scale
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"tiled diffusion + HyperTile: max|err| = {err:.3e}, bound {bound:.3e}")
        assert np.isfinite(got).all() and err <= bound and not np.array_equal(got, off.dxdt(x, SIGMA))
    finally:
        tiled.destroy(), window.destroy(), off.destroy()


# ------------------------------------------------------------------ the public API
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
STEPS = 4


def context(lib, dim=128, hypertile=0, depth=None, opts=()):
    m = F.Mlis(lib)
    m.set("model", "synth:tiny")
    m.set("image_dim", dim, dim)
    m.set("steps", STEPS), m.set("seed", 42), m.set("cfg_scale", 7.0), m.set("method", "euler_a")
    m.set("hypertile", hypertile)
    if depth is not None:
        m.set("hypertile_depth", depth)
    for k, v in opts:
        m.set(k, v)
    return m


def run_generate(lib, m, decoded=True):
    m.tokens(TOKS)
    m.tokens(NTOKS, negative=True)
    m.set("seed", 42)
    m.generate()
    eng = lib.mlis_amd_engine_get(m.ctx)
    a, b, t = C.c_int(), C.c_int(), (C.c_int * 16)()
    assert lib.mlis_amd_hypertile_info(eng, C.byref(a), C.byref(b), t) == 1
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]) if decoded else None, info=lib.mlis_infotext_get(m.ctx, 0).decode(),
                builds=lib.mlis_amd_engine_builds(m.ctx), tiled=(a.value, b.value), tiles=[tuple(t[4 * i:4 * i + 4]) for i in range(4)],
                retries=lib.mlis_amd_handoff_retries(eng))


def generate(lib, setup=None, decoded=True, **kw):
    m = context(lib, **kw)
    try:
        if setup:
            setup(m)
        return run_generate(lib, m, decoded)
    finally:
        m.close()


def test_public_api_end_to_end(lib):
    """fresh contexts: every generation starts its Philox streams at offset 0, so results compare bit for bit"""
    off, a, again = generate(lib), generate(lib, hypertile=64), generate(lib, hypertile=64)
    assert off["builds"] == 1 and "HyperTile" not in off["info"] and off["tiled"] == (0, 7)
    assert a["builds"] == 1 and a["tiled"] == (7, 0) and a["tiles"][:2] == [(8, 8, 2, 2), (4, 4, 2, 2)] and np.isfinite(a["image"]).all() and a["retries"] == 0
    assert not np.array_equal(a["latent"], off["latent"]) and not np.array_equal(a["image"], off["image"])
    assert ", HyperTile: 64, HyperTile depth: 3" in a["info"] and a["info"].replace(", HyperTile: 64, HyperTile depth: 3", "") == off["info"]
    assert again["latent"].tobytes() == a["latent"].tobytes() and again["image"].tobytes() == a["image"].tobytes() and again["info"] == a["info"]
    d0 = generate(lib, hypertile=64, depth=0)
    assert d0["tiled"] == (3, 4) and len({r["latent"].tobytes() for r in (off, a, d0)}) == 3
    # a tile that covers the picture: none of the new code runs, the bytes are those of a run without the option
    whole = generate(lib, hypertile=128)
    assert whole["tiled"] == (0, 7) and whole["latent"].tobytes() == off["latent"].tobytes() and whole["image"].tobytes() == off["image"].tobytes()
    from mlimgsynth_amd import mlimgsynth as M
    assert callable(M.MLImgSynth.hypertile_info)


def test_engine_key(lib):
    """a change of either option builds one more engine and keeps the other resident (one context: its Philox streams run on from generation to generation, so
    results are not compared across them; test_public_api_end_to_end compares fresh contexts)"""
    m = context(lib)
    try:
        first = run_generate(lib, m)
        assert first["builds"] == 1 and first["tiled"] == (0, 7)
        m.set("hypertile", 64)
        on = run_generate(lib, m)
        assert on["builds"] == 2 and on["tiled"] == (7, 0)
        m.set("hypertile", 0)
        back = run_generate(lib, m)
        assert back["builds"] == 2 and back["tiled"] == (0, 7)                                    # the plain engine stayed resident
        m.set("hypertile", 64)
        assert run_generate(lib, m)["builds"] == 2
        m.set("hypertile_depth", 0)
        d0 = run_generate(lib, m)
        assert d0["builds"] == 3 and d0["tiled"] == (3, 4)
        m.set("hypertile_depth", 3)
        d3 = run_generate(lib, m)
        assert d3["builds"] == 3 and d3["tiled"] == (7, 0)                                        # and so did the depth-3 one
        m.set("hypertile", 128)                                                                   # one tile on every level: the plain key again
        whole = run_generate(lib, m)
        assert whole["tiled"] == (0, 7) and whole["builds"] == 4                                  # (the plain engine had left the two slots by now)
        m.set("hypertile", 32)
        t32 = run_generate(lib, m)
        assert t32["tiles"][:2] == [(4, 4, 4, 4), (4, 4, 2, 2)] and t32["builds"] == 5
    finally:
        m.close()


def test_hires_applies_the_rule_per_pass(lib):
    """tiny at 64 px with hypertile 64 and a 2x hires fix: the 8 x 8 first pass is one tile on both levels and runs the plain engine under the plain key, the
    16 x 16 second pass is tiled 2 x 2"""
    DENOISE = 0.6

    def hires(m):
        m.set("hires_scale", 2), m.set("hires_denoise", DENOISE), m.set("hires_steps", 3), m.set("hires_upscaler", "bilinear")

    first_on, first_off = generate(lib, dim=64, hypertile=64, decoded=False, opts=(("no_decode", 1),)), generate(lib, dim=64, decoded=False, opts=(("no_decode", 1),))
    assert first_on["tiled"] == (0, 7) and first_on["latent"].tobytes() == first_off["latent"].tobytes()      # the first pass: the bytes of a run without the option
    h_on, h_off = generate(lib, dim=64, hypertile=64, setup=hires), generate(lib, dim=64, setup=hires)
    assert h_on["builds"] == 2 and h_on["tiled"] == (7, 0) and h_on["tiles"][:2] == [(8, 8, 2, 2), (4, 4, 2, 2)] and h_on["retries"] == 0
    assert h_on["latent"].shape == (1, 4, 16, 16) and not np.array_equal(h_on["latent"], h_off["latent"])      # the second pass differs
    assert ", HyperTile: 64, HyperTile depth: 3" in h_on["info"]
    # by hand: the first pass without the option, its latent resampled, the second pass as img2img with the option
    m = context(lib, dim=64)
    try:
        m.tokens(TOKS), m.tokens(NTOKS, negative=True)
        m.set("no_decode", 1)
        m.generate()
        lib.mlis_amd_tensor_resample.restype, lib.mlis_amd_tensor_resample.argtypes = F.ci, [F.vp, C.POINTER(F.Tensor), C.POINTER(F.Tensor), F.ci, F.ci, F.ci]
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["LATENT"])
        assert lib.mlis_amd_tensor_resample(m.ctx, t, t, 16, 16, 1) == 1, m.err()
        m.tokens(TOKS), m.tokens(NTOKS, negative=True)
        m.set("no_decode", 0), m.set("tensor_use_flags", F.TUF["LATENT"]), m.set("f_t_ini", DENOISE), m.set("steps", 3)
        m.set("hypertile", 64)
        m.generate()
        by_hand = dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]))
        assert lib.mlis_amd_engine_builds(m.ctx) == 2
    finally:
        m.close()
    assert by_hand["latent"].tobytes() == h_on["latent"].tobytes() and by_hand["image"].tobytes() == h_on["image"].tobytes()
