"""ControlNet on the GPU: the two kernels against numpy, one evaluation of a controlled engine against the torch restatement of cldm.py
(tests/controlnet_ref.py) through mlis_amd_dxdt, the gain and the step window, hipGraph replay and weight streaming, tiled engines, and mlis_generate with the
control options: determinism, engine reuse, the hires fix, a ControlNet file against the synthetic one, composition with the other options.

Bound of mlsd_ctrl_add, per element |err| <= 2^-23 (|base| + |gain ctrl|): the kernel rounds the product and the sum once each (relative 2^-24 each), so
|err| <= 2^-24 |gain ctrl| + 2^-24 |base + gain ctrl| (1 + 2^-24) <= 2^-24 (|base| + 2 |gain ctrl|) (1 + 2^-24); a fused multiply-add rounds once and is
inside it too.

Bound of an evaluation, per-image rel-L2 <= tolerances.EVAL_SMALL: the project's bound for ONE test-sized UNet evaluation, held for each of the N = 2B images of
the plan (the cond and the uncond evaluation of every image).  mlis_amd_dxdt returns their CFG mix, cond cfg + uncond (1 - cfg); the two halves are recovered from
its answers at cfg 2 and cfg 3 (controlnet_ref.unmix: exact up to fp32 roundings of the mix, because the engine's evaluations are deterministic).  Comparing the mix
itself would hold cfg + |1 - cfg| evaluation errors to the bound of one.  The mix at this test's cfg 2 is compared as well: the test prints its per-image rel-L2
(measured 0.56e-3 .. 2.56e-3, where the evaluations behind it measure 0.26e-3 .. 1.23e-3) and asserts |dx - ref| <= EVAL_SMALL (2 |c_ref| + |u_ref|), the bound
that follows from the per-evaluation one by the triangle inequality.  The controlled and the uncontrolled references differ by far more than 10 x the bound on every image (asserted), so an engine
that ignored the control, on either half, would fail."""
import ctypes as C

import numpy as np
import pytest

import controlnet_ffi as CF
import tolerances as TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return CF.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ mlsd_ctrl_add
def run_ctrl_add(lib, base, ctrl, gain, ld_dst, C_):
    """base [n][rows][ld_base], ctrl [n_ctrl][rows][ld_ctrl] -> dst [n][rows][ld_dst] (columns past C_ keep their fill)"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    n, rows, ld_base = base.shape
    dst = _lib.from_numpy(np.full((n, rows, ld_dst), 7e30, np.float32))
    b, k, g = _lib.from_numpy(base), _lib.from_numpy(ctrl), _lib.from_numpy(np.array([gain], np.float32))
    assert lib.mlsd_ctrl_add(dst.ptr, ld_dst, b.ptr, ld_base, k.ptr, ctrl.shape[2], n, rows, C_, ctrl.shape[0], g.ptr, None) == 0, _lib.last_error()
    K.sync()
    return dst.download((n, rows, ld_dst), np.float32)


@pytest.mark.parametrize("gain", [0.75, -1.5])
@pytest.mark.parametrize("n_ctrl", [1, 3])
@pytest.mark.parametrize("rows", [1, 63, 257])
def test_ctrl_add_against_float64(lib, rows, n_ctrl, gain):
    Cn, n, ld_base, ld_dst = 64, 3, 96, 64
    rng = np.random.default_rng(rows + 10 * n_ctrl)
    base = (rng.standard_normal((n, rows, ld_base)) * 3).astype(np.float32)
    ctrl = (rng.standard_normal((n_ctrl, rows, Cn)) * 2).astype(np.float32)
    base[0, 0, 0], ctrl[0, 0, 1] = 1e20, -1e-20
    got = run_ctrl_add(lib, base, ctrl, gain, ld_dst, Cn)
    kb = np.stack([ctrl[i % n_ctrl] for i in range(n)]).astype(np.float64) * float(np.float32(gain))
    want = base[:, :, :Cn].astype(np.float64) + kb
    bound = 2.0 ** -23 * (np.abs(base[:, :, :Cn]).astype(np.float64) + np.abs(kb))
    err = np.abs(got[:, :, :Cn].astype(np.float64) - want)
    print(f"ctrl_add rows {rows} n_ctrl {n_ctrl} gain {gain}: max err / bound = {(err / bound).max():.3f}")
    assert np.isfinite(got[:, :, :Cn]).all() and (err <= bound).all()


def test_ctrl_add_gain_zero_copies_the_bits_and_never_reads_ctrl(lib):
    Cn, n, rows = 64, 3, 63
    rng = np.random.default_rng(1)
    base = rng.standard_normal((n, rows, 96)).astype(np.float32)
    base[1, 2, 3], base[0, 0, 0], base[2, 5, 7] = -0.0, np.inf, np.nan
    base.view(np.uint32)[0, 1, 1] = 0x7fc12345                       # a NaN with a payload
    ctrl = np.full((1, rows, Cn), np.nan, np.float32)
    for gain in (0.0, -0.0):
        got = run_ctrl_add(lib, base, ctrl, gain, 64, Cn)
        assert got.tobytes() == np.ascontiguousarray(base[:, :, :Cn]).tobytes()


def test_ctrl_add_honours_the_destination_stride(lib):
    rng = np.random.default_rng(2)
    base, ctrl = rng.standard_normal((3, 63, 64)).astype(np.float32), rng.standard_normal((3, 63, 64)).astype(np.float32)
    got = run_ctrl_add(lib, base, ctrl, 1.0, 96, 64)
    assert (got[:, :, 64:] == np.float32(7e30)).all() and np.array_equal(got[:, :, :64], base + ctrl)


def test_ctrl_add_refuses_bad_arguments(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    buf = _lib.from_numpy(np.zeros(3 * 8 * 64 * 3 + 64, np.float32))
    d, b, k = buf.ptr, buf.ptr + 3 * 8 * 64 * 4, buf.ptr + 2 * 3 * 8 * 64 * 4
    g = buf.ptr + 3 * 3 * 8 * 64 * 4
    call = lambda dst=d, ldd=64, base=b, ldb=64, ctrl=k, ldc=64, n=3, rows=8, Cn=64, nc=3, gain=g: \
        lib.mlsd_ctrl_add(dst, ldd, base, ldb, ctrl, ldc, n, rows, Cn, nc, gain, None)
    assert call() == 0
    for kw in (dict(Cn=6), dict(Cn=62), dict(ldd=66), dict(ldb=62), dict(ldc=65), dict(dst=d + 4), dict(base=b + 8), dict(ctrl=k + 4), dict(dst=None),
               dict(gain=None), dict(n=0), dict(rows=0), dict(nc=0), dict(nc=4), dict(ldd=32), dict(dst=k), dict(dst=b + 16 * 64)):
        assert call(**kw) < 0, kw
    K.sync()


# ------------------------------------------------------------------ mlsd_window_gather_nhwc
def test_window_gather_nhwc_is_a_wrapped_copy(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    W, H, Cn, ww, wh, n_rep = 16, 8, 64, 8, 8, 2
    xs, ys = [0, 4, 12, 8], [0, 0, 0, 3]                                # (12, 0) straddles the seam in x, (8, 3) the one in y
    rng = np.random.default_rng(4)
    src = rng.standard_normal((H, W, Cn)).astype(np.float32)
    src[0, 0, 0], src[7, 15, 63], src[3, 3, 3] = np.nan, -0.0, np.inf
    s, d = _lib.from_numpy(src), _lib.DeviceBuffer(len(xs) * n_rep * wh * ww * Cn * 4)
    assert lib.mlsd_window_gather_nhwc(s.ptr, W, H, Cn, d.ptr, ww, wh, (C.c_int * 4)(*xs), (C.c_int * 4)(*ys), len(xs), n_rep, None) == 0
    K.sync()
    got = d.download((len(xs), n_rep, wh, ww, Cn), np.float32)
    for i, (x0, y0) in enumerate(zip(xs, ys)):
        want = np.take(np.take(src, np.arange(y0, y0 + wh), axis=0, mode="wrap"), np.arange(x0, x0 + ww), axis=1, mode="wrap")
        for r in range(n_rep):
            assert got[i, r].tobytes() == want.tobytes(), (i, r)
    one = (C.c_int * 1)(0)
    for kw in (dict(Cn=6), dict(ww=17), dict(wh=9), dict(x0=16), dict(n_slots=0), dict(n_slots=17), dict(n_rep=0), dict(src=s.ptr + 4)):
        a = dict(src=s.ptr, Cn=Cn, ww=ww, wh=wh, x0=0, n_slots=1, n_rep=1)
        a.update(kw)
        one[0] = a["x0"]
        assert lib.mlsd_window_gather_nhwc(a["src"], W, H, a["Cn"], d.ptr, a["ww"], a["wh"], one, (C.c_int * 1)(0), a["n_slots"], a["n_rep"], None) < 0, kw
    K.sync()


# ------------------------------------------------------------------ one evaluation against the reference
def inputs(model, w, h, B, sigma, seed):
    import controlnet_ref as R
    P = R.UNET[model]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, 4, h, w)) * np.sqrt(1 + sigma * sigma)).astype(np.float32)
    c = lambda: (rng.standard_normal((77, P["n_ctx"])) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P["ch_adm_in"]) * 0.5).astype(np.float32)) if P["ch_adm_in"] else (lambda: None)
    cond = (c(), l(), c(), l())
    hint = rng.random((3, 8 * h, 8 * w)).astype(np.float32)
    return x, cond, hint


CFG, SIGMA = 2.0, 2.5
_REF = {}


def reference(model, w, h, B, gain):
    """controlled (gain) or uncontrolled (gain None) reference of the shared inputs, the N = 2B evaluations [2B,4,h,w]; computed once per case"""
    import controlnet_ref as R
    key = (model, w, h, B, gain)
    if key not in _REF:
        x, (c, l, u, ul), hint = inputs(model, w, h, B, SIGMA, 3)
        if "net" not in _REF:
            _REF["net"] = R.make_net()
        _REF[key] = R.eps_rows(_REF["net"], model, x, SIGMA, c, l, u, ul, hint=None if gain is None else hint[None], gain=gain or 0.0)
        _REF[key].setflags(write=False)
    return _REF[key]


def controlled_engine(model, w, h, B, **kw):
    from mlimgsynth_amd import engine as E
    x, cond, hint = inputs(model, w, h, B, SIGMA, 3)
    g = E.Generator(model, 8 * w, 8 * h, B, cfg_scale=CFG, control=True, **kw)
    g.set_cond(*cond)
    return g, x, hint


def rows(g, x):
    """the N = 2B evaluations behind the engine's dxdt (cond of every image, then uncond), un-mixed from its answers at cfg 2 and cfg 3; leaves cfg at CFG"""
    import controlnet_ref as R
    g.set_sampler(cfg_scale=3.0)
    d3 = g.dxdt(x, SIGMA)
    g.set_sampler(cfg_scale=CFG)
    d2 = g.dxdt(x, SIGMA)
    assert np.isfinite(d2).all() and np.isfinite(d3).all()
    return R.unmix(d2, d3)


def retries(g):
    """(passes the engine re-ran on its hand-off-free plans, launches of the UNet plan and of the ControlNet plan that hand data over inside the launch): the
    retry guard of mlis_amd_dxdt / mlis_amd_denoise covers both plans; after clean runs the counter is 0, as in tests/test_sampler_gpu.py and tests/test_unet_gpu.py"""
    from mlimgsynth_amd import _lib
    l = CF.bind(_lib.LIB_PATH)
    return l.mlis_amd_handoff_retries(g.h), l.mlctx_handoff_ops(g.ctx_at(0).h), l.mlctx_handoff_ops(g.ctx_at(5).h)


def per_image(got, want):
    import controlnet_ref as R
    return [R.rel_l2(got[b], want[b]) for b in range(len(got))]


CASES = [("tiny", 8, 8, 2), ("tinyxl", 8, 8, 1), ("tiny", 8, 16, 1), ("tinyv", 8, 8, 1)]


@pytest.mark.parametrize("model,w,h,B", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}" for c in CASES])
def test_controlled_evaluation_against_the_reference(model, w, h, B):
    want, plain = reference(model, w, h, B, 1.0), reference(model, w, h, B, None)
    margin = min(per_image(want, plain))
    assert margin >= 10 * TOL.EVAL_SMALL, margin          # otherwise an engine that ignored the control would pass
    g, x, hint = controlled_engine(model, w, h, B)
    try:
        assert g.control_info()[0] == {"tiny": 5, "tinyv": 5, "tinyxl": 7}[model]      # skip tensors + the middle block
        before, before_dx = rows(g, x), g.dxdt(x, SIGMA)     # no image yet: gain 0
        assert g.control_info()[1] == 0
        g.set_control_image(hint)
        got, got_dx = rows(g, x), g.dxdt(x, SIGMA)
        assert g.control_info()[1] == 1
        err, err0 = per_image(got, want), per_image(before, plain)
        print(f"{model} {w}x{h} b{B}: controlled rel-L2 {err}, without an image {err0}, controlled vs plain reference {margin:.3f}")
        assert len(err) == 2 * B and max(err) <= TOL.EVAL_SMALL
        assert max(err0) <= TOL.EVAL_SMALL
        # the answer of mlis_amd_dxdt itself, at this test's cfg 2: dx = 2 c - u, so |dx - ref| <= 2 |c - c_ref| + |u - u_ref| <= EVAL_SMALL (2 |c_ref| + |u_ref|) per image
        import controlnet_ref as R
        want_dx = R.mix(want, CFG)
        mixed = per_image(got_dx, want_dx)
        print(f"{model} {w}x{h} b{B}: the mixed dx at cfg {CFG}: rel-L2 {mixed}")
        for b in range(B):
            allowed = TOL.EVAL_SMALL * (CFG * np.linalg.norm(want[b].astype(np.float64)) + (CFG - 1) * np.linalg.norm(want[B + b].astype(np.float64)))
            assert np.linalg.norm(got_dx[b].astype(np.float64) - want_dx[b]) <= allowed
        r = retries(g)
        print(f"{model} {w}x{h} b{B}: hand-off retries {r[0]}, hand-off launches of the UNet plan {r[1]}, of the ControlNet plan {r[2]}")
        assert r[0] == 0
        assert np.array_equal(g.dxdt(x, SIGMA), got_dx)
        g.set_control_image(None)
        assert np.array_equal(g.dxdt(x, SIGMA), before_dx)
    finally:
        g.destroy()


def test_half_strength_against_the_reference():
    model, w, h, B = CASES[0]
    want = reference(model, w, h, B, 0.5)
    assert min(per_image(want, reference(model, w, h, B, 1.0))) >= 10 * TOL.EVAL_SMALL
    g, x, hint = controlled_engine(model, w, h, B)
    try:
        g.set_control_image(hint)
        g.set_control(0.5)
        err = per_image(rows(g, x), want)
        print(f"strength 0.5: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL
    finally:
        g.destroy()


def test_parameter_keys_are_the_names_the_reference_asked_for():
    import controlnet_ref as R
    for model, w, h, B in CASES[:2]:
        x, (c, l, u, ul), hint = inputs(model, w, h, B, SIGMA, 3)
        net = R.make_net()
        R.eps_rows(net, model, x, SIGMA, c, l, u, ul, hint=hint[None])
        asked = {n for n, _, _ in net.W.used if n.startswith("control.")}
        g, _, _ = controlled_engine(model, w, h, B)
        try:
            keys = [k for k, _, _ in g.ctx_at(5).param_list()] + [k for k, _, _ in g.ctx_at(6).param_list()]
            assert len(keys) == len(set(keys)) and set(keys) == asked, set(keys) ^ asked
            assert all(k.startswith("control.hint.") for k, _, _ in g.ctx_at(6).param_list())
        finally:
            g.destroy()


# ------------------------------------------------------------------ gain 0 and the step window
def test_strength_zero_meets_the_uncontrolled_reference():
    model, w, h, B = CASES[1]
    g, x, hint = controlled_engine(model, w, h, B)
    try:
        g.set_control_image(hint)
        g.set_control(0.0)
        got = rows(g, x)
        assert g.control_info()[1] == 0                       # the ControlNet plan never ran: its residuals hold whatever the allocation held
        err = per_image(got, reference(model, w, h, B, None))
        print(f"strength 0: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL
        for bad in ((-0.1, 0, 1), (2.5, 0, 1), (1, 0.6, 0.5), (1, -0.1, 1), (1, 0, 1.1), (float("nan"), 0, 1)):
            with pytest.raises(Exception):
                g.set_control(*bad)
    finally:
        g.destroy()


def test_step_window_counts_and_an_empty_window_is_strength_zero():
    """10 steps, window [0.2, 0.7): the midpoints i + 0.5 with 2 <= i + 0.5 < 7 are those of steps 2 .. 6 -- 5 Euler evaluations.  Heun at 20 requested
    steps runs 10 steps of 2 evaluations (the solver keeps the evaluation count); steps 2 .. 6 again, 2 evaluations each: 10."""
    model, w, h, B = "tiny", 8, 8, 1
    g, x, hint = controlled_engine(model, w, h, B, n_step=10)
    try:
        g.set_control_image(hint)
        g.set_control(1.0, 0.2, 0.7)
        g.generate([5], want_images=False)
        assert g.last_n_step() == 10 and g.control_info()[1] == 5 and retries(g)[0] == 0
        g.set_sampler(20, "heun", cfg_scale=CFG, s_ancestral=0.0)
        g.generate([5], want_images=False)
        assert g.last_n_step() == 10 and g.control_info()[1] == 10
        g.set_sampler(10, "euler", cfg_scale=CFG)
        g.set_control(1.0, 0.0, 1.0)
        full, _ = g.generate([5], want_images=False)
        assert g.control_info()[1] == 10
        g.set_control(1.0, 0.0, 0.0)
        empty, _ = g.generate([5], want_images=False)
        assert g.control_info()[1] == 0
        g.set_control(0.0, 0.0, 1.0)
        zero, _ = g.generate([5], want_images=False)
        assert empty.tobytes() == zero.tobytes() and not np.array_equal(full, zero)
    finally:
        g.destroy()


# ------------------------------------------------------------------ hipGraph replay and weight streaming
@pytest.mark.parametrize("how", ["use_hipgraph", "unet_split"])
def test_hipgraph_and_streaming_are_bit_identical(how):
    model, w, h, B = "tinyxl", 8, 8, 1
    outs = []
    for kw in ({}, {how: 1}):
        g, x, hint = controlled_engine(model, w, h, B, n_step=3, **kw)
        try:
            g.set_control_image(hint)
            a = g.dxdt(x, SIGMA)
            g.set_control(0.5, 0.0, 0.67)                     # the gain changes between replays of the captured graph, and to 0 in the last step
            lat, _ = g.generate([9], want_images=False)
            assert g.control_info()[1] == 2
            g.set_control(1.0)
            outs.append((a, lat, g.dxdt(x, SIGMA)))
            assert retries(g)[0] == 0
        finally:
            g.destroy()
    for p, q in zip(*outs):
        assert np.isfinite(p).all() and p.tobytes() == q.tobytes()
    assert outs[0][0].tobytes() == outs[0][2].tobytes()


# ------------------------------------------------------------------ tiled engines
def tiled_reference(model, x, cond, hint, wins, ww, wh, O, tiling=0):
    """float64 blend of the per-window controlled references; every window sees its crop of the CANVAS's hint embedding"""
    import torch
    import controlnet_ref as R
    import unet_tile_ffi as U
    net = R.make_net()
    c, l, u, ul = cond
    with torch.no_grad():
        hp = torch.from_numpy(hint[None])
        if tiling & 1:                                        # the hint block of a seamless canvas pads circularly along x
            raise NotImplementedError
        emb = R.hint_block(net, R.UNET[model], hp).numpy()
    parts = [R.eps_rows(net, model, U.crop(x, x0, y0, ww, wh), SIGMA, c, l, u, ul, guided=torch.from_numpy(np.ascontiguousarray(U.crop(emb, x0, y0, ww, wh))))
             for x0, y0 in wins]
    H, W = x.shape[-2:]
    return U.blend64(parts, wins, ww, wh, O, H, W)[0]


def test_tiled_engine_against_the_blend_of_controlled_windows():
    import unet_tile_ffi as U
    model, w, h, B = "tiny", 16, 8, 1
    wins, ww, wh = U.windows(w, h, 8, 8, 4)
    assert len(wins) == 3
    x, cond, hint = inputs(model, w, h, B, SIGMA, 3)
    want = tiled_reference(model, x, cond, hint, wins, ww, wh, 4)
    outs = {}
    for pack in (1, 2):
        g, _, _ = controlled_engine(model, w, h, B, unet_tile=64, unet_tile_overlap=32, unet_tile_batch=pack)
        try:
            assert g.tile_info() == (3, 8, 8) and g.tile_pack_info() == ((1, 3) if pack == 1 else (2, 2))
            plain = g.dxdt(x, SIGMA)
            g.set_control_image(hint)
            outs[pack] = g.dxdt(x, SIGMA)
            assert g.control_info()[1] == 1 and not np.array_equal(plain, outs[pack])
            if pack == 1:
                got = rows(g, x)
            assert retries(g)[0] == 0
        finally:
            g.destroy()
    err = per_image(got, want)
    print(f"tiled, 3 windows: rel-L2 {err}")
    assert max(err) <= TOL.EVAL_SMALL
    assert outs[2].tobytes() == outs[1].tobytes()


def test_seamless_ring_with_a_window_across_the_seam():
    """tiling x on a 16-wide canvas with 8-wide windows: a ring of 4 windows at 0, 4, 8, 12, the last one straddles the seam.  The seam is nowhere: the canvas
    and the control image rolled by one window step (4 latent pixels, 32 image pixels) give the rolled answer bit for bit -- the hint block pads circularly
    and the straddling window's crop of the hint embedding wraps like its crop of the latent."""
    model, w, h, B = "tiny", 16, 8, 1
    for pack in (1, 2):
        g, x, hint = controlled_engine(model, w, h, B, unet_tile=64, unet_tile_overlap=32, unet_tile_batch=pack, tiling=1)
        try:
            assert g.tile_info()[0] == 4 and g.tile_windows()[-1] == (12, 0)
            plain = g.dxdt(x, SIGMA)
            g.set_control_image(hint)
            a = g.dxdt(x, SIGMA)
            assert np.isfinite(a).all() and (a != plain)[..., [0, 15]].any()            # the control reaches the columns on both sides of the seam
            g.set_control_image(np.roll(hint, 32, axis=-1))
            b = g.dxdt(np.roll(x, 4, axis=-1), SIGMA)
            assert b.tobytes() == np.roll(a, 4, axis=-1).tobytes()
            g.set_control_image(np.roll(hint, 8, axis=-1))       # one latent pixel: another control, another answer
            assert not np.array_equal(g.dxdt(np.roll(x, 4, axis=-1), SIGMA), b)
        finally:
            g.destroy()


# ------------------------------------------------------------------ the public API
import mlis_ffi as F                # noqa: E402

TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
LONG_TOKS = (np.arange(150, dtype=np.int32) * 37 + 11) % 1000
STEPS = 4


def control_map(side=64, seed=8):
    return np.random.default_rng(seed).integers(0, 256, (side, side, 3), dtype=np.uint8)


def set_control_image(m, arr):
    im = F.Image(arr.ctypes.data_as(C.POINTER(C.c_uint8)), arr.size, arr.shape[1], arr.shape[0], 3, 0)
    assert m.lib.mlis_option_set(m.ctx, CF.CONTROL_IMAGE, C.byref(im)) == 1, m.err()


def context(lib, model="tiny", dim=64, control="synth", opts=()):
    m = F.Mlis(lib)
    m.set("model", f"synth:{model}")
    m.set("image_dim", dim, dim)
    m.set("steps", STEPS), m.set("seed", 42), m.set("cfg_scale", 7.0), m.set("method", "euler_a")
    if control:
        m.set("control_model", control)
        set_control_image(m, control_map())
    for k, v in opts:
        m.set(k, *v) if isinstance(v, tuple) else m.set(k, v)
    return m


def run(lib, m, long=False, decoded=True):
    m.tokens(LONG_TOKS if long else TOKS)
    m.tokens(NTOKS, negative=True)
    m.generate()
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]) if decoded else None, info=lib.mlis_infotext_get(m.ctx, 0).decode(),
                builds=lib.mlis_amd_engine_builds(m.ctx), evals=[lib.mlis_amd_control_evals(m.ctx, p) for p in (0, 1)],
                retries=lib.mlis_amd_handoff_retries(lib.mlis_amd_engine_get(m.ctx)), hint=engine_control_image(lib, m))


def engine_control_image(lib, m):
    """the control image as the engine used last holds it, [3][H][W] at its own pixel size; None without one"""
    from mlimgsynth_amd import _lib
    eng = lib.mlis_amd_engine_get(m.ctx)
    p = lib.mlis_amd_control_image_device(eng)
    if not p:
        return None
    lat = m.tensor(F.TENSOR["LATENT"])
    out = np.empty((3, 8 * lat.shape[2], 8 * lat.shape[3]), np.float32)
    _lib.check(lib.mlsd_memcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(out.nbytes), 1, None), "memcpy")
    _lib.check(lib.mlsd_device_sync(), "sync")
    return out


def resampled(arr, side):
    """the u8 map [h][w][3] as the library converts it (u8 x float(1 / 255), CHW) and resamples it: mlsd_resample2d, bilinear, no wrap"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    src = np.ascontiguousarray(arr.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))
    s, d = _lib.from_numpy(src), _lib.DeviceBuffer(3 * side * side * 4)
    K.resample2d(s.ptr, arr.shape[1], arr.shape[0], d.ptr, side, side, 3, K.RESAMPLE_BILINEAR)
    K.sync()
    return d.download((3, side, side), np.float32)


def generate(lib, long=False, setup=None, **kw):
    m = context(lib, **kw)
    try:
        if setup:
            setup(m)
        return run(lib, m, long)
    finally:
        m.close()


def test_public_api_end_to_end(lib):
    """fresh contexts: every generation starts its Philox streams at offset 0, so results compare bit for bit"""
    plain, a, again = generate(lib, control=None), generate(lib), generate(lib)
    assert plain["builds"] == 1 and "ControlNet" not in plain["info"] and plain["evals"] == [0, -1]
    assert a["builds"] == 1 and a["evals"] == [STEPS, -1] and np.isfinite(a["image"]).all()      # every evaluation (cond and uncond rows are one evaluation)
    assert not np.array_equal(a["latent"], plain["latent"]) and not np.array_equal(a["image"], plain["image"])
    assert ", ControlNet: synth, Control strength: 1, Control window: 0-1, Version: " in a["info"]
    assert a["info"].replace(", ControlNet: synth, Control strength: 1, Control window: 0-1", "") == plain["info"]
    assert again["latent"].tobytes() == a["latent"].tobytes() and again["image"].tobytes() == a["image"].tobytes() and again["info"] == a["info"]
    half = generate(lib, opts=(("control_strength", 0.5),))
    other = generate(lib, setup=lambda m: set_control_image(m, control_map(96, seed=9)))          # another map, another size: resampled
    late = generate(lib, opts=(("control_start", 0.5),))
    seeded = generate(lib, control="synth:77")                                                    # other ControlNet weights
    assert late["evals"] == [2, -1] and ", Control window: 0.5-1, " in late["info"]
    assert len({x["latent"].tobytes() for x in (plain, a, half, other, late, seeded)}) == 6


def test_engine_is_built_once_per_control_setting(lib):
    m = context(lib, control=None)
    try:
        assert run(lib, m)["builds"] == 1
        m.set("control_model", "synth")
        set_control_image(m, control_map())
        r = run(lib, m)
        assert r["builds"] == 2 and r["evals"] == [STEPS, -1]                    # switched on: one more engine, the plain one stays resident
        tag = lib.mlis_amd_control_tag(lib.mlis_amd_engine_get(m.ctx))
        r = run(lib, m)
        assert tag != 0 and lib.mlis_amd_control_tag(lib.mlis_amd_engine_get(m.ctx)) == tag and r["builds"] == 2      # the same image again: the engine keeps the one it holds
        m.set("control_strength", 0.5), m.set("control_end", 0.5)
        set_control_image(m, control_map(96, seed=9))
        r = run(lib, m)
        assert r["builds"] == 2 and r["evals"] == [2, -1]                        # strength, window and image change nothing that is built
        assert lib.mlis_amd_control_tag(lib.mlis_amd_engine_get(m.ctx)) not in (0, tag) and r["hint"].tobytes() == resampled(control_map(96, seed=9), 64).tobytes()
        m.set("control_model", "")
        assert lib.mlis_option_set(m.ctx, CF.CONTROL_IMAGE, C.c_void_p(None)) == 1
        r = run(lib, m)
        assert r["builds"] == 2 and r["evals"] == [0, -1] and "ControlNet" not in r["info"]
    finally:
        m.close()


def test_hires_runs_both_passes_controlled(lib):
    def hires(m):
        m.set("hires_scale", 1.5), m.set("hires_denoise", 0.6), m.set("hires_steps", 3)
    a, off = generate(lib, setup=hires), generate(lib, setup=hires, control=None)
    assert a["latent"].shape == (1, 4, 12, 12) and a["image"].shape == (1, 3, 96, 96) and np.isfinite(a["image"]).all()
    assert a["evals"][0] == STEPS and a["evals"][1] > 0 and a["builds"] == 2 and a["retries"] == 0
    # the engine of the second pass holds the 64 x 64 map resampled to its 96 x 96 pixels, the bits of the resampler; a 64 x 64 generation holds the map itself
    assert a["hint"].shape == (3, 96, 96) and a["hint"].tobytes() == resampled(control_map(), 96).tobytes()
    one = generate(lib)
    assert one["hint"].tobytes() == resampled(control_map(), 64).tobytes() == np.ascontiguousarray(control_map().transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0)).tobytes()
    assert off["hint"] is None
    assert not np.array_equal(a["latent"], off["latent"]) and off["evals"] == [0, 0]
    second_only = generate(lib, setup=lambda m: (hires(m), m.set("control_start", 1.0)))       # an empty window: no pass is controlled
    assert second_only["evals"] == [0, 0] and second_only["latent"].tobytes() == generate(lib, setup=lambda m: (hires(m), m.set("control_strength", 0)))["latent"].tobytes()


def control_file(lib, path, model, prefix="", drop=None, reshape=None):
    """a ControlNet file in the original layout holding the synthetic weights of `model`'s ControlNet and hint plans"""
    import loader_cases as LC
    from safetensors.numpy import save_file
    from mlimgsynth_amd import engine as E
    g = E.Generator(model, 64, 64, 1, control=True)
    try:
        params = g.ctx_at(5).param_list() + g.ctx_at(6).param_list()
    finally:
        g.destroy()
    tensors = {}
    for key, typ, ne in params:
        shape = tuple(ne[::-1])
        v = LC.synth_values(key, shape, typ == 1)
        v = v if ne[3] > 1 else v.reshape(LC.squeeze_shape(shape))          # convolution kernels stay 4-D, the rest is stored as torch does
        name = prefix + CF.original_name(key)
        if name == drop:
            continue
        if name == reshape:
            v = v.reshape(-1)[:-1]
        tensors[name] = v.astype(np.float16) if typ == 1 else v
    tensors[prefix + "output_blocks.0.0.in_layers.0.weight"] = np.zeros(4, np.float32)       # a name the loader must ignore
    save_file(tensors, str(path), metadata={"format": "pt"})


def test_controlnet_file_gives_the_bits_of_the_synthetic_one(lib, tmp_path):
    want = generate(lib, model="tinyxl")
    for prefix in ("", "control_model."):
        p = tmp_path / f"net{len(prefix)}.safetensors"
        control_file(lib, p, "tinyxl", prefix)
        got = generate(lib, model="tinyxl", control=str(p))
        assert got["latent"].tobytes() == want["latent"].tobytes() and got["image"].tobytes() == want["image"].tobytes()
        assert f", ControlNet: net{len(prefix)}, " in got["info"]
    for kw, named in ((dict(drop="zero_convs.3.0.bias"), "control.zero.3.bias"), (dict(reshape="input_hint_block.6.weight"), "control.hint.6.weight"),
                      (dict(drop="label_emb.0.2.weight"), "control.label_embed.2.weight")):
        p = tmp_path / "bad.safetensors"
        control_file(lib, p, "tinyxl", **kw)
        m = context(lib, model="tinyxl", control=str(p))
        try:
            m.tokens(TOKS), m.tokens(NTOKS, negative=True)
            assert lib.mlis_generate(m.ctx) < 0 and named in m.err(), m.err()
        finally:
            m.close()
    p = tmp_path / "sd1like.safetensors"                                    # another architecture: tiny's ControlNet for tinyxl
    control_file(lib, p, "tiny")
    m = context(lib, model="tinyxl", control=str(p))
    try:
        m.tokens(TOKS), m.tokens(NTOKS, negative=True)
        assert lib.mlis_generate(m.ctx) < 0 and "control." in m.err() and "does not fit" in m.err()
    finally:
        m.close()


def img2img_mask(m):
    rgba = np.random.default_rng(3).integers(0, 256, (64, 64, 4), dtype=np.uint8)
    rgba[:, :32, 3], rgba[:, 32:, 3] = 255, 0
    im = F.Image(rgba.ctypes.data_as(C.POINTER(C.c_uint8)), rgba.size, 64, 64, 4, 0)
    assert m.lib.mlis_option_set(m.ctx, F.OPT["IMAGE"], C.byref(im)) == 1, m.err()
    m.set("f_t_ini", 0.6)


COMPOSE = {
    "img2img_mask": dict(setup=img2img_mask),                               # img2img and the in-painting mask (the image's alpha)
    "tiling_xy": dict(opts=(("tiling", "xy"),)),
    "tae": dict(opts=(("tae", "synth"),)),
    "long_prompt": dict(long=True),                                          # 150 tokens: two context windows
    "unet_tile": dict(dim=96, opts=(("unet_tile", 64), ("unet_tile_overlap", 32), ("unet_tile_batch", 2))),
}


@pytest.mark.parametrize("name", list(COMPOSE))
def test_composes_with_the_other_options(lib, name):
    kw = COMPOSE[name]
    a, b, off = generate(lib, **kw), generate(lib, **kw), generate(lib, control=None, **kw)
    assert np.isfinite(a["latent"]).all() and np.isfinite(a["image"]).all()
    assert a["latent"].tobytes() == b["latent"].tobytes() and a["image"].tobytes() == b["image"].tobytes() and a["info"] == b["info"]
    assert not np.array_equal(a["latent"], off["latent"]) and a["evals"][0] > 0 and off["evals"] == [0, -1]
    assert ", ControlNet: synth, " in a["info"] and "ControlNet" not in off["info"] and a["builds"] == off["builds"] == 1
    assert a["retries"] == b["retries"] == off["retries"] == 0            # no pass was run again on the hand-off-free plans (UNet and ControlNet plan share the guard)
