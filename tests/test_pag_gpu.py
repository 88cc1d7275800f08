"""Perturbed-attention guidance on the GPU: the two mix kernels bit for bit against tests/pag_ref.mix, one evaluation of a PAG engine against the torch
restatement through mlis_amd_dxdt, the compositions (HyperTile, ControlNet, FreeU, hipGraph replay, weight streaming, tiled engines) and mlis_generate with the
pag_scale option.

Bounds.  The kernels: none, every operation is rounded once and numpy's float32 arithmetic rounds the same way.  An evaluation: per-image rel-L2 <=
tolerances.EVAL_SMALL for each of the N rows behind mlis_amd_dxdt, un-mixed from its answers at (cfg, scale) = (2, 1), (3, 1), (2, 2) (pag_ref.unmix); before
that the reference's perturbed rows are asserted to lie more than 10 x that bound from its cond rows, so an engine that ignored the perturbation would fail.  A
tiled engine: the blend of window-sized PAG engines within (cfg + |1 - cfg| + 2 s) 1e-6 max|part| -- the same plan and bytes, only the blend's fp32 roundings
(1e-6 relative, as tests/test_unet_tile_gpu.py states them) differ, magnified by the absolute coefficients of dx = c f + u (1 - f) + s c - s p.  A generation:
tolerances.LATENT against a torch loop on the reference."""
import ctypes as C
import math

import numpy as np
import pytest

import freeu_ffi as FF
import mlis_ffi as F
import tolerances as TOL

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = F32(7e30)


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    l = FF.bind(_lib.LIB_PATH)      # (mlis_ffi's table with the engine accessors of controlnet_ffi and freeu_ffi)
    i64, cf, vp, ci = C.c_int64, C.c_float, C.c_void_p, C.c_int
    l.mlsd_vec_axpy.argtypes = [vp, vp, vp, cf, i64, vp]
    l.mlsd_noise_add_s.argtypes = [vp, vp, cf, i64, vp]
    l.mlsd_dxdt_cfg.argtypes = [vp, i64, vp, vp] + [ci] * 3 + [cf, ci, cf, cf, vp]
    l.mlsd_dxdt_pag.argtypes = [vp, i64, vp, vp, ci, ci, ci, cf, cf, ci, cf, cf, vp]
    l.mlsd_euler_pag_update.argtypes = [vp, vp, i64, ci, ci, ci, cf, cf, cf, vp, cf, vp]
    l.mlis_amd_pag_info.restype, l.mlis_amd_pag_info.argtypes = ci, [vp, C.POINTER(ci), C.POINTER(ci)]
    return l


# ------------------------------------------------------------------ 1. the kernels
def kernel_inputs(B, HW, ld, groups):
    rng = np.random.default_rng(B * 100000 + HW * 10 + ld + groups)
    eps = np.full((groups * B, HW, ld), POISON, F32)
    eps[:, :, :4] = (rng.standard_normal((groups * B, HW, 4)) * 2).astype(F32)
    x = (rng.standard_normal((B, 4, HW)) * 3).astype(F32)
    noise = rng.standard_normal((B, 4, HW)).astype(F32)
    return eps, x, noise


def rows_of(eps, x, vparam, c_out, c_skip):
    """NHWC [N][HW][ld] -> rows [N][4][HW] after the v-prediction rescale (unet.c:493), each operation rounded once"""
    r = np.ascontiguousarray(eps[:, :, :4].transpose(0, 2, 1))
    if vparam:
        r = (r * c_out + np.concatenate([x] * (len(r) // len(x))) * c_skip).astype(F32)
    return r


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("HW", [1, 63, 64, 1030])
@pytest.mark.parametrize("B", [1, 3])
def test_kernels_bit_for_bit(lib, B, HW, ld):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    import pag_ref as R
    c_out, c_skip, dt, s_up = F32(0.31), F32(0.29), F32(-0.9), F32(0.4)
    for cfg in (0.5, 7.0):
        groups = 3 if cfg > 1 else 2
        eps, x, noise = kernel_inputs(B, HW, ld, groups)
        de, dxe, dn = _lib.from_numpy(eps), _lib.from_numpy(x), _lib.from_numpy(noise)
        for vparam in (0, 1):
            rows = rows_of(eps, x, vparam, c_out, c_skip)
            for pag in (0.0, 1.5, 3.0):
                out = _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
                K.dxdt_pag(de.ptr, ld, dxe.ptr, out.ptr, B, 4, HW, cfg, pag, vparam, c_out, c_skip)
                K.sync()
                got = out.download((B, 4, HW), F32)
                assert got.tobytes() == R.mix(rows, cfg, pag).tobytes(), (cfg, vparam, pag)
            # pag = 0: mlsd_dxdt_cfg's bytes, and the perturbed rows are not read (NaN there)
            nan = eps.copy()
            nan[-B:] = np.nan
            dnan = _lib.from_numpy(nan)
            a, b = _lib.from_numpy(np.full((B, 4, HW), POISON, F32)), _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
            K.dxdt_pag(dnan.ptr, ld, dxe.ptr, a.ptr, B, 4, HW, cfg, 0.0, vparam, c_out, c_skip)
            _lib.check(lib.mlsd_dxdt_cfg(de.ptr, ld, dxe.ptr, b.ptr, B, 4, HW, cfg, vparam, c_out, c_skip, None))
            K.sync()
            assert a.download((B, 4, HW), F32).tobytes() == b.download((B, 4, HW), F32).tobytes()
            assert np.isfinite(a.download((B, 4, HW), F32)).all()
        # the fused Euler(-ancestral) step == mlsd_dxdt_pag + mlsd_vec_axpy + mlsd_noise_add_s, with and without noise
        for pag in (0.0, 1.5):
            for nz in (None, dn):
                xa, xb, dx = _lib.from_numpy(x), _lib.from_numpy(x), _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
                K.euler_pag_update(xa.ptr, de.ptr, ld, B, 4, HW, cfg, pag, dt, nz.ptr if nz else None, s_up)
                K.dxdt_pag(de.ptr, ld, xb.ptr, dx.ptr, B, 4, HW, cfg, pag, 0, 1.0, 0.0)
                _lib.check(lib.mlsd_vec_axpy(xb.ptr, xb.ptr, dx.ptr, dt, B * 4 * HW, None))
                if nz:
                    _lib.check(lib.mlsd_noise_add_s(xb.ptr, nz.ptr, s_up, B * 4 * HW, None))
                K.sync()
                got = xa.download((B, 4, HW), F32)
                assert got.tobytes() == xb.download((B, 4, HW), F32).tobytes(), (cfg, pag, nz is not None)
                want = (x + R.mix(rows_of(eps, x, 0, c_out, c_skip), cfg, pag) * dt).astype(F32)
                assert got.tobytes() == ((want + noise * s_up).astype(F32) if nz else want).tobytes()


def test_kernels_take_unaligned_and_generic_shapes_and_refuse_bad_arguments(lib):
    """the element-per-thread form (C != 4; an eps base that is not 16-byte aligned) computes the same bytes; bad arguments are refused before any launch"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    import pag_ref as R
    B, HW, ld = 2, 20, 8
    eps, x, _ = kernel_inputs(B, HW, ld, 3)
    shifted = np.concatenate([np.zeros(1, F32), eps.reshape(-1)])
    de, dxe = _lib.from_numpy(shifted), _lib.from_numpy(x)
    out = _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
    K.dxdt_pag(de.ptr + 4, ld, dxe.ptr, out.ptr, B, 4, HW, 7.0, 2.0)
    K.sync()
    assert out.download((B, 4, HW), F32).tobytes() == R.mix(rows_of(eps, x, 0, 1, 0), 7.0, 2.0).tobytes()
    eps3 = np.ascontiguousarray(eps[:, :, :3])                   # C = 3, ld = 3
    out3 = _lib.from_numpy(np.full((B, 3, HW), POISON, F32))
    d3 = _lib.from_numpy(eps3)
    K.dxdt_pag(d3.ptr, 3, dxe.ptr, out3.ptr, B, 3, HW, 7.0, 2.0)
    K.sync()
    assert out3.download((B, 3, HW), F32).tobytes() == R.mix(np.ascontiguousarray(eps3.transpose(0, 2, 1)), 7.0, 2.0).tobytes()
    f = lib.mlsd_dxdt_pag
    for kw in (dict(eps=None), dict(dx=None), dict(B=0), dict(Cn=0), dict(HW=0), dict(ld=3), dict(pag=-1.0), dict(pag=float("nan")), dict(x=None, vparam=1)):
        a = dict(eps=de.ptr + 4, ld=ld, x=dxe.ptr, dx=out.ptr, B=B, Cn=4, HW=HW, cfg=7.0, pag=1.0, vparam=0)
        a.update(kw)
        assert f(a["eps"], a["ld"], a["x"], a["dx"], a["B"], a["Cn"], a["HW"], a["cfg"], a["pag"], a["vparam"], 1.0, 0.0, None) < 0, kw
    assert lib.mlsd_euler_pag_update(None, de.ptr + 4, ld, B, 4, HW, 7.0, 1.0, 0.1, None, 0.0, None) < 0


# ------------------------------------------------------------------ 2. one evaluation against the reference
SIGMA = 2.5
CASES = [("tiny", 8, 8, 2, 2.0), ("tinyxl", 8, 8, 1, 2.0), ("tiny", 8, 16, 1, 2.0), ("tinyv", 8, 8, 1, 2.0), ("tiny", 8, 8, 1, 1.0)]
_REF = {}


def inputs(model, w, h, B):
    from test_freeu_gpu import inputs as freeu_inputs          # the inputs the margins of the issue were measured on
    return freeu_inputs(model, w, h, B)


def net(tile=0):
    import pag_ref as R
    if ("net", tile) not in _REF:
        _REF[("net", tile)] = R.make_net(tile)
    return _REF[("net", tile)]


def reference(model, w, h, B, cfg, tile=0, control=False, freeu=None):
    """the N rows of the shared inputs, [N,4,h,w]; once per case, read-only"""
    import pag_ref as R
    key = (model, w, h, B, cfg > 1, tile, control, freeu)
    if key not in _REF:
        x, (c, l, u, ul), hint = inputs(model, w, h, B)
        rows_fn = None
        if freeu:
            import freeu_ref as FR
            rows_fn = lambda n, m, x_, s, c_, l_, u_, ul_, **kw: FR.eps_rows(n, m, x_, s, c_, l_, u_, ul_, freeu, **kw)
        _REF[key] = R.eps_rows(net(tile), model, x, SIGMA, c, l, u, ul, cfg=cfg, hint=hint[None] if control else None, rows_fn=rows_fn)
        _REF[key].setflags(write=False)
    return _REF[key]


def engine(model, w, h, B, cfg=2.0, **kw):
    from mlimgsynth_amd import engine as E
    x, cond, hint = inputs(model, w, h, B)
    g = E.Generator(model, 8 * w, 8 * h, B, cfg_scale=cfg, pag=True, **kw)
    g.set_cond(*cond) if cfg > 1 else g.set_cond(cond[0], cond[1])
    return g, x, hint


def rows(g, x, cfg):
    """the N rows behind the engine's dxdt (pag_ref.unmix); leaves the engine at (cfg, scale 1)"""
    import pag_ref as R
    out = []
    for f, s in (((2.0, 1.0), (3.0, 1.0), (2.0, 2.0)) if cfg > 1 else ((cfg, 1.0), (cfg, 2.0))):
        g.set_sampler(cfg_scale=f)
        g.set_pag(s)
        out.append(g.dxdt(x, SIGMA))
        assert np.isfinite(out[-1]).all()
    g.set_sampler(cfg_scale=cfg)
    g.set_pag(1.0)
    return R.unmix(out, cfg)


def per_image(got, want):
    import pag_ref as R
    return [R.rel_l2(got[b], want[b]) for b in range(len(want))]


def margin(want, B):
    """how far the reference's perturbed rows lie from its cond rows"""
    return min(per_image(want[-B:], want[:B]))


@pytest.mark.parametrize("model,w,h,B,cfg", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}-cfg{c[4]:g}" for c in CASES])
def test_evaluation_against_the_reference(model, w, h, B, cfg):
    import pag_ref as R
    want = reference(model, w, h, B, cfg)
    N = (3 if cfg > 1 else 2) * B
    m = margin(want, B)
    assert len(want) == N and m > 10 * TOL.EVAL_SMALL, m         # otherwise an engine that ignored the perturbation would pass
    g, x, _ = engine(model, w, h, B, cfg)
    try:
        assert g.pag_info() == (R.N_ATTN[model], N)
        plain = g.dxdt(x, SIGMA)                                 # the flag alone, scale 0: the plain mix of the first groups
        got = rows(g, x, cfg)
        err = per_image(got, want)
        print(f"{model} {w}x{h} b{B} cfg {cfg:g}: PAG rel-L2 per row {err}; perturbed vs cond rows of the reference {m:.3f}")
        assert len(got) == N and max(err) <= TOL.EVAL_SMALL
        assert min(per_image(got[-B:], want[:B])) > 10 * TOL.EVAL_SMALL          # visibly perturbed
        g.set_pag(0)
        assert g.dxdt(x, SIGMA).tobytes() == plain.tobytes()
        want0 = R.mix(want, cfg, 0)
        assert max(per_image(plain, want0)) <= (cfg + abs(1 - cfg) if cfg > 1 else 1) * TOL.EVAL_SMALL
        g.set_pag(1.5)
        again = g.dxdt(x, SIGMA)
        assert np.array_equal(g.dxdt(x, SIGMA), again) and not np.array_equal(again, plain)      # the same bits on a second call
    finally:
        g.destroy()


# ------------------------------------------------------------------ 3. compositions
def test_with_hypertile_at_the_middle_level():
    model, w, h, B, tile = "tiny", 16, 16, 1, 32
    want, untiled = reference(model, w, h, B, 2.0, tile=tile), reference(model, w, h, B, 2.0)
    assert margin(want, B) > 10 * TOL.EVAL_SMALL and min(per_image(want, untiled)) > 10 * TOL.EVAL_SMALL      # neither half alone would pass
    g, x, _ = engine(model, w, h, B, hypertile=tile)
    try:
        assert g.hypertile_info()[2][1] == (4, 4, 2, 2) and g.pag_info() == (1, 3)          # the middle level (8 x 8 tokens) is cut into 4 x 4 tiles
        err = per_image(rows(g, x, 2.0), want)
        print(f"PAG + HyperTile: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL
    finally:
        g.destroy()


@pytest.mark.parametrize("cfg", [2.0, 1.0])
def test_with_a_controlnet_the_perturbed_rows_get_the_cond_residuals(cfg):
    model, w, h, B = "tinyxl", 8, 8, 1
    want, bare = reference(model, w, h, B, cfg, control=True), reference(model, w, h, B, cfg)
    assert margin(want, B) > 10 * TOL.EVAL_SMALL and min(per_image(want, bare)) > 10 * TOL.EVAL_SMALL
    g, x, hint = engine(model, w, h, B, cfg, control=True)
    try:
        assert g.cfg.control == 9 and g.control_info()[0] > 0
        g.set_control_image(hint)
        err = per_image(rows(g, x, cfg), want)
        print(f"PAG + ControlNet at cfg {cfg:g}: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL and g.control_info()[1] == 1
    finally:
        g.destroy()


def test_with_freeu():
    model, w, h, B, ON = "tiny", 8, 8, 2, (1.4, 1.6, 0.9, 0.2)
    want, bare = reference(model, w, h, B, 2.0, freeu=ON), reference(model, w, h, B, 2.0)
    assert margin(want, B) > 10 * TOL.EVAL_SMALL and min(per_image(want, bare)) > 10 * TOL.EVAL_SMALL
    g, x, _ = engine(model, w, h, B, freeu=True)
    try:
        g.set_freeu(*ON)
        err = per_image(rows(g, x, 2.0), want)
        print(f"PAG + FreeU: rel-L2 {err}")
        assert max(err) <= TOL.EVAL_SMALL and g.freeu_info() == (3, 1)
    finally:
        g.destroy()


@pytest.mark.parametrize("how", ["use_hipgraph", "unet_split"])
def test_hipgraph_and_streaming_are_bit_identical(lib, how):
    model, w, h, B = "tinyxl", 8, 8, 1
    outs = []
    for kw in ({}, {how: 1}):
        g, x, _ = engine(model, w, h, B, n_step=3, **kw)
        try:
            g.set_pag(3.0)
            a = g.dxdt(x, SIGMA)
            g.set_pag(1.25)                                      # the scale changes between replays of the captured evaluation
            lat, _ = g.generate([9], want_images=False)
            g.set_pag(3.0)
            outs.append((a, lat, g.dxdt(x, SIGMA)))
            assert lib.mlis_amd_handoff_retries(g.h) == 0
        finally:
            g.destroy()
    for p, q in zip(*outs):
        assert np.isfinite(p).all() and p.tobytes() == q.tobytes()
    assert outs[0][0].tobytes() == outs[0][2].tobytes()


def test_tiled_engine_equals_the_blend_of_pag_windows():
    import unet_tile_ffi as U
    from mlimgsynth_amd import engine as E
    model, cfg, s, B = "tiny", 7.0, 1.5, 2
    x, cond, _ = inputs(model, 12, 12, B)
    wins, ww, wh = U.windows(12, 12, 8, 8, 4)
    tiled = E.Generator(model, 96, 96, B, cfg_scale=cfg, unet_tile=64, unet_tile_overlap=32, pag=True)
    packed = E.Generator(model, 96, 96, B, cfg_scale=cfg, unet_tile=64, unet_tile_overlap=32, unet_tile_batch=2, pag=True)
    plain = E.Generator(model, 64, 64, B, cfg_scale=cfg, pag=True)
    try:
        assert tiled.tile_info() == (4, 8, 8) and tiled.pag_info() == plain.pag_info() == (1, 6) and packed.tile_pack_info() == (2, 2)
        for g in (tiled, packed, plain):
            g.set_cond(*cond)
        off = tiled.dxdt(x, SIGMA)
        for g in (tiled, packed, plain):
            g.set_pag(s)
        got = tiled.dxdt(x, SIGMA)
        parts = [plain.dxdt(U.crop(x, x0, y0, ww, wh), SIGMA) for x0, y0 in wins]
        want, _ = U.blend64(parts, wins, ww, wh, 4, 12, 12)
        scale = max(np.abs(p).max() for p in parts)
        coef = cfg + abs(1 - cfg) + 2 * s
        bound = coef * 1e-6 * scale
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"tiled PAG: max|err| = {err:.3e}, bound {bound:.3e}")
        assert np.isfinite(got).all() and err <= bound and not np.array_equal(got, off)
        # packed windows: another batch size of the same plan, within the evaluation tolerance of the unpacked answer weighed by the mix's coefficients
        assert max(per_image(packed.dxdt(x, SIGMA), got)) <= coef * TOL.EVAL_SMALL
    finally:
        tiled.destroy(), packed.destroy(), plain.destroy()


# ------------------------------------------------------------------ 4. generation through the C-ABI
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
STEPS, SEED, GCFG, GSCALE = 6, 42, 2.0, 1.5


def context(lib, method="euler_a", pag=None):
    m = F.Mlis(lib)
    m.set("model", "synth:tiny")
    m.set("image_dim", 64, 64)
    m.set("steps", STEPS), m.set("seed", SEED), m.set("cfg_scale", GCFG), m.set("method", method)
    if pag is not None:
        m.set("pag_scale", pag)
    return m


def run_generate(lib, m):
    m.tokens(TOKS)
    m.tokens(NTOKS, negative=True)
    m.generate()
    eng = lib.mlis_amd_engine_get(m.ctx)
    n, r = C.c_int(), C.c_int()
    assert lib.mlis_amd_pag_info(eng, C.byref(n), C.byref(r)) == 1
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]), info=lib.mlis_infotext_get(m.ctx, 0).decode(),
                builds=lib.mlis_amd_engine_builds(m.ctx), pag=(n.value, r.value), cond=m.tensor(F.TENSOR["COND"])[0, 0], ncond=m.tensor(F.TENSOR["NCOND"])[0, 0])


def torch_loop(method, cond, ncond, scale):
    """the generation on the reference: schedule, Philox draws and the ancestral split from the library's host functions, every evaluation on pag_ref"""
    import pag_ref as R
    from mlimgsynth_amd import engine as E
    sig = E.schedule("tiny", STEPS)
    n = len(sig) - 1
    draw = lambda k: E.randn(SEED, k, 4 * 64)[0].reshape(1, 4, 8, 8)
    dxdt = lambda x, s: R.mix(R.eps_rows(net(), "tiny", x.astype(F32), s, cond, None, ncond, None, cfg=GCFG), GCFG, scale)
    x = (draw(0) * sig[0]).astype(F32)
    k = 1
    if method == "euler_a":
        for i in range(n):
            sd, su = C.c_float(), C.c_float()
            E._proto2().dnsamp_ancestral(float(sig[i]), float(sig[i + 1]), 1.0, C.byref(sd), C.byref(su))
            x = (x + dxdt(x, float(sig[i])) * F32(F32(sd.value) - sig[i])).astype(F32)
            if su.value > 0 and i + 1 != n:
                x = (x + draw(k) * F32(su.value)).astype(F32)
                k += 1
        return x
    h_last, dprev = 0.0, np.zeros_like(x)                       # dpmpp2m (solvers.c:207-233)
    for i in range(n):
        t0, t1 = F32(sig[i]), F32(sig[i + 1])
        a = F32(t1 / t0)
        hh = -math.log(a) if a > 0 else math.inf
        c = F32(hh / (2 * h_last)) if (i > 0 and t1 > 0) else F32(0)
        d0 = x - t0 * dxdt(x, float(t0))
        d = (F32(1) + c) * d0 - c * dprev
        x = (a * x + (F32(1) - a) * d).astype(F32)
        dprev, h_last = d0, hh
    return x


@pytest.mark.parametrize("method", ["euler_a", "dpmpp2m"])
def test_generation_against_a_torch_loop(lib, method):
    import pag_ref as R
    m = context(lib, method, GSCALE)
    try:
        a = run_generate(lib, m)
    finally:
        m.close()
    assert a["builds"] == 1 and a["pag"] == (1, 3) and np.isfinite(a["image"]).all() and f", PAG: {GSCALE:g}, " in a["info"]
    want = torch_loop(method, a["cond"], a["ncond"], GSCALE)
    plain = torch_loop(method, a["cond"], a["ncond"], 0.0)
    e, apart = R.rel_l2(a["latent"], want), R.rel_l2(plain, want)
    print(f"{method}: final latent vs the torch loop rel-L2 {e:.3e}; the loop without PAG lies {apart:.3f} away")
    assert apart > 10 * TOL.LATENT and e < TOL.LATENT


def test_scale_zero_is_the_plain_engine_and_the_value_builds_nothing(lib):
    """fresh contexts start their Philox streams at offset 0, so results compare bit for bit"""
    def one(pag):
        m = context(lib, pag=pag)
        try:
            return run_generate(lib, m)
        finally:
            m.close()
    never, zero, on = one(None), one(0), one(GSCALE)
    assert zero["latent"].tobytes() == never["latent"].tobytes() and zero["image"].tobytes() == never["image"].tobytes() and zero["info"] == never["info"]
    assert zero["builds"] == never["builds"] == 1 and zero["pag"] == never["pag"] == (0, 2) and "PAG" not in zero["info"]
    assert on["pag"] == (1, 3) and not np.array_equal(on["latent"], never["latent"])
    # the parameters text gains the scale, and the NFE count follows the rows: 3 evaluations per image and step, not 2
    assert f"NFE: {3 * STEPS}, " in on["info"] and on["info"].replace(f", PAG: {GSCALE:g}", "").replace(f"NFE: {3 * STEPS},", f"NFE: {2 * STEPS},") == never["info"]
    m = context(lib, pag=0)
    try:
        first = run_generate(lib, m)
        assert first["builds"] == 1 and first["latent"].tobytes() == never["latent"].tobytes()
        m.set("pag_scale", GSCALE), m.set("seed", SEED)
        second = run_generate(lib, m)
        assert second["builds"] == 2 and second["pag"] == (1, 3)                 # switched on: one more engine, the plain one stays resident
        m.set("pag_scale", 3), m.set("seed", SEED)
        third = run_generate(lib, m)
        assert third["builds"] == 2 and ", PAG: 3, " in third["info"] and not np.array_equal(third["latent"], second["latent"])      # the value builds nothing
        m.set("pag_scale", 0), m.set("seed", SEED)
        assert run_generate(lib, m)["builds"] == 2                               # back on the resident plain engine
    finally:
        m.close()
    # a batch whose rows the engine refuses is a bad option value, before anything is built
    m = context(lib, pag=GSCALE)
    try:
        m.set("batch_size", 43)
        m.tokens(TOKS), m.tokens(NTOKS, negative=True)
        assert lib.mlis_generate(m.ctx) == -4 and "pag_scale" in m.err() and lib.mlis_amd_engine_builds(m.ctx) == 0
    finally:
        m.close()
