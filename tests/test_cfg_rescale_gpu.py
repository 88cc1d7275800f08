"""v-prediction / zero-terminal-SNR / guidance rescale on the GPU: the statistics kernel against float64, the two apply kernels bit for bit against a numpy float32
restatement of the rule, one evaluation of an engine (mlis_amd_dxdt) and whole generations against a loop on the engine's own evaluations, and the options through
the C-ABI.

The rule (include/mlsd_kernels.h), per image over its n = C*HW elements, c / u / p the raw outputs of the row groups:
    g = fadd(fmul(c, cfg), fmul(u, 1 - cfg))  (cfg > 1; else c);   g = fadd(g, fmul(pag, fsub(c, p)))  (pag != 0)
    f = phi*sqrt(M2(c) / M2(g)) + (1 - phi);   r = fmul(g, f);   dx = vparam ? fadd(fmul(r, c_out), fmul(x, c_skip)) : r

Bounds.  factor: 2 float ulps of the float64 value (double accumulation over n <= 3e5 elements errs below 1e-10; what is left is the one rounding to float).  The
apply kernels: none, every operation is rounded once and numpy's float32 arithmetic rounds the same way.  An engine's evaluation: derived in expected64 from the
fp32 roundings of the chain.  A generation: tolerances.LATENT, as tests/test_pag_gpu.py."""
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
PHI = F32(0.7)
U32 = 2.0 ** -24      # unit roundoff of float32


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    l = FF.bind(_lib.LIB_PATH)
    i64, cf, vp, ci = C.c_int64, C.c_float, C.c_void_p, C.c_int
    l.mlsd_vec_axpy.argtypes = [vp, vp, vp, cf, i64, vp]
    l.mlsd_noise_add_s.argtypes = [vp, vp, cf, i64, vp]
    l.mlsd_guidance_stats.argtypes = [vp, i64, ci, ci, ci, cf, cf, cf, vp, C.c_size_t, vp, vp]
    l.mlsd_dxdt_rescaled.argtypes = [vp, i64, vp, vp, ci, ci, ci, cf, cf, vp, ci, cf, cf, vp]
    l.mlsd_euler_rescaled_update.argtypes = [vp, vp, i64, ci, ci, ci, cf, cf, vp, cf, vp, cf, vp]
    l.mlis_amd_pag_info.restype, l.mlis_amd_pag_info.argtypes = ci, [vp, C.POINTER(ci), C.POINTER(ci)]
    return l


# ------------------------------------------------------------------ the rule in numpy
def guided32(rows, B, cfg, pag):
    """rows [N][C][HW] raw outputs -> (c, g) float32, each operation rounded once like the kernels'"""
    c = rows[:B]
    g = c
    if cfg > 1:
        g = (c * F32(cfg) + rows[B:2 * B] * (F32(1) - F32(cfg))).astype(F32)
    if pag != 0:
        g = (g + F32(pag) * (c - rows[-B:])).astype(F32)
    return c, g


def factor64(c, g, phi):
    """float64 factors of float32 c, g [B][...]"""
    out = []
    for cb, gb in zip(c.astype(np.float64), g.astype(np.float64)):
        m2c, m2g = ((cb - cb.mean()) ** 2).sum(), ((gb - gb.mean()) ** 2).sum()
        ok = cb.size > 1 and m2g > 0 and np.isfinite(m2g)
        out.append(float(phi) * math.sqrt(m2c / m2g) + (1.0 - float(phi)) if ok else 1.0)
    return np.array(out)


def ulps(got, want64):
    return np.abs(got.astype(np.float64) - want64) / np.spacing(want64.astype(F32)).astype(np.float64)


def stat_inputs(B, HW, ld, groups, Cn=4):
    """unit normals with a per-image mean offset of 5: float32 sums of squares would lose digits on this"""
    rng = np.random.default_rng(B * 1000003 + HW * 10 + ld + groups)
    eps = np.full((groups * B, HW, ld), POISON, F32)
    eps[:, :, :Cn] = (rng.standard_normal((groups * B, HW, Cn)) + 5.0 + rng.standard_normal((groups * B, 1, 1))).astype(F32)
    return eps


def run_stats(K, _lib, de_ptr, ld, B, Cn, HW, cfg, pag, phi=PHI):
    nb = K.guidance_scratch_bytes(B, HW)
    scratch = _lib.from_numpy(np.full(nb // 8, np.nan, np.float64))
    fac = _lib.from_numpy(np.full(B, POISON, F32))
    K.guidance_stats(de_ptr, ld, B, Cn, HW, cfg, pag, phi, scratch.ptr, nb, fac.ptr)
    K.sync()
    return fac, fac.download((B,), F32)


# ------------------------------------------------------------------ 1. the statistics
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("HW", [1, 63, 64, 1030, 66001])
@pytest.mark.parametrize("B", [1, 3])
def test_factor_against_float64(lib, B, HW, ld):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    eps = stat_inputs(B, HW, ld, 3)
    de = _lib.from_numpy(eps)
    rows3 = np.ascontiguousarray(eps[:, :, :4].transpose(0, 2, 1))
    for cfg in (1.0, 7.5):
        for pag in (0.0, 3.0):
            # the groups the kernel reads at this mode: [cond | uncond (cfg > 1) | perturbed (pag)], packed from the front of the buffer
            n_groups = 1 + (cfg > 1) + (pag != 0)
            rows = rows3[:n_groups * B]
            c, g = guided32(rows, B, cfg, pag)
            want = factor64(c, g, PHI)
            _, got = run_stats(K, _lib, de.ptr, ld, B, 4, HW, cfg, pag)
            _, again = run_stats(K, _lib, de.ptr, ld, B, 4, HW, cfg, pag)
            e = ulps(got, want)
            print(f"B {B} HW {HW} ld {ld} cfg {cfg} pag {pag}: factors {got}, error in ulps {e}")
            assert got.tobytes() == again.tobytes()
            assert (e <= 2).all(), (cfg, pag, got, want)
            if cfg == 1.0 and pag == 0.0:
                assert (got == 1.0).all()                                   # g is c: exactly 1
            else:
                assert (np.abs(got - 1) > 1e-3).all()                       # (the inputs make the rescale visible)


def test_factor_generic_shapes_and_degenerate_cases(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    # C = 3, ld = 3: the element-by-element form
    B, HW = 2, 1030
    eps = stat_inputs(B, HW, 3, 3, Cn=3)
    de = _lib.from_numpy(eps)
    rows = np.ascontiguousarray(eps.transpose(0, 2, 1))
    c, g = guided32(rows, B, 7.5, 3.0)
    _, got = run_stats(K, _lib, de.ptr, 3, B, 3, HW, 7.5, 3.0)
    assert (ulps(got, factor64(c, g, PHI)) <= 2).all()
    # C = 4 on a base that is not 16-byte aligned: the same form, the same factors as the aligned launch to 2 ulps of float64
    eps4 = stat_inputs(B, HW, 8, 2)
    shifted = _lib.from_numpy(np.concatenate([np.zeros(1, F32), eps4.reshape(-1)]))
    c, g = guided32(np.ascontiguousarray(eps4[:, :, :4].transpose(0, 2, 1)), B, 7.5, 0.0)
    _, got = run_stats(K, _lib, shifted.ptr + 4, 8, B, 4, HW, 7.5, 0.0)
    assert (ulps(got, factor64(c, g, PHI)) <= 2).all()
    # phi 0 -> 1 exactly, phi 1 -> the plain ratio
    _, got0 = run_stats(K, _lib, shifted.ptr + 4, 8, B, 4, HW, 7.5, 0.0, phi=0.0)
    _, got1 = run_stats(K, _lib, shifted.ptr + 4, 8, B, 4, HW, 7.5, 0.0, phi=1.0)
    assert (got0 == 1.0).all() and (ulps(got1, factor64(c, g, 1.0)) <= 2).all()
    # degenerate: a constant g (c and u constant per image), n = 1, and g = c
    const = np.full((2 * B, 64, 4), POISON, F32)
    const[:B], const[B:] = F32(1.25), F32(-0.5)
    dconst = _lib.from_numpy(const)
    _, got = run_stats(K, _lib, dconst.ptr, 4, B, 4, 64, 7.5, 0.0)
    assert got.tolist() == [1.0] * B
    one = np.array([[[2.0]], [[3.0]]], F32)                                # B = 1, C = 1, HW = 1, two groups
    done = _lib.from_numpy(one)
    _, got = run_stats(K, _lib, done.ptr, 1, 1, 1, 1, 7.5, 0.0)
    assert got.tolist() == [1.0]
    _, got = run_stats(K, _lib, de.ptr, 3, B, 3, HW, 1.0, 0.0)
    assert got.tolist() == [1.0] * B
    nan = stat_inputs(1, 64, 4, 2)
    nan[1, 5, 2] = np.nan                                                  # a non-finite M2(g)
    dnan = _lib.from_numpy(nan)
    _, got = run_stats(K, _lib, dnan.ptr, 4, 1, 4, 64, 7.5, 0.0)
    assert got.tolist() == [1.0]


# ------------------------------------------------------------------ 2. the apply kernels
def kernel_inputs(B, HW, ld, groups):
    rng = np.random.default_rng(B * 100000 + HW * 10 + ld + groups)
    eps = np.full((groups * B, HW, ld), POISON, F32)
    eps[:, :, :4] = (rng.standard_normal((groups * B, HW, 4)) * 2 + rng.standard_normal((groups * B, 1, 1))).astype(F32)
    x = (rng.standard_normal((B, 4, HW)) * 3).astype(F32)
    noise = rng.standard_normal((B, 4, HW)).astype(F32)
    return eps, x, noise


def apply32(rows, x, B, cfg, pag, fac, vparam, c_out, c_skip):
    _, g = guided32(rows, B, cfg, pag)
    r = (g * fac.reshape(B, 1, 1)).astype(F32)
    return (r * c_out + x * c_skip).astype(F32) if vparam else r


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("HW", [1, 63, 64, 1030])
@pytest.mark.parametrize("B", [1, 3])
def test_apply_kernels_bit_for_bit(lib, B, HW, ld):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    c_out, c_skip, dt, s_up = F32(0.31), F32(0.29), F32(-0.9), F32(0.4)
    for cfg in (0.5, 7.0):
        for pag in (0.0, 1.5):
            groups = 1 + (cfg > 1) + (pag != 0)
            eps, x, noise = kernel_inputs(B, HW, ld, groups)
            rows = np.ascontiguousarray(eps[:, :, :4].transpose(0, 2, 1))
            de, dxe, dn = _lib.from_numpy(eps), _lib.from_numpy(x), _lib.from_numpy(noise)
            dfac, fac = run_stats(K, _lib, de.ptr, ld, B, 4, HW, cfg, pag)
            assert np.isfinite(fac).all() and (groups == 1) == bool((fac == 1).all())
            for vparam in (0, 1):
                outs = []
                for _ in range(2):
                    out = _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
                    K.dxdt_rescaled(de.ptr, ld, dxe.ptr, out.ptr, B, 4, HW, cfg, pag, dfac.ptr, vparam, c_out, c_skip)
                    K.sync()
                    outs.append(out.download((B, 4, HW), F32))
                assert outs[0].tobytes() == outs[1].tobytes()                                    # two launches, the same bytes
                assert outs[0].tobytes() == apply32(rows, x, B, cfg, pag, fac, vparam, c_out, c_skip).tobytes(), (cfg, pag, vparam)
            # the fused Euler(-ancestral) step == mlsd_dxdt_rescaled + mlsd_vec_axpy + mlsd_noise_add_s, with and without noise
            for nz in (None, dn):
                xa, xb, dx = _lib.from_numpy(x), _lib.from_numpy(x), _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
                K.euler_rescaled_update(xa.ptr, de.ptr, ld, B, 4, HW, cfg, pag, dfac.ptr, dt, nz.ptr if nz else None, s_up)
                K.dxdt_rescaled(de.ptr, ld, xb.ptr, dx.ptr, B, 4, HW, cfg, pag, dfac.ptr, 0, 1.0, 0.0)
                _lib.check(lib.mlsd_vec_axpy(xb.ptr, xb.ptr, dx.ptr, dt, B * 4 * HW, None))
                if nz:
                    _lib.check(lib.mlsd_noise_add_s(xb.ptr, nz.ptr, s_up, B * 4 * HW, None))
                K.sync()
                got = xa.download((B, 4, HW), F32)
                assert got.tobytes() == xb.download((B, 4, HW), F32).tobytes(), (cfg, pag, nz is not None)
                want = (x + apply32(rows, x, B, cfg, pag, fac, 0, c_out, c_skip) * dt).astype(F32)
                assert got.tobytes() == ((want + noise * s_up).astype(F32) if nz else want).tobytes()


def test_apply_generic_shapes_and_bad_arguments(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    B, HW, ld = 2, 20, 8
    eps, x, _ = kernel_inputs(B, HW, ld, 3)
    rows = np.ascontiguousarray(eps[:, :, :4].transpose(0, 2, 1))
    shifted = np.concatenate([np.zeros(1, F32), eps.reshape(-1)])
    de, dxe = _lib.from_numpy(shifted), _lib.from_numpy(x)
    dfac, fac = run_stats(K, _lib, de.ptr + 4, ld, B, 4, HW, 7.0, 2.0)
    out = _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
    K.dxdt_rescaled(de.ptr + 4, ld, dxe.ptr, out.ptr, B, 4, HW, 7.0, 2.0, dfac.ptr)      # an eps base that is not 16-byte aligned
    K.sync()
    assert out.download((B, 4, HW), F32).tobytes() == apply32(rows, x, B, 7.0, 2.0, fac, 0, 1, 0).tobytes()
    eps3 = np.ascontiguousarray(eps[:, :, :3])                                           # C = 3, ld = 3
    d3, out3 = _lib.from_numpy(eps3), _lib.from_numpy(np.full((B, 3, HW), POISON, F32))
    dfac3, fac3 = run_stats(K, _lib, d3.ptr, 3, B, 3, HW, 7.0, 2.0)
    x3 = np.ascontiguousarray(x[:, :3])
    dx3 = _lib.from_numpy(x3)
    K.dxdt_rescaled(d3.ptr, 3, dx3.ptr, out3.ptr, B, 3, HW, 7.0, 2.0, dfac3.ptr, 1, 0.5, 0.25)
    K.sync()
    assert out3.download((B, 3, HW), F32).tobytes() == apply32(np.ascontiguousarray(eps3.transpose(0, 2, 1)), x3, B, 7.0, 2.0, fac3, 1, F32(0.5), F32(0.25)).tobytes()
    # refused before any launch: the output keeps its poison
    nb = K.guidance_scratch_bytes(B, HW)
    scratch = _lib.from_numpy(np.zeros(nb // 8, np.float64))
    f = lib.mlsd_dxdt_rescaled
    for kw in (dict(eps=None), dict(dx=None), dict(fac=None), dict(B=0), dict(Cn=0), dict(HW=0), dict(ld=3), dict(pag=-1.0), dict(pag=float("nan")), dict(x=None, vparam=1),
               dict(B=1 << 20, HW=1 << 10)):
        a = dict(eps=de.ptr + 4, ld=ld, x=dxe.ptr, dx=out.ptr, B=B, Cn=4, HW=HW, cfg=7.0, pag=1.0, fac=dfac.ptr, vparam=0)
        a.update(kw)
        assert f(a["eps"], a["ld"], a["x"], a["dx"], a["B"], a["Cn"], a["HW"], a["cfg"], a["pag"], a["fac"], a["vparam"], 1.0, 0.0, None) < 0, kw
    assert lib.mlsd_euler_rescaled_update(None, de.ptr + 4, ld, B, 4, HW, 7.0, 1.0, dfac.ptr, 0.1, None, 0.0, None) < 0
    assert lib.mlsd_euler_rescaled_update(dxe.ptr, de.ptr + 4, ld, B, 4, HW, 7.0, 1.0, None, 0.1, None, 0.0, None) < 0
    s = lib.mlsd_guidance_stats
    for kw in (dict(eps=None), dict(scratch=None), dict(fac=None), dict(B=0), dict(Cn=0), dict(HW=0), dict(ld=3), dict(pag=-1.0), dict(phi=-0.1), dict(phi=1.5),
               dict(phi=float("nan")), dict(nb=nb - 8), dict(B=1 << 20, HW=1 << 10)):
        a = dict(eps=de.ptr + 4, ld=ld, B=B, Cn=4, HW=HW, cfg=7.0, pag=1.0, phi=0.7, scratch=scratch.ptr, nb=nb, fac=dfac.ptr)
        a.update(kw)
        assert s(a["eps"], a["ld"], a["B"], a["Cn"], a["HW"], a["cfg"], a["pag"], a["phi"], a["scratch"], a["nb"], a["fac"], None) < 0, kw
    K.sync()
    assert dfac.download((B,), F32).tobytes() == fac.tobytes()


# ------------------------------------------------------------------ 3. one evaluation of an engine
SIGMA = 2.5
CFG = 5.0


def engine_inputs(model, w, h, B):
    from test_freeu_gpu import inputs
    return inputs(model, w, h, B)


def coefficients(sigma):
    """c_skip and c_out as dxdt_finish forms them (float arithmetic, the square root in double)"""
    s = F32(sigma)
    q = F32(s * s + F32(1))
    return F32(s / q), F32(1.0 / math.sqrt(float(q)))


def expected64(rows, x, B, cfg, pag, phi, vparam, sigma):
    """float64 dx of the rule from the engine's own raw rows, the factors, and the bound of the fp32 chain per element.
    Roundings (u = 2^-24): the guided prediction is 3 operations on the terms cfg|c|, |1 - cfg||u| (and 3 more on pag|c|, pag|p| and the sum), each below u times
    the sum T of the terms' magnitudes: 6 u T.  The factor is rounded once and the product once: 2 u |g f|.  The v map is 3 more operations on |r c_out| and
    |x c_skip|, and c_out / c_skip themselves are known to one rounding each: 4 u (|r c_out| + |x c_skip|)."""
    r = rows.astype(np.float64)
    c = r[:B]
    g, T = c.copy(), np.abs(c)
    if cfg > 1:
        g = c * cfg + r[B:2 * B] * (1 - cfg)
        T = cfg * np.abs(c) + abs(1 - cfg) * np.abs(r[B:2 * B])
    if pag != 0:
        g = g + pag * (c - r[-B:])
        T = T + pag * (np.abs(c) + np.abs(r[-B:]))
    f = factor64(*guided32(rows, B, cfg, pag), phi)                      # (the statistics see the float32 g the kernels form)
    fb = f.reshape(B, 1, 1, 1)
    rr = g * fb
    bound = 6 * U32 * T * fb + 2 * U32 * np.abs(rr)
    if not vparam:
        return rr, f, bound
    c_skip, c_out = (float(v) for v in coefficients(sigma))
    return rr * c_out + x.astype(np.float64) * c_skip, f, bound * c_out + 4 * U32 * (np.abs(rr * c_out) + np.abs(x * c_skip))


def plain_bound(rows, x, B, cfg, pag, vparam, sigma):
    """the fp32 chain of the PLAIN mix kernels (phi 0), which map every group through the v map first and mix afterwards: 4 u on each mapped group's terms (3
    operations, c_out / c_skip known to one rounding), carried through the mix's coefficients, and 6 u on the mix's own terms (3 operations, 3 more with PAG)"""
    r = np.abs(rows.astype(np.float64))
    c_skip, c_out = (float(v) for v in coefficients(sigma)) if vparam else (0.0, 1.0)
    m = r * c_out + np.abs(np.concatenate([x] * (len(r) // B)).astype(np.float64)) * c_skip      # the magnitude of every mapped group's terms
    T = cfg * m[:B] + abs(1 - cfg) * m[B:2 * B] if cfg > 1 else m[:B]
    if pag != 0:
        T = T + pag * (m[:B] + m[-B:])
    return (4 * U32 * bool(vparam) + 6 * U32) * T


ENGINES = [("tiny", {}, None, SIGMA), ("tinyv", {}, None, SIGMA), ("tinyxl", {}, (1, 1), SIGMA), ("tinyxl", {}, (1, 1), "max"), ("tiny", dict(pag=True), None, SIGMA),
           ("tiny", dict(unet_tile=64, unet_tile_overlap=32), None, SIGMA)]


@pytest.mark.parametrize("model,kw,pred,sigma", ENGINES, ids=["tiny", "tinyv", "tinyxl-v-zsnr", "tinyxl-v-zsnr-sigma-max", "tiny-pag", "tiny-tiled"])
def test_one_evaluation_of_an_engine(model, kw, pred, sigma):
    """c, u, p are the engine's own raw rows of the evaluation (mlis_amd_last_rows: what the mix read, so the cond row is exactly what cfg 1 would give and the
    phi = 0 answer is checked against them first); the phi = 0.7 answer is held to the float64 rule on them."""
    from mlimgsynth_amd import engine as E
    B = 2
    lat = 12 if "unet_tile" in kw else 8
    x, cond, _ = engine_inputs(model, lat, lat, B)
    g = E.Generator(model, 8 * lat, 8 * lat, B, cfg_scale=CFG, **kw)
    try:
        g.set_cond(*cond)
        pag = 0.0
        if kw.get("pag"):
            pag = 3.0
            g.set_pag(pag)
        info = g.guidance_info()
        assert (info["vparam"], info["zsnr"], info["cfg_rescale"], info["n_evals"], len(info["factors"])) == (int(model == "tinyv"), 0, 0.0, 0, 0)
        assert info["sigma_max"] == F32(14.614641)
        if pred:
            g.set_prediction(*pred)
            info = g.guidance_info()
            assert (info["vparam"], info["zsnr"]) == pred and abs(info["sigma_max"] - 4518.76) < 0.01 and info["sigma_min"] == F32(0.029167158)
        vparam = info["vparam"]
        if sigma == "max":
            sigma = float(info["sigma_max"])
            x = (x * F32(sigma / SIGMA)).astype(F32)                       # a latent as noisy as that sigma says
        plain = g.dxdt(x, sigma)
        rows = g.last_rows()
        assert rows.shape[0] == (3 if pag else 2) * B and np.isfinite(rows).all()
        want0 = expected64(rows, x, B, CFG, pag, 0.0, vparam, sigma)[0]
        assert (np.abs(plain - want0) <= plain_bound(rows, x, B, CFG, pag, vparam, sigma)).all()      # the rows are what the plain mix read
        assert g.guidance_info()["n_evals"] == 0                            # phi 0: the plain kernels
        g.set_cfg_rescale(float(PHI))
        got = g.dxdt(x, sigma)
        assert g.last_rows().tobytes() == rows.tobytes()                    # the same evaluation
        want, f64, bound = expected64(rows, x, B, CFG, pag, PHI, vparam, sigma)
        info = g.guidance_info()
        err = np.abs(got - want)
        print(f"{model} {kw} sigma {sigma:g}: factors {info['factors']} (float64 {f64}), max err / bound {float((err / bound).max()):.3f}, max |dx| {float(np.abs(want).max()):.3g}")
        assert np.isfinite(got).all() and (err <= bound).all()
        assert info["n_evals"] == 1 and info["cfg_rescale"] == PHI and (ulps(info["factors"], f64) <= 2).all()
        assert (np.abs(f64 - 1) > 1e-3).all() and not np.array_equal(got, plain)
        assert g.dxdt(x, sigma).tobytes() == got.tobytes() and g.guidance_info()["n_evals"] == 2      # the same bits on a second call
        g.set_cfg_rescale(0)
        assert g.dxdt(x, sigma).tobytes() == plain.tobytes() and g.guidance_info()["n_evals"] == 2    # off again: the plain kernels' bytes
        with pytest.raises(RuntimeError):
            g.set_cfg_rescale(1.5)
        if pred:
            g.set_prediction(-1, -1)
            info = g.guidance_info()
            assert (info["vparam"], info["zsnr"], info["sigma_max"]) == (0, 0, F32(14.614641))
    finally:
        g.destroy()


# ------------------------------------------------------------------ 4. generation through the C-ABI
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
STEPS, SEED = 6, 42


def context(lib, model, method="euler", **opts):
    m = F.Mlis(lib)
    m.set("model", "synth:" + model)
    m.set("image_dim", 64, 64)
    m.set("steps", STEPS), m.set("seed", SEED), m.set("cfg_scale", CFG), m.set("method", method)
    for k, v in opts.items():
        m.set(k, v)
    return m


def run_generate(lib, m):
    from mlimgsynth_amd import engine as E
    m.tokens(TOKS)
    m.tokens(NTOKS, negative=True)
    m.generate()
    eng = lib.mlis_amd_engine_get(m.ctx)
    label = lambda k: (m.tensor(F.TENSOR[k]).reshape(-1) if lib.mlis_tensor_get(m.ctx, F.TENSOR[k]).contents.d else None)
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]), info=lib.mlis_infotext_get(m.ctx, 0).decode(),
                builds=lib.mlis_amd_engine_builds(m.ctx), guidance=E.guidance_info(eng, 1), nfe=E._proto2().mlis_amd_last_nfe(eng),
                cond=m.tensor(F.TENSOR["COND"])[0, 0], ncond=m.tensor(F.TENSOR["NCOND"])[0, 0], label=label("LABEL"), nlabel=label("NLABEL"))


def numpy_loop(model, method, a, pred, phi):
    """the generation on the engine's own evaluations: the schedule and the Philox draws from the library's host functions, every evaluation one mlis_amd_dxdt of
    a plain engine on the same weights (phi 0) whose raw rows are rescaled here in float64"""
    from mlimgsynth_amd import engine as E
    vparam, zsnr = pred
    sig = E.schedule(model, STEPS, zsnr=bool(zsnr))
    n = len(sig) - 1
    g = E.Generator(model, 64, 64, 1, cfg_scale=CFG)
    try:
        g.set_cond(a["cond"], a["label"], a["ncond"], a["nlabel"])
        g.set_prediction(vparam, zsnr)

        def dxdt(x, s):
            d = g.dxdt(x.astype(F32), float(s))
            return expected64(g.last_rows(), x, 1, CFG, 0.0, phi, vparam, float(s))[0].astype(F32) if phi else d
        x = (E.randn(SEED, 0, 4 * 64)[0].reshape(1, 4, 8, 8) * sig[0]).astype(F32)
        if method == "euler":
            for i in range(n):
                x = (x + dxdt(x, sig[i]) * F32(sig[i + 1] - sig[i])).astype(F32)
            return x
        h_last, dprev = 0.0, np.zeros_like(x)                       # dpmpp2m (solvers.c:207-233)
        for i in range(n):
            t0, t1 = F32(sig[i]), F32(sig[i + 1])
            q = F32(t1 / t0)
            hh = -math.log(q) if q > 0 else math.inf
            c = F32(hh / (2 * h_last)) if (i > 0 and t1 > 0) else F32(0)
            d0 = x - t0 * dxdt(x, t0)
            d = (F32(1) + c) * d0 - c * dprev
            x = (q * x + (F32(1) - q) * d).astype(F32)
            dprev, h_last = d0, hh
        return x
    finally:
        g.destroy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


GENERATIONS = [("tinyv", {}, (1, 0)), ("tinyxl", dict(prediction="v", zsnr="on"), (1, 1)), ("tiny", {}, (0, 0))]


@pytest.mark.parametrize("method", ["euler", "dpmpp2m"])
@pytest.mark.parametrize("model,opts,pred", GENERATIONS, ids=["tinyv", "tinyxl-v-zsnr", "tiny-eps"])
def test_generation_against_a_loop_on_the_engines_evaluations(lib, model, opts, pred, method):
    """(tiny as an eps model is here for the fused Euler step of the engine, which v models do not take)"""
    m = context(lib, model, method, cfg_rescale=float(PHI), **opts)
    try:
        a = run_generate(lib, m)
    finally:
        m.close()
    gi = a["guidance"]
    assert a["builds"] == 1 and np.isfinite(a["image"]).all() and (gi["vparam"], gi["zsnr"]) == pred and gi["n_evals"] == STEPS and a["nfe"] == 2 * STEPS
    assert ", CFG rescale: 0.7" in a["info"] and ("Schedule: zsnr" in a["info"]) == bool(pred[1]) and ("Prediction: v-prediction" in a["info"]) == (model == "tinyxl")
    assert len(gi["factors"]) == 1 and 0.3 < gi["factors"][0] < 1.0
    want = numpy_loop(model, method, a, pred, PHI)
    plain = numpy_loop(model, method, a, pred, 0.0)
    e, apart = rel_l2(a["latent"], want), rel_l2(plain, want)
    print(f"{model} {method}: final latent vs the loop rel-L2 {e:.3e}; the loop without the rescale lies {apart:.3f} away; last factor {gi['factors']}")
    assert apart > 10 * TOL.LATENT and e < TOL.LATENT


@pytest.mark.parametrize("how", ["use_hipgraph", "unet_split"])
def test_hipgraph_and_streaming_are_bit_identical(lib, how):
    from mlimgsynth_amd import engine as E
    x, cond, _ = engine_inputs("tinyxl", 8, 8, 1)
    outs = []
    for kw in ({}, {how: 1}):
        g = E.Generator("tinyxl", 64, 64, 1, cfg_scale=CFG, n_step=3, **kw)
        try:
            g.set_cond(*cond)
            g.set_prediction(1, 1)
            g.set_cfg_rescale(float(PHI))
            a = g.dxdt(x, SIGMA)
            lat, _ = g.generate([9], want_images=False)
            outs.append((a, lat, g.dxdt(x, SIGMA), g.guidance_info()["factors"]))
            assert lib.mlis_amd_handoff_retries(g.h) == 0 and g.guidance_info()["n_evals"] == 5
        finally:
            g.destroy()
    for p, q in zip(*outs):
        assert np.isfinite(p).all() and p.tobytes() == q.tobytes()
    assert outs[0][0].tobytes() == outs[0][2].tobytes()


def test_hires_rescales_in_both_passes(lib):
    m = context(lib, "tinyv", "euler", cfg_rescale=float(PHI))
    try:
        m.set("hires_scale", 2), m.set("hires_steps", 4), m.set("hires_denoise", 0.5)
        a = run_generate(lib, m)
        second = a["guidance"]
        assert a["builds"] == 2 and a["latent"].shape[-1] == 16 and ", CFG rescale: 0.7" in a["info"]
        # the engine used last is the second pass's: its mixes were all rescaled (2 of 4 steps at denoise 0.5), and the first pass's engine, the other resident
        # slot, did its STEPS: a second generation at the first size reuses it and adds STEPS more
        assert second["n_evals"] == a["nfe"] // 2 == 2 and len(second["factors"]) == 1 and second["factors"][0] != 1.0
        m.set("hires_scale", 1), m.set("seed", SEED)
        b = run_generate(lib, m)
        assert b["builds"] == 2 and b["guidance"]["n_evals"] == 2 * STEPS and b["nfe"] == 2 * STEPS
    finally:
        m.close()


def test_off_is_off_and_the_options_build_nothing(lib):
    """fresh contexts start their Philox streams at offset 0, so results compare bit for bit"""
    for model in ("tiny", "tinyxl"):
        def one(**opts):
            m = context(lib, model, "euler_a", **opts)
            try:
                return run_generate(lib, m)
            finally:
                m.close()
        never, off = one(), one(cfg_rescale=0, prediction="auto", zsnr="auto")
        assert off["latent"].tobytes() == never["latent"].tobytes() and off["image"].tobytes() == never["image"].tobytes() and off["info"] == never["info"]
        assert off["builds"] == never["builds"] == 1 and off["guidance"]["n_evals"] == 0 and "rescale" not in off["info"] and "zsnr" not in off["info"]
    m = context(lib, "tinyv", "euler_a")      # (a v model: an eps model with random weights does not come down from sigma 4518)
    try:
        first = run_generate(lib, m)
        m.set("cfg_rescale", 0.7), m.set("seed", SEED)
        second = run_generate(lib, m)
        m.set("cfg_rescale", 0.3), m.set("zsnr", "on"), m.set("seed", SEED)
        third = run_generate(lib, m)
        m.set("cfg_rescale", 0), m.set("zsnr", "auto"), m.set("seed", SEED)
        fourth = run_generate(lib, m)
        assert [r["builds"] for r in (first, second, third, fourth)] == [1, 1, 1, 1]             # none of the options creates an engine
        assert second["guidance"]["n_evals"] == STEPS and third["guidance"]["n_evals"] == 2 * STEPS and third["guidance"]["zsnr"] == 1
        assert not np.array_equal(second["latent"], first["latent"]) and not np.array_equal(third["latent"], second["latent"])
        assert fourth["guidance"]["zsnr"] == 0 and fourth["guidance"]["n_evals"] == 2 * STEPS and fourth["info"] == first["info"]
    finally:
        m.close()


def test_the_wrong_prediction_type_is_visibly_wrong(lib):
    def one(model, **opts):
        m = context(lib, model, "euler", **opts)
        try:
            return run_generate(lib, m)
        finally:
            m.close()
    for model, wrong, want_v in (("tinyv", "eps", 0), ("tiny", "v", 1), ("tinyxl", "v", 1)):
        auto, other = one(model), one(model, prediction=wrong)
        assert auto["guidance"]["vparam"] == 1 - want_v and other["guidance"]["vparam"] == want_v
        d = rel_l2(other["latent"], auto["latent"])
        print(f"{model} with prediction {wrong}: rel-L2 {d:.3f} from auto")
        assert np.isfinite(other["latent"]).all() and d > 10 * TOL.LATENT
        assert ("Prediction: " + ("v-prediction" if want_v else "eps")) in other["info"] and "Prediction" not in auto["info"]
