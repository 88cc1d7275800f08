"""Guidance limiters on the GPU (include/mlsd_kernels.h states the rules): the radix select against np.partition bit for bit, the sums against float64, the limited
mix against a numpy float32 restatement and against float64, and an engine's evaluation against the kernels composed by hand."""
import numpy as np
import pytest

from guidance_limit_ref import F32, limited, mix32, plane_inputs, triples32

pytestmark = pytest.mark.gpu

U24, U53, POISON, CFG, MIMIC = 2.0 ** -24, 2.0 ** -53, F32(7e30), 12.0, 5.0
LIMIT_HW = 128 * 1024 // 4      # mlsd_guidance_select_lds_limit() / 4, asserted below: a plane of exactly this size still takes the LDS path


def nhwc(rows, ld):
    eps = np.full((rows.shape[0], rows.shape[2], ld), POISON, F32)
    eps[:, :, :rows.shape[1]] = rows.transpose(0, 2, 1)
    return eps


def stats(de, ld, B, Cn, HW, cfg, mode, a, b):      # the statistics launches on a device eps -> (device lim, host means, host triples / coefficients)
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    nb = K.guidance_limit_scratch_bytes(B, Cn, HW)
    scratch = _lib.from_numpy(np.full(nb // 8, np.nan, np.float64))
    means, lim = _lib.from_numpy(np.full((B, Cn, 2), POISON, F32)), _lib.from_numpy(np.full((B, Cn, 3), POISON, F32))
    if mode == 2:
        K.guidance_apg_coef(de.ptr, ld, B, Cn, HW, cfg, a, b, scratch.ptr, nb, lim.ptr)
    else:
        K.guidance_plane_means(de.ptr, ld, B, Cn, HW, cfg, a, scratch.ptr, nb, means.ptr)
        K.guidance_plane_select(de.ptr, ld, B, Cn, HW, cfg, a, b, means.ptr, lim.ptr)
    K.sync()
    return lim, means.download((B, Cn, 2), F32), lim.download((B, Cn, 3), F32) if mode == 1 else lim.download((B, 2), F32)


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 2, 63, 4096, LIMIT_HW, LIMIT_HW + 1])
def test_selection_is_exact(HW, B, ld):
    """planes (b, ch) take the input kinds of guidance_limit_ref.KINDS in turn; p = 0.75 makes pos integral where HW % 4 == 1, p = 0.5 where HW is odd"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    assert K.guidance_select_lds_limit() == 4 * LIMIT_HW
    rows = plane_inputs(B, HW)
    de = _lib.from_numpy(nhwc(rows, ld))
    for p in (0.5, 0.75, 0.995, 1.0):
        _, means, got = stats(de, ld, B, 4, HW, CFG, 1, MIMIC, p)
        assert got.tobytes() == triples32(rows, B, HW, CFG, MIMIC, p, means).tobytes() == stats(de, ld, B, 4, HW, CFG, 1, MIMIC, p)[2].tobytes(), p


@pytest.mark.parametrize("HW,ld", [(1, 4), (63, 4), (1030, 8), (66001, 4)])
def test_means_and_apg_coefficients_against_float64(HW, ld):
    """A mean adds HW floats in double: every addition errs below 2^-53 of the running sum, itself below HW max|g|, so the sum is off by at most HW^2 2^-53 max|g| and
    the mean by HW 2^-53 max|g|; the one rounding to float adds 2^-24 |mean|.  APG's three sums have n = 4 HW terms, each formed with at most two roundings in
    double: with e = (n + 2) 2^-53, S_dd and S_cc are known to e of themselves and S_dc to e (S_dd + S_cc) / 2 (|d c| <= (d^2 + c^2) / 2).  So alpha = S_dc / S_cc
    is off by at most e (k + |alpha|) with k = (S_dd + S_cc) / (2 S_cc), and s, a quotient by a square root, by 2 e s.  With w = (cfg - 1) s that gives B = -w to
    2 e |w| and A = 1 + w (1 - (1 - eta) alpha) to |w| e (k + |alpha|) + 2 e |w| (1 + |alpha|), plus 2 e (1 + |w| (1 + |alpha|)) for the remaining double operations;
    the rounding to float adds 2^-24 of the value."""
    from mlimgsynth_amd import _lib
    B = 3
    rng = np.random.default_rng(HW)
    rows = (rng.standard_normal((2 * B, 4, HW)) + 3.0 + rng.standard_normal((2 * B, 1, 1))).astype(F32)
    de = _lib.from_numpy(nhwc(rows, ld))
    _, means, _ = stats(de, ld, B, 4, HW, CFG, 1, MIMIC, 1.0)
    for k, s in enumerate((CFG, MIMIC)):
        g = mix32(rows[:B], rows[B:], s).astype(np.float64)
        err, bound = np.abs(means[..., k] - g.mean(-1)), HW * U53 * np.abs(g).max(-1) + U24 * np.abs(g.mean(-1))
        assert (err <= bound).all()
    c = rows[:B].astype(np.float64).reshape(B, -1)
    d = c - rows[B:].astype(np.float64).reshape(B, -1)
    sdd, sdc, scc = (d * d).sum(-1), (d * c).sum(-1), (c * c).sum(-1)
    alpha, k, e = sdc / scc, (sdd + scc) / (2 * scc), (4 * HW + 2) * U53
    for eta, norm in ((0.0, 0.0), (0.5, 0.5), (1.0, 1e4)):
        got = stats(de, ld, B, 4, HW, CFG, 2, eta, norm)[2]
        w = (CFG - 1) * (np.minimum(1.0, norm / np.sqrt(sdd)) if norm > 0 else 1.0)
        for v, ref in ((got[:, 0], 1 + w * (1 - (1 - eta) * alpha)), (got[:, 1], -w)):
            bound = U24 * np.abs(ref) + e * (np.abs(w) * (k + np.abs(alpha)) + 4 * (1 + np.abs(w) * (1 + np.abs(alpha))))
            assert (np.abs(v - ref) <= bound).all()


@pytest.mark.parametrize("vparam", [0, 1])
@pytest.mark.parametrize("pag", [0.0, 3.0])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Cn,ld,HW", [(4, 4, 63), (4, 8, 1028), (3, 3, 20)])
def test_limited_mix_per_element(Cn, ld, HW, mode, pag, vparam):
    """Bit for bit the numpy float32 restatement of the rule, given the library's triples or coefficients.  Against float64 of the rule on the same triples, relative
    to S = the plane's max|g| + |mean| (g the mix at cfg, mean 0 for APG): thresholding is 6 operations rounded once each -- the mix's two products and sum, fsub,
    fmul by r <= 1, fadd; the clamp is exact and only shrinks -- and APG's 3 are fewer: 6 u S.  PAG adds 3 roundings on pag (|c| + |p|) and the sum, the v map 3 more
    on |g c_out| + |x c_skip| with its input's error carried through c_out.  (The two products of the mix round relative to their own size, cfg |c| and
    |1 - cfg| |u|, which can exceed |g| where they cancel: S is the plane's scale, not each element's, and the worst ratio is printed; the float32 check is exact.)"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    B, c_out, c_skip = 2, F32(0.31), F32(0.29)
    rng = np.random.default_rng(HW + mode)
    rows = (rng.standard_normal((3 * B, Cn, HW)) * 2 + rng.standard_normal((3 * B, Cn, 1))).astype(F32)
    x = (rng.standard_normal((B, Cn, HW)) * 3).astype(F32)
    de, dxe = _lib.from_numpy(nhwc(rows, ld)), _lib.from_numpy(x)
    a, b = (MIMIC, 0.995) if mode == 1 else (0.25, 3.0)
    dlim, _, lim = stats(de, ld, B, Cn, HW, CFG, mode, a, b)
    out, plain = (_lib.from_numpy(np.full((B, Cn, HW), POISON, F32)) for _ in range(2))
    K.dxdt_limited(de.ptr, ld, dxe.ptr, out.ptr, B, Cn, HW, mode, CFG, pag, dlim.ptr, vparam, c_out, c_skip)
    K.sync()
    got = out.download((B, Cn, HW), F32)
    assert got.tobytes() == limited(rows, x, B, mode, CFG, pag, lim, vparam, c_out, c_skip, F32).tobytes()
    want = limited(rows, x, B, mode, CFG, pag, lim, vparam, c_out, c_skip, np.float64)
    S = np.abs(rows[:B].astype(np.float64) * CFG + rows[B:2 * B] * (1.0 - CFG)).max(-1, keepdims=True) + (np.abs(lim[..., :1]) if mode == 1 else 0)
    bound = U24 * (6 * S + (3 * pag * (np.abs(rows[:B]) + np.abs(rows[2 * B:])) + 3 * S if pag else 0))
    bound = bound * c_out + 3 * U24 * (np.abs(want) + 2 * np.abs(x * c_skip)) if vparam else bound
    ratio = float((np.abs(got - want) / bound).max())
    print(f"C {Cn} ld {ld} HW {HW} mode {mode} pag {pag} v {vparam}: worst err / bound {ratio:.3f}")
    assert ratio <= 1
    # cfg 1: nothing to limit, no statistics, the bytes of mlsd_dxdt_guided (lim is not read)
    K.dxdt_limited(de.ptr, ld, dxe.ptr, out.ptr, B, Cn, HW, mode, 1.0, pag, None, vparam, c_out, c_skip)
    K.dxdt_guided(de.ptr, ld, dxe.ptr, plain.ptr, B, Cn, HW, 1.0, pag, None, vparam, c_out, c_skip)
    K.sync()
    assert out.download((B, Cn, HW), F32).tobytes() == plain.download((B, Cn, HW), F32).tobytes()


@pytest.mark.parametrize("model,kw,lat", [("tinyxl", {}, 8), ("tinyxl", dict(use_hipgraph=1), 8), ("tiny", dict(unet_tile=64, unet_tile_overlap=32), 12)],
                         ids=["tinyxl", "tinyxl-hipgraph", "tiny-tiled"])
def test_engine_evaluation_equals_the_kernels_composed_by_hand(model, kw, lat):
    """mlis_amd_dxdt on the engine's own raw rows (mlis_amd_last_rows; of the tiled engine the blended canvas); the settings change between calls and between
    generations, under a captured graph too, and the answers are those of the kernels on the same rows every time.  (The engine has no rebuild counter of its own,
    and mlis_amd_engine_builds belongs to the public context, which has no hipgraph switch: the use_hipgraph case shows by the bytes that nothing stale is replayed.)"""
    from test_freeu_gpu import inputs
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    B, HW, sigma = 2, lat * lat, 2.5
    x, cond, _ = inputs(model, lat, lat, B)
    g = E.Generator(model, 8 * lat, 8 * lat, B, cfg_scale=CFG, n_step=3, **kw)
    try:
        g.set_cond(*cond)
        plain = g.dxdt(x, sigma)
        rows = g.last_rows().reshape(-1, 4, HW)
        de, out = _lib.from_numpy(nhwc(rows, 4)), _lib.from_numpy(np.full((B, 4, HW), POISON, F32))
        K.dxdt_guided(de.ptr, 4, None, out.ptr, B, 4, HW, CFG)
        K.sync()
        assert plain.tobytes() == out.download((B, 4, HW), F32).tobytes() and g.guidance_limit_info()["n_evals"] == 0      # off: the parent's mix
        for n, (mode, a, b) in enumerate(((1, MIMIC, 0.995), (2, 0.25, 3.0), (1, 2.0, 0.5))):
            g.set_guidance_limit(mode, a, b, a, b)
            got = g.dxdt(x, sigma)
            dlim, _, lim = stats(de, 4, B, 4, HW, CFG, mode, a, b)
            K.dxdt_limited(de.ptr, 4, None, out.ptr, B, 4, HW, mode, CFG, 0.0, dlim.ptr)
            K.sync()
            assert got.tobytes() == out.download((B, 4, HW), F32).tobytes() and not np.array_equal(got, plain) and g.last_rows().tobytes() == rows.tobytes(), mode
            assert g.guidance_limit_info()["n_evals"] > n and g.guidance_limit_info()["values"].tobytes() == lim.tobytes()
            assert np.isfinite(g.generate([9], want_images=False)[0]).all()      # a generation between two settings: nothing is rebuilt or captured again
        g.set_guidance_limit("off")
        assert g.dxdt(x, sigma).tobytes() == plain.tobytes()
    finally:
        g.destroy()

