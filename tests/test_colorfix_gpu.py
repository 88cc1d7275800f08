"""Colour fix on the GPU: the kernels of hip/colorfix.hip against tests/colorfix_ref.py in float64; the driver on synth:tiny against the public calls by hand, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import colorfix_ref as R
import inpaint_ffi as IF
import test_colorfix_cpu as TC
import test_inpaint_gpu as TI
from test_inpaint_gpu import m  # noqa: F401  (the context fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return TC.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ kernels
def run(mode, content, target, levels=5, in_place=False):      # one call on device copies: (out[, coef [B][c][2] | counts [B c + nt c][256], lut [B][c][256]])
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    (B, c, h, w), (nt, _, th, tw) = content.shape, target.shape
    dc, dt = _lib.from_numpy(content), _lib.from_numpy(target)
    dst = dc if in_place else _lib.from_numpy(np.full(content.shape, 9e9, np.float32))
    ws = _lib.DeviceBuffer(K.colorfix_ws_bytes(mode, w, h, tw, th, c, B, nt))
    extras = ()
    if mode == K.COLORFIX_WAVELET:
        K.colorfix_wavelet(dc.ptr, dt.ptr, dst.ptr, w, h, c, B, nt, levels, ws.ptr if in_place else None)
    elif mode == K.COLORFIX_ADAIN:
        coef = _lib.from_numpy(np.full((B * c, 2), 9e9, np.float32))
        K.colorfix_adain(dc.ptr, w, h, dt.ptr, tw, th, dst.ptr, c, B, nt, ws.ptr, coef.ptr)
        extras = (coef.download((B, c, 2), np.float32),)
    else:
        counts, lut = _lib.from_numpy(np.full(((B + nt) * c, 256), 77, np.uint32)), _lib.from_numpy(np.full((B * c, 256), 9e9, np.float32))
        K.colorfix_histogram(dc.ptr, w, h, dt.ptr, tw, th, dst.ptr, c, B, nt, ws.ptr, counts.ptr, lut.ptr)
        extras = (counts.download(((B + nt) * c, 256), np.uint32), lut.download((B, c, 256), np.float32))
    K.sync()
    return (dst.download(content.shape, np.float32),) + extras


@pytest.mark.parametrize("B,nt", [(1, 1), (2, 1), (2, 2)])
@pytest.mark.parametrize("levels", [1, 5])
@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (64, 64), (65, 63), (130, 70)])      # smaller than the halo, one tile, one pixel over an edge, several tiles
def test_wavelet_against_float64(lib, w, h, levels, B, nt):
    content, target = TC.pictures(w, h, B, nt)
    got, = run(TC.WAVELET, content, target, levels)
    want = R.wavelet(content, target, levels)
    bound = 64 * 2.0 ** -24 * (float(np.abs(content).max()) + float(np.abs(target).max()))      # 4 roundings a level, d and the last sum: 22 at 5 levels
    assert float(np.abs(got.astype(np.float64) - want).max()) <= bound


def test_wavelet_in_place_and_of_a_picture_with_itself(lib):
    content, target = TC.pictures(130, 70, 2, 1)
    assert run(TC.WAVELET, content, target, 5, in_place=True)[0].tobytes() == run(TC.WAVELET, content, target, 5)[0].tobytes()
    for w, h in ((7, 5), (130, 70)):
        x, _ = TC.pictures(w, h, 2, 2)
        assert run(TC.WAVELET, x, x.copy(), 5)[0].tobytes() == x.tobytes()                    # d is 0: content, bit for bit


@pytest.mark.parametrize("w,h,tw,th", [(1, 1, 4, 2), (3, 2, 5, 4), (257, 3, 31, 9), (300, 200, 150, 111)])
def test_adain_against_float64(lib, w, h, tw, th):
    for B, nt in ((2, 1), (2, 2)):
        content, target = TC.pictures(w, h, B, nt, tw, th, c=3)
        got, coef = run(TC.ADAIN, content, target)
        a, b = R.adain_coef(content, target)
        a, b = np.broadcast_to(a, (B, 3)), np.broadcast_to(b, (B, 3))
        assert (np.abs(coef[..., 0] - a) <= np.spacing(a.astype(np.float32))).all() and (np.abs(coef[..., 1] - b) <= np.spacing(np.abs(b).astype(np.float32))).all()
        if w * h < 2:
            assert got.tobytes() == content.tobytes() and (coef == np.float32([1, 0])).all()     # the identity rule
            continue
        ca = content.astype(np.float64) * a[:, :, None, None]
        err, bound = np.abs(got - (ca + b[:, :, None, None])), 4 * 2.0 ** -24 * (np.abs(ca) + np.abs(b)[:, :, None, None])
        assert (err <= bound).all()


@pytest.mark.parametrize("w,h,tw,th", [(1, 1, 4, 2), (17, 3, 5, 4), (300, 200, 150, 111)])
@pytest.mark.parametrize("kind", ["random", "constant content", "two-level target"])
def test_histogram_counts_lut_and_map(lib, w, h, tw, th, kind):
    for B, nt in ((2, 1), (2, 2)):
        content, target = TC.pictures(w, h, B, nt, tw, th, c=3)
        if kind == "constant content":
            content[:] = np.float32(0.4)                                                      # a single occupied bin
        if kind == "two-level target":
            target = np.where(target > 0.5, np.float32(0.75), np.float32(0.25)).astype(np.float32)
        got, counts, lut = run(TC.HISTOGRAM, content, target)
        for b in range(B):
            for k in range(3):
                kc, kt, want = R.hist_lut(content[b, k], target[b % nt, k])
                assert np.array_equal(counts[b * 3 + k], kc) and np.array_equal(counts[(B + b % nt) * 3 + k], kt)
                assert np.abs(lut[b, k] - want).max() <= 2.0 ** -22
                assert got[b, k].tobytes() == lut[b, k][R.quant(content[b, k])].tobytes()


# ------------------------------------------------------------------ the driver on synth:tiny
def driven(lib, img, mask=None, modes=(None,), **opts):
    """one context, one generation per mode in turn: [(generation, images corrected, engine builds so far)]; mode None: mlis_amd_color_fix is not called"""
    c, n, out = TI.context(lib, **opts), C.c_int(-1), []
    try:
        for mode in modes:
            assert mode is None or lib.mlis_amd_color_fix(c.ctx, mode, 0) == 1
            TI.set_inputs(lib, c, img, mask)
            g = TI.generate(lib, c)
            assert lib.mlis_amd_color_fix_info(c.ctx, None, None, n) == 1
            out.append((g, n.value, lib.mlis_amd_engine_builds(c.ctx)))
        return out
    finally:
        c.close()


def test_img2img_with_a_fix_equals_the_plain_generation_and_the_call(lib, m):
    img = TI.picture(64, 64, seed=35)
    (plain, n0, _), (off, n1, _), (g, n, _) = (driven(lib, img, modes=(k,))[0] for k in (None, TC.OFF, TC.WAVELET))
    r, want = TC.color_fix(lib, m, plain["image"], TI.as_library_tensor(img), TC.WAVELET, 0)
    assert r == 1 and (n0, n1, n) == (0, 0, 2)
    assert g["image"].tobytes() == want.tobytes() != plain["image"].tobytes() and g["latent"].tobytes() == plain["latent"].tobytes()
    assert ", Color fix: wavelet," in g["info"] and "Color fix" not in plain["info"]
    assert off["info"] == plain["info"] and off["image"].tobytes() == plain["image"].tobytes() and off["latent"].tobytes() == plain["latent"].tobytes()


def test_a_change_of_mode_builds_no_engine(lib):
    runs = driven(lib, TI.picture(64, 64, seed=35), modes=(TC.WAVELET, TC.HISTOGRAM, TC.OFF, TC.ADAIN))
    assert [n for _, n, _ in runs] == [2, 2, 0, 2] and [b for _, _, b in runs] == [runs[0][2]] * 4 and runs[0][2] >= 1
    assert ", Color fix: histogram," in runs[1][0]["info"] and "Color fix" not in runs[2][0]["info"]


def test_masked_inpainting_fixes_the_crop_before_the_composite(lib, m):
    hand = TI.masked_by_hand(lib, TI.picture(), TI.keep_mask())
    x0, y0, x1, y1 = hand["region"]
    back = TI.resample(lib, m, hand["pass_"]["image"], x1 - x0, y1 - y0)
    r, fixed = TC.color_fix(lib, m, back, np.ascontiguousarray(hand["orig"][:, :, y0:y1, x0:x1]), TC.WAVELET, 0)
    want = IF.composite(lib, m, hand["orig"], fixed, hand["p"], x0, y0)
    a, n, _ = driven(lib, TI.picture(), TI.keep_mask(), (TC.WAVELET,), inpaint_area="masked", inpaint_padding=8, mask_blur=2, mask_grow=2)[0]
    assert r == 1 and n == 2 and a["region"] == hand["region"]
    assert a["image"].tobytes() == want.tobytes() != hand["final"].tobytes()
