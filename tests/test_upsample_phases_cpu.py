"""The phase form of an upsampling convolution, on the host: the weight-derivation rule and the tap / pixel index maps of the library
(hip/ups_phase.hip: the rule runs on the host in the dry runtime, the maps are restated there from the kernel's expressions) against a numpy
restatement written here from the identity alone.

A 3x3 convolution (pad 1) over a nearest-2x upsampled H x W source computes output pixel (2y + py, 2x + px) from upsampled rows 2y + py - 1 + kh,
i.e. source rows (2y + py - 1 + kh) // 2: three taps of an axis meet two source pixels.  So the four output parities are four 2x2 convolutions
over the SOURCE, window origin (y - 1 + py, x - 1 + px), weights = the sums of the 3x3 weights that meet the same pixel.  The last test checks the
identity itself in float64 (no rounding anywhere: the two forms agree to the last bit of a float64 sum of the same products, reordered).
"""
import ctypes
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def K():
    from mlimgsynth_amd import _lib, kernels
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    L.mlsd_conv_tap_source.restype = ctypes.c_long
    L.mlsd_conv_out_pixel.restype = ctypes.c_long
    yield kernels, L
    L.mlsd_runtime_dry(0)


def tap_sets(par):
    """source offset a (0, 1) of the 2-wide window of parity par -> the 3x3 taps of that axis that land on it (from (par - 1 + k) // 2)"""
    s = {0: [], 1: []}
    for k in range(3):
        s[(par - 1 + k) // 2 - (par - 1) // 2].append(k)
    return s


def test_tap_sets_are_the_ones_the_issue_states():
    assert tap_sets(0) == {0: [0], 1: [1, 2]} and tap_sets(1) == {0: [0, 1], 1: [2]}


def derive_np(w):
    """w fp16 [cout][3][3][cin] -> fp16 [4][cout][2][2][cin]: fp32 sums in ascending (kh, kw) order, one rounding to fp16"""
    cout, _, _, cin = w.shape
    out = np.empty((4, cout, 2, 2, cin), np.float16)
    for py, px, a, b in itertools.product(range(2), repeat=4):
        s = None
        for kh in tap_sets(py)[a]:
            for kw in tap_sets(px)[b]:
                t = w[:, kh, kw, :].astype(np.float32)
                s = t if s is None else (s + t).astype(np.float32)
        with np.errstate(over="ignore"):          # (a sum beyond the fp16 range rounds to infinity, as on the device)
            out[2 * py + px, :, a, b, :] = s.astype(np.float16)
    return out


@pytest.mark.parametrize("cout,cin,scale", [(5, 8, 0.02), (16, 24, 1.0), (3, 8, 10000.0)])
def test_derived_weights_match_the_numpy_rule_bit_for_bit(K, cout, cin, scale):
    _, L = K
    rng = np.random.default_rng(cout * 131 + cin)
    w = (rng.standard_normal((cout, 3, 3, cin)) * scale).astype(np.float16)
    w[0, 0, 0, 0], w[0, 1, 1, 1] = -0.0, 6.0e-8          # a lone negative zero keeps its sign; subnormals add exactly
    if scale > 1000:
        w[1] = 40000.0                                        # sums of 2 and 4 overflow fp16: +inf, as fp16_rne of the fp32 sum
    dst = np.full((4, cout, 2, 2, cin), np.nan, np.float16)
    assert L.mlsd_ups_phase_weights(w.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p), cout, cin, None) == 0
    want = derive_np(w)
    assert np.array_equal(dst.view(np.uint16), want.view(np.uint16))
    assert np.signbit(dst[0, 0, 0, 0, 0]) and dst[0, 0, 0, 0, 0] == 0            # phase (0, 0), tap (0, 0) is the lone w[.., 0, 0, ..]
    if scale > 1000:
        assert np.isinf(dst[3, 1, 0, 0, 0]) and not np.isinf(dst[3, 1, 1, 1, 0])       # (kh, kw) in {0,1} x {0,1}: 160000; the lone (2, 2): 40000


def phase_args(kernels, n, H, W, py, px, wrap):
    return kernels.GemmArgs(conv=1, n_img=n, H=H, W=W, Cin=64, OH=H, OW=W, KH=2, KW=2, stride=1, pad=1, M=n * H * W, N=64, K=256, wrap=wrap,
                            tap_oy=py, tap_ox=px, out_phase=1 + 2 * py + px)


@pytest.mark.parametrize("H,W", [(4, 16), (5, 16), (1, 16), (3, 32)])
@pytest.mark.parametrize("wrap", [0, 1, 2, 3])
def test_tap_and_pixel_maps_match_the_upsampled_form(K, H, W, wrap):
    """Every row, phase and tap: the source pixel the phase launch reads is the one the upsampled 3x3 form reads for each of the taps summed into that weight, zero
    or wrapped at every border alike (odd H and H = 1 included); and the four launches' output pixels tile the 2H x 2W image exactly once."""
    kernels, L = K
    n = 2
    seen = np.zeros(n * 2 * H * 2 * W, np.int32)
    for py, px in itertools.product(range(2), repeat=2):
        a = phase_args(kernels, n, H, W, py, px, wrap)
        for m in range(a.M):
            img, y, x = m // (H * W), (m // W) % H, m % W
            op = L.mlsd_conv_out_pixel(ctypes.byref(a), m)
            assert op == (img * 2 * H + 2 * y + py) * 2 * W + 2 * x + px
            seen[op] += 1
            for ta, tb in itertools.product(range(2), repeat=2):
                got = L.mlsd_conv_tap_source(ctypes.byref(a), m, ta, tb)
                for kh in tap_sets(py)[ta]:
                    for kw in tap_sets(px)[tb]:
                        uy, ux = 2 * y + py - 1 + kh, 2 * x + px - 1 + kw          # the tap of the 3x3 form, in the upsampled image
                        if wrap & 2:
                            uy %= 2 * H
                        if wrap & 1:
                            ux %= 2 * W
                        inside = 0 <= uy < 2 * H and 0 <= ux < 2 * W
                        want = (img * H + uy // 2) * W + ux // 2 if inside else -1
                        assert got == want, (H, W, wrap, py, px, m, ta, tb, kh, kw, got, want)
    assert (seen == 1).all()


def test_maps_without_the_new_fields_are_todays(K):
    kernels, L = K
    a = kernels.GemmArgs(conv=1, n_img=1, H=4, W=16, Cin=64, OH=4, OW=16, KH=3, KW=3, stride=1, pad=1, M=64, N=64, K=576)
    assert L.mlsd_conv_out_pixel(ctypes.byref(a), 37) == 37
    assert L.mlsd_conv_tap_source(ctypes.byref(a), 0, 0, 0) == -1 and L.mlsd_conv_tap_source(ctypes.byref(a), 17, 1, 1) == 17
    assert L.mlsd_conv_tap_source(ctypes.byref(a), 17, 0, 2) == 2


@pytest.mark.parametrize("H,wrap", [(4, 0), (5, 0), (4, 3), (5, 3), (1, 2)])
def test_the_two_forms_are_identical_in_exact_arithmetic(H, wrap):
    """float64 on small integers (every product and sum exact): upsample + 3x3 == the four assembled 2x2 phases with the UNROUNDED summed weights"""
    rng = np.random.default_rng(H * 7 + wrap)
    n, W, cin, cout = 2, 6, 3, 4
    x = rng.integers(-8, 9, (n, H, W, cin)).astype(np.float64)
    w = rng.integers(-8, 9, (cout, 3, 3, cin)).astype(np.float64)

    def at(img, iy, ix, hh, ww):
        if wrap & 2:
            iy %= hh
        if wrap & 1:
            ix %= ww
        return img[iy, ix] if 0 <= iy < hh and 0 <= ix < ww else np.zeros(cin)
    ref = np.zeros((n, 2 * H, 2 * W, cout))
    up = x.repeat(2, axis=1).repeat(2, axis=2)
    for b, oy, ox in itertools.product(range(n), range(2 * H), range(2 * W)):
        for kh, kw in itertools.product(range(3), repeat=2):
            ref[b, oy, ox] += w[:, kh, kw] @ at(up[b], oy - 1 + kh, ox - 1 + kw, 2 * H, 2 * W)
    got = np.zeros_like(ref)
    for py, px in itertools.product(range(2), repeat=2):
        for b, y, xx in itertools.product(range(n), range(H), range(W)):
            for ta, tb in itertools.product(range(2), repeat=2):
                wsum = sum(w[:, kh, kw] for kh in tap_sets(py)[ta] for kw in tap_sets(px)[tb])
                got[b, 2 * y + py, 2 * xx + px] += wsum @ at(x[b], y - 1 + py + ta, xx - 1 + px + tb, H, W)
    assert np.array_equal(got, ref)
