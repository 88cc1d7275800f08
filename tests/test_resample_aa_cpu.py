"""Antialiased resampling, the parts that need no GPU: the host tap tables (mlsd_resample_aa_taps) against the float64 restatement of their definition
(tests/resample_aa_ref.py), that restatement against independent references -- torch's interpolate(antialias=True) in float64 without and with wrap, PIL's
Image.resize on mode-"F" images, avg_pool2d --, and the downscale_filter option (id 161) with the CLI flags.

Bounds: a weight of the table and of the restatement are the same real number, rounded once to fp32 by the library: half an ulp, which is 2^-24 absolute for
anything below 2 in magnitude (weights are at most 1 but for the negative lobes of cubic and lanczos, which can lift a weight of a clipped window slightly above
it; the test asserts |w| <= 2 beside the bound).  A table's sum differs from 1 by at most one such rounding per tap.  The restatement and torch both compute in float64 with a handful of operations per
weight and at most a few hundred taps: 1e-12 max|x|.  PIL computes its weights in double but stores coefficients, intermediate and result of mode "F" in
fp32: 4e-7 max|x| (about 3 fp32 roundings of values up to max|x| per pass, two passes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mlis_ffi as F
import resample_aa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
E_OPT_VALUE = -4
AXIS_PAIRS = [(53, 20), (200, 24), (20, 53), (7, 2), (3, 1), (1, 7), (300, 7), (64, 64)]
SIZES = [((37, 53), (16, 20)), ((200, 9), (24, 9)), ((16, 20), (37, 53)), ((5, 7), (1, 2)), ((2, 3), (1, 1)), ((64, 64), (17, 64))]
SIZE_IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SIZES]


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return R.bind(_lib.LIB_PATH)


@pytest.fixture()
def m(lib):
    m = F.Mlis(lib)
    yield m
    m.close()


# ------------------------------------------------------------------ tap tables
@pytest.mark.parametrize("wrap", [0, 1])
@pytest.mark.parametrize("filter", range(4), ids=R.FILTERS)
def test_tap_tables_equal_the_restatement(filter, wrap):
    from mlimgsynth_amd import kernels as K
    for s_in, s_out in AXIS_PAIRS:
        start, count, w = K.resample_aa_taps(s_in, s_out, filter, wrap)
        r_start, r_count, r_w = R.taps(s_in, s_out, filter, wrap)
        what = (R.FILTERS[filter], wrap, s_in, s_out)
        assert np.array_equal(start, r_start) and np.array_equal(count, r_count), what
        assert w.shape == (s_out, count.max()) and count.min() >= 1 and count.max() <= K.resample_aa_max_taps(s_in, s_out, filter), what
        if wrap:
            assert count.max() == K.resample_aa_max_taps(s_in, s_out, filter), what
        else:
            assert start.min() >= 0 and (start + count).max() <= s_in, what
        worst = 0.0
        for d in range(s_out):
            worst = max(worst, np.abs(w[d, :count[d]].astype(np.float64) - r_w[d]).max())
            assert np.abs(r_w[d]).max() <= 2 and not w[d, count[d]:].any(), what
            assert abs(w[d, :count[d]].astype(np.float64).sum() - 1) <= count[d] * R.U32, what
        print(f"{what}: max |w - restatement| = {worst:.3e} (bound {R.U32:.3e})")
        assert worst <= R.U32, what


def test_tap_call_refuses_bad_arguments():
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    assert K.resample_aa_max_taps(0, 4, 0) == -1 and K.resample_aa_max_taps(4, 0, 0) == -1 and K.resample_aa_max_taps(4, 4, 4) == -1 and K.resample_aa_max_taps(4, 4, -1) == -1
    assert K.resample_aa_max_taps((1 << 22) + 1, 4, 0) == -1 and K.resample_aa_taps(4, 4, 7) is None
    assert K.resample_aa_max_taps(64, 64, 3) == 6 and K.resample_aa_max_taps(64, 64, 0) == 1 and K.resample_aa_max_taps(300, 7, 3) >= 257
    start, count, w = (C.c_int * 7)(), (C.c_int * 7)(), (C.c_float * (7 * 300))()
    assert L.mlsd_resample_aa_taps(300, 7, 3, 0, start, count, w, 8) == -1           # k_max below the widest window
    assert L.mlsd_resample_aa_taps(300, 7, 3, 2, start, count, w, 300) == -1         # wrap_axis is 0 or 1
    assert L.mlsd_resample_aa_taps(300, 7, 3, 0, None, count, w, 300) == -1
    assert L.mlsd_resample_aa_taps(300, 7, 3, 0, start, count, w, 300) == K.resample_aa_taps(300, 7, 3)[1].max()
    assert K.resample2d_aa_ws_bytes(0, 4, 4, 4, 1, 0) == 0 and K.resample2d_aa_ws_bytes(8, 8, 4, 4, 1, 5) == 0 and K.resample2d_aa_ws_bytes(8, 8, 4, 4, 3, 3) >= 3 * 8 * 4 * 4


# ------------------------------------------------------------------ the restatement against independent references
def data(size, seed):
    x = np.random.default_rng(seed).standard_normal((2,) + size)
    x[-1, 0, size[1] - 1] = 1e4            # a corner: it must come around the edge under wrap
    return x


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("filter", [1, 2], ids=["bilinear", "bicubic"])
def test_restatement_equals_torch_antialias(filter, size):
    (sh, sw), (dh, dw) = size
    x = data((sh, sw), 10 * filter + sh)
    got, want = R.resample64(x, dh, dw, filter), R.torch64(x, dh, dw, filter)
    err = np.abs(got - want).max() / np.abs(x).max()
    print(f"{R.FILTERS[filter]} {sh}x{sw}->{dh}x{dw}: max|err| / max|x| = {err:.3e}")
    assert got.shape == want.shape and err <= 1e-12


@pytest.mark.parametrize("wrap", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("filter", [1, 2], ids=["bilinear", "bicubic"])
def test_restatement_wrap_equals_torch_on_a_circular_tiling(filter, size, wrap):
    (sh, sw), (dh, dw) = size
    x = data((sh, sw), 100 * wrap + 10 * filter + sh)
    got, want = R.resample64(x, dh, dw, filter, wrap), R.torch64_wrapped(x, dh, dw, filter, wrap)
    err = np.abs(got - want).max() / np.abs(x).max()
    print(f"{R.FILTERS[filter]} {sh}x{sw}->{dh}x{dw} wrap {wrap}: max|err| / max|x| = {err:.3e}")
    assert got.shape == want.shape and err <= 1e-12
    if size == SIZES[0]:           # the wrap is not a no-op (at 2 -> 1 it is: both rules average the two)
        assert not np.array_equal(got, R.resample64(x, dh, dw, filter, 0))


def test_copies_needed_exceeds_three_at_the_smallest_sizes():
    """what the wrap reference relies on: (5, 7) -> (1, 2) and (2, 3) -> (1, 1) have windows that reach further than one copy"""
    assert R.copies_needed(2, 1, 2) > 3 and R.copies_needed(5, 1, 2) > 3 and R.copies_needed(53, 20, 2) == 3
    for s_in, s_out, f in ((2, 1, 2), (5, 1, 2), (3, 1, 1), (7, 2, 2), (53, 20, 2)):
        start, count, _ = R.taps(s_in, s_out, f, 1)
        n = R.copies_needed(s_in, s_out, f)
        assert start.min() >= -(n // 2) * s_in and (start + count).max() <= (n // 2 + 1) * s_in


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("filter", [0, 3], ids=["box", "lanczos"])
def test_restatement_equals_pil(filter, size):
    try:
        from PIL import Image
    except ImportError:
        pytest.skip("PIL cannot be imported")
    (sh, sw), (dh, dw) = size
    x = data((sh, sw), 7 * filter + sw).astype(np.float32)
    how = Image.Resampling.BOX if filter == 0 else Image.Resampling.LANCZOS
    for p in x:
        want = np.asarray(Image.fromarray(p, mode="F").resize((dw, dh), how), np.float64)
        got = R.resample64(p, dh, dw, filter)
        err = np.abs(got - want).max() / np.abs(p).max()
        print(f"{R.FILTERS[filter]} {sh}x{sw}->{dh}x{dw}: max|err| / max|x| against PIL = {err:.3e}")
        assert got.shape == want.shape and err <= 4e-7


def test_box_at_integer_factors_is_the_block_average():
    import torch
    import torch.nn.functional as TF
    x = data((24, 36), 3)
    for fy, fx in ((2, 2), (3, 4), (1, 6), (8, 1)):
        want = TF.avg_pool2d(torch.from_numpy(x[None]), (fy, fx)).numpy()[0]
        got = R.resample64(x, 24 // fy, 36 // fx, 0)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max(), (fy, fx)


# ------------------------------------------------------------------ the option
def test_option_name_id_values_and_default(lib, m):
    assert lib.mlis_option_str(R.DOWNSCALE_FILTER) == b"downscale_filter" and lib.mlis_option_str(162) == b"???"
    assert lib.mlis_option_fromz(b"downscale_filter") == R.DOWNSCALE_FILTER == lib.mlis_option_fromz(b"DOWNSCALE-FILTER")
    assert lib.mlis_option_str(152) == b"hires_use_model" and lib.mlis_option_str(35) == b"no_prompt_parse"      # nothing moved
    assert R.get_filter(lib, m) == 0
    for i, name in enumerate(R.DOWNSCALE_VALUES):
        for val in (name, name.upper(), str(i)):
            m.set("downscale_filter", val)
            assert R.get_filter(lib, m) == i
        m.set("downscale_filter", "none")
        assert lib.mlis_option_set(m.ctx, R.DOWNSCALE_FILTER, i) == 1 and R.get_filter(lib, m) == i


@pytest.mark.parametrize("bad", ["5", "-1", "", "area"])
def test_option_refuses(lib, m, bad):
    m.set("downscale_filter", "bicubic")
    assert lib.mlis_option_set_str(m.ctx, b"downscale_filter", bad.encode()) == E_OPT_VALUE
    assert "downscale_filter" in m.err() and R.get_filter(lib, m) == 3
    for v in (5, -1):
        assert lib.mlis_option_set(m.ctx, R.DOWNSCALE_FILTER, v) == E_OPT_VALUE
    assert lib.mlis_option_set_str(m.ctx, b"hires_upscaler", b"lanczos") == E_OPT_VALUE        # the latent upscaler keeps its three values


def test_public_call_checks_its_arguments(lib, m):
    x = np.zeros((1, 4, 8, 8), np.float32)
    t = F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(8, 8, 4, 1), 0)
    out = F.Tensor()
    for w, h, f in ((4, 4, 4), (4, 4, -1), (0, 4, 1), (4, -3, 1), (70000, 4, 1)):
        assert lib.mlis_amd_tensor_resample_aa(m.ctx, C.byref(t), C.byref(out), w, h, f) == E_OPT_VALUE, (w, h, f)
    assert lib.mlis_amd_tensor_resample_aa(m.ctx, C.byref(F.Tensor()), C.byref(out), 4, 4, 1) == E_OPT_VALUE


def test_python_mirrors():
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as W
    assert W.MLIS_OPT_AMD_DOWNSCALE_FILTER == 161 and W.MLIS_OPT_AMD_HIRES_USE_MODEL == 152
    assert (W.MLIS_AMD_AA_BOX, W.MLIS_AMD_AA_TRIANGLE, W.MLIS_AMD_AA_CUBIC, W.MLIS_AMD_AA_LANCZOS) == (0, 1, 2, 3) == (K.AA_BOX, K.AA_TRIANGLE, K.AA_CUBIC, K.AA_LANCZOS3)
    assert callable(W.MLImgSynth.tensor_resample_aa) and callable(K.resample2d_aa)
    with W.MLImgSynth() as s:
        v = C.c_int(-1)
        s.option_get(W.MLIS_OPT_AMD_DOWNSCALE_FILTER, v)
        assert v.value == 0
        s.option_set("downscale_filter", "lanczos")
        s.option_get(W.MLIS_OPT_AMD_DOWNSCALE_FILTER, v)
        assert v.value == 4
        with pytest.raises(ValueError):
            s.upscale(W.tensor_from_numpy(np.zeros((1, 3, 4, 4), np.float32)), outscale=0)
        with pytest.raises(ValueError):
            s.upscale(W.tensor_from_numpy(np.zeros((1, 3, 4, 4), np.float32)), outscale=4.5)


def cli(*args):
    return subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=60)


def test_cli_flags():
    h = cli("--help")
    assert h.returncode == 0 and "--downscale-filter" in h.stdout and "--outscale" in h.stdout
    for args in (("generate", "--downscale-filter", "nope"), ("upscale", "--outscale", "0"), ("upscale", "--outscale", "4.5"), ("upscale", "--outscale", "2x")):
        r = cli(*args)
        assert r.returncode != 0 and args[1] in r.stderr, (args, r.stderr)
    r = cli("--downscale-filter", "lanczos", "--outscale", "2", "--version")       # accepted: the parse goes on to --version
    assert r.returncode == 0 and "mlimgsynth-amd" in r.stdout, r.stderr
