"""Hires fix (two-pass generation with a GPU latent upscaler), the parts that need no GPU: the four options (ids 102..105) by id and by name,
their defaults and ranges, the exported symbols, the Python mirrors, the CLI flags, and the yardstick of the GPU tests -- a numpy float64
restatement of the three resampling modes with clamped and wrapped taps equals torch's F.interpolate in float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hires_ffi as H
import mlis_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
E_OPT_VALUE = -4


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return H.bind(_lib.LIB_PATH)


@pytest.fixture()
def m(lib):
    m = F.Mlis(lib)
    yield m
    m.close()


def test_option_table_round_trips(lib):
    for oid, name in H.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid) == name.encode()
        assert lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.upper().replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(101) == b"tiling" and lib.mlis_option_str(106) == b"???"
    assert lib.mlis_option_str(35) == b"no_prompt_parse" and lib.mlis_option_str(36) == b"???"     # MLIS_OPT__LAST stays 35


def test_defaults(lib, m):
    assert H.get(lib, m, H.HIRES_SCALE) == 0
    assert H.get(lib, m, H.HIRES_DENOISE) == np.float32(0.7)
    assert H.get(lib, m, H.HIRES_STEPS) == 0
    assert H.get(lib, m, H.HIRES_UPSCALER) == H.MODES.index("bilinear")


def test_set_by_name_and_by_id(lib, m):
    for val in (0.0, 1.0, 1.25, 2.0, 4.0):
        m.set("hires_scale", val)
        assert H.get(lib, m, H.HIRES_SCALE) == np.float32(val)
        assert lib.mlis_option_set(m.ctx, H.HIRES_SCALE, C.c_double(val)) == 1
        assert H.get(lib, m, H.HIRES_SCALE) == np.float32(val)
    for val in (0.05, 0.5, 1.0):
        m.set("hires-denoise", val)
        assert H.get(lib, m, H.HIRES_DENOISE) == np.float32(val)
        assert lib.mlis_option_set(m.ctx, H.HIRES_DENOISE, C.c_double(val)) == 1
    for val in (0, 1, 30, 1000):
        m.set("HIRES_STEPS", val)
        assert H.get(lib, m, H.HIRES_STEPS) == val
        assert lib.mlis_option_set(m.ctx, H.HIRES_STEPS, val) == 1
    for i, name in enumerate(H.MODES):
        for val in (name, name.upper(), str(i)):
            m.set("hires_upscaler", val)
            assert H.get(lib, m, H.HIRES_UPSCALER) == i
        assert lib.mlis_option_set(m.ctx, H.HIRES_UPSCALER, i) == 1 and H.get(lib, m, H.HIRES_UPSCALER) == i


@pytest.mark.parametrize("name,bad", [("hires_scale", "0.5"), ("hires_scale", "4.5"), ("hires_scale", "-1"), ("hires_scale", ""), ("hires_scale", "2x"),
                                      ("hires_denoise", "0"), ("hires_denoise", "1.5"), ("hires_denoise", "-0.1"), ("hires_denoise", ""),
                                      ("hires_steps", "-1"), ("hires_steps", "1001"), ("hires_steps", "2.5"),
                                      ("hires_upscaler", "lanczos"), ("hires_upscaler", "3"), ("hires_upscaler", "-1"), ("hires_upscaler", "")])
def test_range_errors_by_name(lib, m, name, bad):
    oid = lib.mlis_option_fromz(name.encode())
    m.set("hires_scale", 2), m.set("hires_denoise", 0.5), m.set("hires_steps", 7), m.set("hires_upscaler", "bicubic")
    before = H.get(lib, m, oid)
    assert lib.mlis_option_set_str(m.ctx, name.encode(), bad.encode()) == E_OPT_VALUE, (name, bad)
    assert name in m.err()
    assert H.get(lib, m, oid) == before                     # a refused value leaves the option alone


def test_range_errors_by_id(lib, m):
    for oid, bad in ((H.HIRES_SCALE, C.c_double(0.5)), (H.HIRES_SCALE, C.c_double(4.5)), (H.HIRES_DENOISE, C.c_double(0.0)),
                     (H.HIRES_DENOISE, C.c_double(1.5)), (H.HIRES_STEPS, -1), (H.HIRES_UPSCALER, 3), (H.HIRES_UPSCALER, -1)):
        assert lib.mlis_option_set(m.ctx, oid, bad) == E_OPT_VALUE, (oid, bad)


def test_symbols_are_exported(lib):
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    for name in ("mlsd_resample2d", "mlis_amd_tensor_resample", "mlis_amd_engine_builds"):
        assert hasattr(L, name), name
    m = F.Mlis(lib)
    try:
        assert lib.mlis_amd_engine_builds(m.ctx) == 0
    finally:
        m.close()


def test_resample_call_checks_its_arguments(lib, m):
    x = np.zeros((1, 4, 8, 8), np.float32)
    t = F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(8, 8, 4, 1), 0)
    out = F.Tensor()
    for w, h, mode in ((12, 12, 3), (12, 12, -1), (0, 12, 1), (12, -3, 1), (70000, 12, 1)):
        assert lib.mlis_amd_tensor_resample(m.ctx, C.byref(t), C.byref(out), w, h, mode) == E_OPT_VALUE, (w, h, mode)
    empty = F.Tensor()
    assert lib.mlis_amd_tensor_resample(m.ctx, C.byref(empty), C.byref(out), 12, 12, 1) == E_OPT_VALUE


def test_python_mirrors():
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as W
    assert (W.MLIS_OPT_AMD_HIRES_SCALE, W.MLIS_OPT_AMD_HIRES_DENOISE, W.MLIS_OPT_AMD_HIRES_STEPS, W.MLIS_OPT_AMD_HIRES_UPSCALER) == (102, 103, 104, 105)
    assert W.MLIS_OPT__LAST == 35 and W.MLIS_OPT_AMD_TILING == 101
    assert (W.MLIS_AMD_RESAMPLE_NEAREST, W.MLIS_AMD_RESAMPLE_BILINEAR, W.MLIS_AMD_RESAMPLE_BICUBIC) == (0, 1, 2)
    assert (K.RESAMPLE_NEAREST, K.RESAMPLE_BILINEAR, K.RESAMPLE_BICUBIC) == (0, 1, 2) and callable(K.resample2d)
    for name in ("hires_set", "tensor_resample", "engine_builds"):
        assert callable(getattr(W.MLImgSynth, name))
    with W.MLImgSynth() as s:
        s.hires_set(1.5, denoise=0.6, steps=12, upscaler="bicubic")
        v, f = C.c_int(), C.c_float()
        s.option_get(W.MLIS_OPT_AMD_HIRES_UPSCALER, v)
        s.option_get(W.MLIS_OPT_AMD_HIRES_SCALE, f)
        assert v.value == 2 and f.value == 1.5 and s.engine_builds() == 0
        with pytest.raises(RuntimeError, match="hires_scale"):
            s.hires_set(5)


def test_cli_lists_and_checks_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--hires-scale F", "--hires-denoise F", "--hires-steps N", "--hires-upscaler nearest|bilinear|bicubic"):
        assert flag in r.stdout, flag
    r = subprocess.run([CLI, "generate", "--hires-upscaler", "lanczos"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "hires_upscaler" in r.stderr
    r = subprocess.run([CLI, "generate", "--hires-scale", "4.5"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "hires_scale" in r.stderr


# ------------------------------------------------------------------ the yardstick of the GPU tests
SIZES = [((8, 8), (12, 12)), ((7, 9), (14, 27)), ((1, 5), (3, 5)), ((64, 64), (96, 96)), ((5, 6), (5, 6)), ((9, 12), (6, 5))]


@pytest.mark.parametrize("mode", range(3), ids=H.MODES)
def test_numpy_restatement_equals_torch(mode):
    rng = np.random.default_rng(11)
    for (sh, sw), (dh, dw) in SIZES:
        x = rng.standard_normal((3, sh, sw))
        x[2, sh // 2, sw // 3] = 1e4
        got, want = H.resample64(x, dh, dw, mode), H.torch64(x, dh, dw, mode)
        if mode == 0 or (sh, sw) == (dh, dw):
            assert np.array_equal(got, want), (sh, sw, dh, dw)
        else:
            err = np.abs(got - want).max(axis=(1, 2)) / np.abs(x).max(axis=(1, 2))
            assert (err <= 1e-12).all(), (sh, sw, dh, dw, err)


@pytest.mark.parametrize("mode", range(3), ids=H.MODES)
@pytest.mark.parametrize("s", [1.25, 1.5, 2])
def test_numpy_restatement_wraps_like_circular_padding(mode, s):
    """wrap = interpolate on the input padded circularly by p = 4 source pixels, cropped by p s (F.pad mode="circular"; np.pad's "wrap",
    which the GPU tests use because it also takes an extent smaller than the padding, is the same thing)"""
    import torch
    import torch.nn.functional as TF
    rng = np.random.default_rng(12)
    p = H.PAD
    for sh, sw in ((8, 8), (8, 12), (16, 4)):
        dh, dw = int(sh * s), int(sw * s)
        x = rng.standard_normal((2, 1, sh, sw))
        x[1, 0, 0, sw - 1] = 1e4
        kw = {} if mode == 0 else dict(align_corners=False)
        for wrap in (1, 2, 3):
            xp = torch.from_numpy(x)
            xp = TF.pad(xp, (0, 0, p, p), mode="circular" if wrap & 2 else "replicate")
            xp = TF.pad(xp, (p, p, 0, 0), mode="circular" if wrap & 1 else "replicate")
            py, px = int(p * s), int(p * s)
            assert py == p * s
            want = TF.interpolate(xp, size=(dh + 2 * py, dw + 2 * px), mode=H.TORCH_MODES[mode], **kw).numpy()[:, 0, py:py + dh, px:px + dw]
            assert np.array_equal(H.torch64(x[:, 0], dh, dw, mode, wrap), want)                 # (np.pad == F.pad)
            got = H.resample64(x[:, 0], dh, dw, mode, wrap)
            if mode == 0:
                assert np.array_equal(got, want), (sh, sw, s, wrap)
            else:
                err = np.abs(got - want).max(axis=(1, 2)) / np.abs(x[:, 0]).max(axis=(1, 2))
                assert (err <= 1e-12).all(), (sh, sw, s, wrap, err)
            assert not np.array_equal(got, H.resample64(x[:, 0], dh, dw, mode, 0)) or mode == 0
