"""Colour fix without a GPU: what the two calls refuse, the CLI's option, and the restatement of tests/colorfix_ref.py held to its own two-filter form and to skimage."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import colorfix_ref as R
import inpaint_ffi as IF
import mlis_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, WAVELET, ADAIN, HISTOGRAM = 0, 1, 2, 3
TP, PI = C.POINTER(F.Tensor), C.POINTER(C.c_int)
PROTOTYPES = [("mlis_amd_tensor_color_fix", F.ci, [F.vp, TP, TP, TP, F.ci, F.ci]), ("mlis_amd_color_fix", F.ci, [F.vp, F.ci, F.ci]),
              ("mlis_amd_color_fix_info", F.ci, [F.vp, PI, PI, PI])]


def pictures(w, h, B, nt, tw=None, th=None, c=2, seed=0):      # content uniform in 0..1, target = content x 0.8 + 0.1 plus noise (a fresh picture where the sizes differ)
    rng = np.random.default_rng(seed + 1000 * w + h)
    content = rng.random((B, c, h, w), dtype=np.float32)
    base = content[:nt] if (tw or w, th or h) == (w, h) else rng.random((nt, c, th or h, tw or w), dtype=np.float32)
    return content, (base * np.float32(0.8) + np.float32(0.1) + np.float32(0.02) * rng.standard_normal(base.shape).astype(np.float32)).astype(np.float32)


def bind(path):
    lib = IF.bind(path)
    for name, res, args in PROTOTYPES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def color_fix(lib, m, content, target, mode, levels=0):      # mlis_amd_tensor_color_fix on float32 arrays: (return code, result or None)
    content, target = np.ascontiguousarray(content, np.float32), np.ascontiguousarray(target, np.float32)
    out = F.Tensor()
    r = lib.mlis_amd_tensor_color_fix(m.ctx, C.byref(IF.as_tensor(content)), C.byref(IF.as_tensor(target)), C.byref(out), mode, levels)
    got = F.tensor_np(out) if r == 1 else None
    lib.mlis_tensor_free(C.byref(out))
    return r, got


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return bind(_lib.LIB_PATH)


def test_the_calls_refuse_bad_arguments_before_any_gpu_work(lib):
    m = F.Mlis(lib)
    try:
        x = np.zeros((2, 3, 5, 6), np.float32)
        bad = [(x, x, 4, 0), (x, x, -1, 0), (x, x, WAVELET, 6), (x, x, ADAIN, -1),                    # mode, levels
               (x, x[:, :2], ADAIN, 0), (np.zeros((3, 3, 5, 6), np.float32), x, HISTOGRAM, 0),          # channels, batch (2 images for 3)
               (x, np.zeros((1, 3, 5, 7), np.float32), WAVELET, 0), (x, np.zeros((2, 3, 4, 6), np.float32), WAVELET, 5)]      # wavelet size
        for content, target, mode, levels in bad:
            r, _ = color_fix(lib, m, content, target, mode, levels)
            assert r == -4 and "color fix" in m.err(), (mode, levels, target.shape)
        assert lib.mlis_amd_tensor_color_fix(m.ctx, None, None, None, ADAIN, 0) == -4
        r, got = color_fix(lib, m, x + 0.25, x[:1], OFF, 0)                                             # off: a copy, no GPU
        assert r == 1 and got.tobytes() == (x + np.float32(0.25)).tobytes()
        mode, levels, applied = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.mlis_amd_color_fix_info(m.ctx, mode, levels, applied) == 1 and (mode.value, levels.value, applied.value) == (0, 5, 0)
        for args, want in (((WAVELET, 3), (1, 3)), ((HISTOGRAM, 0), (3, 5)), ((OFF, 0), (0, 5))):
            assert lib.mlis_amd_color_fix(m.ctx, *args) == 1 and lib.mlis_amd_color_fix_info(m.ctx, mode, levels, None) == 1
            assert (mode.value, levels.value) == want
        for args in ((4, 0), (-1, 0), (WAVELET, 6), (ADAIN, -1)):
            assert lib.mlis_amd_color_fix(m.ctx, *args) == -4
        assert lib.mlis_amd_color_fix_info(m.ctx, mode, None, None) == 1 and mode.value == 0               # a refused value changes nothing
    finally:
        m.close()


def test_wrapper_and_cli(lib):
    from mlimgsynth_amd import mlimgsynth as M
    with M.MLImgSynth() as s:
        s.color_fix_set("wavelet", levels=4)
        assert s.color_fix_info() == dict(mode="wavelet", levels=4, applied=0)
        with pytest.raises(ValueError):
            s.color_fix_set("wavelet", levels=9)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--color-fix none|wavelet|adain|histogram[:LEVELS]" in out and "| colorfix |" in out
    for bad in ("lab", "wavelet:6", "wavelet:", "adain:x"):
        r = subprocess.run([exe, "colorfix", "--color-fix", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--color-fix" in r.stderr, bad
    r = subprocess.run([exe, "colorfix", "--color-fix", "wavelet:3"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "colorfix needs --input and --target" in r.stderr                      # the option parsed


def test_the_wavelet_rule_equals_its_two_filter_form():      # out = content + Low(target - content) rests on Low being linear: held here in float64
    for (w, h), levels in (((7, 5), 5), ((65, 63), 5), ((130, 70), 3), ((1, 1), 1)):
        content, target = pictures(w, h, 2, 1)
        assert np.abs(R.wavelet(content, target, levels) - R.wavelet_two_filters(content, target, levels)).max() <= 1e-12


def test_the_histogram_rule_equals_skimage():
    exposure = pytest.importorskip("skimage.exposure")
    content, target = pictures(40, 30, 1, 1, 25, 35, c=1)
    _, _, lut = R.hist_lut(content[0, 0], target[0, 0])
    want = exposure.match_histograms(R.quant(content[0, 0]).astype(np.uint8), R.quant(target[0, 0]).astype(np.uint8))
    assert np.abs(lut[R.quant(content[0, 0])] * 255.0 - want).max() <= 1e-9
