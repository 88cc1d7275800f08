"""Canny without a GPU: the two restatements of the rules against each other on every input the GPU tests use, the threshold rule, the option table, the
exported symbols, the wrapper and the CLI, and what the kernel entry points refuse before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import canny_ffi as CN
import canny_ref as R
import mlis_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return CN.bind(_lib.LIB_PATH)


@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ the reference
def test_restatements_agree_on_every_gpu_input(lib):
    cases = R.cases(CN.tile(lib))
    n = 0
    for name, (u8, thr) in cases.items():
        for planes in (1, 3):
            for l2 in (0, 1):
                for wrap in range(4):
                    e, cls, m, lo, hi = R.expected(name, u8, thr, planes, l2, wrap)
                    other = R.canny_scipy(R.as_float(u8[:planes]), lo, hi, l2, wrap)
                    assert np.array_equal(e, other), (name, planes, l2, wrap, int((e != other).sum()))
                    n += 1
    assert n == 16 * len(cases)                # planes x l2 x wrap per case
    # the input of the overshoot test (values below 0 and above 1), at the wraps the GPU tests use it with
    x = R.overshoot_input()
    assert (x < 0).any() and (x > 1).any()
    for planes in (1, 3):
        for l2 in (0, 1):
            for wrap in range(4):
                lo, hi = R.thresholds(100, 200, l2)
                e = R.canny(x[:planes], lo, hi, l2, wrap)
                assert e.any() and np.array_equal(e, R.canny_scipy(x[:planes], lo, hi, l2, wrap)), (planes, l2, wrap)


def test_inputs_are_not_vacuous(lib):
    tile = CN.tile(lib)
    cases = R.cases(tile)
    sy = tile[3]
    for l2 in (0, 1):
        e, cls, m, lo, hi = R.expected("rand_300x200", *cases["rand_300x200"], 3, l2, 0)
        assert (cls == 1).mean() >= 0.05 and (cls == 2).mean() >= 0.05
        # the serpentine: every candidate is lit from the few strong pixels at one end, the edge passes the sweep tile's border row 20 times or more; without
        # the strong spot the same candidates stay dark
        e, cls, *_ = R.expected("serpentine_lit", *cases["serpentine_lit"], 3, l2, 0)
        assert 0 < (cls == 2).sum() < 10 and (cls == 1).sum() > 4000 and e.sum() == (cls > 0).sum()
        assert (e[sy - 1] & e[sy]).sum() >= 20 and e.shape[0] > sy and e.shape[1] > tile[2]
        e, cls, *_ = R.expected("serpentine_dark", *cases["serpentine_dark"], 3, l2, 0)
        assert e.sum() == 0 and (cls == 1).sum() > 4000
        # the seam cases: the part beyond the gap is lit only around the wrapped axis
        for name, bit in (("seam_x", 1), ("seam_y", 2)):
            far = (lambda a: a[:, :80]) if bit == 1 else (lambda a: a[:80, :])
            for wrap in range(4):
                e = R.expected(name, *cases[name], 3, l2, wrap)[0]
                assert (far(e).sum() > 50) == bool(wrap & bit), (name, wrap)
    # every branch of the suppression is taken by the ramps, with either sign of dx ^ dy in the diagonal one
    seen = set()
    for name, (u8, thr) in cases.items():
        if name.startswith("ramp_"):
            dx, dy, m = R.gradient(R.quantise(R.as_float(u8[:1])), 0, 0)
            x, y = np.abs(dx), np.abs(dy) << 15
            sel = m > 20
            seen |= {"h"} if (sel & (y < x * 13573)).any() else set()
            seen |= {"v"} if (sel & (y > x * 13573 + (x << 16))).any() else set()
            d = sel & ~(y < x * 13573) & ~(y > x * 13573 + (x << 16))
            seen |= {"d+"} if (d & ((dx ^ dy) >= 0)).any() else set()
            seen |= {"d-"} if (d & ((dx ^ dy) < 0)).any() else set()
    assert seen == {"h", "v", "d+", "d-"}
    # equal neighbouring magnitudes above the low threshold: the > / >= cases
    m = R.gradient(R.quantise(R.as_float(cases["stairs_x"][0][:1])), 0, 0)[2]
    assert ((m[:, 1:] == m[:, :-1]) & (m[:, 1:] > 50)).any()
    # different planes win at different pixels, and two planes tie
    for name in ("planes_differ", "planes_tie"):
        q = R.quantise(R.as_float(cases[name][0]))
        per = [R.gradient(q[p:p + 1], 0, 0)[2] for p in range(3)]
        if name == "planes_differ":
            assert len({int(k) for k in np.unique(np.argmax(per, 0)[np.max(per, 0) > 50])}) == 3
        else:
            assert ((per[0] == per[1]) & (per[0] > 50)).any()


def test_quantise_clamps_overshoot():
    x = np.array([-0.2, 1.3, 0.0, 1.0, 0.5, 127 / 255, 0.4999 / 255], np.float32)
    assert R.quantise(x).tolist() == [0, 255, 0, 255, 128, 127, 0]
    u8 = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.quantise(R.as_float(u8)), u8) and np.array_equal(R.quantise(u8.astype(np.float32) * np.float32(1 / 255.0)), u8)


# ------------------------------------------------------------------ thresholds
def test_thresholds(lib):
    lo, hi = C.c_int(), C.c_int()

    def t(low, high, l2):
        assert lib.mlsd_canny_thresholds(low, high, l2, C.byref(lo), C.byref(hi)) == 0
        assert (lo.value, hi.value) == R.thresholds(low, high, l2)
        return lo.value, hi.value
    assert t(100, 200, 0) == (100, 200)
    assert t(200, 100, 0) == (100, 200)                    # swapped
    assert t(100.9, 200.999, 0) == (100, 200)              # floor
    assert t(100.9, 200, 1) == (10000, 40000)              # L2: the squares of the floors
    assert t(40000, 10, 1) == (100, 32767 * 32767)         # limited to 32767, then squared
    assert t(0, 0, 0) == (0, 0) and t(0, 0.5, 1) == (0, 0) and t(32767, 32767, 1) == (32767 ** 2, 32767 ** 2)
    assert lib.mlsd_canny_thresholds(float("nan"), 1.0, 0, C.byref(lo), C.byref(hi)) == -1
    assert lib.mlsd_canny_thresholds(1.0, 2.0, 0, None, C.byref(hi)) == -1
    from mlimgsynth_amd import kernels as K
    assert K.canny_thresholds(200, 100.5, True) == (10000, 40000)


# ------------------------------------------------------------------ options, symbols, wrapper, CLI
def test_option_table_round_trips(lib):
    for oid, name in CN.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid).decode() == name and lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(170) == b"???" and lib.mlis_option_str(175) == b"???"


def test_options_defaults_ranges_and_refusals(lib):
    m = F.Mlis(lib)
    try:
        f, i = C.c_float(-1), C.c_int(-1)

        def geti(oid):
            assert lib.mlis_option_get(m.ctx, oid, C.byref(i)) == 1
            return i.value

        def getf(oid):
            assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1
            return f.value
        assert geti(CN.CONTROL_PREPROCESS) == 0 and getf(CN.CANNY_LOW) == 100 and getf(CN.CANNY_HIGH) == 200 and geti(CN.CANNY_L2) == 0
        for text, want in (("canny", 1), ("invert", 2), ("none", 0), ("2", 2), ("0", 0)):
            m.set("control_preprocess", text)
            assert geti(CN.CONTROL_PREPROCESS) == want
        assert lib.mlis_option_set(m.ctx, CN.CONTROL_PREPROCESS, 1) == 1 and geti(CN.CONTROL_PREPROCESS) == 1
        for bad in ("3", "-1", "sobel", "canny2", ""):
            assert lib.mlis_option_set_str(m.ctx, b"control_preprocess", bad.encode()) == -4, bad        # MLIS_E_OPT_VALUE
        assert lib.mlis_option_set(m.ctx, CN.CONTROL_PREPROCESS, 3) == -4 and lib.mlis_option_set(m.ctx, CN.CONTROL_PREPROCESS, -1) == -4
        assert geti(CN.CONTROL_PREPROCESS) == 1                                                          # a refused value changes nothing
        for text, want in (("y", 1), ("n", 0), ("1", 1), ("0", 0)):
            m.set("canny_l2", text)
            assert geti(CN.CANNY_L2) == want
        assert lib.mlis_option_set(m.ctx, CN.CANNY_L2, 1) == 1 and geti(CN.CANNY_L2) == 1
        assert lib.mlis_option_set(m.ctx, CN.CANNY_L2, 2) == -4 and lib.mlis_option_set_str(m.ctx, b"canny_l2", b"maybe") == -4 and geti(CN.CANNY_L2) == 1
        for oid, name in ((CN.CANNY_LOW, "canny_low"), (CN.CANNY_HIGH, "canny_high")):
            m.set(name, 0), m.set(name, 32767), m.set(name, 50.5)
            assert getf(oid) == 50.5
            assert lib.mlis_option_set(m.ctx, oid, C.c_double(77.25)) == 1 and getf(oid) == 77.25
            for bad in ("-0.1", "32768", "x", "1.5x", "nan"):
                assert lib.mlis_option_set_str(m.ctx, name.encode(), bad.encode()) == -4, (name, bad)
            assert lib.mlis_option_set(m.ctx, oid, C.c_double(-1.0)) == -4 and lib.mlis_option_set(m.ctx, oid, C.c_double(40000.0)) == -4
            assert getf(oid) == 77.25
    finally:
        m.close()


def test_symbols_wrapper_and_cli(lib):
    for name in CN.EXPORTS:
        assert hasattr(lib, name), name
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert (M.MLIS_OPT_AMD_CONTROL_PREPROCESS, M.MLIS_OPT_AMD_CANNY_LOW, M.MLIS_OPT_AMD_CANNY_HIGH, M.MLIS_OPT_AMD_CANNY_L2) == (171, 172, 173, 174)
    assert (M.MLIS_AMD_PREPROCESS_NONE, M.MLIS_AMD_PREPROCESS_CANNY, M.MLIS_AMD_PREPROCESS_INVERT) == (0, 1, 2)
    assert callable(M.MLImgSynth.canny) and callable(K.canny) and callable(K.invert) and callable(E.Generator.control_image)
    assert K.canny_ws_bytes(300, 200) == lib.mlsd_canny_ws_bytes(300, 200) and K.canny_tile(2) == lib.mlsd_canny_tile(2)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--control-preprocess none|canny|invert", "--canny-low", "--canny-high", "--canny-l2", "| canny |", "canny -i IN -o OUT"):
        assert flag in out, flag
    r = subprocess.run([exe, "generate", "--control-preprocess", "canny", "--canny-low", "40000"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "canny-low" in r.stderr
    r = subprocess.run([exe, "canny", "--canny-l2", "y"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "canny needs --input" in r.stderr


def test_python_wrapper_sets_the_options(lib):
    from mlimgsynth_amd import mlimgsynth as M
    m = M.MLImgSynth()
    m.control_set(preprocess="canny", canny_low=30, canny_l2=True)
    i, f = C.c_int(), C.c_float()
    m.option_get(M.MLIS_OPT_AMD_CONTROL_PREPROCESS, i)
    assert i.value == M.MLIS_AMD_PREPROCESS_CANNY
    m.option_get(M.MLIS_OPT_AMD_CANNY_L2, i)
    assert i.value == 1
    for oid, want in ((M.MLIS_OPT_AMD_CANNY_LOW, 30), (M.MLIS_OPT_AMD_CANNY_HIGH, 200)):
        m.option_get(oid, f)
        assert f.value == want
    m.control_set(preprocess="none", canny_high=150.5, canny_l2=False)
    m.option_get(M.MLIS_OPT_AMD_CONTROL_PREPROCESS, i)
    assert i.value == 0
    m.option_get(M.MLIS_OPT_AMD_CANNY_HIGH, f)
    assert f.value == 150.5
    with pytest.raises(RuntimeError):
        m.control_set(canny_low=-3)
    with pytest.raises(RuntimeError):
        m.control_set(preprocess="sobel")
    with pytest.raises(ValueError):
        m.canny(np.zeros((4, 4), np.float32))
    m.close()


def test_tensor_canny_refuses_bad_arguments_before_the_backend(lib):
    m = F.Mlis(lib)
    try:
        x = np.zeros((1, 3, 5, 6), np.float32)

        def call(a, low=100.0, high=200.0, l2=0, wrap=0):
            b, c, h, w = a.shape
            t, out = F.Tensor(a.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, b), 0), F.Tensor()
            return lib.mlis_amd_tensor_canny(m.ctx, C.byref(t), C.byref(out), low, high, l2, wrap)
        for kw in (dict(low=-1.0), dict(high=40000.0), dict(low=float("nan")), dict(l2=2), dict(wrap=4), dict(wrap=-1)):
            assert call(x, **kw) == -4 and "canny" in m.err(), kw
        assert call(np.zeros((1, 2, 5, 6), np.float32)) == -4 and call(np.zeros((2, 3, 5, 6), np.float32)) == -4 and call(np.zeros((1, 4, 5, 6), np.float32)) == -4
        assert lib.mlis_amd_tensor_canny(m.ctx, None, None, 100.0, 200.0, 0, 0) == -4
    finally:
        m.close()


# ------------------------------------------------------------------ what the kernels refuse (before any launch: the dry runtime's buffers are host memory)
def test_kernels_refuse_bad_arguments(dry):
    w, h = 40, 30
    ws_bytes = dry.mlsd_canny_ws_bytes(w, h)
    assert ws_bytes >= 2 * w * h
    buf = np.zeros(2 * 3 * w * h + ws_bytes // 4 + 256, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data % 256)
    s, d = base, base + 3 * w * h * 4
    ws = d + 3 * w * h * 4 + (-(3 * w * h * 4) % 256)
    n = C.c_int(-5)
    cn = lambda src=s, w_=w, h_=h, planes=3, l2=0, wrap=0, dst=d, po=3, ws_=ws: dry.mlsd_canny(src, w_, h_, planes, 100, 200, l2, wrap, dst, po, ws_, C.byref(n), None)
    OK = -2                                                # arguments accepted: the dry runtime then declines the launch (-2); a refused argument is -1
    assert cn() == OK and cn(planes=1, po=1) == OK and cn(planes=1) == OK and cn(po=1, wrap=3, l2=1) == OK
    assert cn(w_=1, h_=1) == OK and cn(w_=1, h_=7) == OK and cn(w_=7, h_=1) == OK
    for kw in (dict(planes=0), dict(planes=2), dict(planes=4), dict(planes=-1), dict(po=0), dict(po=2), dict(po=4), dict(w_=0), dict(h_=0), dict(w_=-3), dict(h_=-1),
               dict(w_=(1 << 20) + 1, h_=1), dict(w_=1, h_=(1 << 20) + 1), dict(w_=1 << 20, h_=1 << 10), dict(wrap=4), dict(wrap=-1), dict(l2=2), dict(src=None),
               dict(dst=None), dict(ws_=None), dict(dst=s + 16), dict(ws_=s + 64), dict(ws_=d + 256)):
        assert cn(**kw) == -1, kw
        assert n.value == 0
    from mlimgsynth_amd import _lib
    assert "mlsd_canny" in _lib.last_error()
    # the workspace grows with w h; a refused size has none
    sizes = [dry.mlsd_canny_ws_bytes(a, b) for a, b in ((1, 1), (64, 64), (300, 200), (1024, 1024), (4096, 4096))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 2 * 4096 * 4096
    assert dry.mlsd_canny_ws_bytes(0, 5) == 0 and dry.mlsd_canny_ws_bytes(5, -1) == 0 and dry.mlsd_canny_ws_bytes((1 << 20) + 1, 1) == 0
    assert dry.mlsd_canny_ws_bytes(1 << 20, 1 << 10) == 0
    assert CN.tile(dry) == tuple(dry.mlsd_canny_tile(i) for i in range(4)) and all(t >= 16 for t in CN.tile(dry)) and dry.mlsd_canny_tile(4) >= 1
    assert dry.mlsd_canny_tile(5) == -1 and dry.mlsd_canny_tile(-1) == -1
    assert dry.mlsd_invert(s, d, 100, None) == OK and dry.mlsd_invert(s, s, 100, None) == OK
    assert dry.mlsd_invert(None, d, 100, None) == -1 and dry.mlsd_invert(s, None, 100, None) == -1 and dry.mlsd_invert(s, d, 0, None) == -1


def test_no_plan_op_kind_was_added(dry):
    """the preprocessor runs in control_apply and in a public tensor call, outside every plan: the list of kinds tests/test_op_kinds_cpu.py pins has no new entry"""
    from mlimgsynth_amd import engine
    names = [name for name, _ in engine.op_kinds()]
    assert len(names) == 16 and not any("canny" in n or "invert" in n for n in names)
