"""Region inpainting without a GPU: the region rule against its restatement in Python integers on an exhaustive small grid, the Gaussian taps against numpy's
double arithmetic, the two restatements of the grow against each other, the option table, the refusals that need no GPU, the exports, the wrapper and the CLI."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import inpaint_ffi as IF
import inpaint_ref as R
import mlis_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return IF.bind(_lib.LIB_PATH)


@pytest.fixture()
def m(lib):
    ctx = F.Mlis(lib)
    yield ctx
    ctx.close()


@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ the region rule
def lattice(n):
    return sorted({0, 1, n // 3, n // 2, n - 1, n} & set(range(n + 1)))


@pytest.mark.parametrize("tw,th", [(64, 64), (96, 64), (64, 96)])
def test_region_rule_on_an_exhaustive_small_grid(lib, tw, th):
    n = 0
    for W, H in itertools.product((1, 7, 64, 100), repeat=2):
        for (bx0, bx1), (by0, by1) in itertools.product(itertools.combinations(lattice(W), 2), itertools.combinations(lattice(H), 2)):
            for pad in (0, 3, 200):
                box = (bx0, by0, bx1, by1)
                got, want = IF.region(lib, W, H, box, pad, tw, th), R.region(W, H, box, pad, tw, th)
                assert got == want and got is not None, (W, H, box, pad, got, want)
                x0, y0, x1, y1 = got
                assert 0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H                           # inside the image
                px0, py0, px1, py1 = max(0, bx0 - pad), max(0, by0 - pad), min(W, bx1 + pad), min(H, by1 + pad)
                assert x0 <= px0 and y0 <= py0 and x1 >= px1 and y1 >= py1               # contains the padded box
                cw, ch, pw, ph = x1 - x0, y1 - y0, px1 - px0, py1 - py0
                # only the shorter side grew, and |cw th - ch tw| is minimal given the caps: among the extents from the padded box's up to the image's, no other
                # one that reaches the aspect (or, if none does, no other at all) is closer to it
                if pw * th < ph * tw:
                    assert ch == ph
                    reach = [c for c in range(pw, W + 1) if c * th >= ph * tw] or [W]
                    assert cw == min(reach, key=lambda c: abs(c * th - ph * tw))
                else:
                    assert cw == pw
                    reach = [c for c in range(ph, H + 1) if c * tw >= pw * th] or [H]
                    assert ch == min(reach, key=lambda c: abs(pw * th - c * tw))
                n += 1
    assert n == 6348                 # 16 image sizes x every corner pair of the lattice x 3 paddings


def test_region_rule_places_the_extra_pixels(lib):
    # 20 x 40 box in the middle, 1:1: 20 extra columns, 10 on each side; an odd extra gives the right side the larger share
    assert IF.region(lib, 200, 200, (90, 80, 110, 120), 0, 64, 64) == (80, 80, 120, 120)
    assert IF.region(lib, 200, 200, (90, 80, 111, 121), 0, 64, 64) == (80, 80, 121, 121)
    assert IF.region(lib, 200, 200, (90, 80, 110, 121), 0, 64, 64) == (80, 80, 121, 121)      # 21 extra: 10 left, 11 right
    # shifted back inside at an edge, capped at the image
    assert IF.region(lib, 200, 200, (0, 80, 10, 120), 0, 64, 64) == (0, 80, 40, 120)
    assert IF.region(lib, 200, 200, (195, 80, 200, 120), 0, 64, 64) == (160, 80, 200, 120)
    assert IF.region(lib, 30, 200, (10, 0, 20, 200), 0, 64, 64) == (0, 0, 30, 200)
    assert IF.region(lib, 100, 84, (40, 30, 70, 50), 8, 64, 64) == R.region(100, 84, (40, 30, 70, 50), 8, 64, 64) == (32, 17, 78, 63)


def test_region_rule_refuses(lib):
    for args in ((0, 10, (0, 0, 1, 1), 0, 64, 64), (10, 10, (3, 3, 3, 5), 0, 64, 64), (10, 10, (0, 0, 0, 0), 0, 64, 64), (10, 10, (0, 0, 11, 5), 0, 64, 64),
                 (10, 10, (-1, 0, 5, 5), 0, 64, 64), (10, 10, (0, 0, 5, 5), -1, 64, 64), (10, 10, (0, 0, 5, 5), 0, 0, 64), (10, 10, (5, 5, 2, 8), 0, 64, 64)):
        assert IF.region(lib, *args) is None and R.region(*args) is None, args
    assert lib.mlis_amd_inpaint_region(10, 10, None, 0, 8, 8, (C.c_int * 4)()) == -1


# ------------------------------------------------------------------ the Gaussian taps
@pytest.mark.parametrize("sigma,r", [(0.0, 0), (0.19, 0), (0.2, 1), (1.0, 3), (4.0, 10), (16.0, 40), (64.0, 160)])
def test_gauss_taps_against_numpy_double(lib, sigma, r):
    t = IF.taps(lib, sigma)
    assert t is not None and t.dtype == np.float32 and len(t) == 2 * r + 1 == 2 * R.gauss_radius(sigma) + 1
    if r == 0:
        assert t.tolist() == [1.0]
        return
    k = np.arange(-r, r + 1, dtype=np.float64)
    want = np.exp(-(k * k) / (2.0 * float(np.float32(sigma)) ** 2))
    want = (want / want.sum()).astype(np.float32)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(t.astype(np.float64) - want.astype(np.float64)) <= ulp).all()            # two libms' exp may differ in the last place before the rounding
    assert np.array_equal(want, R.gauss_taps(sigma))
    assert abs(t.astype(np.float64).sum() - 1.0) <= (2 * r + 1) * 2.0 ** -25
    assert np.array_equal(t, t[::-1]) and (t > 0).all() and t.argmax() == r


def test_gauss_taps_refuses(lib):
    assert IF.taps(lib, 4.0, k_max=20) is None and IF.taps(lib, 4.0, k_max=21) is not None
    assert IF.taps(lib, 64.0, k_max=320) is None
    for bad in (-0.5, 64.5, float("nan"), float("inf")):
        assert IF.taps(lib, bad) is None, bad
    assert lib.mlsd_gauss_taps(1.0, None, 321) == -1


# ------------------------------------------------------------------ the restatements
def test_grow_restatements_agree():
    rng = np.random.default_rng(5)
    for h, w in ((29, 37), (70, 131)):
        x = (rng.random((h, w)) < 0.02).astype(np.float32)
        for radius in (0, 1, 5, -5, 40, -40):
            for wrap in range(4):
                a, b = R.grow(x, radius, wrap), R.grow_scipy(x, radius, wrap)
                assert np.array_equal(a, b), (h, w, radius, wrap)
    x = np.zeros((29, 37), np.float32)
    x[0, 0] = 1
    assert R.grow(x, 2, 0).sum() == 9 and R.grow(x, 2, 3).sum() == 25 and R.grow(x, 40, 1).sum() == 29 * 37 and R.grow(x, 30, 0).sum() == 29 * 31


def test_blur_matrix_rows_sum_to_one():
    for wrap in (0, 1):
        for n, sigma in ((37, 1.0), (37, 16.0), (29, 64.0)):
            A = R.blur_matrix(n, R.gauss_taps(sigma), wrap)
            assert np.allclose(A.sum(axis=1), 1.0, atol=1e-6)
            if wrap:
                assert np.allclose(A.sum(axis=0), 1.0, atol=1e-6)       # circulant


def test_weight_bbox_and_composite_restatements():
    m = np.array([0.0, 1.0, 0.25, -3.0, 7.0, np.nan], np.float32)
    assert R.mask_weight(m, 0).tolist() == [1.0, 0.0, 0.75, 1.0, 0.0, 0.0] and R.mask_weight(m, 1).tolist() == [0.0, 1.0, 0.25, 0.0, 1.0, 0.0]
    p = np.zeros((5, 7), np.float32)
    assert R.bbox(p) == (0, 0, 0, 0)
    p[2, 3], p[4, 6] = 1e-30, -0.0
    assert R.bbox(p) == (3, 2, 4, 3)
    orig, patch = np.full((1, 3, 5, 7), 2, np.float32), np.full((2, 3, 2, 2), 4, np.float32)
    w = np.zeros((5, 7), np.float32)
    w[1, 1], w[2, 2] = 1, 0.5
    out = R.composite(orig, patch, w, 1, 1)
    assert out.shape == (2, 3, 5, 7) and out[1, 2, 1, 1] == 4 and out[0, 0, 2, 2] == 3 and out[0, 0, 1, 2] == 2 and out[0, 0, 0, 0] == 2


# ------------------------------------------------------------------ options
def test_option_table_round_trips(lib):
    for oid, name in IF.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid).decode() == name and lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(180) == b"???" and lib.mlis_option_str(187) == b"???"


def test_options_defaults_ranges_and_enum_strings(lib, m):
    f, i = C.c_float(-1), C.c_int(-1)

    def geti(oid):
        assert lib.mlis_option_get(m.ctx, oid, C.byref(i)) == 1
        return i.value

    def getf(oid):
        assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1
        return f.value
    assert (geti(IF.INPAINT_AREA), geti(IF.INPAINT_PADDING), getf(IF.MASK_BLUR), geti(IF.MASK_GROW), geti(IF.MASK_INVERT), geti(IF.INPAINT_COMPOSITE)) == (0, 32, 0, 0, 0, 0)
    for text, want in (("masked", 1), ("whole", 0), ("1", 1), ("0", 0), ("MASKED", 1)):
        m.set("inpaint_area", text)
        assert geti(IF.INPAINT_AREA) == want
    assert lib.mlis_option_set(m.ctx, IF.INPAINT_AREA, 1) == 1 and geti(IF.INPAINT_AREA) == 1
    for bad in ("2", "-1", "only_masked", ""):
        assert lib.mlis_option_set_str(m.ctx, b"inpaint_area", bad.encode()) == -4, bad
    assert lib.mlis_option_set(m.ctx, IF.INPAINT_AREA, 2) == -4 and geti(IF.INPAINT_AREA) == 1
    for name, oid, lo, hi in (("inpaint_padding", IF.INPAINT_PADDING, 0, 512), ("mask_grow", IF.MASK_GROW, -256, 256)):
        for v in (lo, hi, 7):
            m.set(name, v)
            assert geti(oid) == v
        for bad in (str(lo - 1), str(hi + 1), "x", "1.5"):
            assert lib.mlis_option_set_str(m.ctx, name.encode(), bad.encode()) == -4, (name, bad)
        assert lib.mlis_option_set(m.ctx, oid, hi + 1) == -4 and geti(oid) == 7
    for v in (0, 64, 2.5):
        m.set("mask_blur", v)
        assert getf(IF.MASK_BLUR) == v
    assert lib.mlis_option_set(m.ctx, IF.MASK_BLUR, C.c_double(1.25)) == 1 and getf(IF.MASK_BLUR) == 1.25
    for bad in ("-0.1", "64.5", "nan", "x"):
        assert lib.mlis_option_set_str(m.ctx, b"mask_blur", bad.encode()) == -4, bad
    assert lib.mlis_option_set(m.ctx, IF.MASK_BLUR, C.c_double(-1.0)) == -4 and getf(IF.MASK_BLUR) == 1.25
    for name, oid in (("mask_invert", IF.MASK_INVERT), ("inpaint_composite", IF.INPAINT_COMPOSITE)):
        for text, want in (("y", 1), ("n", 0), ("1", 1), ("0", 0)):
            m.set(name, text)
            assert geti(oid) == want
        assert lib.mlis_option_set(m.ctx, oid, 1) == 1 and geti(oid) == 1
        assert lib.mlis_option_set(m.ctx, oid, 2) == -4 and lib.mlis_option_set_str(m.ctx, name.encode(), b"maybe") == -4 and geti(oid) == 1


def set_image_and_mask(lib, m, w=16, h=16, mask=True):
    rgb = np.full((h, w, 3), 128, np.uint8)
    im = F.Image(rgb.ctypes.data_as(C.POINTER(C.c_uint8)), rgb.size, w, h, 3, 0)
    assert lib.mlis_option_set(m.ctx, F.OPT["IMAGE"], C.byref(im)) == 1, m.err()
    if mask:
        a = np.full((h, w, 1), 255, np.uint8)
        a[4:8, 4:8] = 0
        mk = F.Image(a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, w, h, 1, 0)
        assert lib.mlis_option_set(m.ctx, F.OPT["IMAGE_MASK"], C.byref(mk)) == 1, m.err()


def test_generate_refuses_before_any_model_or_gpu_is_needed(lib, m):
    """no model is set: each refusal comes before the set-up; without the inpainting options the same call fails at the set-up"""
    m.set("inpaint_area", "masked")
    assert lib.mlis_generate(m.ctx) == -4 and "needs an input image" in m.err() and "masked" in m.err()
    set_image_and_mask(lib, m, mask=False)
    assert lib.mlis_generate(m.ctx) == -4 and "needs an input image" in m.err()              # an image alone
    set_image_and_mask(lib, m)
    m.set("tiling", "x")
    assert lib.mlis_generate(m.ctx) == -4 and "tiling 'x'" in m.err() and "not periodic" in m.err()
    m.set("tiling", "none")
    m.set("no_decode", 1)
    assert lib.mlis_generate(m.ctx) == -4 and "no_decode" in m.err()
    m.set("inpaint_area", "whole"), m.set("inpaint_composite", 1)
    assert lib.mlis_generate(m.ctx) == -4 and "inpaint_composite cannot be combined with no_decode" in m.err()
    m.set("no_decode", 0)
    m.set("tensor_use_flags", 0)
    assert lib.mlis_generate(m.ctx) == -4 and "inpaint_composite needs an input image" in m.err()
    set_image_and_mask(lib, m)
    set_image_and_mask(lib, m, w=24, mask=False)                                           # the mask no longer fits the image
    assert lib.mlis_generate(m.ctx) == -8 and "does not match" in m.err()
    m.set("inpaint_composite", 0)
    r = lib.mlis_generate(m.ctx)
    assert r < 0 and "inpaint" not in m.err() and "match" not in m.err()                   # the defaults: this code does not run


def test_tensor_calls_refuse_bad_arguments_before_the_backend(lib, m):
    x = np.zeros((1, 1, 5, 6), np.float32)
    out = F.Tensor()

    def t(a):
        return C.byref(IF.as_tensor(a))
    assert lib.mlis_amd_tensor_mask_weight(m.ctx, t(x), C.byref(out), 2) == -4
    assert lib.mlis_amd_tensor_mask_grow(m.ctx, t(x), C.byref(out), 257, 0) == -4 and lib.mlis_amd_tensor_mask_grow(m.ctx, t(x), C.byref(out), 1, 4) == -4
    assert lib.mlis_amd_tensor_mask_grow(m.ctx, t(np.zeros((1, 3, 5, 6), np.float32)), C.byref(out), 1, 0) == -4 and "one plane" in m.err()
    assert lib.mlis_amd_tensor_gauss_blur(m.ctx, t(x), C.byref(out), 64.5, 0) == -4 and lib.mlis_amd_tensor_gauss_blur(m.ctx, t(x), C.byref(out), float("nan"), 0) == -4
    assert lib.mlis_amd_tensor_gauss_blur(m.ctx, t(x), C.byref(out), 1.0, -1) == -4 and lib.mlis_amd_tensor_gauss_blur(m.ctx, None, None, 1.0, 0) == -4
    assert lib.mlis_amd_tensor_mask_bbox(m.ctx, t(np.zeros((2, 1, 5, 6), np.float32)), (C.c_int * 4)()) == -4 and lib.mlis_amd_tensor_mask_bbox(m.ctx, t(x), None) == -4
    orig, patch = np.zeros((1, 3, 5, 6), np.float32), np.zeros((2, 3, 2, 2), np.float32)
    for o, pt, p, x0, y0 in ((orig, patch, x, 5, 0), (orig, patch, x, 0, 4), (orig, patch, x, -1, 0), (orig, patch[:, :2].copy(), x, 0, 0), (orig, patch, x[:, :, :4].copy(), 0, 0),
                             (np.zeros((3, 3, 5, 6), np.float32), patch, x, 0, 0)):
        assert lib.mlis_amd_tensor_composite(m.ctx, C.byref(out), t(o), t(pt), t(p), x0, y0) == -4 and "composite" in m.err()
    assert out.d is None or not out.d


def test_kernels_refuse_bad_arguments(dry):
    """before any launch: the dry runtime's buffers are host memory"""
    w, h = 40, 30
    a, b, ws = (np.zeros(3 * w * h + 1024, np.float32) for _ in range(3))
    pa, pb, pw = (C.c_void_p(v.ctypes.data) for v in (a, b, ws))
    assert dry.mlsd_mask_weight(pa, pb, 0, 0, None) == -1 and dry.mlsd_mask_weight(pa, pb, 10, 2, None) == -1 and dry.mlsd_mask_weight(None, pb, 10, 0, None) == -1
    assert dry.mlsd_mask_grow(pa, pb, w, h, 257, 0, pw, None) == -1 and dry.mlsd_mask_grow(pa, pb, w, h, -257, 0, pw, None) == -1
    assert dry.mlsd_mask_grow(pa, pb, w, h, 1, 4, pw, None) == -1 and dry.mlsd_mask_grow(pa, pb, 0, h, 1, 0, pw, None) == -1
    assert dry.mlsd_mask_grow(pa, pa, w, h, 1, 0, pw, None) == -1 and dry.mlsd_mask_grow(pa, pb, w, h, 1, 0, None, None) == -1
    assert dry.mlsd_gauss_blur(pa, pb, w, h, 3, 64.5, 0, pw, None) == -1 and dry.mlsd_gauss_blur(pa, pb, w, h, 3, -1.0, 0, pw, None) == -1
    assert dry.mlsd_gauss_blur(pa, pb, w, h, 0, 1.0, 0, pw, None) == -1 and dry.mlsd_gauss_blur(pa, pb, w, h, 3, 1.0, 4, pw, None) == -1
    assert dry.mlsd_gauss_blur(pa, pa, w, h, 3, 1.0, 0, pw, None) == -1 and dry.mlsd_gauss_blur(pa, pb, w, h, 3, 1.0, 0, None, None) == -1
    assert dry.mlsd_gauss_blur_ws_bytes(0, 5, 1) == 0 and dry.mlsd_gauss_blur_ws_bytes(w, h, 3) >= 4 * (321 + 3 * w * h)
    assert dry.mlsd_mask_bbox(pa, w, 0, pb, None) == -1 and dry.mlsd_mask_bbox(pa, w, h, None, None) == -1
    ok = dict(n_orig=1, W=w, H=h, planes=3, B=1, x0=0, y0=0, cw=8, ch=8)
    for kw in (dict(n_orig=2), dict(B=0), dict(planes=0), dict(x0=-1), dict(x0=33), dict(y0=23), dict(cw=0), dict(ch=31), dict(n_orig=3, B=2)):
        k = dict(ok, **kw)
        assert dry.mlsd_composite(pa, pb, k["n_orig"], pw, pw, k["W"], k["H"], k["planes"], k["B"], k["x0"], k["y0"], k["cw"], k["ch"], None) == -1, kw
    pc = C.c_void_p(ws.ctypes.data + 4 * 2048)
    assert dry.mlsd_composite(pa, pa, 1, pw, pc, w, h, 1, 2, 0, 0, 8, 8, None) == -1      # in place needs n_orig == B
    assert dry.mlsd_composite(pa, pb, 1, pa, pw, w, h, 1, 1, 0, 0, 8, 8, None) == -1      # dst is the patch
    # good arguments reach the launch, which the dry runtime refuses with its own code
    assert dry.mlsd_composite(pa, pb, 1, pw, pc, w, h, 1, 1, 0, 0, 8, 8, None) == -2 and dry.mlsd_composite(pa, pa, 1, pw, pc, w, h, 1, 1, 0, 0, 8, 8, None) == -2
    assert dry.mlsd_gauss_blur(pa, pb, w, h, 3, 1.0, 0, pw, None) == -2 and dry.mlsd_mask_grow(pa, pb, w, h, 1, 0, pw, None) == -2
    # the test hook: 0 .. 32768, a negative value only asks
    was = dry.mlsd_gauss_blur_lds_limit(-1)
    assert was == 32768 and dry.mlsd_gauss_blur_lds_limit(0) == 32768 and dry.mlsd_gauss_blur_lds_limit(1 << 20) == 0 and dry.mlsd_gauss_blur_lds_limit(-1) == 32768


# ------------------------------------------------------------------ symbols, wrapper, CLI
def test_symbols_wrapper_and_cli(lib):
    for name in IF.EXPORTS:
        assert hasattr(lib, name), name
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert (M.MLIS_OPT_AMD_INPAINT_AREA, M.MLIS_OPT_AMD_INPAINT_PADDING, M.MLIS_OPT_AMD_MASK_BLUR, M.MLIS_OPT_AMD_MASK_GROW, M.MLIS_OPT_AMD_MASK_INVERT,
            M.MLIS_OPT_AMD_INPAINT_COMPOSITE) == (181, 182, 183, 184, 185, 186)
    assert (M.MLIS_AMD_INPAINT_WHOLE, M.MLIS_AMD_INPAINT_MASKED) == (0, 1)
    for f in (M.MLImgSynth.inpaint_set, M.MLImgSynth.mask_process, M.MLImgSynth.composite, M.MLImgSynth.mask_bbox, M.MLImgSynth.inpaint_info, K.mask_weight, K.mask_grow,
              K.gauss_blur, K.mask_bbox, K.composite):
        assert callable(f)
    assert M.inpaint_region(100, 84, (40, 30, 70, 50), 8, 64, 64) == (32, 17, 78, 63) and M.inpaint_region(10, 10, (3, 3, 3, 5), 0, 8, 8) is None
    assert np.array_equal(np.array(K.gauss_taps(4.0), np.float32), IF.taps(lib, 4.0)) and K.gauss_taps(4.0, 5) is None
    assert K.gauss_blur_ws_bytes(300, 200, 3) == lib.mlsd_gauss_blur_ws_bytes(300, 200, 3) and K.gauss_blur_lds_limit() == 32768
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--inpaint-area whole|masked", "--inpaint-padding", "--mask-blur", "--mask-grow", "--mask-invert", "--inpaint-composite"):
        assert flag in out, flag
    r = subprocess.run([exe, "generate", "--inpaint-area", "masked", "--mask-blur", "65"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "mask-blur" in r.stderr
    r = subprocess.run([exe, "generate", "--inpaint-area", "masked", "--tiling", "xy"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "inpaint_area masked" in r.stderr


def test_python_wrapper_sets_the_options(lib):
    from mlimgsynth_amd import mlimgsynth as M
    s = M.MLImgSynth()
    s.inpaint_set(area="masked", padding=12, mask_blur=2.5, mask_grow=-3, invert=True, composite=True)
    i, f = C.c_int(), C.c_float()
    for oid, want in ((M.MLIS_OPT_AMD_INPAINT_AREA, 1), (M.MLIS_OPT_AMD_INPAINT_PADDING, 12), (M.MLIS_OPT_AMD_MASK_GROW, -3), (M.MLIS_OPT_AMD_MASK_INVERT, 1),
                      (M.MLIS_OPT_AMD_INPAINT_COMPOSITE, 1)):
        s.option_get(oid, i)
        assert i.value == want, oid
    s.option_get(M.MLIS_OPT_AMD_MASK_BLUR, f)
    assert f.value == 2.5
    s.inpaint_set(area="whole", invert=False)
    s.option_get(M.MLIS_OPT_AMD_INPAINT_AREA, i)
    assert i.value == 0
    s.option_get(M.MLIS_OPT_AMD_INPAINT_PADDING, i)
    assert i.value == 12                                  # None keeps a setting
    with pytest.raises(RuntimeError):
        s.inpaint_set(padding=513)
    with pytest.raises(RuntimeError):
        s.inpaint_set(area="outside")
    assert s.inpaint_info() is None
    s.close()
