"""Antialiased resampling on the GPU: mlsd_resample2d_aa against float64 per element, the public call, and the three places the downscale_filter option
reaches -- the hires fix through the upscale model, the control image, upscale(outscale=...) -- each against its own composition by hand.

The kernel's reference is formed from the library's OWN fp32 tables (mlsd_resample_aa_taps; tests/test_resample_aa_cpu.py pins those to the float64
restatement, and that to torch and PIL): want = My @ x @ Mx.T in float64.  Per element the bound is

    (Kx + Ky + 2) 2^-24 (|My| @ |x| @ |Mx|.T),      Kx, Ky the axes' largest tap counts:

in a sum of K products added in sequence a term passes its product's rounding and at most K - 1 additions, K roundings of u = 2^-24 each, so the sum is off
by at most ((1 + u)^K - 1) sum |w x| <= (K + 1) u sum |w x| for the K this runs at (a few hundred); the column pass does the same to the rounded rows, and
the two compose to (Kx + 1) + (Ky + 1) to first order.  |M| is the taps' magnitudes folded into the plane (resample_aa_ref.table_matrix: where a wrapped
window passes a pixel twice the magnitudes add).  It is the bound of the fp32 sums in the stated order, not a measured number."""
import ctypes as C

import numpy as np
import pytest

import mlis_ffi as F
import resample_aa_ref as R

pytestmark = pytest.mark.gpu

CASES = [((37, 53), (16, 20), 3), ((200, 9), (24, 9), 2), ((9, 200), (9, 24), 2), ((16, 20), (37, 53), 1), ((5, 7), (1, 2), 1), ((2, 3), (1, 1), 1),
         ((1, 300), (1, 7), 1), ((257, 130), (64, 33), 5), ((512, 768), (200, 301), 3)]
CASE_IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}-p{p}" for a, b, p in CASES]


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return R.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ kernel
def planes_data(rng, planes, sh, sw):
    x = rng.standard_normal((planes, sh, sw)).astype(np.float32)
    x[-1, 0, sw - 1] = 1e4           # one outlier in a corner
    return x


def run_kernel(x, dh, dw, filter, wrap=0):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    planes, sh, sw = x.shape
    src, dst = _lib.from_numpy(x), _lib.DeviceBuffer(planes * dh * dw * 4)
    ws = _lib.DeviceBuffer(K.resample2d_aa_ws_bytes(sw, sh, dw, dh, planes, filter))
    K.resample2d_aa(src.ptr, sw, sh, dst.ptr, dw, dh, planes, filter, wrap, ws.ptr)
    K.sync()
    return dst.download((planes, dh, dw), np.float32)


_inputs = {}


def case_input(i):
    """one input per case, shared by its filters and wraps and left unchanged"""
    if i not in _inputs:
        (sh, sw), _, planes = CASES[i]
        _inputs[i] = planes_data(np.random.default_rng(50 + i), planes, sh, sw)
        _inputs[i].setflags(write=False)
    return _inputs[i]


@pytest.mark.parametrize("wrap", range(4))
@pytest.mark.parametrize("filter", range(4), ids=R.FILTERS)
@pytest.mark.parametrize("case", range(len(CASES)), ids=CASE_IDS)
def test_kernel_against_float64_of_its_own_tables(case, filter, wrap):
    from mlimgsynth_amd import kernels as K
    (sh, sw), (dh, dw), planes = CASES[case]
    x = case_input(case)
    sx, cx, wx = K.resample_aa_taps(sw, dw, filter, wrap & 1)
    sy, cy, wy = K.resample_aa_taps(sh, dh, filter, (wrap >> 1) & 1)
    (Mx, Ax), (My, Ay) = R.table_matrix(sw, sx, cx, wx), R.table_matrix(sh, sy, cy, wy)
    x64 = x.astype(np.float64)
    want = My @ x64 @ Mx.T
    bound = (cx.max() + cy.max() + 2) * R.U32 * (Ay @ np.abs(x64) @ Ax.T)
    got = run_kernel(x, dh, dw, filter, wrap)
    assert got.shape == want.shape and np.isfinite(got).all()
    ratio = np.abs(got.astype(np.float64) - want) / bound
    print(f"{R.FILTERS[filter]} {sh}x{sw}->{dh}x{dw} planes {planes} wrap {wrap}: taps {cx.max()} x {cy.max()}, worst |err| / bound = {ratio.max():.3f}")
    assert (ratio <= 1).all()


def test_direct_read_fallback_is_what_the_widest_case_runs():
    """(1, 300) -> (1, 7) with lanczos: 64 output columns' span and weights exceed the block's 32 KiB of LDS, the fewest rows a tile takes, 4, x span + taps x 64 floats"""
    from mlimgsynth_amd import kernels as K
    start, count, w = K.resample_aa_taps(300, 7, 3, 1)
    span = start[-1] + count[-1] - start[0]
    assert 4 * (4 * span + 64 * count.max()) > 32 * 1024 and count.max() >= 257


def test_equal_sizes_copy_the_bits():
    x = np.array([[[0.0, -0.0, np.inf], [-np.inf, np.nan, 1e-45]]], np.float32)
    for filter in range(4):
        for wrap in (0, 3):
            assert run_kernel(x, 2, 3, filter, wrap).tobytes() == x.tobytes()


def test_two_launches_on_alternating_operands_are_bit_identical():
    a, b = case_input(0), planes_data(np.random.default_rng(9), 3, 37, 53)
    first = [run_kernel(v, 16, 20, 3, 1) for v in (a, b)]
    again = [run_kernel(v, 16, 20, 3, 1) for v in (a, b)]
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[0].tobytes() != first[1].tobytes()


def test_kernel_refuses_bad_arguments():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    buf, out, ws = _lib.DeviceBuffer(4096), _lib.DeviceBuffer(4096), _lib.DeviceBuffer(1 << 16)
    canary = np.full(1024, -7.25, np.float32)
    out.upload(canary)
    v = C.c_void_p
    big = (1 << 22) + 1             # MLSD_RESAMPLE_MAX_EXTENT + 1
    bad = [(0, 4, 4, 4, 1, 1, 0), (4, 4, 0, 4, 1, 1, 0), (4, -4, 4, 4, 1, 1, 0), (4, 4, 4, 4, 0, 1, 0),           # non-positive extents
           (big, 1, 4, 1, 1, 1, 0), (1, big, 1, 4, 1, 1, 0), (4, 1, big, 1, 1, 1, 0), (1, 4, 1, big, 1, 1, 0),      # extents above the maximum
           (1 << 20, 1 << 11, 1, 1, 1, 1, 0), (1, 1, 1 << 20, 1 << 11, 1, 1, 0), (1, 1 << 20, 1 << 11, 1, 1, 1, 0),   # 2^31 elements in src, dst, the intermediate
           (8, 8, 4, 4, 1, 4, 0), (8, 8, 4, 4, 1, -1, 0), (8, 8, 4, 4, 1, 1, 4), (8, 8, 4, 4, 1, 1, -1)]            # filter, wrap
    for sw, sh, dw, dh, planes, filter, wrap in bad:
        assert L.mlsd_resample2d_aa(v(buf.ptr), sw, sh, v(out.ptr), dw, dh, planes, filter, wrap, v(ws.ptr), None) == -1, (sw, sh, dw, dh, planes, filter, wrap)
    assert L.mlsd_resample2d_aa(v(buf.ptr), 8, 8, v(out.ptr), 4, 4, 1, 1, 0, None, None) == -1                        # no workspace
    assert L.mlsd_resample2d_aa(None, 8, 8, v(out.ptr), 4, 4, 1, 1, 0, v(ws.ptr), None) == -1
    assert L.mlsd_resample2d_aa(v(buf.ptr), 8, 8, v(buf.ptr + 16), 4, 4, 1, 1, 0, v(ws.ptr), None) == -1              # src / dst
    assert L.mlsd_resample2d_aa(v(buf.ptr), 8, 8, v(out.ptr), 4, 4, 1, 1, 0, v(buf.ptr + 64), None) == -1             # src / ws
    assert L.mlsd_resample2d_aa(v(buf.ptr), 8, 8, v(out.ptr), 4, 4, 1, 1, 0, v(out.ptr + 32), None) == -1             # dst / ws
    assert out.download((1024,), np.float32).tobytes() == canary.tobytes()
    assert L.mlsd_resample2d_aa(v(buf.ptr), 8, 8, v(out.ptr), 4, 4, 1, 1, 0, v(ws.ptr), None) == 0                    # the same call with good arguments runs


# ------------------------------------------------------------------ public call
def as_tensor(x):
    b, c, h, w = x.shape
    return F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, b), 0)


@pytest.mark.parametrize("filter", range(4), ids=R.FILTERS)
def test_public_call_equals_the_kernel_and_follows_tiling(lib, filter):
    x = np.random.default_rng(3).standard_normal((2, 3, 20, 26)).astype(np.float32)
    m = F.Mlis(lib)
    try:
        for tiling, wrap in ((None, 0), ("xy", 3), ("x", 1), ("y", 2), ("none", 0)):
            if tiling:
                m.set("tiling", tiling)
            out = F.Tensor()
            assert lib.mlis_amd_tensor_resample_aa(m.ctx, C.byref(as_tensor(x)), C.byref(out), 11, 7, filter) == 1, m.err()
            assert [out.n[i] for i in range(4)] == [11, 7, 3, 2]
            got = F.tensor_np(out)
            lib.mlis_tensor_free(C.byref(out))
            assert got.tobytes() == run_kernel(x.reshape(6, 20, 26), 7, 11, filter, wrap).tobytes(), (tiling, filter)
        # in place, on one of the context's own tensors
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["IMAGE"])
        lib.mlis_tensor_resize(t, 26, 20, 3, 2)
        C.memmove(t.contents.d, x.ctypes.data, x.nbytes)
        assert lib.mlis_amd_tensor_resample_aa(m.ctx, t, t, 9, 13, filter) == 1, m.err()
        assert m.tensor(F.TENSOR["IMAGE"]).tobytes() == run_kernel(x.reshape(6, 20, 26), 13, 9, filter).tobytes()
        for bad in (4, -1):
            assert lib.mlis_amd_tensor_resample_aa(m.ctx, t, t, 5, 5, bad) == -4 and "filter" in m.err()
        assert m.tensor(F.TENSOR["IMAGE"]).shape == (2, 3, 13, 9)
    finally:
        m.close()
    from mlimgsynth_amd import mlimgsynth as W
    with W.MLImgSynth() as s:
        s.option_set("tiling", "xy")
        out = s.tensor_resample_aa(W.tensor_from_numpy(x), 11, 7, filter)
        assert out.n == (11, 7, 3, 2) and out.numpy().tobytes() == run_kernel(x.reshape(6, 20, 26), 7, 11, filter, 3).tobytes()


# ------------------------------------------------------------------ hires fix through the upscale model
def test_hires_with_the_model_and_a_filter_equals_its_manual_composition(lib):
    import test_upscale_gpu as TU
    ulib = TU.U.bind(_lib_path())

    def hires(filter):
        m = TU.context(ulib, 1)
        try:
            m.set("hires_scale", 2), m.set("hires_denoise", TU.DENOISE), m.set("hires_steps", TU.HIRES_STEPS), m.set("hires_use_model", 1)
            m.set("downscale_filter", filter)
            TU.prompt(m)
            m.generate()
            return TU.results(ulib, m)
        finally:
            m.close()

    def by_hand():
        m = TU.context(ulib, 1)
        try:
            TU.prompt(m)
            m.generate()
            t = ulib.mlis_tensor_get(m.ctx, F.TENSOR["IMAGE"])
            assert ulib.mlis_amd_tensor_upscale(m.ctx, t, t) == 1, m.err()
            assert tuple(t.contents.n) == (256, 256, 3, 1)
            assert lib.mlis_amd_tensor_resample_aa(m.ctx, t, t, 128, 128, 3) == 1, m.err()
            TU.prompt(m)
            m.set("tensor_use_flags", F.TUF["IMAGE"]), m.set("f_t_ini", TU.DENOISE), m.set("steps", TU.HIRES_STEPS)
            m.generate()
            return TU.results(ulib, m)
        finally:
            m.close()

    h, man, plain = hires("lanczos"), by_hand(), hires("none")
    assert h["latent"].shape == (1, 4, 16, 16) and h["image"].shape == (1, 3, 128, 128)
    assert h["latent"].tobytes() == man["latent"].tobytes() and h["image"].tobytes() == man["image"].tobytes()
    assert not np.array_equal(h["image"], plain["image"]) and not np.array_equal(h["latent"], plain["latent"])
    assert ", Downscale filter: lanczos" in h["info"] and "Downscale filter" not in plain["info"]
    assert h["info"].replace(", Downscale filter: lanczos", "") == plain["info"]


def _lib_path():
    from mlimgsynth_amd import _lib
    return _lib.LIB_PATH


# ------------------------------------------------------------------ control image
def control_hint_by_hand(arr, side, filter):
    """the u8 map [h][w][3] as the library converts it (u8 x float(1 / 255), CHW), through resample2d_aa, no wrap"""
    src = np.ascontiguousarray(arr.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))
    return run_kernel(src, side, side, filter)


def test_control_image_is_filtered_down_and_not_reused_across_a_filter_change(lib):
    import controlnet_ffi as CF
    import test_controlnet_gpu as TC
    clib = CF.bind(_lib_path())
    big, small = TC.control_map(192, seed=11), TC.control_map(32, seed=12)
    m = TC.context(clib)
    try:
        TC.set_control_image(m, big)
        m.set("downscale_filter", "box")
        r = TC.run(clib, m)
        assert r["hint"].shape == (3, 64, 64) and r["hint"].tobytes() == control_hint_by_hand(big, 64, 0).tobytes()
        assert ", Downscale filter: box" in r["info"]
        tag = clib.mlis_amd_control_tag(clib.mlis_amd_engine_get(m.ctx))
        again = TC.run(clib, m)                                  # nothing changed: the engine keeps the image it holds
        assert clib.mlis_amd_control_tag(clib.mlis_amd_engine_get(m.ctx)) == tag and again["hint"].tobytes() == r["hint"].tobytes() and again["builds"] == 1
        m.set("downscale_filter", "none")                        # today's bilinear hint again: the cached image is not reused
        plain = TC.run(clib, m)
        assert plain["hint"].tobytes() == TC.resampled(big, 64).tobytes() and plain["hint"].tobytes() != r["hint"].tobytes()
        assert clib.mlis_amd_control_tag(clib.mlis_amd_engine_get(m.ctx)) != tag and plain["builds"] == 1 and "Downscale filter" not in plain["info"]
        m.set("downscale_filter", "lanczos")
        assert TC.run(clib, m)["hint"].tobytes() == control_hint_by_hand(big, 64, 3).tobytes()
        # a map smaller than the pass: neither axis shrinks, the option changes nothing
        TC.set_control_image(m, small)
        with_filter = TC.run(clib, m)
        m.set("downscale_filter", "none")
        without = TC.run(clib, m)
        assert with_filter["hint"].tobytes() == without["hint"].tobytes() == TC.resampled(small, 64).tobytes()
    finally:
        m.close()


# ------------------------------------------------------------------ outscale
def test_outscale(lib):
    import test_upscale_gpu as TU
    from mlimgsynth_amd import mlimgsynth as W
    x = np.random.default_rng(4).random((1, 3, 10, 14)).astype(np.float32)
    with W.MLImgSynth() as s:
        s.option_set("upscale_model", TU.SPEC)
        t = W.tensor_from_numpy(x)
        x4 = s.upscale(t)
        assert x4.n == (56, 40, 3, 1)
        assert s.upscale(t, outscale=4).numpy().tobytes() == x4.numpy().tobytes()
        half = s.upscale(t, outscale=2)
        assert half.n == (28, 20, 3, 1) and half.numpy().tobytes() == s.tensor_resample_aa(x4, 28, 20, W.MLIS_AMD_AA_LANCZOS).numpy().tobytes()
        odd = s.upscale(t, outscale=2.5)                         # round(2.5 * 14) x round(2.5 * 10)
        assert odd.n == (35, 25, 3, 1)
        s.option_set("downscale_filter", "bicubic")              # the option's filter where it is set
        assert s.upscale(t, outscale=2).numpy().tobytes() == s.tensor_resample_aa(x4, 28, 20, W.MLIS_AMD_AA_CUBIC).numpy().tobytes()
        assert s.upscale(t, outscale=2).numpy().tobytes() != half.numpy().tobytes()
