"""Canny on the GPU: mlsd_canny against the reference of tests/canny_ref.py bit for bit -- the pipeline is integer arithmetic from the 8-bit value on, so every
comparison is array_equal with no exempt pixel --, mlsd_invert, the public tensor call and the wrapper, and the control_preprocess option end to end: what a pass
is conditioned on equals the composition by hand (resample to the pass's size, then Canny with the tiling as wrap), at the hires second pass's and a tiled
canvas's own size too."""
import ctypes as C

import numpy as np
import pytest

import canny_ffi as CN
import canny_ref as R
import mlis_ffi as F

pytestmark = pytest.mark.gpu

NAMES = list(R.cases((8, 8, 8, 8)))       # the names do not depend on the tile


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return CN.bind(_lib.LIB_PATH)


_cases = {}


def cases(lib):
    if not _cases:
        _cases.update(R.cases(CN.tile(lib)))
    return _cases


# ------------------------------------------------------------------ kernel
def run_kernel(x, lo, hi, l2, wrap, planes_out):
    """x float32 [planes][h][w] -> (float32 [planes_out][h][w], n_passes)"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    planes, h, w = x.shape
    src, dst, ws = _lib.from_numpy(x), _lib.DeviceBuffer(planes_out * h * w * 4), _lib.DeviceBuffer(K.canny_ws_bytes(w, h))
    n = K.canny(src.ptr, w, h, planes, lo, hi, l2, wrap, dst.ptr, planes_out, ws.ptr)
    K.sync()
    return dst.download((planes_out, h, w), np.float32), n


def configs():
    for name in NAMES:
        for wrap in range(4):
            for l2 in (0, 1):
                yield pytest.param(name, l2, wrap, id=f"{name}-{'l2' if l2 else 'l1'}-w{wrap}")


@pytest.mark.parametrize("name,l2,wrap", configs())
def test_kernel_equals_the_reference(lib, name, l2, wrap):
    u8, thr = cases(lib)[name]
    for planes in (1, 3):
        want, cls, m, lo, hi = R.expected(name, u8, thr, planes, l2, wrap)
        x = R.as_float(u8[:planes])
        for planes_out in (1, 3):
            got, n = run_kernel(x, lo, hi, l2, wrap, planes_out)
            diff = int((got != want[None].astype(np.float32)).sum())
            print(f"{name} planes {planes}->{planes_out} l2 {l2} wrap {wrap}: lo {lo} hi {hi}, weak {(cls == 1).sum()} strong {(cls == 2).sum()} edges {want.sum()}, "
                  f"sweeps {n}, pixels that differ {diff}")
            assert got.shape == (planes_out,) + want.shape and np.array_equal(got, np.broadcast_to(want.astype(np.float32), got.shape))
            assert 1 <= n <= want.size + 1
            if name == "serpentine_lit":
                assert n >= 2                  # the multi-sweep path ran: the edge is lit across tile borders
                assert want.sum() > 4000 and (wrap & 2 or want.sum() == (cls > 0).sum())      # the whole line (a wrapped y axis adds an edge at its seam that no strong pixel touches)
            if name == "serpentine_dark" and not wrap:
                assert not got.any()


def test_overshoot_clamps(lib):
    """values a bicubic or lanczos resample leaves outside [0, 1]"""
    x = np.array(R.overshoot_input())
    for l2 in (0, 1):
        for wrap in (0, 3):
            lo, hi = R.thresholds(100, 200, l2)
            want = R.canny(x, lo, hi, l2, wrap)
            assert want.any() and np.array_equal(R.quantise(np.array([-0.2, 1.3], np.float32)), [0, 255])
            got, _ = run_kernel(x, lo, hi, l2, wrap, 3)
            assert np.array_equal(got, np.broadcast_to(want.astype(np.float32), got.shape))
            # the same image with the overshoot clamped by hand
            assert np.array_equal(run_kernel(np.clip(x, 0, 1), lo, hi, l2, wrap, 3)[0], got)


def test_invert_is_exact(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    x = np.random.default_rng(6).standard_normal(100003).astype(np.float32)
    src, dst = _lib.from_numpy(x), _lib.DeviceBuffer(x.nbytes)
    K.invert(src.ptr, dst.ptr, x.size)
    K.sync()
    assert dst.download(x.shape, np.float32).tobytes() == (np.float32(1) - x).tobytes()
    K.invert(src.ptr, src.ptr, x.size)           # in place
    K.sync()
    assert src.download(x.shape, np.float32).tobytes() == (np.float32(1) - x).tobytes()


def test_two_calls_give_identical_bytes(lib):
    u8, thr = cases(lib)["rand_300x200"]
    x = R.as_float(u8)
    lo, hi = R.expected("rand_300x200", u8, thr, 3, 0, 3)[3:]
    (a, na), (b, nb) = run_kernel(x, lo, hi, 0, 3, 3), run_kernel(x, lo, hi, 0, 3, 3)
    assert a.tobytes() == b.tobytes() and na == nb


# ------------------------------------------------------------------ public call
def as_tensor(x):
    b, c, h, w = x.shape
    return F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, b), 0)


def test_public_call_and_wrapper_equal_the_kernel(lib):
    from mlimgsynth_amd import mlimgsynth as W
    u8 = cases(lib)["rand_37x29"][0]
    m = F.Mlis(lib)
    try:
        for planes, low, high, l2, wrap in ((3, 100.0, 200.0, 0, 0), (1, 250.5, 120.0, 1, 3), (3, 80.0, 160.0, 0, 1), (3, 0.0, 32767.0, 1, 2)):
            x = np.ascontiguousarray(R.as_float(u8[:planes])[None])
            lo, hi = R.thresholds(low, high, l2)
            want = run_kernel(x[0], lo, hi, l2, wrap, 3)[0]
            out = F.Tensor()
            assert lib.mlis_amd_tensor_canny(m.ctx, C.byref(as_tensor(x)), C.byref(out), low, high, l2, wrap) == 1, m.err()
            assert [out.n[i] for i in range(4)] == [37, 29, 3, 1]
            got = F.tensor_np(out)
            lib.mlis_tensor_free(C.byref(out))
            assert got[0].tobytes() == want.tobytes() and np.array_equal(want[0], R.canny(x[0], lo, hi, l2, wrap).astype(np.float32))
            with W.MLImgSynth() as s:
                t = s.canny(W.tensor_from_numpy(x), low, high, bool(l2), wrap)
                assert t.n == (37, 29, 3, 1) and t.numpy()[0].tobytes() == want.tobytes()
                if planes == 3:
                    assert s.canny(np.ascontiguousarray(u8.transpose(1, 2, 0)), low, high, bool(l2), wrap).numpy()[0].tobytes() == want.tobytes()
                else:
                    assert s.canny(u8[0], low, high, bool(l2), wrap).numpy()[0].tobytes() == want.tobytes()
        # in place, on one of the context's own tensors
        x = np.ascontiguousarray(R.as_float(u8)[None])
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["IMAGE"])
        lib.mlis_tensor_resize(t, 37, 29, 3, 1)
        C.memmove(t.contents.d, x.ctypes.data, x.nbytes)
        assert lib.mlis_amd_tensor_canny(m.ctx, t, t, 100.0, 200.0, 0, 0) == 1, m.err()
        assert m.tensor(F.TENSOR["IMAGE"])[0].tobytes() == run_kernel(x[0], 100, 200, 0, 0, 3)[0].tobytes()
    finally:
        m.close()


# ------------------------------------------------------------------ end to end: tinyxl, control_model synth, the sizes of tests/test_controlnet_gpu.py
def source_map(w=96, h=80, seed=21):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def as_library_tensor(arr):
    """the u8 map [h][w][3] as the control_image option converts it: u8 x float(1 / 255), [1][3][h][w]"""
    return np.ascontiguousarray(arr.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))[None]


def by_hand(lib, m, arr, w, h, low=100.0, high=200.0, l2=0, filter=None, wrap=0, invert=False, plain=False):
    """the map of a w x h pass by hand, on the public tensor calls of the context m (they follow its tiling): resample, then Canny or 1 - x; float32 [3][h][w]"""
    x = as_library_tensor(arr)
    t = F.Tensor()
    if filter is not None and (w < arr.shape[1] or h < arr.shape[0]):
        assert lib.mlis_amd_tensor_resample_aa(m.ctx, C.byref(as_tensor(x)), C.byref(t), w, h, filter) == 1, m.err()
    else:
        assert lib.mlis_amd_tensor_resample(m.ctx, C.byref(as_tensor(x)), C.byref(t), w, h, 1) == 1, m.err()
    if invert or plain:
        out = np.float32(1) - F.tensor_np(t)[0] if invert else F.tensor_np(t)[0]
    else:
        assert lib.mlis_amd_tensor_canny(m.ctx, C.byref(t), C.byref(t), low, high, l2, wrap) == 1, m.err()
        out = F.tensor_np(t)[0]
    lib.mlis_tensor_free(C.byref(t))
    return out


def held_map(lib, m):
    """mlis_amd_control_image_get of the engine used last: float32 [3][h][w]"""
    eng = lib.mlis_amd_engine_get(m.ctx)
    w, h = C.c_int(), C.c_int()
    assert lib.mlis_amd_control_image_get(eng, None, C.byref(w), C.byref(h)) == 1
    out = np.empty((3, h.value, w.value), np.float32)
    assert lib.mlis_amd_control_image_get(eng, out.ctypes.data_as(C.POINTER(C.c_float)), None, None) == 1
    return out


def as_u8_image(map01):
    """a 0 / 1 map [3][h][w] as the u8 control image that converts back to it exactly (255 x float(1 / 255) == 1)"""
    assert np.isin(map01, (0, 1)).all()
    return np.ascontiguousarray((map01 * 255).astype(np.uint8).transpose(1, 2, 0))


def context(lib, arr, **opts):
    import test_controlnet_gpu as TC
    m = TC.context(lib, model="tinyxl")
    TC.set_control_image(m, arr)
    for k, v in opts.items():
        m.set(k, v)
    return m


def run(lib, m):
    import test_controlnet_gpu as TC
    r = TC.run(lib, m)
    r["map"] = held_map(lib, m)
    return r


@pytest.mark.parametrize("how", ["bilinear", "lanczos"])
def test_generate_with_canny_equals_the_map_made_by_hand(lib, how):
    """(i), (ii), (vi): the 96 x 80 map bilinearly to the 64 x 64 pass, or a 200 x 150 one through the antialiased lanczos filter"""
    arr = source_map() if how == "bilinear" else source_map(200, 150, seed=22)
    opts = {} if how == "bilinear" else dict(downscale_filter="lanczos")
    m = context(lib, arr, control_preprocess="canny", **opts)
    try:
        a = run(lib, m)
        hand = by_hand(lib, m, arr, 64, 64, filter=None if how == "bilinear" else 3)
    finally:
        m.close()
    assert hand.shape == (3, 64, 64) and hand.any() and not hand.all() and np.array_equal(hand[0], hand[1]) and np.array_equal(hand[0], hand[2])
    assert a["map"].tobytes() == hand.tobytes() and a["hint"].tobytes() == hand.tobytes()
    m = context(lib, as_u8_image(hand), **opts)
    try:
        b = run(lib, m)
    finally:
        m.close()
    assert b["map"].tobytes() == hand.tobytes()
    assert a["latent"].tobytes() == b["latent"].tobytes() and a["image"].tobytes() == b["image"].tobytes()
    assert ", Control preprocess: canny 100 200" in a["info"] and "Control preprocess" not in b["info"]
    assert a["info"].replace(", Control preprocess: canny 100 200", "") == b["info"]
    assert a["builds"] == 1 and b["builds"] == 1


def test_changed_thresholds_recompute_the_map_without_a_rebuild(lib):
    """(iii), and the same for canny_high, canny_l2 and the preprocessor itself; an unchanged setting keeps the image the engine holds.  The thresholds lie inside
    the magnitudes of the resampled noise (its quartiles are near 330, 410 and 510), so each step moves hundreds of pixels"""
    arr = source_map()
    m = context(lib, arr, control_preprocess="canny", canny_low=300, canny_high=600)
    try:
        first = run(lib, m)
        tag = lib.mlis_amd_control_tag(lib.mlis_amd_engine_get(m.ctx))
        m.set("canny_low", 300)                      # the value it has
        again = run(lib, m)
        assert lib.mlis_amd_control_tag(lib.mlis_amd_engine_get(m.ctx)) == tag and again["map"].tobytes() == first["map"].tobytes()
        seen = [first["map"].tobytes()]
        assert first["map"].tobytes() == by_hand(lib, m, arr, 64, 64, low=300.0, high=600.0).tobytes()
        for name, value, kw, text in (("canny_low", 450, dict(low=450.0, high=600.0), "canny 450 600"), ("canny_high", 500, dict(low=450.0, high=500.0), "canny 450 500"),
                                      ("canny_l2", "y", dict(low=450.0, high=500.0, l2=1), "canny 450 500 L2")):
            m.set(name, value)
            r = run(lib, m)
            assert r["map"].tobytes() == by_hand(lib, m, arr, 64, 64, **kw).tobytes() and r["map"].tobytes() not in seen
            assert f", Control preprocess: {text}," in r["info"] and r["builds"] == 1
            assert lib.mlis_amd_control_tag(lib.mlis_amd_engine_get(m.ctx)) not in (0, tag)
            seen.append(r["map"].tobytes())
        m.set("control_preprocess", "none")
        r = run(lib, m)
        assert r["map"].tobytes() == by_hand(lib, m, arr, 64, 64, plain=True).tobytes() and r["map"].tobytes() not in seen
        assert "Control preprocess" not in r["info"] and r["builds"] == 1
    finally:
        m.close()


def test_hires_second_pass_holds_the_map_of_its_own_size(lib):
    """(iv): 64 x 64 first pass, 96 x 96 second: the second engine's map is Canny at 96 x 96, not the first's resampled"""
    arr = source_map()
    m = context(lib, arr, control_preprocess="canny", hires_scale=1.5, hires_denoise=0.6, hires_steps=3)
    try:
        r = run(lib, m)
        big, small = by_hand(lib, m, arr, 96, 96), by_hand(lib, m, arr, 64, 64)
        assert r["latent"].shape == (1, 4, 12, 12) and r["evals"][0] > 0 and r["evals"][1] > 0 and r["builds"] == 2
        assert r["map"].shape == (3, 96, 96) and r["map"].tobytes() == big.tobytes()
        assert np.isin(r["map"], (0, 1)).all()       # one-pixel edges at the pass's own resolution: nothing resampled into grey
        # the first pass's engine is the other resident one: a plain generation at its size finds it and the map it holds
        m.set("hires_scale", 0)
        one = run(lib, m)
        assert one["builds"] == 2 and one["map"].shape == (3, 64, 64) and one["map"].tobytes() == small.tobytes()
    finally:
        m.close()


def test_invert(lib):
    """(v): the map is 1 - x of the resampled image; and on byte values whose complement is exact in fp32 the generation equals one on the complemented image"""
    arr = source_map()
    m = context(lib, arr, control_preprocess="invert")
    try:
        r = run(lib, m)
        assert r["map"].tobytes() == by_hand(lib, m, arr, 64, 64, invert=True).tobytes()
        assert ", Control preprocess: invert," in r["info"]
    finally:
        m.close()
    f = np.float32(1 / 255.0)
    exact = np.array([u for u in range(256) if np.float32(1) - np.float32(u) * f == np.float32(255 - u) * f], np.uint8)
    assert exact.size >= 16
    arr = np.random.default_rng(23).choice(exact, (64, 64, 3)).astype(np.uint8)
    res = []
    for image, opts in ((arr, dict(control_preprocess="invert")), (255 - arr, {})):
        m = context(lib, image, **opts)
        try:
            res.append(run(lib, m))
        finally:
            m.close()
    a, b = res
    assert a["map"].tobytes() == b["map"].tobytes() == (np.float32(1) - as_library_tensor(arr)[0]).tobytes()
    assert a["latent"].tobytes() == b["latent"].tobytes() and a["image"].tobytes() == b["image"].tobytes()


def test_tiled_canvas_and_seamless_tiling(lib):
    """(vii): a 96 x 64 canvas of two 64 x 64 windows holds one map of the canvas's size; with tiling x the Canny wraps as the resample does"""
    arr = source_map()
    for tiling, wrap in (("none", 0), ("x", 1)):
        m = context(lib, arr, control_preprocess="canny", unet_tile=64, unet_tile_overlap=32, tiling=tiling)
        try:
            m.set("image_dim", 96, 64)
            r = run(lib, m)
            hand = by_hand(lib, m, arr, 96, 64, wrap=wrap)
            assert r["latent"].shape == (1, 4, 8, 12) and r["map"].shape == (3, 64, 96) and r["map"].tobytes() == hand.tobytes()
            if wrap:
                assert hand.tobytes() != by_hand(lib, m, arr, 96, 64, wrap=0).tobytes()
        finally:
            m.close()


# ------------------------------------------------------------------ the command
def test_canny_command_writes_the_map_of_the_public_call(lib, tmp_path):
    """canny -i IN -o OUT, no model: the written PNG (and PGM-family file) is mlis_amd_tensor_canny of the read image, 255 on edges; the tiling option is the wrap"""
    import test_cli as TCLI
    u8 = cases(lib)["rand_37x29"][0]
    hwc = np.ascontiguousarray(u8.transpose(1, 2, 0))
    src = tmp_path / "in.ppm"
    src.write_bytes(b"P6\n37 29\n255\n" + hwc.tobytes())
    m = F.Mlis(lib)
    try:
        for args, low, high, l2, wrap in (((), 100.0, 200.0, 0, 0), (("--canny-low", "80.5", "--canny-high", "160", "--canny-l2", "y", "--tiling", "xy"), 80.5, 160.0, 1, 3)):
            x = as_library_tensor(hwc)             # the command converts as the library does: u8 x float(1 / 255)... and u8 / 255.0f; both quantise back to u8
            out = F.Tensor()
            assert lib.mlis_amd_tensor_canny(m.ctx, C.byref(as_tensor(x)), C.byref(out), low, high, l2, wrap) == 1, m.err()
            want = (F.tensor_np(out)[0] * 255).astype(np.uint8).transpose(1, 2, 0)
            lib.mlis_tensor_free(C.byref(out))
            assert want.any() and np.isin(want, (0, 255)).all()
            png, ppm = tmp_path / "out.png", tmp_path / "out.ppm"
            TCLI.run("canny", "-i", str(src), "-o", str(png), *args)
            TCLI.run("canny", "-i", str(src), "-o", str(ppm), *args)
            px, text = TCLI.png_pixels(png.read_bytes())
            assert px.shape == (29, 37, 3) and np.array_equal(px, want) and not text
            raw = ppm.read_bytes()
            assert raw.startswith(b"P6\n37 29\n255\n") and raw[len(b"P6\n37 29\n255\n"):] == want.tobytes()
    finally:
        m.close()
    r = TCLI.run("canny", "-i", str(tmp_path / "missing.ppm"), "-o", str(tmp_path / "x.png"), ok=False)
    assert r.returncode != 0
