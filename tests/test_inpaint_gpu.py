"""Region inpainting on the GPU: the kernels of hip/inpaint.hip against the restatements of tests/inpaint_ref.py -- grow, bounding box and composite bit for bit,
the blur per element against float64 of the library's own float taps within the bound of fp32 sums in the stated order --, the public tensor calls and the wrapper,
and the driver end to end on synth:tiny: what mlis_generate returns equals, bit for bit, the composition by hand of the public calls."""
import ctypes as C
import functools

import numpy as np
import pytest

import inpaint_ffi as IF
import inpaint_ref as R
import mlis_ffi as F

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29), (131, 70), (300, 200)]       # w, h: no multiple of any tile, narrower than a large radius; several tiles


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


# ------------------------------------------------------------------ kernels
def run_weight(x, invert):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    src, dst = _lib.from_numpy(x), _lib.DeviceBuffer(x.nbytes)
    K.mask_weight(src.ptr, dst.ptr, x.size, invert)
    K.sync()
    return dst.download(x.shape, np.float32)


def run_grow(x, radius, wrap):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    h, w = x.shape
    src, dst, ws = _lib.from_numpy(x), _lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(x.nbytes)
    K.mask_grow(src.ptr, dst.ptr, w, h, radius, wrap, ws.ptr)
    K.sync()
    return dst.download(x.shape, np.float32)


def run_blur(x, sigma, wrap):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    planes, h, w = x.shape
    src, dst, ws = _lib.from_numpy(x), _lib.DeviceBuffer(x.nbytes), _lib.DeviceBuffer(K.gauss_blur_ws_bytes(w, h, planes))
    K.gauss_blur(src.ptr, dst.ptr, w, h, planes, sigma, wrap, ws.ptr)
    K.sync()
    return dst.download(x.shape, np.float32)


def run_bbox(p):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    h, w = p.shape
    src, out = _lib.from_numpy(p), _lib.from_numpy(np.full(4, -7, np.int32))
    K.mask_bbox(src.ptr, w, h, out.ptr)
    K.sync()
    return tuple(int(v) for v in out.download((4,), np.int32))


def run_composite(orig, patch, p, x0, y0, in_place=False):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    B, c, ch, cw = patch.shape
    H, W = p.shape
    o, t, w = _lib.from_numpy(orig), _lib.from_numpy(patch), _lib.from_numpy(p)
    dst = o if in_place else _lib.from_numpy(np.full((B, c, H, W), 9e9, np.float32))
    K.composite(dst.ptr, o.ptr, orig.shape[0], t.ptr, w.ptr, W, H, c, B, x0, y0, cw, ch)
    K.sync()
    return dst.download((B, c, H, W), np.float32)


def test_mask_weight(lib):
    x = np.random.default_rng(1).standard_normal(100003).astype(np.float32)
    x[:6] = [0.0, 1.0, np.nan, -0.0, 2.0, 0.25]
    for invert in (0, 1):
        got, want = run_weight(x, invert), R.mask_weight(x, invert)
        assert got.tobytes() == want.tobytes() and got.min() == 0 and got.max() == 1 and got[2] == 0


@pytest.mark.parametrize("w,h", SHAPES)
def test_grow_bit_for_bit(lib, w, h):
    rng = np.random.default_rng(w)
    masks = {"random": (rng.random((h, w)) < 0.03).astype(np.float32), "dense": (rng.random((h, w)) < 0.9).astype(np.float32)}
    for name, (y, x) in (("c00", (0, 0)), ("c01", (0, w - 1)), ("c10", (h - 1, 0)), ("c11", (h - 1, w - 1)), ("border", (min(h - 1, 16), min(w - 1, 256 if w > 256 else 64)))):
        masks[name] = np.zeros((h, w), np.float32)
        masks[name][y, x] = 1
    for name, x in masks.items():
        for radius in (0, 1, 5, -5, 40, -40):       # 40 on the 37-wide image wraps more than once
            if name not in ("random", "dense") and radius < 0:
                continue                             # the minimum of a single lit pixel is all zeros
            for wrap in range(4):
                got = run_grow(x, radius, wrap)
                a, b = R.grow(x, radius, wrap), R.grow_scipy(x, radius, wrap)
                assert got.tobytes() == a.tobytes() and got.tobytes() == b.tobytes(), (name, radius, wrap, int((got != a).sum()))
    assert run_grow(masks["c00"], 5, 0).sum() == 36 and run_grow(masks["c00"], 5, 3).sum() == 121
    assert run_grow(masks["random"], 5, 3).tobytes() == run_grow(masks["random"], 5, 3).tobytes()


@functools.lru_cache(maxsize=None)
def blur_matrices(lib_taps, n, wrap):
    taps = np.frombuffer(lib_taps, np.float32)
    return R.blur_matrix(n, taps, wrap), R.blur_matrix_abs(n, taps, wrap)


@pytest.mark.parametrize("sigma", [0.1, 1.0, 4.0, 16.0, 64.0])
@pytest.mark.parametrize("w,h", SHAPES)
def test_blur_against_float64_of_the_librarys_taps(lib, w, h, sigma):
    rng = np.random.default_rng(int(sigma * 10) + w)
    taps = IF.taps(lib, sigma)
    r = len(taps) // 2
    assert r == R.gauss_radius(sigma)
    worst = 0.0
    for planes in (1, 3):
        x = rng.standard_normal((planes, h, w)).astype(np.float32)
        x[0] = (rng.random((h, w)) < 0.3).astype(np.float32)       # plane 0: a mask in [0, 1]
        if planes == 3:
            x[1] = np.float32(0.7)                                  # a constant plane
        for wrap in range(4):
            got = run_blur(x, sigma, wrap)
            if r == 0:
                assert got.tobytes() == x.tobytes()                # identity: the bytes of the input
                continue
            Ax, Axa = blur_matrices(taps.tobytes(), w, wrap & 1)
            Ay, Aya = blur_matrices(taps.tobytes(), h, (wrap >> 1) & 1)
            x64 = x.astype(np.float64)
            want = Ay @ x64 @ Ax.T
            bound = (2 * (2 * r + 1) + 2) * 2.0 ** -24 * (Aya @ np.abs(x64) @ Axa.T)
            err = np.abs(got.astype(np.float64) - want)
            ratio = float((err / np.maximum(bound, 1e-300)).max())
            worst = max(worst, ratio)
            assert (err <= bound).all(), (planes, wrap, ratio)
            assert got[0].min() >= 0 and (got[0] <= 1 + bound[0]).all()                          # a mask stays in [0, 1 + bound]
            if planes == 3:
                assert (np.abs(got[1].astype(np.float64) - float(np.float32(0.7))) <= bound[1]).all()   # a constant stays constant
            # the direct and the LDS row pass, switched by the test hook, give identical bytes; and a second call repeats the first
            was = lib.mlsd_gauss_blur_lds_limit(0)
            try:
                direct = run_blur(x, sigma, wrap)
            finally:
                lib.mlsd_gauss_blur_lds_limit(was)
            assert was == 32768 and direct.tobytes() == got.tobytes() and run_blur(x, sigma, wrap).tobytes() == got.tobytes()
    print(f"blur {w}x{h} sigma {sigma} (r {r}): worst err / bound = {worst:.3f}")


def test_blur_small_lds_limit_changes_the_tile_not_the_result(lib):
    """limits between 0 and 32 KiB: fewer rows per tile, then the direct path"""
    x = np.random.default_rng(3).standard_normal((3, 70, 131)).astype(np.float32)
    want = run_blur(x, 16.0, 1)
    for limit in (20000, 8192, 4096, 1000):
        was = lib.mlsd_gauss_blur_lds_limit(limit)
        try:
            assert run_blur(x, 16.0, 1).tobytes() == want.tobytes(), limit
        finally:
            lib.mlsd_gauss_blur_lds_limit(was)


@pytest.mark.parametrize("w,h", SHAPES)
def test_bbox(lib, w, h):
    z = np.zeros((h, w), np.float32)
    assert run_bbox(z) == (0, 0, 0, 0) and run_bbox(z + 1) == (0, 0, w, h)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w - 1), (h - 1, w // 3)):
        p = z.copy()
        p[y, x] = 0.5
        assert run_bbox(p) == (x, y, x + 1, y + 1) == R.bbox(p)
    p = z.copy()
    p[:] = -0.0
    p[3, 5], p[7, 2], p[1, 1] = 1e-30, -1.0, np.nan
    assert run_bbox(p) == (5, 3, 6, 4) == R.bbox(p)               # 1e-30 counts; -0.0, 0.0, negatives and NaN do not
    rng = np.random.default_rng(h)
    for k in range(6):
        p = np.where(rng.random((h, w)) < 0.002 * (k + 1), rng.random((h, w)).astype(np.float32), np.float32(0)).astype(np.float32)
        ys, xs = np.nonzero(p)
        want = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1) if xs.size else (0, 0, 0, 0)
        assert run_bbox(p) == want == R.bbox(p)


@pytest.mark.parametrize("B,n_orig", [(1, 1), (2, 1), (2, 2)])
def test_composite_bit_for_bit(lib, B, n_orig):
    rng = np.random.default_rng(10 * B + n_orig)
    for (W, H), planes in (((37, 29), 3), ((131, 70), 1)):
        orig = rng.standard_normal((n_orig, planes, H, W)).astype(np.float32)
        p = rng.random((H, W)).astype(np.float32)
        p[rng.random((H, W)) < 0.3] = 0
        p[rng.random((H, W)) < 0.3] = 1
        for x0, y0, cw, ch in ((0, 0, 5, 4), (W - 6, H - 3, 6, 3), (0, 0, W, H), (W // 2, H // 2, 1, 1), (3, 2, W - 7, H - 5)):
            patch = rng.standard_normal((B, planes, ch, cw)).astype(np.float32)
            got, want = run_composite(orig, patch, p, x0, y0), R.composite(orig, patch, p, x0, y0)
            assert np.array_equal(got, want), (W, H, x0, y0, cw, ch)
            inside = np.zeros((H, W), bool)
            inside[y0:y0 + ch, x0:x0 + cw] = True
            full = np.broadcast_to(orig, want.shape)
            keep = np.broadcast_to(~inside | (p == 0), want.shape)
            assert np.array_equal(got[keep], full[keep])                                         # outside the rectangle and where p == 0: the original
            assert got[:, :, ~inside].tobytes() == np.ascontiguousarray(full[:, :, ~inside]).tobytes()   # outside: a copy of the bits
            sel = (p == 1)[y0:y0 + ch, x0:x0 + cw]
            assert np.array_equal(got[:, :, y0:y0 + ch, x0:x0 + cw][:, :, sel], patch[:, :, sel])  # where p == 1: the patch
            if n_orig == B:
                assert run_composite(orig, patch, p, x0, y0, in_place=True).tobytes() == got.tobytes()


# ------------------------------------------------------------------ public calls and the wrapper
def test_public_calls_and_wrapper_equal_the_kernels(lib, m):
    from mlimgsynth_amd import mlimgsynth as W
    rng = np.random.default_rng(8)
    w, h = 37, 29
    mask = (rng.random((1, 1, h, w)) < 0.95).astype(np.float32)
    mask[0, 0, 10:14, 20:30] = 0
    p0 = IF.call_tensor(lib, m, lib.mlis_amd_tensor_mask_weight, mask, 0)
    assert p0[0, 0].tobytes() == run_weight(mask[0, 0], 0).tobytes()
    assert IF.call_tensor(lib, m, lib.mlis_amd_tensor_mask_weight, 1 - mask, 1).tobytes() == p0.tobytes()
    for radius, wrap in ((3, 0), (-1, 3), (40, 1)):
        g = IF.call_tensor(lib, m, lib.mlis_amd_tensor_mask_grow, p0, radius, wrap)
        assert g[0, 0].tobytes() == run_grow(p0[0, 0], radius, wrap).tobytes() and g.shape == p0.shape
    x = rng.standard_normal((2, 3, h, w)).astype(np.float32)
    for sigma, wrap in ((2.0, 0), (16.0, 3), (0.1, 0)):
        b = IF.call_tensor(lib, m, lib.mlis_amd_tensor_gauss_blur, x, sigma, wrap)
        assert b.reshape(6, h, w).tobytes() == run_blur(x.reshape(6, h, w), sigma, wrap).tobytes()
    g = IF.call_tensor(lib, m, lib.mlis_amd_tensor_mask_grow, p0, 2, 0)
    p = IF.call_tensor(lib, m, lib.mlis_amd_tensor_gauss_blur, g, 2.0, 0)
    assert IF.bbox(lib, m, p) == run_bbox(p[0, 0]) == R.bbox(p[0, 0]) and IF.bbox(lib, m, np.zeros((1, 1, h, w), np.float32)) == (0, 0, 0, 0)
    orig, patch = rng.standard_normal((1, 3, h, w)).astype(np.float32), rng.standard_normal((2, 3, 9, 11)).astype(np.float32)
    c = IF.composite(lib, m, orig, patch, p, 5, 7)
    assert c.tobytes() == run_composite(orig, patch, p[0, 0], 5, 7).tobytes() and np.array_equal(c, R.composite(orig, patch, p[0, 0], 5, 7))
    # in place on one of the context's own tensors: dst is the patch
    t = lib.mlis_tensor_get(m.ctx, F.TENSOR["IMAGE"])
    full = rng.standard_normal((2, 3, h, w)).astype(np.float32)
    lib.mlis_tensor_resize(t, w, h, 3, 2)
    C.memmove(t.contents.d, full.ctypes.data, full.nbytes)
    assert lib.mlis_amd_tensor_composite(m.ctx, t, C.byref(IF.as_tensor(orig)), t, C.byref(IF.as_tensor(p)), 0, 0) == 1, m.err()
    assert m.tensor(F.TENSOR["IMAGE"]).tobytes() == run_composite(orig, full, p[0, 0], 0, 0).tobytes()
    with W.MLImgSynth() as s:
        tp = s.mask_process(W.tensor_from_numpy(mask), grow=2, blur=2.0)
        assert tp.n == (w, h, 1, 1) and tp.numpy().tobytes() == p.tobytes()
        assert s.mask_process(W.tensor_from_numpy(1 - mask), grow=2, blur=2.0, invert=True).numpy().tobytes() == p.tobytes()
        assert s.mask_process(W.tensor_from_numpy(mask)).numpy().tobytes() == p0.tobytes()
        assert s.mask_bbox(tp) == R.bbox(p[0, 0])
        assert s.composite(W.tensor_from_numpy(orig), W.tensor_from_numpy(patch), tp, 5, 7).numpy().tobytes() == c.tobytes()
        assert s.gauss_blur(W.tensor_from_numpy(x), 16.0, 3).numpy().tobytes() == IF.call_tensor(lib, m, lib.mlis_amd_tensor_gauss_blur, x, 16.0, 3).tobytes()


# ------------------------------------------------------------------ end to end on synth:tiny
TOKS, NTOKS = np.array([5, 17, 300, 42, 7], np.int32), np.array([9, 250], np.int32)       # ids inside the synthetic models' small vocabulary
W0, H0 = 100, 84                                  # no multiple of 8, on purpose
RECT = (52, 30, 82, 50)                           # the repainted rectangle, about 30 x 20, off-centre


def picture(w=W0, h=H0, seed=31):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def keep_mask(w=W0, h=H0, rect=RECT):
    a = np.full((h, w, 1), 255, np.uint8)
    a[rect[1]:rect[3], rect[0]:rect[2]] = 0
    return a


def as_library_tensor(arr):
    """u8 [h][w][c] as the IMAGE / IMAGE_MASK options convert it: u8 x float(1 / 255), [1][c][h][w]"""
    return np.ascontiguousarray(arr.transpose(2, 0, 1).astype(np.float32) * np.float32(1 / 255.0))[None]


def context(lib, model="tiny", batch=2, **opts):
    c = F.Mlis(lib)
    c.set("model", f"synth:{model}")
    c.set("image_dim", 64, 64)
    c.set("steps", 4), c.set("seed", 42), c.set("cfg_scale", 7.0), c.set("method", "euler_a"), c.set("batch_size", batch)
    for k, v in opts.items():
        c.set(k, v)
    return c


def set_inputs(lib, c, img, mask):
    im = F.Image(img.ctypes.data_as(C.POINTER(C.c_uint8)), img.size, img.shape[1], img.shape[0], 3, 0)
    assert lib.mlis_option_set(c.ctx, F.OPT["IMAGE"], C.byref(im)) == 1, c.err()
    if mask is not None:
        mk = F.Image(mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.size, mask.shape[1], mask.shape[0], 1, 0)
        assert lib.mlis_option_set(c.ctx, F.OPT["IMAGE_MASK"], C.byref(mk)) == 1, c.err()
    c.set("f_t_ini", 0.6)


def set_tensor(lib, c, tid, x):
    b, ch, h, w = x.shape
    t = lib.mlis_tensor_get(c.ctx, tid)
    lib.mlis_tensor_resize(t, w, h, ch, b)
    x = np.ascontiguousarray(x, np.float32)
    C.memmove(t.contents.d, x.ctypes.data, x.nbytes)


def generate(lib, c):
    c.tokens(TOKS)
    c.tokens(NTOKS, negative=True)
    c.generate()
    reg, proc = (C.c_int * 4)(), (C.c_int * 2)()
    done = lib.mlis_amd_inpaint_info(c.ctx, reg, proc)

    def opt(tid):           # a tensor the generation may have freed
        t = lib.mlis_tensor_get(c.ctx, tid).contents
        return F.tensor_np(t) if t.d else None
    return dict(image=c.tensor(F.TENSOR["IMAGE"]), latent=c.tensor(F.TENSOR["LATENT"]), mask=opt(F.TENSOR["MASK"]), lmask=opt(F.TENSOR["LMASK"]),
                info=lib.mlis_infotext_get(c.ctx, 0).decode(), done=done, region=tuple(reg), proc=tuple(proc))


def resample(lib, c, x, w, h, filter=None, mode=1):
    """what the driver chooses: antialiased with the filter where one is set and an axis shrinks, else plain"""
    if filter is not None and (w < x.shape[3] or h < x.shape[2]):
        return IF.call_tensor(lib, c, lib.mlis_amd_tensor_resample_aa, x, w, h, filter)
    return IF.call_tensor(lib, c, lib.mlis_amd_tensor_resample, x, w, h, mode)


def weight_by_hand(lib, c, mask_u8, grow, blur, invert=0):
    p = IF.call_tensor(lib, c, lib.mlis_amd_tensor_mask_weight, as_library_tensor(mask_u8), invert)
    if grow:
        p = IF.call_tensor(lib, c, lib.mlis_amd_tensor_mask_grow, p, grow, 0)
    if blur > 0:
        p = IF.call_tensor(lib, c, lib.mlis_amd_tensor_gauss_blur, p, blur, 0)
    return p


def masked_by_hand(lib, img, mask, filter=None, **opts):
    """the composition by hand through the public calls, on a context of its own: same seed, Philox offset 0"""
    c = context(lib, **opts)
    try:
        p = weight_by_hand(lib, c, mask, 2, 2.0)
        box = IF.bbox(lib, c, p)
        reg = R.region(W0, H0, box, 8, 64, 64)
        x0, y0, x1, y1 = reg
        orig = as_library_tensor(img)
        crop = np.ascontiguousarray(orig[:, :, y0:y1, x0:x1])
        mcrop = np.ascontiguousarray((np.float32(1) - p)[:, :, y0:y1, x0:x1])
        set_tensor(lib, c, F.TENSOR["IMAGE"], resample(lib, c, crop, 64, 64, filter))
        set_tensor(lib, c, F.TENSOR["MASK"], resample(lib, c, mcrop, 64, 64, filter))
        c.set("tensor_use_flags", F.TUF["IMAGE"] | F.TUF["MASK"])
        c.set("f_t_ini", 0.6)
        g = generate(lib, c)
        assert g["done"] == 0 and g["image"].shape == (2, 3, 64, 64)
        back = resample(lib, c, g["image"], x1 - x0, y1 - y0, filter)
        final = IF.composite(lib, c, orig, back, p, x0, y0)
        return dict(final=final, p=p, region=reg, box=box, pass_=g, orig=orig)
    finally:
        c.close()


def masked_by_driver(lib, img, mask, **opts):
    c = context(lib, inpaint_area="masked", inpaint_padding=8, mask_blur=2, mask_grow=2, **opts)
    try:
        set_inputs(lib, c, img, mask)
        a = generate(lib, c)
        set_inputs(lib, c, img, mask)
        c.set("seed", 42)
        return a, c
    except Exception:
        c.close()
        raise


@pytest.fixture(scope="module")
def hand(lib):
    return masked_by_hand(lib, picture(), keep_mask())


def test_masked_equals_the_composition_by_hand(lib, hand):
    a, c = masked_by_driver(lib, picture(), keep_mask())
    c.close()
    assert a["done"] == 1 and a["region"] == hand["region"] == R.region(W0, H0, hand["box"], 8, 64, 64) and a["proc"] == (64, 64)
    x0, y0, x1, y1 = a["region"]
    assert hand["box"] == (RECT[0] - 7, RECT[1] - 7, RECT[2] + 7, RECT[3] + 7)      # grown by 2, blurred over a radius of 5
    assert (x1 - x0) * 64 == (y1 - y0) * 64 and x0 <= hand["box"][0] - 8 and y1 >= hand["box"][3] + 8
    assert a["image"].shape == (2, 3, H0, W0) and a["image"].tobytes() == hand["final"].tobytes()
    # the latent, the mask and the latent mask are those of the pass
    for k in ("latent", "mask", "lmask"):
        assert a[k].tobytes() == hand["pass_"][k].tobytes(), k
    assert a["latent"].shape == (2, 4, 8, 8) and a["mask"].shape == (1, 1, 64, 64)
    p, orig = hand["p"][0, 0], hand["orig"]
    kept = np.broadcast_to(p == 0, a["image"].shape)
    assert (p == 0).sum() > 4000 and np.array_equal(a["image"][kept], np.broadcast_to(orig, a["image"].shape)[kept])      # kept pixels: the input's floats, exactly
    core = p >= np.float32(0.999)
    assert core.sum() > 100 and (p == 1).sum() >= 0
    changed = a["image"][:, :, core] != np.broadcast_to(orig, a["image"].shape)[:, :, core]
    assert changed.mean() > 0.9                                                          # repainted where p is 1
    assert not np.array_equal(a["image"][0], a["image"][1])                              # two seeds
    assert ", Inpaint area: masked, Padding: 8, Mask blur: 2, Mask grow: 2," in a["info"] and ", Mode: inpaint, f_t_ini: 0.6," in a["info"]
    assert f", Size: {W0}x{H0}," in a["info"] and "Mask invert" not in a["info"]


def test_masked_twice_gives_identical_bytes_and_the_offset_runs_on(lib, hand):
    a, c = masked_by_driver(lib, picture(), keep_mask())
    try:
        b = generate(lib, c)             # the same context again: the Philox offset ran on, so another image, in the same place
        assert b["region"] == a["region"] and b["image"].tobytes() != a["image"].tobytes()
        kept = np.broadcast_to(hand["p"][0, 0] == 0, a["image"].shape)
        assert np.array_equal(a["image"][kept], b["image"][kept])
    finally:
        c.close()
    a2, c2 = masked_by_driver(lib, picture(), keep_mask())
    c2.close()
    assert a2["image"].tobytes() == a["image"].tobytes() == hand["final"].tobytes()


def test_masked_with_a_downscale_filter_goes_through_resample_aa(lib, hand):
    h2 = masked_by_hand(lib, picture(), keep_mask(), filter=3, downscale_filter="lanczos")
    a, c = masked_by_driver(lib, picture(), keep_mask(), downscale_filter="lanczos")
    c.close()
    assert a["region"] == h2["region"] == hand["region"] and a["region"][2] - a["region"][0] < 64      # the way back shrinks
    assert a["image"].tobytes() == h2["final"].tobytes() and a["image"].tobytes() != hand["final"].tobytes()
    assert a["latent"].tobytes() == hand["pass_"]["latent"].tobytes()                      # the way in enlarges: the pass is the same
    assert ", Downscale filter: lanczos" in a["info"]


def test_masked_with_mask_invert_and_the_inverted_mask(lib, hand):
    a, c = masked_by_driver(lib, picture(), 255 - keep_mask(), mask_invert=1)
    c.close()
    assert a["image"].tobytes() == hand["final"].tobytes() and ", Mask invert: 1" in a["info"]


def test_whole_with_composite_equals_generate_and_composite_by_hand(lib):
    img, mask = picture(64, 64, seed=33), keep_mask(64, 64, (20, 12, 44, 36))
    c = context(lib, inpaint_composite=1, mask_blur=2, mask_grow=2)
    try:
        set_inputs(lib, c, img, mask)
        a = generate(lib, c)
    finally:
        c.close()
    c = context(lib)
    try:
        p = weight_by_hand(lib, c, mask, 2, 2.0)
        orig = as_library_tensor(img)
        set_tensor(lib, c, F.TENSOR["IMAGE"], orig)
        set_tensor(lib, c, F.TENSOR["MASK"], np.float32(1) - p)
        c.set("tensor_use_flags", F.TUF["IMAGE"] | F.TUF["MASK"]), c.set("f_t_ini", 0.6)
        g = generate(lib, c)
        final = IF.composite(lib, c, orig, g["image"], p, 0, 0)
    finally:
        c.close()
    assert a["done"] == 1 and a["region"] == (0, 0, 64, 64) and a["proc"] == (64, 64) and g["done"] == 0
    assert a["image"].tobytes() == final.tobytes() and a["latent"].tobytes() == g["latent"].tobytes() and a["image"].tobytes() != g["image"].tobytes()
    kept = np.broadcast_to(p[0, 0] == 0, final.shape)
    assert kept.any() and np.array_equal(a["image"][kept], np.broadcast_to(orig, final.shape)[kept])
    assert not np.array_equal(g["image"][kept], np.broadcast_to(orig, final.shape)[kept])      # the round trip through the VAE did not keep them
    assert ", Inpaint area: whole, Composite: 1, Mask blur: 2, Mask grow: 2," in a["info"]


def test_defaults_are_a_bypass(lib):
    img, mask = picture(64, 64, seed=34), keep_mask(64, 64, (20, 12, 44, 36))
    res = []
    for explicit in (False, True):
        c = context(lib)
        try:
            if explicit:
                c.set("inpaint_area", "whole"), c.set("inpaint_padding", 32), c.set("mask_blur", 0), c.set("mask_grow", 0), c.set("mask_invert", 0), c.set("inpaint_composite", 0)
            set_inputs(lib, c, img, mask)
            res.append(generate(lib, c))
        finally:
            c.close()
    a, b = res
    assert a["done"] == 0 and b["done"] == 0 and a["info"] == b["info"] and "Inpaint area" not in a["info"] and "Mask" not in a["info"].replace("Mode: inpaint", "")
    for k in ("latent", "image", "mask", "lmask"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["mask"].tobytes() == as_library_tensor(mask).tobytes()                       # the mask as given: no 1 - (1 - m)


def test_refusals_leave_a_usable_context(lib):
    c = context(lib, batch=1)
    try:
        def refused(text):
            c.tokens(TOKS), c.tokens(NTOKS, negative=True)
            r = lib.mlis_generate(c.ctx)
            assert r < 0 and text in c.err(), (r, c.err())
        c.set("inpaint_area", "masked")
        set_inputs(lib, c, picture(), None)
        refused("needs an input image (image) and a mask")                                 # masked without a mask
        set_inputs(lib, c, picture(), np.full((H0, W0, 1), 255, np.uint8))
        refused("nothing to repaint")                                                      # everything is kept
        set_inputs(lib, c, picture(), keep_mask())
        c.set("tiling", "xy")
        refused("not periodic")
        c.set("tiling", "none"), c.set("inpaint_area", "whole"), c.set("tensor_use_flags", 0), c.set("f_t_ini", 1)
        g = generate(lib, c)                                                               # the next plain generation
        assert g["image"].shape == (1, 3, 64, 64) and np.isfinite(g["image"]).all() and g["done"] == 0
        c.set("inpaint_area", "masked")
        set_inputs(lib, c, picture(), keep_mask())
        g = generate(lib, c)
        assert g["done"] == 1 and g["image"].shape == (1, 3, H0, W0)
    finally:
        c.close()


# ------------------------------------------------------------------ ControlNet
def test_control_image_is_cropped_to_the_region(lib, hand):
    import test_canny_gpu as TG
    import test_controlnet_gpu as TC
    arr = TG.source_map()                           # 96 x 80: taken to cover the 100 x 84 picture
    for area in ("masked", "whole"):
        c = TC.context(lib)
        try:
            TC.set_control_image(c, arr)
            img, mask = (picture(), keep_mask()) if area == "masked" else (picture(64, 64, seed=33), keep_mask(64, 64, (20, 12, 44, 36)))
            c.set("inpaint_area", area), c.set("inpaint_padding", 8), c.set("mask_blur", 2), c.set("mask_grow", 2)
            set_inputs(lib, c, img, mask)
            r = TC.run(lib, c)
            held = TG.held_map(lib, c)
            src = TG.as_library_tensor(arr)
            if area == "masked":
                box = (C.c_int * 4)()
                assert lib.mlis_amd_inpaint_info(c.ctx, box, None) == 1
                reg = tuple(box)
                assert reg == hand["region"]
                cx0, cy0, cx1, cy1 = R.control_rect(reg, W0, H0, 96, 80)
                assert (cx0, cy0, cx1, cy1) == (reg[0] * 96 // 100, reg[1] * 80 // 84, -(-reg[2] * 96 // 100), -(-reg[3] * 80 // 84))
                src = np.ascontiguousarray(src[:, :, cy0:cy1, cx0:cx1])
            want = IF.call_tensor(lib, c, lib.mlis_amd_tensor_resample, src, 64, 64, 1)[0]
            assert held.shape == (3, 64, 64) and held.tobytes() == want.tobytes(), area
            assert r["evals"][0] > 0 and np.isfinite(r["image"]).all()
            if area == "whole":
                assert held.tobytes() == TG.by_hand(lib, c, arr, 64, 64, plain=True).tobytes()      # no rectangle: today's path
        finally:
            c.close()
