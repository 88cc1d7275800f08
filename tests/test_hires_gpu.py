"""Hires fix on the GPU: the resampling kernel against torch in float64 per element (clamped and wrapped taps), the public resampling call,
and the two-pass mlis_generate against its own manual composition through the public API -- generate (NO_DECODE), mlis_amd_tensor_resample,
generate (MLIS_TUF_LATENT) on a fresh context with the same seed -- which takes the same kernels, plans and Philox offsets: bit-identical.

The bound of the bilinear / bicubic kernel, max |err| <= 1e-5 max |x| per plane: fp32 eps 6e-8, about 26 rounded operations per output (16 taps
plus the weight polynomials), tap weight abs-sum <= 1.6 for a = -0.75 give ~2.5e-6; the bound is four times that.  nearest and equal-size
calls are bit-exact."""
import ctypes as C
import re

import numpy as np
import pytest

import hires_ffi as H
import mlis_ffi as F

pytestmark = pytest.mark.gpu

BOUND = 1e-5
SIZES = [((8, 8), (12, 12)), ((7, 9), (14, 27)), ((1, 5), (3, 5)), ((64, 64), (96, 96)), ((128, 128), (256, 256))]
SIZE_IDS = ["8x8-12x12", "7x9-14x27", "1x5-3x5", "64x64-96x96", "128x128-256x256"]


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return H.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ kernel
def planes_data(rng, planes, sh, sw, outlier):
    x = rng.standard_normal((planes, sh, sw)).astype(np.float32)
    if outlier:
        x[-1, sh // 2, sw // 3] = 1e4
    return x


def run_kernel(x, dh, dw, mode, wrap=0):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    planes, sh, sw = x.shape
    src = _lib.from_numpy(x)
    dst = _lib.DeviceBuffer(planes * dh * dw * 4)
    K.resample2d(src.ptr, sw, sh, dst.ptr, dw, dh, planes, mode, wrap)
    K.sync()
    return dst.download((planes, dh, dw), np.float32)


def check(got, x, want, exact, what):
    """every element of got against the float64 reference; per plane max |err| / max |x|"""
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - want).max(axis=(1, 2)) / np.abs(x).max(axis=(1, 2))
    print(f"{what}: worst max|err| / max|x| over the planes = {err.max():.3e}")
    if exact:
        assert np.array_equal(got.astype(np.float64), want), what
    else:
        assert (err <= BOUND).all(), (what, err.max())


@pytest.mark.parametrize("planes", [1, 4, 16])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("mode", range(3), ids=H.MODES)
def test_kernel_against_torch_float64(mode, size, planes):
    (sh, sw), (dh, dw) = size
    rng = np.random.default_rng(100 * mode + planes)
    for outlier in ((False, True) if planes == 1 else (True,)):         # one plane carries the 1e4 outlier, the others are plain normal data
        x = planes_data(rng, planes, sh, sw, outlier)
        what = f"{H.MODES[mode]} {sh}x{sw}->{dh}x{dw} planes {planes} outlier {outlier}"
        check(run_kernel(x, dh, dw, mode), x, H.torch64(x, dh, dw, mode), mode == 0, what)
        same = run_kernel(x, sh, sw, mode)                               # equal sizes: an exact copy
        assert same.tobytes() == x.tobytes(), what
        check(same, x, H.torch64(x, sh, sw, mode), True, what + " (equal size)")


def test_kernel_copies_special_values_at_equal_size():
    x = np.array([[[0.0, -0.0, np.inf], [-np.inf, np.nan, 1e-45]]], np.float32)
    for mode in range(3):
        assert run_kernel(x, 2, 3, mode).tobytes() == x.tobytes()


def test_kernel_refuses_bad_arguments():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    buf = _lib.DeviceBuffer(4096)
    out = _lib.DeviceBuffer(4096)
    v = C.c_void_p
    for sw, sh, dw, dh, planes, mode, wrap in ((0, 4, 4, 4, 1, 1, 0), (4, 4, 0, 4, 1, 1, 0), (4, 4, 4, 4, 0, 1, 0), (4, 4, 4, 4, 1, 3, 0), (4, 4, 4, 4, 1, 1, 4)):
        assert L.mlsd_resample2d(v(buf.ptr), sw, sh, v(out.ptr), dw, dh, planes, mode, wrap, None) < 0
    assert L.mlsd_resample2d(v(buf.ptr), 4, 4, v(buf.ptr + 16), 8, 8, 1, 1, 0, None) < 0      # overlap
    big = (1 << 22) + 1             # MLSD_RESAMPLE_MAX_EXTENT + 1: refused before any launch, the fraction would no longer stay below 1
    for sw, sh, dw, dh in ((big, 1, 4, 1), (1, big, 1, 4), (4, 1, big, 1), (1, 4, 1, big)):
        assert L.mlsd_resample2d(v(buf.ptr), sw, sh, v(out.ptr), dw, dh, 1, 1, 0, None) < 0


@pytest.mark.parametrize("wrap", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("mode", range(3), ids=H.MODES)
def test_kernel_wrap_against_circularly_padded_torch(mode, size, wrap):
    (sh, sw), (dh, dw) = size
    rng = np.random.default_rng(1000 + 10 * mode + wrap)
    x = planes_data(rng, 4, sh, sw, True)
    x[-1, 0, sw - 1] = -1e4                                              # a second outlier in a corner: it must come around the edge
    what = f"{H.MODES[mode]} {sh}x{sw}->{dh}x{dw} wrap {wrap}"
    check(run_kernel(x, dh, dw, mode, wrap), x, H.torch64(x, dh, dw, mode, wrap), mode == 0, what)


@pytest.mark.parametrize("size", SIZES[3:], ids=SIZE_IDS[3:])
@pytest.mark.parametrize("mode", [1, 2], ids=H.MODES[1:])
def test_wrap_changes_the_border_only(mode, size):
    (sh, sw), (dh, dw) = size
    x = planes_data(np.random.default_rng(5), 4, sh, sw, False)
    y0, y3 = run_kernel(x, dh, dw, mode, 0), run_kernel(x, dh, dw, mode, 3)
    m = 3 * -(-dh // sh)            # bicubic taps reach two source pixels: 2 s output pixels, with room
    assert y0[:, m:-m, m:-m].tobytes() == y3[:, m:-m, m:-m].tobytes()
    for edge in (y0[:, 0] != y3[:, 0], y0[:, -1] != y3[:, -1], y0[:, :, 0] != y3[:, :, 0], y0[:, :, -1] != y3[:, :, -1]):
        assert edge.mean() > 0.9
    y1 = run_kernel(x, dh, dw, mode, 1)                                  # columns only: the first and last rows are the clamped ones
    assert y1[:, :, m:-m].tobytes() == y0[:, :, m:-m].tobytes() and y1[:, m:-m].tobytes() == y3[:, m:-m].tobytes()


# ------------------------------------------------------------------ public resampling call
def as_tensor(x):
    b, c, h, w = x.shape
    return F.Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, b), 0)


@pytest.mark.parametrize("mode", range(3), ids=H.MODES)
def test_public_call_equals_the_kernel_and_follows_tiling(lib, mode):
    x = np.random.default_rng(3).standard_normal((2, 4, 8, 10)).astype(np.float32)
    m = F.Mlis(lib)
    try:
        for tiling, wrap in ((None, 0), ("xy", 3), ("x", 1), ("y", 2), ("none", 0)):
            if tiling:
                m.set("tiling", tiling)
            out = F.Tensor()
            assert lib.mlis_amd_tensor_resample(m.ctx, C.byref(as_tensor(x)), C.byref(out), 15, 12, mode) == 1, m.err()
            assert [out.n[i] for i in range(4)] == [15, 12, 4, 2]
            got = F.tensor_np(out)
            lib.mlis_tensor_free(C.byref(out))
            want = run_kernel(x.reshape(8, 8, 10), 12, 15, mode, wrap).reshape(2, 4, 12, 15)
            assert got.tobytes() == want.tobytes(), (tiling, mode)
        # in place, on one of the context's own tensors
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["LATENT"])
        lib.mlis_tensor_resize(t, 10, 8, 4, 2)
        C.memmove(t.contents.d, x.ctypes.data, x.nbytes)
        assert lib.mlis_amd_tensor_resample(m.ctx, t, t, 20, 16, mode) == 1, m.err()
        assert m.tensor(F.TENSOR["LATENT"]).tobytes() == run_kernel(x.reshape(8, 8, 10), 16, 20, mode).tobytes()
    finally:
        m.close()
    # the Python wrapper's method
    from mlimgsynth_amd import mlimgsynth as W
    with W.MLImgSynth() as s:
        s.option_set("tiling", "xy")
        out = s.tensor_resample(W.tensor_from_numpy(x), 15, 12, mode)
        assert out.n == (15, 12, 4, 2)
        assert out.numpy().tobytes() == run_kernel(x.reshape(8, 8, 10), 12, 15, mode, 3).tobytes()


# ------------------------------------------------------------------ the two-pass generation
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
LONG_TOKS = (np.arange(100, dtype=np.int32) * 37 + 11) % 1000
STEPS, DENOISE = 4, 0.6


def context(lib, model="tiny", batch=1, cfg=7.0, tiling=None, tae=False, vae_tile=0, unet_split=False, seed=42, dim=64, **_):
    m = F.Mlis(lib)
    m.set("model", f"synth:{model}")
    m.set("image_dim", dim, dim)
    m.set("steps", STEPS)
    m.set("seed", seed)
    m.set("cfg_scale", cfg)
    m.set("method", "euler_a")                       # ancestral: every step draws noise, so the Philox offsets of the two passes matter
    if batch > 1:
        m.set("batch_size", batch)
    if tiling:
        m.set("tiling", tiling)
    if tae:
        m.set("tae", "synth")
    if vae_tile:
        m.set("vae_tile", vae_tile)
    if unet_split:
        m.set("unet_split", 1)
    return m


def prompt(m, cfg=7.0, long=False, **_):
    m.tokens(LONG_TOKS if long else TOKS)
    if cfg > 1:
        m.tokens(NTOKS, negative=True)


def target(l, s):
    return int(np.floor(l * s + 0.5))


def has_vae_tile_plan(lib, m):
    """whether the engine of the last pass holds a tile-sized decoder plan (mlis_amd_ctx_at 3): vae_tile only tiles an image larger than one tile + margins"""
    lib.mlis_amd_engine_get.restype, lib.mlis_amd_engine_get.argtypes = C.c_void_p, [C.c_void_p]
    lib.mlis_amd_ctx_at.restype, lib.mlis_amd_ctx_at.argtypes = C.c_void_p, [C.c_void_p, C.c_int]
    eng = lib.mlis_amd_engine_get(m.ctx)
    return bool(eng and lib.mlis_amd_ctx_at(eng, 3))


def results(lib, m, decoded=True):
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]) if decoded else None,
                info=lib.mlis_infotext_get(m.ctx, 0).decode(), builds=lib.mlis_amd_engine_builds(m.ctx), vae_tiled=has_vae_tile_plan(lib, m))


def nfe_of(info):
    return int(re.search(r"NFE: (\d+)", info).group(1))


def hires_generate(lib, scale, upscaler, hires_steps=0, **kw):
    m = context(lib, **kw)
    try:
        m.set("hires_scale", scale)
        m.set("hires_denoise", DENOISE)
        m.set("hires_steps", hires_steps)
        m.set("hires_upscaler", upscaler)
        prompt(m, **kw)
        m.generate()
        return results(lib, m)
    finally:
        m.close()


def manual_generate(lib, scale, upscaler, hires_steps=0, resample_tiling=None, **kw):
    """the same through the public API, step by step"""
    m = context(lib, **kw)
    try:
        prompt(m, **kw)
        m.set("no_decode", 1)
        m.generate()
        nfe1 = nfe_of(lib.mlis_infotext_get(m.ctx, 0).decode())
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["LATENT"])
        lw, lh = t.contents.n[0], t.contents.n[1]
        if resample_tiling:
            m.set("tiling", resample_tiling)
        assert lib.mlis_amd_tensor_resample(m.ctx, t, t, target(lw, scale), target(lh, scale), H.MODES.index(upscaler)) == 1, m.err()
        if resample_tiling:
            m.set("tiling", kw["tiling"])
        prompt(m, **kw)
        m.set("no_decode", 0)
        m.set("tensor_use_flags", F.TUF["LATENT"])
        m.set("f_t_ini", DENOISE)
        if hires_steps:
            m.set("steps", hires_steps)
        m.generate()
        r = results(lib, m)
        r["nfe"] = (nfe1, nfe_of(r["info"]))
        return r
    finally:
        m.close()


def assert_same(a, b, what):
    assert a["latent"].shape == b["latent"].shape and a["image"].shape == b["image"].shape, what
    assert a["latent"].tobytes() == b["latent"].tobytes(), (what, "latent", np.abs(a["latent"] - b["latent"]).max())
    assert a["image"].tobytes() == b["image"].tobytes(), (what, "image", np.abs(a["image"] - b["image"]).max())


MODELS = [dict(model="tiny", scale=1.5, batch=1), dict(model="tiny", scale=1.5, batch=2), dict(model="tinyxl", scale=2, batch=1),
          dict(model="tinyv", scale=1.5, batch=1)]


@pytest.mark.parametrize("upscaler", H.MODES)
@pytest.mark.parametrize("cfg", [7.0, 1.0])
@pytest.mark.parametrize("case", MODELS, ids=lambda c: f"{c['model']}-b{c['batch']}")
def test_hires_equals_its_manual_composition(lib, case, cfg, upscaler):
    kw = dict(case, cfg=cfg, upscaler=upscaler, hires_steps=3 if cfg > 1 else 0)
    h, man = hires_generate(lib, **kw), manual_generate(lib, **kw)
    lat = target(8, case["scale"])
    assert h["latent"].shape == (case["batch"], 4, lat, lat) and h["image"].shape == (case["batch"], 3, 8 * lat, 8 * lat)
    assert_same(h, man, kw)
    assert nfe_of(h["info"]) == sum(man["nfe"])
    assert h["builds"] == 2 and man["builds"] == 2
    if case["batch"] == 2:
        assert not np.array_equal(h["latent"][0], h["latent"][1])


@pytest.mark.parametrize("extra", [dict(tae=True), dict(vae_tile=32), dict(unet_split=True), dict(long=True), dict(tae=True, vae_tile=32, tiling="xy"),
                                   dict(vae_tile=64, dim=128, scale=2)],
                         ids=["tae", "vae_tile", "unet_split", "long_prompt", "tae_tiling", "vae_tile_256"])
def test_hires_composes_with_the_other_options(lib, extra):
    """vae_tile 32 at 96 x 96 is one VAE tile (the option is taken, the decode is the untiled one); 128 -> 256 x 256 at vae_tile 64 decodes the second pass in 2 x 2 tiles"""
    kw = dict(dict(model="tiny", scale=1.5, batch=2, cfg=7.0, upscaler="bicubic", hires_steps=3), **extra)
    h, man = hires_generate(lib, **kw), manual_generate(lib, **kw)
    assert_same(h, man, extra)
    assert h["vae_tiled"] == man["vae_tiled"] == (extra.get("dim") == 128)
    if extra.get("dim") == 128:
        assert h["image"].shape == (2, 3, 256, 256)


def test_hires_wraps_under_tiling(lib):
    kw = dict(model="tiny", scale=1.5, batch=1, cfg=7.0, upscaler="bilinear", tiling="xy")
    h = hires_generate(lib, **kw)
    assert_same(h, manual_generate(lib, **kw), "tiling xy")
    assert ", Tiling: xy" in h["info"]
    unwrapped = manual_generate(lib, resample_tiling="none", **kw)
    assert not np.array_equal(h["latent"], unwrapped["latent"])
    assert not np.array_equal(h["latent"], hires_generate(lib, **dict(kw, tiling=None))["latent"])


def plain_generate(lib, hires_scale=None, **kw):
    m = context(lib, **kw)
    try:
        if hires_scale is not None:
            m.set("hires_scale", hires_scale)
        prompt(m, **kw)
        m.generate()
        return results(lib, m)
    finally:
        m.close()


def test_off_is_the_old_behaviour(lib):
    base = plain_generate(lib)
    for s in (0, 1, "0", "1.0"):
        off = plain_generate(lib, hires_scale=s)
        assert off["image"].tobytes() == base["image"].tobytes() and off["latent"].tobytes() == base["latent"].tobytes(), s
        assert off["info"] == base["info"] and off["builds"] == 1, s
    assert "Hires" not in base["info"] and "Denoising strength" not in base["info"]
    on = hires_generate(lib, 1.5, "bicubic", hires_steps=3)
    clause = ", Hires upscale: 1.5, Hires steps: 3, Hires upscaler: bicubic, Denoising strength: 0.6"
    assert clause + ", Version: " in on["info"]
    assert ", Size: 96x96," in on["info"] and ", Size: 64x64," in base["info"]
    norm = lambda s: re.sub(r"(Size: \d+x\d+|NFE: \d+|Steps: \d+)", "#", s)
    assert norm(on["info"].replace(clause, "")) == norm(base["info"])
    assert "Mode:" not in on["info"]
    # hires_steps 0: the STEPS value
    assert f", Hires steps: {STEPS}," in hires_generate(lib, 1.5, "nearest")["info"]


def test_options_persist_and_the_rest_is_reset(lib):
    m = context(lib)
    try:
        m.set("hires_scale", 1.5), m.set("hires_denoise", DENOISE), m.set("hires_steps", 3), m.set("hires_upscaler", "nearest")
        for _ in range(2):
            prompt(m)
            m.generate()
            assert [H.get(lib, m, o) for o in (H.HIRES_SCALE, H.HIRES_DENOISE, H.HIRES_STEPS, H.HIRES_UPSCALER)] == [1.5, np.float32(DENOISE), 3, 0]
            info = lib.mlis_infotext_get(m.ctx, 0).decode()
            assert f", Steps: {STEPS}," in info and "Hires steps: 3" in info and "f_t_ini" not in info
            assert m.tensor(F.TENSOR["LATENT"]).shape == (1, 4, 12, 12)
        # the prompt was cleared after the second pass, not after the first
        p = C.c_char_p()
        assert lib.mlis_option_get(m.ctx, F.OPT["PROMPT"], C.byref(p)) == 1 and p.value == b""
    finally:
        m.close()


def test_engine_slots(lib):
    m = context(lib)
    try:
        assert lib.mlis_amd_engine_builds(m.ctx) == 0
        m.set("hires_scale", 1.5)
        for _ in range(2):
            prompt(m)
            m.generate()
            assert lib.mlis_amd_engine_builds(m.ctx) == 2           # 8x8 and 12x12, both kept
        m.set("hires_scale", 2)
        prompt(m)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 3               # 16x16 takes the place of 12x12; 8x8 was used after it
        m.set("hires_scale", 0)
        prompt(m)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 3               # plain txt2img at the base size
        assert m.tensor(F.TENSOR["LATENT"]).shape == (1, 4, 8, 8)
        lib.mlis_amd_engine_get.restype = C.c_void_p
        lib.mlis_amd_engine_get.argtypes = [C.c_void_p]
        assert lib.mlis_amd_engine_get(m.ctx)
        m.set("hires_scale", 1.5)                                    # 12x12 again: the third slot does not exist
        prompt(m)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 4
    finally:
        m.close()


def test_repeated_hires_generations_are_deterministic(lib):
    """the second generation of a context runs on the two kept engines and continues the Philox streams: two contexts agree on it"""
    out = []
    for _ in range(2):
        m = context(lib, batch=2)
        try:
            m.set("hires_scale", 1.5)
            for _ in range(2):
                prompt(m)
                m.generate()
            out.append(results(lib, m))
        finally:
            m.close()
    assert_same(out[0], out[1], "second generation")


def test_refusals(lib):
    rgb = np.zeros((64, 64, 3), np.uint8)
    mono = np.full((64, 64, 1), 255, np.uint8)

    def refused(setup, *names):
        m = context(lib)
        try:
            m.set("hires_scale", 1.5)
            prompt(m)
            setup(m)
            assert lib.mlis_generate(m.ctx) == -4, m.err()
            for n in ("hires_scale",) + names:
                assert n in m.err(), (n, m.err())
            assert lib.mlis_amd_engine_builds(m.ctx) == 0
        finally:
            m.close()

    def image_opt(opt, arr):
        def f(m):
            im = F.Image(arr.ctypes.data_as(C.POINTER(C.c_uint8)), arr.size, 64, 64, arr.shape[2], 0)
            assert lib.mlis_option_set(m.ctx, F.OPT[opt], C.byref(im)) == 1, m.err()
        return f

    def latent(m):
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["LATENT"])
        lib.mlis_tensor_resize(t, 8, 8, 4, 1)
        C.memset(t.contents.d, 0, 8 * 8 * 4 * 4)
        m.set("tensor_use_flags", F.TUF["LATENT"])

    def lmask(m):
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["LMASK"])
        lib.mlis_tensor_resize(t, 8, 8, 1, 1)
        C.memset(t.contents.d, 0, 8 * 8 * 4)
        m.set("tensor_use_flags", F.TUF["LMASK"])

    refused(image_opt("IMAGE", rgb), "image")
    refused(latent, "latent", "tensor_use_flags")
    refused(image_opt("IMAGE_MASK", mono), "image_mask")
    refused(lmask, "lmask", "tensor_use_flags")


def test_callback_sees_two_denoise_sequences(lib):
    DENOISE_STAGE, DECODE_STAGE = 4, 3
    kw = dict(model="tiny", scale=1.5, batch=1, cfg=7.0, upscaler="bilinear", hires_steps=3)

    def run(abort_in_second=0):
        seen = []

        def cb(ud, ctx, p):
            p = p.contents
            seen.append((p.stage, p.step, p.step_end, p.nfe))
            seqs = sum(1 for s in seen if s[0] == DENOISE_STAGE and s[1] == 1)
            return abort_in_second if (abort_in_second and p.stage == DENOISE_STAGE and seqs == 2) else 0

        thunk = F.CALLBACK(cb)
        m = context(lib, **kw)
        try:
            m.set("hires_scale", kw["scale"]), m.set("hires_denoise", DENOISE), m.set("hires_steps", 3)
            assert lib.mlis_option_set(m.ctx, F.OPT["CALLBACK"], thunk, C.c_void_p(None)) == 1
            prompt(m, **kw)
            r = lib.mlis_generate(m.ctx)
            return r, seen, (None if r < 0 else m.tensor(F.TENSOR["LATENT"]))
        finally:
            m.close()

    r, seen, latent = run()
    assert r == 1
    den = [s for s in seen if s[0] == DENOISE_STAGE]
    starts = [i for i, s in enumerate(den) if s[1] == 1]
    assert len(starts) == 2, den
    first, second = den[:starts[1]], den[starts[1]:]
    assert [s[1] for s in first] == list(range(1, STEPS + 1)) and first[-1][2] == STEPS
    assert [s[1] for s in second] == list(range(1, second[-1][2] + 1)) and 1 <= second[-1][2] <= 3
    nfes = [s[3] for s in den]
    assert nfes == sorted(nfes) and second[0][3] > first[-1][3]           # the count runs on through the second pass
    man = manual_generate(lib, **kw)
    assert first[-1][3] == man["nfe"][0] and second[-1][3] == sum(man["nfe"])
    assert seen[-1][0] == DECODE_STAGE and seen[-1][3] == sum(man["nfe"])
    assert sum(1 for s in seen if s[0] == DECODE_STAGE) == 1                  # the first pass is never decoded
    assert latent.tobytes() == man["latent"].tobytes()                       # (a callback does not change the result)
    r, seen, _ = run(abort_in_second=-77)
    assert r == -77
    assert sum(1 for s in seen if s[0] == DENOISE_STAGE and s[1] == 1) == 2 and not any(s[0] == DECODE_STAGE for s in seen)
