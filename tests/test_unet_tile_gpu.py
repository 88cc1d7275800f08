"""Tiled diffusion on the GPU: the gather and blend kernels against numpy, the tiled engine against its own composition -- the float64 weighted
average of window-sized plain engines evaluated on the crops -- through mlis_amd_dxdt, the ring of windows under seamless tiling, and
mlis_generate with unet_tile: determinism, off == the old behaviour, composition with the other options, refusals, the callback.

Bound of the blend kernel, |err| <= 1e-6 max|eps| per element: at most 4 windows cover a pixel; each contributes one division, one multiply
and one add at fp32 eps 6e-8 with weights of at most 1, about 2.5e-7 in all; the bound is four times that.  (The weights themselves, rounded
quotients like 1/5, move a term by another 1e-7 of its size at most; the margin takes it.)  Where one window covers a pixel w / wsum is
exactly 1 and the canvas was zero: the result is the window's value, bit for bit.

Bound of the engine test, |err| <= (cfg + |1 - cfg|) 1e-6 max_j max|dx_j|: the window evaluations of the tiled engine are the plain engine's
plan on the same bytes, so only the blend's rounding differs, magnified by the coefficients of the CFG mix."""
import ctypes as C
import re

import numpy as np
import pytest

import mlis_ffi as F
import unet_tile_ffi as U

pytestmark = pytest.mark.gpu

TILE, OVERLAP = 64, 32              # pixels: 8 x 8 latent windows sharing 4


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return U.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ kernels
def gather(lib, x, ww, wh, x0, y0):
    from mlimgsynth_amd import _lib
    planes, H, W = x.shape
    src, dst = _lib.from_numpy(x), _lib.DeviceBuffer(planes * wh * ww * 4)
    assert lib.mlsd_window_gather(src.ptr, W, H, dst.ptr, ww, wh, x0, y0, planes, None) == 0
    return dst.download((planes, wh, ww), np.float32)


@pytest.mark.parametrize("planes", [1, 4, 8])
def test_gather_is_a_wrapped_copy(lib, planes):
    rng = np.random.default_rng(planes)
    for (H, W), (wh, ww), (y0, x0) in (((9, 7), (5, 3), (0, 0)), ((9, 7), (5, 3), (4, 4)), ((9, 7), (5, 3), (7, 6)), ((9, 7), (9, 7), (3, 2)),
                                       ((12, 12), (8, 8), (8, 8)), ((40, 33), (17, 20), (30, 25))):
        x = rng.standard_normal((planes, H, W)).astype(np.float32)
        x[0, 0, 0], x[-1, H - 1, W - 1], x[0, H // 2, W // 2], x[0, 1, 1] = np.inf, np.nan, -0.0, -np.inf
        x.view(np.uint32)[0, 2, 2] = 0x7fc12345                 # a NaN with a payload
        got = gather(lib, x, ww, wh, x0, y0)
        assert got.tobytes() == U.crop(x, x0, y0, ww, wh).tobytes(), (H, W, wh, ww, y0, x0)


def test_gather_refuses_bad_arguments(lib):
    from mlimgsynth_amd import _lib
    buf = _lib.DeviceBuffer(4 * 9 * 7 * 4 * 2)
    src, dst = buf.ptr, buf.ptr + 4 * 9 * 7 * 4
    call = lambda W=7, H=9, ww=3, wh=5, x0=0, y0=0, planes=4, s=src, d=dst: lib.mlsd_window_gather(s, W, H, d, ww, wh, x0, y0, planes, None)
    assert call() == 0
    for kw in (dict(W=0), dict(H=-1), dict(ww=0), dict(wh=0), dict(planes=0), dict(ww=8), dict(wh=10), dict(x0=-1), dict(x0=7), dict(y0=9), dict(y0=-2),
               dict(s=None), dict(d=None), dict(d=src), dict(d=src + 4 * 9 * 7 * 4 - 4), dict(W=65536, H=65536, ww=1, wh=1, planes=1),
               dict(W=40000, H=40000, ww=40000, wh=40000, planes=2)):
        assert call(**kw) < 0, kw
    from mlimgsynth_amd import kernels as K
    K.sync()


def run_blend(lib, eps_wins, wins, W, H, ww, wh, O, ld):
    """the engine's sequence: weight sums, a zeroed canvas, one blend launch per window in order"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    N = eps_wins[0].shape[0]
    xs, ys = sorted({w[0] for w in wins}), sorted({w[1] for w in wins})
    assert [(x, y) for y in ys for x in xs] == wins
    wsum = _lib.DeviceBuffer(H * W * 4)
    assert lib.mlsd_window_wsum(wsum.ptr, W, H, ww, wh, (C.c_int * len(xs))(*xs), len(xs), (C.c_int * len(ys))(*ys), len(ys), O, O, None) == 0
    canvas = _lib.from_numpy(np.zeros((N, H * W, 4), np.float32))
    keep = []
    for e, (x0, y0) in zip(eps_wins, wins):
        padded = np.full((N, wh * ww, ld), 1e30, np.float32)        # the columns past C belong to someone else: a stride slip would show
        padded[:, :, :4] = e
        keep.append(_lib.from_numpy(padded))
        assert lib.mlsd_window_blend(keep[-1].ptr, ld, canvas.ptr, wsum.ptr, W, H, ww, wh, x0, y0, O, O, N, 4, None) == 0
    K.sync()
    return canvas.download((N, H * W, 4), np.float32), wsum.download((H, W), np.float32)


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("tiling", [0, 3], ids=["open", "wrapped"])
def test_blend_against_float64(lib, tiling, ld):
    W = H = 12
    N, O = 4, 4
    wins, ww, wh = U.windows(W, H, 8, 8, O, tiling)
    assert len(wins) == (9 if tiling else 4)
    rng = np.random.default_rng(5 + ld + tiling)
    eps = [rng.standard_normal((N, wh * ww, 4)).astype(np.float32) for _ in wins]
    eps[1][2, 3 * ww + 5, 1] = 1e4                                   # an outlier
    got, wsum = run_blend(lib, eps, wins, W, H, ww, wh, O, ld)
    parts = [e.reshape(N, wh, ww, 4).transpose(0, 3, 1, 2) for e in eps]
    want, cnt = U.blend64(parts, wins, ww, wh, O, H, W)
    want = want.transpose(0, 2, 3, 1).reshape(N, H * W, 4)
    scale = max(np.abs(e).max() for e in eps)
    err = np.abs(got.astype(np.float64) - want).max() / scale
    print(f"blend tiling {tiling} ld {ld}: covers {cnt.min()}..{cnt.max()}, max|err| / max|eps| = {err:.3e}")
    assert cnt.max() <= 4 and np.isfinite(got).all()
    assert err <= 1e-6
    den = np.zeros((H, W))
    for x0, y0 in wins:
        iy, ix = np.ix_((np.arange(wh) + y0) % H, (np.arange(ww) + x0) % W)
        den[iy, ix] += U.weight(wh, ww, O, O)
    assert np.abs(wsum - den).max() <= 1e-6 * den.max()             # 4 terms of 3 roundings each and 3 additions at 6e-8
    single = (cnt == 1).reshape(-1)
    assert single.any() == (tiling == 0)
    if tiling == 0:                                                  # the four corners: one window each, the very value
        for e, (x0, y0) in zip(eps, wins):
            full = np.zeros((N, H, W, 4), np.float32)
            full[:, y0:y0 + wh, x0:x0 + ww] = e.reshape(N, wh, ww, 4)
            own = np.zeros((H, W), bool)
            own[y0:y0 + wh, x0:x0 + ww] = True
            own &= cnt == 1
            assert own.sum() == 16
            assert np.array_equal(got.reshape(N, H, W, 4)[:, own], full[:, own])
    again, _ = run_blend(lib, eps, wins, W, H, ww, wh, O, ld)
    assert again.tobytes() == got.tobytes()


def test_blend_refuses_bad_arguments(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    win, can, ws = _lib.DeviceBuffer(2 * 64 * 8 * 4), _lib.from_numpy(np.zeros((2, 144, 4), np.float32)), _lib.from_numpy(np.ones(144, np.float32))
    call = lambda e=win.ptr, ld=8, c=can.ptr, s=ws.ptr, W=12, H=12, ww=8, wh=8, x0=0, y0=0, ox=4, oy=4, N=2, Cn=4: \
        lib.mlsd_window_blend(e, ld, c, s, W, H, ww, wh, x0, y0, ox, oy, N, Cn, None)
    for kw in (dict(e=None), dict(c=None), dict(s=None), dict(ld=3), dict(W=0), dict(ww=13), dict(wh=0), dict(x0=12), dict(y0=-1), dict(ox=-1), dict(N=0),
               dict(Cn=3), dict(Cn=8), dict(c=can.ptr + 4), dict(e=can.ptr), dict(W=30000, H=30000, ww=1, wh=1)):
        assert call(**kw) < 0, kw
    K.sync()
    assert not can.download((2, 144, 4), np.float32).any()


# ------------------------------------------------------------------ engine
def conditioning(model, rng):
    from mlimgsynth_amd import engine as E
    P = E.unet_params(model)
    c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P.ch_adm_in) * 0.5).astype(np.float32)) if P.ch_adm_in else (lambda: None)
    return c(), l(), c(), l()


def engines(model, cfg, w, h, tiling=0, plain_tiling=0, seed=7):
    from mlimgsynth_amd import engine as E
    cond = conditioning(model, np.random.default_rng(seed))
    tiled = E.Generator(model, w, h, 2, cfg_scale=cfg, unet_tile=TILE, unet_tile_overlap=OVERLAP, tiling=tiling)
    plain = E.Generator(model, min(w, TILE), min(h, TILE), 2, cfg_scale=cfg, tiling=plain_tiling)
    for g in (tiled, plain):
        g.set_cond(*cond) if cfg > 1 else g.set_cond(cond[0], cond[1])
    return tiled, plain


def composition(tiled, plain, x, sigma, wins, ww, wh, O):
    H, W = x.shape[-2:]
    parts = [plain.dxdt(U.crop(x, x0, y0, ww, wh), sigma) for x0, y0 in wins]
    want, cnt = U.blend64(parts, wins, ww, wh, O, H, W)
    return parts, want, cnt


@pytest.mark.parametrize("cfg", [7.0, 1.0])
@pytest.mark.parametrize("model", ["tiny", "tinyv", "tinyxl"])
def test_tiled_engine_equals_its_composition(model, cfg):
    w = h = 96
    tiled, plain = engines(model, cfg, w, h)
    try:
        wins, ww, wh = U.windows(12, 12, 8, 8, 4)
        assert tiled.tile_info() == (4, 8, 8) and tiled.tile_windows() == wins == [(0, 0), (4, 0), (0, 4), (4, 4)]
        assert plain.tile_info() == (0, 8, 8) and plain.tile_windows() == []
        rng = np.random.default_rng(11)
        for sigma in (1.5, 12.0):
            x = (rng.standard_normal((2, 4, 12, 12)) * np.sqrt(1 + sigma * sigma)).astype(np.float32)
            got = tiled.dxdt(x, sigma)
            parts, want, cnt = composition(tiled, plain, x, sigma, wins, ww, wh, 4)
            scale = max(np.abs(p).max() for p in parts)
            bound = (cfg + abs(1 - cfg)) * 1e-6 * scale
            err = np.abs(got.astype(np.float64) - want).max()
            print(f"{model} cfg {cfg} sigma {sigma}: max|err| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
            assert np.isfinite(got).all() and err <= bound
            for p, (x0, y0) in zip(parts, wins):                    # corners: a single window
                own = np.zeros((12, 12), bool)
                own[y0:y0 + wh, x0:x0 + ww] = True
                own &= cnt == 1
                assert own.sum() == 16
                full = np.zeros_like(got)
                full[:, :, y0:y0 + wh, x0:x0 + ww] = p
                assert np.array_equal(got[:, :, own], full[:, :, own]), (x0, y0)
            assert np.array_equal(tiled.dxdt(x, sigma), got)
            assert not np.array_equal(got[0], got[1])
    finally:
        tiled.destroy(), plain.destroy()


def test_non_square_canvas_and_info():
    tiled, plain = engines("tiny", 7.0, 128, 64)
    try:
        wins, ww, wh = U.windows(16, 8, 8, 8, 4)
        assert tiled.tile_info() == (3, 8, 8) and tiled.tile_windows() == wins == [(0, 0), (4, 0), (8, 0)]
        x = (np.random.default_rng(12).standard_normal((2, 4, 8, 16)) * 3).astype(np.float32)
        got = tiled.dxdt(x, 3.0)
        parts, want, _ = composition(tiled, plain, x, 3.0, wins, ww, wh, 4)
        bound = 13e-6 * max(np.abs(p).max() for p in parts)
        err = np.abs(got - want).max()
        print(f"128x64: max|err| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        assert tiled.info()["unet_flops"] == 3 * plain.info()["unet_flops"]
    finally:
        tiled.destroy(), plain.destroy()


def test_ring_of_windows_under_tiling():
    from mlimgsynth_amd import engine as E
    x = (np.random.default_rng(13).standard_normal((2, 4, 8, 12)) * 3).astype(np.float32)
    sigma = 3.0
    ring, plain = engines("tiny", 7.0, 96, 64, tiling=1)
    try:
        assert ring.tile_info() == (3, 8, 8) and [w[0] for w in ring.tile_windows()] == [0, 4, 8]
        a = ring.dxdt(x, sigma)
        b = ring.dxdt(np.roll(x, 4, axis=-1), sigma)
        assert b.tobytes() == np.roll(a, 4, axis=-1).tobytes()        # the seam is nowhere: two covers per pixel, a two-term sum has no order
        wins, ww, wh = U.windows(12, 8, 8, 8, 4, 1)
        parts, want, cnt = composition(ring, plain, x, sigma, wins, ww, wh, 4)
        assert (cnt == 2).all()
        assert np.abs(a - want).max() <= 13e-6 * max(np.abs(p).max() for p in parts)
    finally:
        ring.destroy(), plain.destroy()
    open_, plain = engines("tiny", 7.0, 96, 64, tiling=0)
    try:
        assert open_.tile_info() == (2, 8, 8)
        assert not np.array_equal(open_.dxdt(x, sigma), a)
    finally:
        open_.destroy(), plain.destroy()
    # tiling y on this canvas: the window spans the whole y axis, so the plan itself wraps there
    ty, plain_y = engines("tiny", 7.0, 96, 64, tiling=2, plain_tiling=2)
    try:
        wins, ww, wh = U.windows(12, 8, 8, 8, 4, 2)
        assert ty.tile_windows() == wins == [(0, 0), (4, 0)]
        got = ty.dxdt(x, sigma)
        parts, want, _ = composition(ty, plain_y, x, sigma, wins, ww, wh, 4)
        assert np.abs(got - want).max() <= 13e-6 * max(np.abs(p).max() for p in parts)
        nowrap = E.Generator("tiny", 64, 64, 2, cfg_scale=7.0)
        try:
            nowrap.set_cond(*conditioning("tiny", np.random.default_rng(7)))
            assert not np.array_equal(nowrap.dxdt(U.crop(x, 0, 0, 8, 8), sigma), parts[0])
        finally:
            nowrap.destroy()
    finally:
        ty.destroy(), plain_y.destroy()


def test_create_tiled_falls_back_and_refuses():
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd._lib import MlsdError
    for tile in (64, 128, (64, 96)):
        g = E.Generator("tiny", 64, 64, 1, unet_tile=tile, unet_tile_overlap=32)
        assert g.tile_info() == (0, 8, 8)
        g.destroy()
    for tile, ov in ((60, 16), (64, 12), (64, 40), (64, -8)):
        with pytest.raises(MlsdError):
            E.Generator("tiny", 96, 96, 1, unet_tile=tile, unet_tile_overlap=ov)
    g = E.Generator("tiny", 96, 96, 1, unet_tile=64, unet_tile_overlap=0)      # no overlap: hard seams, still a partition
    assert g.tile_info() == (4, 8, 8) and g.tile_windows() == [(0, 0), (4, 0), (0, 4), (4, 4)]
    with pytest.raises(MlsdError, match="conditioning"):
        g.dxdt(np.zeros((1, 4, 12, 12), np.float32), 1.0)
    g.destroy()


@pytest.mark.parametrize("method", ["euler", "heun", "dpmpp2m"])
def test_tiled_denoise_runs_every_solver_family(method):
    """the fused Euler update, a two-evaluation solver and a multistep one read the blended output through the one accessor"""
    from mlimgsynth_amd import engine as E
    out = []
    for graph in (False, True):
        g = E.Generator("tiny", 96, 96, 2, n_step=3, method=method, unet_tile=TILE, unet_tile_overlap=OVERLAP, use_hipgraph=graph)
        try:
            g.set_cond(*conditioning("tiny", np.random.default_rng(7)))
            lat, _ = g.generate([1, 2], want_images=False)
            assert np.isfinite(lat).all() and g.last_nfe() >= 4
            out.append(lat)
        finally:
            g.destroy()
    assert out[0].tobytes() == out[1].tobytes()                         # a captured plan replays the same windows


# ------------------------------------------------------------------ mlis_generate
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
LONG_TOKS = (np.arange(100, dtype=np.int32) * 37 + 11) % 1000
STEPS = 4


def context(lib, model="tiny", dim=96, batch=2, unet_tile=None, overlap=OVERLAP, opts=()):
    m = F.Mlis(lib)
    m.set("model", f"synth:{model}")
    m.set("image_dim", dim, dim)
    m.set("steps", STEPS)
    m.set("seed", 42)
    m.set("cfg_scale", 7.0)
    m.set("method", "euler_a")
    m.set("batch_size", batch)
    if unet_tile is not None:
        m.set("unet_tile", unet_tile)
        m.set("unet_tile_overlap", overlap)
    for k, v in opts:
        m.set(k, *v) if isinstance(v, tuple) else m.set(k, v)
    return m


def prompt(m, long=False):
    m.tokens(LONG_TOKS if long else TOKS)
    m.tokens(NTOKS, negative=True)


def has_vae_tile_plan(lib, m):
    """whether the context's engine holds a tile-sized decoder plan (mlis_amd_ctx_at 3): vae_tile only tiles an image larger than one tile + margins"""
    lib.mlis_amd_engine_get.restype, lib.mlis_amd_engine_get.argtypes = C.c_void_p, [C.c_void_p]
    lib.mlis_amd_ctx_at.restype, lib.mlis_amd_ctx_at.argtypes = C.c_void_p, [C.c_void_p, C.c_int]
    eng = lib.mlis_amd_engine_get(m.ctx)
    return bool(eng and lib.mlis_amd_ctx_at(eng, 3))


def results(lib, m, decoded=True):
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]) if decoded else None,
                info=lib.mlis_infotext_get(m.ctx, 0).decode(), builds=lib.mlis_amd_engine_builds(m.ctx), vae_tiled=has_vae_tile_plan(lib, m))


def generate(lib, setup=None, long=False, decoded=True, **kw):
    m = context(lib, **kw)
    try:
        prompt(m, long)
        if setup:
            setup(m)
        m.generate()
        return results(lib, m, decoded)
    finally:
        m.close()


def nfe_of(info):
    return int(re.search(r"NFE: (\d+)", info).group(1))


def same(a, b):
    return a["latent"].tobytes() == b["latent"].tobytes() and (a["image"] is None or a["image"].tobytes() == b["image"].tobytes())


_plain = {}


def plain96(lib):
    if "r" not in _plain:
        _plain["r"] = generate(lib)
    return _plain["r"]


def test_generate_is_deterministic_and_tiled(lib):
    a, b = generate(lib, unet_tile=TILE), generate(lib, unet_tile=TILE)
    assert a["latent"].shape == (2, 4, 12, 12) and a["image"].shape == (2, 3, 96, 96)
    assert np.isfinite(a["latent"]).all() and np.isfinite(a["image"]).all()
    assert same(a, b) and a["info"] == b["info"] and a["builds"] == 1
    base = plain96(lib)
    assert not np.array_equal(a["latent"], base["latent"])
    clause = f", Tiled diffusion: {TILE}, Tile overlap: {OVERLAP}"
    assert clause + ", Version: " in a["info"] and "Tiled diffusion" not in base["info"]
    assert a["info"].replace(clause, "") == base["info"]                  # NFE, steps and size included
    assert nfe_of(a["info"]) == nfe_of(base["info"]) == 2 * STEPS
    auto = generate(lib, unet_tile=TILE, overlap=-1)
    assert f", Tiled diffusion: {TILE}, Tile overlap: 16, Version: " in auto["info"]
    assert not np.array_equal(auto["latent"], a["latent"])


@pytest.mark.parametrize("tile", [0, 96, 128])
def test_off_is_the_old_behaviour(lib, tile):
    base, off = plain96(lib), generate(lib, unet_tile=tile)
    assert same(off, base) and off["info"] == base["info"] and off["builds"] == base["builds"] == 1


def hires_opts(m):
    m.set("hires_scale", 1.5), m.set("hires_denoise", 0.6), m.set("hires_steps", 3)


def img2img_mask(m):
    rgba = np.random.default_rng(3).integers(0, 256, (96, 96, 4), dtype=np.uint8)
    rgba[:, :48, 3], rgba[:, 48:, 3] = 255, 0
    im = F.Image(rgba.ctypes.data_as(C.POINTER(C.c_uint8)), rgba.size, 96, 96, 4, 0)
    assert m.lib.mlis_option_set(m.ctx, F.OPT["IMAGE"], C.byref(im)) == 1, m.err()
    m.set("f_t_ini", 0.6)


COMPOSE = {
    "hires": dict(dim=64, setup=hires_opts),
    "tae": dict(opts=(("tae", "synth"),)),
    "vae_tile": dict(opts=(("vae_tile", 32),)),                     # 96 x 96 is one VAE tile: the option is taken, the decode is the untiled one
    "vae_tile_256": dict(dim=256, opts=(("vae_tile", 64),)),        # 32 x 32 latent: 2 x 2 VAE tiles of 24 decode the canvas the UNet windows blended
    "unet_split": dict(opts=(("unet_split", 1),)),
    "long_prompt": dict(long=True),
    "img2img_mask": dict(setup=img2img_mask),
    "no_decode": dict(opts=(("no_decode", 1),), decoded=False),
    "tiling_x": dict(opts=(("tiling", "x"),)),
}


@pytest.mark.parametrize("name", list(COMPOSE))
def test_composes_with_the_other_options(lib, name):
    kw = COMPOSE[name]
    a, b = generate(lib, unet_tile=TILE, **kw), generate(lib, unet_tile=TILE, **kw)
    lat = 32 if name == "vae_tile_256" else 12
    assert a["latent"].shape == (2, 4, lat, lat) and np.isfinite(a["latent"]).all()
    if a["image"] is not None:
        assert a["image"].shape == (2, 3, 8 * lat, 8 * lat) and np.isfinite(a["image"]).all()
    assert a["vae_tiled"] == b["vae_tiled"] == (name == "vae_tile_256")
    assert same(a, b) and a["info"] == b["info"]
    assert f", Tiled diffusion: {TILE}, Tile overlap: {OVERLAP}, Version: " in a["info"]
    assert a["builds"] == (2 if name == "hires" else 1)                   # hires: the first pass fits the tile and runs on the plain engine
    off = generate(lib, **kw)
    assert not np.array_equal(off["latent"], a["latent"]) and "Tiled diffusion" not in off["info"]
    if name == "hires":
        assert nfe_of(a["info"]) == nfe_of(off["info"])


def test_lora_change_reaches_the_tiled_engine(lib, tmp_path):
    """an adapter switched on between two generations is patched into the resident tiled engine; the result is a fresh context's"""
    import loader_cases as LC
    import lora_ffi as LF
    import test_lora_gpu as TL
    (tmp_path / "loras" / "tiny").mkdir(parents=True)
    files = dict(loras=str(tmp_path / "loras"), tiny=str(tmp_path / "tiny.safetensors"))
    LC.write_checkpoint(files["tiny"], "tiny", "F16")
    TL.write_model_adapter(str(tmp_path / "loras" / "tiny" / "style.safetensors"), "tiny", 21)
    llib = LF.bind(lib._name)
    opts = (("image_dim", (96, 96)), ("unet_tile", TILE), ("unet_tile_overlap", OVERLAP))
    w = TL.Warm(llib, files, "tiny", opts)
    try:
        assert w.equals_cold(())
        assert w.equals_cold((("style", 0.75),))
        assert w.builds() == 1 and w.stats()[1] > 0 and w.stats()[2] == 0
        assert "Tiled diffusion: 64" in llib.mlis_infotext_get(w.m.ctx, 0).decode()
        assert not TL.same(TL.cold(llib, files, "tiny", opts, (("style", 0.75),), 1), TL.cold(llib, files, "tiny", opts, (), 1))
    finally:
        w.m.close()


def test_refusals(lib):
    m = context(lib)
    try:
        for name, bad in (("unet_tile", 60), ("unet_tile", -8), ("unet_tile_overlap", 12), ("unet_tile_overlap", -16)):
            assert lib.mlis_option_set_str(m.ctx, name.encode(), str(bad).encode()) == -4, (name, bad)
            assert name in m.err()
        m.set("unet_tile", TILE), m.set("unet_tile_overlap", 40)          # each is fine alone
        prompt(m)
        assert lib.mlis_generate(m.ctx) == -4
        assert "unet_tile_overlap" in m.err() and "unet_tile 64" in m.err()
        assert lib.mlis_amd_engine_builds(m.ctx) == 0
        m.set("unet_tile_overlap", 32)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 1
    finally:
        m.close()


def test_callback_counts_steps_not_windows(lib):
    seen = []

    def cb(ud, ctx, p):
        seen.append((p.contents.stage, p.contents.step, p.contents.step_end, p.contents.nfe))
        return 0

    thunk = F.CALLBACK(cb)
    m = context(lib, unet_tile=TILE)
    try:
        assert lib.mlis_option_set(m.ctx, F.OPT["CALLBACK"], thunk, C.c_void_p(None)) == 1
        prompt(m)
        m.generate()
        den = [s for s in seen if s[0] == 4]
        assert [s[1] for s in den] == list(range(1, STEPS + 1)) and all(s[2] == STEPS for s in den)
        assert [s[3] for s in den] == [2 * (i + 1) for i in range(STEPS)]
        assert m.tensor(F.TENSOR["LATENT"]).tobytes() == generate(lib, unet_tile=TILE)["latent"].tobytes()
    finally:
        m.close()
