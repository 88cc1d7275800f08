"""Packed tiled diffusion on the GPU: the packed gather and blend kernels against numpy and against the single-window launches they replace, the
packed engine against its own composition -- the float64 weighted average of a plain engine of batch P B evaluated on the stacked crops -- through
mlis_amd_dxdt, and mlis_generate with unet_tile_batch: determinism, pack 1 == the old behaviour, composition with the other options, the callback,
the engine cache.

The packed blend is held to the bytes of successive mlsd_window_blend launches in slot order: one thread per canvas pixel performs the very
operations of those launches in their order, so there is no tolerance to state.  The engine tests keep the bound of test_unet_tile_gpu.py,
|err| <= (cfg + |1 - cfg|) 1e-6 max_j max|dx_j|: the packed plan is the plain engine's batch-P B plan on the same bytes, so only the blend's
rounding differs.  Packed against unpacked compares two plans of different batch: each is within tolerances.EVAL_SMALL of the oracle (the bound the
project states for evaluations at test-sized latents, whatever the batch), so they are within twice that of each other; likewise 2 LATENT for
whole generations."""
import ctypes as C

import numpy as np
import pytest

import mlis_ffi as F
import test_unet_tile_gpu as T
import tolerances
import unet_tile_ffi as U
import unet_tile_pack_ffi as UP

pytestmark = pytest.mark.gpu

TILE, OVERLAP = T.TILE, T.OVERLAP


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return UP.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ kernels
GATHER_CASES = [((9, 7), (5, 3), [(0, 0), (4, 4), (6, 7)]),                                     # (x0, y0); the last one wraps on both axes
                ((12, 12), (8, 8), [(0, 0), (4, 0), (0, 4), (4, 4)]),
                ((40, 33), (17, 20), [(3 * s % 33, 7 * (s // 2) % 40) for s in range(8)] * 2)]  # 16 slots, every start twice


@pytest.mark.parametrize("planes", [1, 4, 8])
def test_gather_packed_is_a_stack_of_wrapped_copies(lib, planes):
    from mlimgsynth_amd import _lib
    rng = np.random.default_rng(planes)
    for (H, W), (wh, ww), slots in GATHER_CASES:
        x = rng.standard_normal((planes, H, W)).astype(np.float32)
        x[0, 0, 0], x[-1, H - 1, W - 1], x[0, H // 2, W // 2], x[0, 1, 1] = np.inf, np.nan, -0.0, -np.inf
        x.view(np.uint32)[0, 2, 2] = 0x7fc12345                 # a NaN with a payload
        n = len(slots)
        src, dst = _lib.from_numpy(x), _lib.from_numpy(np.full((n, planes, wh, ww), 7.0, np.float32))
        assert lib.mlsd_window_gather_packed(src.ptr, W, H, dst.ptr, ww, wh, UP.ints([s[0] for s in slots]), UP.ints([s[1] for s in slots]), n, planes, None) == 0
        got = dst.download((n, planes, wh, ww), np.float32)
        want = np.stack([U.crop(x, x0, y0, ww, wh) for x0, y0 in slots])
        assert got.tobytes() == want.tobytes(), (H, W, wh, ww, slots)
    assert len(GATHER_CASES[2][2]) == 16


def test_gather_packed_refuses_bad_arguments(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    n_can, n_win = 4 * 9 * 7, 2 * 4 * 5 * 3
    buf = _lib.from_numpy(np.zeros(n_can + n_win, np.float32))
    src, dst = buf.ptr, buf.ptr + n_can * 4

    def call(W=7, H=9, ww=3, wh=5, xs=(0, 4), ys=(0, 7), n=None, planes=4, s=src, d=dst):
        return lib.mlsd_window_gather_packed(s, W, H, d, ww, wh, UP.ints(xs) if xs is not None else None, UP.ints(ys) if ys is not None else None,
                                             len(xs if xs is not None else ys) if n is None else n, planes, None)
    assert call(xs=(0, 0), ys=(0, 0)) == 0                                   # (the canvas is zero: so is what was written)
    for kw in (dict(W=0), dict(H=-1), dict(ww=0), dict(wh=0), dict(planes=0), dict(ww=8), dict(wh=10), dict(xs=(0, -1)), dict(xs=(7, 0)), dict(ys=(0, 9)),
               dict(ys=(-2, 0)), dict(s=None), dict(d=None), dict(xs=None), dict(ys=None), dict(n=0), dict(n=-1), dict(xs=(0,) * 17, ys=(0,) * 17),
               dict(d=src), dict(d=src + n_can * 4 - 4), dict(W=65536, H=65536, ww=1, wh=1, planes=1),
               dict(W=20000, H=20000, ww=20000, wh=20000, planes=1, xs=(0,) * 8, ys=(0,) * 8)):
        assert call(**kw) < 0, kw
    K.sync()
    assert not buf.download((n_can + n_win,), np.float32).any()


def single_blends(lib, eps, wins, W, H, ww, wh, O, ld):
    """the reference: weight sums, a zeroed canvas, one mlsd_window_blend launch per window in order; eps[j] [N][wh ww][4]"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    N = eps[0].shape[0]
    xs, ys = sorted({w[0] for w in wins}), sorted({w[1] for w in wins})
    wsum = _lib.DeviceBuffer(H * W * 4)
    assert lib.mlsd_window_wsum(wsum.ptr, W, H, ww, wh, UP.ints(xs), len(xs), UP.ints(ys), len(ys), O, O, None) == 0
    canvas = _lib.from_numpy(np.zeros((N, H * W, 4), np.float32))
    keep = []
    for e, (x0, y0) in zip(eps, wins):
        padded = np.full((N, wh * ww, ld), 1e30, np.float32)
        padded[:, :, :4] = e
        keep.append(_lib.from_numpy(padded))
        assert lib.mlsd_window_blend(keep[-1].ptr, ld, canvas.ptr, wsum.ptr, W, H, ww, wh, x0, y0, O, O, N, 4, None) == 0
    K.sync()
    return canvas.download((N, H * W, 4), np.float32), wsum


def packed_blends(lib, eps, wins, launches, wsum, W, H, ww, wh, O, ld, B, G):
    """launches: [(n_used, n_slots)]; the columns past 4 hold 1e30 and every unused slot NaN, its start repeating the launch's last window"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    canvas = _lib.from_numpy(np.zeros((G * B, H * W, 4), np.float32))
    keep, j = [], 0
    for n_used, n_slots in launches:
        buf = np.full((G, n_slots, B, wh * ww, ld), np.nan, np.float32)
        buf[:, :n_used, :, :, 4:] = 1e30
        for s in range(n_used):
            buf[:, s, :, :, :4] = eps[j + s].reshape(G, B, wh * ww, 4)
        slots = [wins[j + min(s, n_used - 1)] for s in range(n_slots)]
        keep.append(_lib.from_numpy(buf))
        assert lib.mlsd_window_blend_packed(keep[-1].ptr, ld, canvas.ptr, wsum.ptr, W, H, ww, wh, UP.ints([s[0] for s in slots]), UP.ints([s[1] for s in slots]),
                                            n_used, n_slots, O, O, B, G, 4, None) == 0
        j += n_used
    assert j == len(wins)
    K.sync()
    return canvas.download((G * B, H * W, 4), np.float32)


LAUNCHES = {0: [[(4, 4)], [(2, 2), (2, 2)], [(3, 3), (1, 3)]],
            3: [[(9, 9)], [(5, 5), (4, 5)], [(3, 3)] * 3, [(9, 16)]]}


@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("tiling", [0, 3], ids=["open", "wrapped"])
def test_blend_packed_equals_the_single_blends(lib, tiling, B, G, ld):
    W = H = 12
    O, N = 4, G * B
    wins, ww, wh = U.windows(W, H, 8, 8, O, tiling)
    assert len(wins) == (9 if tiling else 4)
    rng = np.random.default_rng(100 + 8 * tiling + 4 * B + 2 * G + ld)
    eps = [rng.standard_normal((N, wh * ww, 4)).astype(np.float32) for _ in wins]
    eps[1][N - 1, 3 * ww + 5, 1] = 1e4                                   # an outlier
    want, wsum = single_blends(lib, eps, wins, W, H, ww, wh, O, ld)
    assert np.isfinite(want).all()
    for launches in LAUNCHES[tiling]:
        got = packed_blends(lib, eps, wins, launches, wsum, W, H, ww, wh, O, ld, B, G)
        assert np.isfinite(got).all(), launches
        assert got.tobytes() == want.tobytes(), launches
        again = packed_blends(lib, eps, wins, launches, wsum, W, H, ww, wh, O, ld, B, G)
        assert again.tobytes() == got.tobytes(), launches                # threads that raced on a canvas pixel would differ from run to run
    if (B, G, ld) == (2, 2, 8):                                          # and the sum itself, once: the float64 weighted average at the blend's bound
        parts = [e.reshape(N, wh, ww, 4).transpose(0, 3, 1, 2) for e in eps]
        ref, cnt = U.blend64(parts, wins, ww, wh, O, H, W)
        ref = ref.transpose(0, 2, 3, 1).reshape(N, H * W, 4)
        err = np.abs(got.astype(np.float64) - ref).max() / max(np.abs(e).max() for e in eps)
        print(f"packed blend tiling {tiling}: covers {cnt.min()}..{cnt.max()}, max|err| / max|eps| = {err:.3e}")
        assert cnt.max() <= 4 and (cnt.min() == 4) == (tiling == 3)
        assert err <= 1e-6


def test_blend_packed_refuses_bad_arguments(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    # G 2, 2 slots, B 1: 4 rows of 64 pixels, ld 8
    win, can, ws = _lib.DeviceBuffer(4 * 64 * 8 * 4), _lib.from_numpy(np.zeros((2, 144, 4), np.float32)), _lib.from_numpy(np.ones(144, np.float32))

    def call(e=win.ptr, ld=8, c=can.ptr, s=ws.ptr, W=12, H=12, ww=8, wh=8, xs=(0, 4), ys=(0, 4), used=2, n=None, ox=4, oy=4, B=1, G=2, Cn=4):
        return lib.mlsd_window_blend_packed(e, ld, c, s, W, H, ww, wh, UP.ints(xs) if xs is not None else None, UP.ints(ys) if ys is not None else None,
                                            used, len(xs if xs is not None else ys) if n is None else n, ox, oy, B, G, Cn, None)
    for kw in (dict(e=None), dict(c=None), dict(s=None), dict(xs=None), dict(ys=None), dict(ld=3), dict(W=0), dict(H=0), dict(ww=13), dict(wh=0),
               dict(xs=(0, 12)), dict(ys=(-1, 4)), dict(ox=-1), dict(oy=-1),
               dict(n=0), dict(xs=(0,) * 17, ys=(0,) * 17), dict(used=0), dict(used=3), dict(used=-1), dict(B=0), dict(G=0), dict(G=3), dict(Cn=3), dict(Cn=8),
               dict(c=can.ptr + 4), dict(e=can.ptr), dict(s=can.ptr), dict(W=30000, H=30000, ww=1, wh=1), dict(ld=1 << 20, B=4096, G=2)):
        assert call(**kw) < 0, kw
    K.sync()
    assert not can.download((2, 144, 4), np.float32).any()


# ------------------------------------------------------------------ engine
def engines(model, cfg, w, h, pack, tiling=0, plain_tiling=0, seed=7):
    """the packed canvas engine (batch 2) and the plain engine its plan is: one window, batch 2 P, the same conditioning"""
    from mlimgsynth_amd import engine as E
    cond = T.conditioning(model, np.random.default_rng(seed))
    tiled = E.Generator(model, w, h, 2, cfg_scale=cfg, unet_tile=TILE, unet_tile_overlap=OVERLAP, tiling=tiling, unet_tile_batch=pack)
    P = tiled.tile_pack_info()[0]
    plain = E.Generator(model, min(w, TILE), min(h, TILE), 2 * P, cfg_scale=cfg, tiling=plain_tiling)
    for g in (tiled, plain):
        g.set_cond(*cond) if cfg > 1 else g.set_cond(cond[0], cond[1])
    return tiled, plain


def composition(tiled, plain, x, sigma, wins, ww, wh, O, pack):
    """per group, ONE evaluation of the plain engine on the group's crops stacked in slot order (slot-major, image-minor; the padded slots repeat the
    group's last crop), split back per slot; then the float64 weighted average"""
    H, W = x.shape[-2:]
    B = x.shape[0]
    parts = []
    for slots, n_used in UP.groups(len(wins), B, pack):
        out = plain.dxdt(np.concatenate([U.crop(x, *wins[j], ww, wh) for j in slots]), sigma)
        parts += [out[s * B:(s + 1) * B] for s in range(n_used)]
    assert len(parts) == len(wins)
    want, cnt = U.blend64(parts, wins, ww, wh, O, H, W)
    return parts, want, cnt


@pytest.mark.parametrize("pack,info", [(2, (2, 2)), (3, (2, 2)), (4, (4, 1))])
@pytest.mark.parametrize("cfg", [7.0, 1.0])
@pytest.mark.parametrize("model", ["tiny", "tinyv", "tinyxl"])
def test_packed_engine_equals_its_composition(model, cfg, pack, info):
    tiled, plain = engines(model, cfg, 96, 96, pack)
    try:
        wins, ww, wh = U.windows(12, 12, 8, 8, 4)
        assert tiled.tile_pack_info() == info and plain.tile_pack_info() == (0, 1)
        assert tiled.tile_info() == (4, 8, 8) and tiled.tile_windows() == wins
        rng = np.random.default_rng(11)
        for sigma in (1.5, 12.0):
            x = (rng.standard_normal((2, 4, 12, 12)) * np.sqrt(1 + sigma * sigma)).astype(np.float32)
            got = tiled.dxdt(x, sigma)
            parts, want, cnt = composition(tiled, plain, x, sigma, wins, ww, wh, 4, pack)
            scale = max(np.abs(p).max() for p in parts)
            bound = (cfg + abs(1 - cfg)) * 1e-6 * scale
            err = np.abs(got.astype(np.float64) - want).max()
            print(f"{model} cfg {cfg} pack {pack} sigma {sigma}: max|err| = {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
            assert np.isfinite(got).all() and err <= bound
            for p, (x0, y0) in zip(parts, wins):                    # corners: a single window, the very value
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


def test_ragged_last_group_and_info():
    tiled, plain = engines("tiny", 7.0, 128, 64, 2)
    try:
        wins, ww, wh = U.windows(16, 8, 8, 8, 4)
        assert tiled.tile_info() == (3, 8, 8) and tiled.tile_pack_info() == (2, 2)
        assert UP.groups(3, 2, 2) == [([0, 1], 2), ([2, 2], 1)]     # one real and one repeated slot
        x = (np.random.default_rng(12).standard_normal((2, 4, 8, 16)) * 3).astype(np.float32)
        got = tiled.dxdt(x, 3.0)
        parts, want, _ = composition(tiled, plain, x, 3.0, wins, ww, wh, 4, 2)
        bound = 13e-6 * max(np.abs(p).max() for p in parts)
        err = np.abs(got - want).max()
        print(f"128x64 pack 2: max|err| = {err:.3e}, bound {bound:.3e}")
        assert np.isfinite(got).all() and err <= bound
        assert tiled.info()["unet_flops"] == 2 * plain.info()["unet_flops"]         # the work done: two evaluations of the batch-4 plan
    finally:
        tiled.destroy(), plain.destroy()


def test_ring_of_windows_in_one_evaluation():
    x = (np.random.default_rng(13).standard_normal((2, 4, 8, 12)) * 3).astype(np.float32)
    sigma = 3.0
    ring, plain = engines("tiny", 7.0, 96, 64, 3, tiling=1)
    try:
        assert ring.tile_info() == (3, 8, 8) and [w[0] for w in ring.tile_windows()] == [0, 4, 8] and ring.tile_pack_info() == (3, 1)
        a = ring.dxdt(x, sigma)
        b = ring.dxdt(np.roll(x, 4, axis=-1), sigma)
        assert b.tobytes() == np.roll(a, 4, axis=-1).tobytes()        # the seam is nowhere
        wins, ww, wh = U.windows(12, 8, 8, 8, 4, 1)
        parts, want, cnt = composition(ring, plain, x, sigma, wins, ww, wh, 4, 3)
        assert (cnt == 2).all()
        assert np.abs(a - want).max() <= 13e-6 * max(np.abs(p).max() for p in parts)
    finally:
        ring.destroy(), plain.destroy()


@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
def test_packed_against_unpacked(model):
    from mlimgsynth_amd import engine as E
    cond = T.conditioning(model, np.random.default_rng(7))
    x = (np.random.default_rng(14).standard_normal((2, 4, 12, 12)) * np.sqrt(10.0)).astype(np.float32)
    out = []
    for pack in (1, 2):
        g = E.Generator(model, 96, 96, 2, cfg_scale=1.0, unet_tile=TILE, unet_tile_overlap=OVERLAP, unet_tile_batch=pack)
        try:
            assert g.tile_pack_info() == ((1, 4) if pack == 1 else (2, 2))
            g.set_cond(cond[0], cond[1])
            out.append(g.dxdt(x, 3.0).astype(np.float64))
        finally:
            g.destroy()
    rel = np.linalg.norm(out[1] - out[0]) / np.linalg.norm(out[0])
    print(f"{model}: pack 2 against pack 1, rel-L2 of dxdt = {rel:.3e} (bound {2 * tolerances.EVAL_SMALL:.1e})")
    assert rel <= 2 * tolerances.EVAL_SMALL


@pytest.mark.parametrize("method", ["euler", "heun", "dpmpp2m"])
def test_packed_denoise_runs_every_solver_family(method):
    from mlimgsynth_amd import engine as E
    out = []
    for graph in (False, True):
        g = E.Generator("tiny", 96, 96, 2, n_step=3, method=method, unet_tile=TILE, unet_tile_overlap=OVERLAP, use_hipgraph=graph, unet_tile_batch=2)
        try:
            assert g.tile_pack_info() == (2, 2)
            g.set_cond(*T.conditioning("tiny", np.random.default_rng(7)))
            lat, _ = g.generate([1, 2], want_images=False)
            assert np.isfinite(lat).all() and g.last_nfe() >= 4
            out.append(lat)
        finally:
            g.destroy()
    assert out[0].tobytes() == out[1].tobytes()                         # a captured plan replays the same groups


# ------------------------------------------------------------------ mlis_generate
STEPS = T.STEPS
CLAUSE = f", Tiled diffusion: {TILE}, Tile overlap: {OVERLAP}, Tile batch: 2, Version: "
_cache = {}


def packed(lib, pack=2, opts=(), **kw):
    return T.generate(lib, unet_tile=TILE, opts=tuple(opts) + (("unet_tile_batch", pack),), **kw)


def unpacked96(lib):
    if "r" not in _cache:
        _cache["r"] = T.generate(lib, unet_tile=TILE)
    return _cache["r"]


def test_generate_packed_is_deterministic(lib):
    a, b = packed(lib), packed(lib)
    assert a["latent"].shape == (2, 4, 12, 12) and a["image"].shape == (2, 3, 96, 96)
    assert np.isfinite(a["latent"]).all() and np.isfinite(a["image"]).all()
    assert T.same(a, b) and a["info"] == b["info"] and a["builds"] == 1
    assert CLAUSE in a["info"]
    base = unpacked96(lib)
    assert a["info"].replace(", Tile batch: 2", "") == base["info"]       # NFE, steps and size included
    assert T.nfe_of(a["info"]) == T.nfe_of(base["info"]) == 2 * STEPS
    x, y = a["latent"].astype(np.float64), base["latent"].astype(np.float64)
    rel = np.linalg.norm(x - y) / np.linalg.norm(y)
    print(f"generate: pack 2 against pack 1, rel-L2 of the final latent = {rel:.3e} (bound {2 * tolerances.LATENT:.1e})")
    assert rel <= 2 * tolerances.LATENT


def test_pack_one_and_untiled_are_the_old_behaviour(lib):
    base = unpacked96(lib)
    one = packed(lib, pack=1)
    assert T.same(one, base) and one["info"] == base["info"] and one["builds"] == 1 and "Tile batch" not in one["info"]
    plain = T.plain96(lib)
    off = T.generate(lib, unet_tile=0, opts=(("unet_tile_batch", 4),))
    assert T.same(off, plain) and off["info"] == plain["info"] and off["builds"] == 1 and "Tile batch" not in off["info"]


@pytest.mark.parametrize("name", ["hires", "unet_split", "long_prompt", "img2img_mask", "tiling_x", "tae"])
def test_packed_composes_with_the_other_options(lib, name):
    kw = dict(T.COMPOSE[name])
    opts = kw.pop("opts", ())
    a, b = packed(lib, opts=opts, **kw), packed(lib, opts=opts, **kw)
    assert a["latent"].shape == (2, 4, 12, 12) and np.isfinite(a["latent"]).all()
    assert a["image"].shape == (2, 3, 96, 96) and np.isfinite(a["image"]).all()
    assert T.same(a, b) and a["info"] == b["info"]
    assert CLAUSE in a["info"]
    assert a["builds"] == (2 if name == "hires" else 1)


def test_callback_counts_steps_not_groups(lib):
    seen = []

    def cb(ud, ctx, p):
        seen.append((p.contents.stage, p.contents.step, p.contents.step_end, p.contents.nfe))
        return 0

    thunk = F.CALLBACK(cb)
    m = T.context(lib, unet_tile=TILE, opts=(("unet_tile_batch", 2),))
    try:
        assert lib.mlis_option_set(m.ctx, F.OPT["CALLBACK"], thunk, C.c_void_p(None)) == 1
        T.prompt(m)
        m.generate()
        den = [s for s in seen if s[0] == 4]
        assert [s[1] for s in den] == list(range(1, STEPS + 1)) and all(s[2] == STEPS for s in den)
        assert [s[3] for s in den] == [2 * (i + 1) for i in range(STEPS)]
    finally:
        m.close()


def test_a_changed_pack_is_another_engine(lib):
    m = T.context(lib, unet_tile=TILE, opts=(("unet_tile_batch", 2),))
    try:
        T.prompt(m)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 1 and "Tile batch: 2" in lib.mlis_infotext_get(m.ctx, 0).decode()
        m.set("unet_tile_batch", 1)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 2 and "Tile batch" not in lib.mlis_infotext_get(m.ctx, 0).decode()
        m.set("unet_tile_batch", 2)
        m.generate()
        assert lib.mlis_amd_engine_builds(m.ctx) == 2                    # the context keeps two engines: changing back builds none
        assert "Tile batch: 2" in lib.mlis_infotext_get(m.ctx, 0).decode() and np.isfinite(m.tensor(F.TENSOR["LATENT"])).all()
    finally:
        m.close()
