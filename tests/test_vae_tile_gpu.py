"""Tiled VAE decode and encode (MLIS_OPT_VAE_TILE; decode_tiled / encode_tiled of csrc/host/engine.c) at every tile geometry the walk has, on the model "tiny"
(f_down 8, margin k = 8 latent pixels): the smallest sizes at which each branch exists.

Per geometry, for decode and for encode:
  nothing unwritten   the image buffer is filled with 0xFF bytes (NaN) before the decode; an encode follows the encode of another image on the same engine and must
                      give the bits of a fresh engine (moments left over from the other image would show)
  geometry            EXACT: the tiled result equals, bit for bit, the paste (by tests/vae_tile_ref.py's walk) of every distinct tile run alone through a Generator of
                      the tile's own size with vae_tile off -- the tile plan is that plan (same builder, same size, same weights)
  numerics            T.EVAL, the project's bound for one VAE pass, on the rel-L2 of EVERY paste window by itself against vae_tile_ref (the oracle's untiled codec on
                      each tile slice): one misplaced strip cannot hide in a whole-image norm.  With more than one tile the result is also farther from the oracle's
                      untiled decode than from the tiled one (tests/test_sampler_gpu.py's condition)
  tile count          EXACT: plan evaluations of the pass == distinct tile origins x images (the tile plans take one image: a batch walks them image by image, so
                      an image's tiles are computed by the same launches at any batch size)

Rows 24 x 32, 32 x 24 (one dimension covered by one tile: the reference leaves 8 latent columns unwritten), 16 x 32 (its step is 0: division by zero) and 8 x 32 (negative
step: no tile ran) are where this project extends the reference; see include/mlimgsynth_amd.h at mlis_amd_set_vae_tile.  The last test changes the tile size on a live
engine through the public API (the tile buffers must follow the tile)."""
import ctypes as C

import numpy as np
import pytest

import mlis_ffi as F
import oracle_lib as O
import tolerances as T
import vae_tile_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32

#       id            latent W, H  tile_px  B
ROWS = [("3origins",      40, 32,   64,    1),     # origins {0, 8, 16} in x: an interior tile with a margin on both sides
        ("clamped",       28, 32,   64,    1),     # origins {0, 4}: the clamped last origin is no multiple of the step
        ("tile128",       40, 40,   128,   1),     # tile 32, origins {0, 8}
        ("tile65",        40, 40,   65,    1),     # rounds up to 128: the row above, bit for bit
        ("onetile_x",     24, 32,   64,    1),     # x covered by one tile, y tiled
        ("onetile_y",     32, 24,   64,    1),
        ("step0",         16, 32,   64,    1),     # 16 = 2 k
        ("negstep",       8,  32,   64,    1),     # below 2 k
        ("batch2",        32, 32,   64,    2)]
IDS = [r[0] for r in ROWS]
DISTINCT = dict(zip(IDS, (6, 4, 4, 4, 2, 2, 2, 2, 4)))          # distinct tile origins = plan evaluations of one pass


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def orc():
    return R.Oracle("tiny")


@pytest.fixture(scope="module")
def E():
    from mlimgsynth_amd import engine
    return engine


def latent_of(lw, lh, B):
    return (np.random.default_rng(1000 * lw + lh).standard_normal((B, 4, lh, lw)) * 0.5).astype(F32)


def image_of(lw, lh, B, seed=0):
    return np.random.default_rng(77 * lw + lh + seed).random((B, 3, 8 * lh, 8 * lw)).astype(F32)


def poison_image(g):
    """0xFF in every byte of the engine's image buffer: every float a NaN until a paste writes it"""
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    _lib.check(L.mlsd_memset(C.c_void_p(g.image_ptr()), C.c_int(0xFF), C.c_size_t(g.B * 3 * g.w * g.h_px * 4), None))
    _lib.check(L.mlsd_device_sync())
    assert np.isnan(g.image()).all()


def tiled_decode(E, z, tile_px):
    B, _, lh, lw = z.shape
    g = E.Generator("tiny", 8 * lw, 8 * lh, B, n_step=2)
    try:
        g.set_vae_tile(tile_px)
        g.set_init_latent(z)
        poison_image(g)
        g.decode()
        return g.image(), g.vae_tile_info()
    finally:
        g.destroy()


_decoded = {}


def decoded(E, name):
    """one tiled decode per row, shared by the tests that look at it"""
    if name not in _decoded:
        _, lw, lh, tile_px, B = ROWS[IDS.index(name)]
        z = latent_of(lw, lh, B)
        _decoded[name] = (z,) + tiled_decode(E, z, tile_px)
    return _decoded[name]


@pytest.mark.parametrize("name", IDS)
def test_decode(E, orc, name):
    _, lw, lh, tile_px, B = ROWS[IDS.index(name)]
    z, img, info = decoded(E, name)
    n0, n1, wins = R.windows(lw, lh, tile_px, 8, 8)
    origins = [w[0] for w in wins]
    # ---- nothing unwritten, and no tile evaluated twice
    assert np.isfinite(img).all(), f"{np.isnan(img).sum()} pixels of the image were never written"
    assert info is not None and info["tile"] == (n0, n1)
    assert len(set(origins)) == len(origins) == DISTINCT[name] == info["n_tiles"] and info["n_evals"] == B * DISTINCT[name]
    # ---- geometry, bit for bit: every distinct tile of every image alone on a one-image plan of the tile's size, pasted by the Python walk
    gt = E.Generator("tiny", 8 * n0, 8 * n1, 1, n_step=2)
    try:
        assert not gt.vae_tile_prepare()
        tiles = {}
        for i0, i1 in origins:
            one = []
            for b in range(B):
                gt.set_init_latent(np.ascontiguousarray(z[b:b + 1, :, i1:i1 + n1, i0:i0 + n0]))
                gt.decode()
                one.append(gt.image()[0])
            tiles[(i0, i1)] = np.stack(one)
    finally:
        gt.destroy()
    want = R.compose(np.full_like(img, np.nan), tiles, wins, 8, 1)
    assert img.tobytes() == want.tobytes(), ("tiled decode differs from the paste of its tiles", int((img != want).sum()), float(np.abs(img - want).max()))
    # ---- numerics: every paste window by itself
    ref, pwins, n = R.decode_ref(orc, z, tile_px)
    assert n == DISTINCT[name] and np.isfinite(ref).all()
    worst = 0.0
    for (x0, x1), (y0, y1) in pwins:
        for b in range(B):
            e = rel(img[b, :, y0:y1, x0:x1] - 0.5, ref[b, :, y0:y1, x0:x1] - 0.5)
            worst = max(worst, e)
            assert e < T.EVAL, (name, b, (x0, x1), (y0, y1), e)
    e_t = rel(img - 0.5, ref - 0.5)
    e_full = rel(img - 0.5, np.stack([orc.decode(z[b]) for b in range(B)]) - 0.5)
    print(f"{name}: {n} tiles of {n0}x{n1}; worst window rel-L2 {worst:.3e}, whole image {e_t:.3e}, against the untiled oracle decode {e_full:.3e}")
    assert e_t < T.EVAL and e_full > 2 * e_t          # it really is the tiled result (every row has more than one tile)


def test_decode_tile65_is_tile128(E):
    assert decoded(E, "tile65")[1].tobytes() == decoded(E, "tile128")[1].tobytes()


def test_decode_batch_images_are_their_own_single_runs(E):
    """Each image of the B = 2 decode against the B = 1 decode of its latent, bit for bit.  The tile plans take one image and a batch walks them image by image; a
    tile plan of B images would pick its GEMM tiles and K splits by M = B x pixels (at 24 x 24: variant 0 unsplit for one image, variants 1 and 2 with split-K 16
    for two) and differ from the single run by 1.6e-3 (measured, rel-L2 8.4e-4)."""
    z, img, _ = decoded(E, "batch2")
    assert not np.array_equal(z[0], z[1])
    singles = []
    for b in range(2):
        one, info = tiled_decode(E, z[b:b + 1], 64)
        assert info["n_evals"] == 4
        print(f"image {b}: B = 2 against B = 1, max |difference| {np.abs(one[0] - img[b]).max():.3e}, rel-L2 {rel(img[b] - 0.5, one[0] - 0.5):.3e}")
        singles.append(one[0])
    for b in range(2):
        assert singles[b].tobytes() == img[b].tobytes(), (b, float(np.abs(singles[b] - img[b]).max()))


def test_decode_batch_slots(E):
    """the two latents in the other order on an engine of the same batch size: each image keeps its bits in the other slot (copy_slice2 and nhwc_to_nchw_f32 index
    B x planes; the plan's input moves from image to image)"""
    z, img, _ = decoded(E, "batch2")
    swapped, info = tiled_decode(E, np.ascontiguousarray(z[::-1]), 64)
    assert info["n_evals"] == 8
    assert swapped[1].tobytes() == img[0].tobytes() and swapped[0].tobytes() == img[1].tobytes()
    assert img[0].tobytes() != img[1].tobytes()


def tiled_encode(E, src, tile_px, seeds, first=None):
    """(sampled latent, mean latent, tile info) of src; `first`: an image encoded on the same engine before"""
    B, _, H, W = src.shape
    g = E.Generator("tiny", W, H, B, n_step=2)
    try:
        g.set_vae_tile(tile_px)
        if first is not None:
            g.seed([s + 100 for s in seeds])
            g.encode(first, sample=True)
        g.seed(seeds)
        s = g.encode(src, sample=True)
        info = g.vae_tile_info(encoder=True)
        m = g.encode(src, sample=False)
        return s, m, info
    finally:
        g.destroy()


@pytest.mark.parametrize("name", IDS)
def test_encode(E, orc, name):
    _, lw, lh, tile_px, B = ROWS[IDS.index(name)]
    src, other = image_of(lw, lh, B), image_of(lw, lh, B, seed=1)
    seeds = [5 + b for b in range(B)]
    lat_s, lat_m, info = tiled_encode(E, src, tile_px, seeds, first=other)
    n0, n1, wins = R.windows(8 * lw, 8 * lh, tile_px, 1, 64)
    origins = [w[0] for w in wins]
    assert info is not None and info["tile"] == (n0, n1)
    assert len(set(origins)) == len(origins) == DISTINCT[name] == info["n_tiles"] and info["n_evals"] == B * DISTINCT[name]
    # ---- nothing unwritten: no moment of the image encoded before is left
    assert np.isfinite(lat_s).all() and np.isfinite(lat_m).all()
    fresh_s, fresh_m, _ = tiled_encode(E, src, tile_px, seeds)
    assert lat_s.tobytes() == fresh_s.tobytes() and lat_m.tobytes() == fresh_m.tobytes(), "the encode depends on what the engine encoded before"
    # ---- geometry, bit for bit (the mean: value * scale_factor per element commutes with the paste; the sampled latent draws its noise by position in the whole image)
    gt = E.Generator("tiny", n0, n1, 1, n_step=2)            # one image at a time, like the tile plan
    try:
        tiles = {(i0, i1): np.concatenate([gt.encode(np.ascontiguousarray(src[b:b + 1, :, i1:i1 + n1, i0:i0 + n0]), sample=False) for b in range(B)])
                 for i0, i1 in origins}
    finally:
        gt.destroy()
    want = R.compose(np.full_like(lat_m, np.nan), tiles, wins, 1, 8)
    assert lat_m.tobytes() == want.tobytes(), ("tiled encode differs from the paste of its tiles", int((lat_m != want).sum()), float(np.abs(lat_m - want).max()))
    # ---- numerics: every paste window by itself, mean and sampled
    mom, pwins, n = R.encode_moments_ref(orc, src, tile_px)
    assert n == DISTINCT[name] and np.isfinite(mom).all()
    rnd = [O.randn(s, 0, 4 * lh * lw) for s in seeds]
    ref_m, ref_s = R.latent_sample(orc, mom), R.latent_sample(orc, mom, rnd)
    worst = 0.0
    for (x0, x1), (y0, y1) in pwins:
        for b in range(B):
            for got, ref in ((lat_m, ref_m), (lat_s, ref_s)):
                e = rel(got[b, :, y0:y1, x0:x1], ref[b, :, y0:y1, x0:x1])
                worst = max(worst, e)
                assert e < T.EVAL, (name, b, (x0, x1), (y0, y1), e)
    print(f"{name}: {n} tiles of {n0}x{n1}; worst window rel-L2 {worst:.3e}, whole latent mean {rel(lat_m, ref_m):.3e} sampled {rel(lat_s, ref_s):.3e}")


# ------------------------------------------------------------------ a tile change on a live engine, through the public API
TOKS = np.array([5, 17, 300, 42, 7], np.int32)


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    l = F.bind(_lib.LIB_PATH)
    l.mlis_amd_engine_builds.argtypes = [C.c_void_p]
    l.mlis_amd_engine_get.restype, l.mlis_amd_engine_get.argtypes = C.c_void_p, [C.c_void_p]
    l.mlis_amd_ctx_at.restype, l.mlis_amd_ctx_at.argtypes = C.c_void_p, [C.c_void_p, C.c_int]
    return l


def context320(lib):
    m = F.Mlis(lib)
    m.set("model", "synth:tiny")
    m.set("image_dim", 320, 320)
    m.set("steps", 2)
    return m


def generate320(lib, m, vae_tile):
    m.set("seed", 42)
    m.set("vae_tile", vae_tile)
    m.tokens(TOKS)
    m.generate()
    eng = lib.mlis_amd_engine_get(m.ctx)
    return m.tensor(F.TENSOR["IMAGE"]), bool(eng and lib.mlis_amd_ctx_at(eng, 3)), m.tensor(F.TENSOR["LATENT"])


ORDER = (64, 128, 192, 0, 64)


def test_tile_change_on_a_live_engine(lib):
    """vae_tile 64, 128, 192, 0, 64 on ONE context at 320 x 320 (40 x 40 latent: tiles of 24, 32, none, none, 24): the engine stays, the tile plan and its buffers are
    replaced; every image is the one a fresh context gives with that option.  (Buffers kept from the 24-tile were overrun by the 32-tile.)
    A context's Philox offset goes on from generation to generation like the reference's global generator, so the fresh context of generation k first generates
    k times with vae_tile off -- no tile plan and no tile buffer exists before its one tiled decode -- and then holds the same latent."""
    m = context320(lib)
    live = []
    try:
        for v in ORDER:
            live.append(generate320(lib, m, v))
        assert lib.mlis_amd_engine_builds(m.ctx) == 1
    finally:
        m.close()
    assert [t for _, t, _ in live] == [True, True, False, False, True]
    for k, v in enumerate(ORDER):
        m = context320(lib)
        try:
            for _ in range(k):
                generate320(lib, m, 0)
            img, tiled, lat = generate320(lib, m, v)
        finally:
            m.close()
        assert np.isfinite(img).all() and img.shape == (1, 3, 320, 320)
        assert lat.tobytes() == live[k][2].tobytes(), (k, v, "the latents differ: the comparison of the decodes means nothing")
        assert tiled == live[k][1], (k, v)
        assert img.tobytes() == live[k][0].tobytes(), (k, v, float(np.abs(img - live[k][0]).max()))
    # the options do different things: on one latent the two tile sizes differ from each other and from the untiled decode, which the one-tile size equals
    one = {}
    for v in (0, 64, 128, 192):
        m = context320(lib)
        try:
            one[v] = generate320(lib, m, v)[0]
        finally:
            m.close()
    assert one[64].tobytes() == live[0][0].tobytes() and one[192].tobytes() == one[0].tobytes()
    assert len({one[v].tobytes() for v in (0, 64, 128)}) == 3
