"""Tiled VAE decode / encode without a GPU: the engine's one tile walk (mlis_amd_vae_tile_walk) against tests/vae_tile_ref.py for every length 1 .. 200 latent pixels,
the properties a walk must have (no hole, no window outside its tile or the output, no repeated origin, the reference's last writer on every pixel of a tiled dimension),
the tile plans and tile buffers of a dry engine through tile-size changes, the lengths at which the reference's loop divides by zero or runs no tile, and
vae_tile_ref's composition against the oracle's restatement of src/vae.c where both dimensions are tiled.

What needs a device is in tests/test_vae_tile_gpu.py."""
import numpy as np
import pytest

import vae_tile_ref as R

TILES = (1, 64, 65, 128, 192, 512)
UNITS = ((8, 8), (1, 64))            # (unit, margin k): decode over latent pixels, encode over image pixels


@pytest.fixture(scope="module")
def E():
    from mlimgsynth_amd import engine
    engine._proto2()
    return engine


@pytest.fixture()
def dry(E):
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield E
    L.mlsd_runtime_dry(0)


def reference_last_writers(full, tile_px, unit, k):
    """the loop of src/vae.c:353-384 (decode) / 257-289 (encode) over one TILED dimension as it stands, repeats included:
    per output pixel the (origin, index inside the tile) of the tile that wrote it last; None where nothing wrote"""
    n = min((tile_px + 63) // 64 * 64 // unit + k * 2, full)
    assert n < full
    step = n - k * 2
    n_tile = (full + step - 1) // step
    who = [None] * full
    for t in range(n_tile):
        i0 = min(t * step, full - n)
        d0 = k if i0 else 0
        for x in range(n - k):
            who[i0 + d0 + x] = (i0, d0 + x)
    return who, n_tile


@pytest.mark.parametrize("unit,k", UNITS, ids=["latent", "image"])
@pytest.mark.parametrize("tile_px", TILES)
def test_walk_every_length(E, tile_px, unit, k):
    f = 8 // unit
    for lat in range(1, 201):
        full = lat * f
        n, org, off, wid = E.vae_tile_walk(full, tile_px, unit, k)
        assert (n, org, off, wid) == R.walk_records(full, tile_px, unit, k), (full, tile_px)
        assert n == min((tile_px + 63) // 64 * 64 // unit + 2 * k, full)
        # no origin twice, in increasing order; first and last tile touch both ends of the input and of the output
        assert org == sorted(set(org)) and org[0] == 0 and org[-1] + n == full
        assert off[0] == 0 and org[-1] + off[-1] + wid[-1] == full
        who = [None] * full
        for o, d, w in zip(org, off, wid):
            assert w > 0 and 0 <= d and d + w <= n, "window outside its tile"
            assert 0 <= o and o + n <= full and o + d + w <= full, "tile or window outside the output"
            for x in range(w):
                who[o + d + x] = (o, d + x)
        assert None not in who, (full, tile_px, "hole")
        if n == full:
            assert (org, off, wid) == ([0], [0], [full])        # one tile, pasted whole
        else:
            ref, n_ref = reference_last_writers(full, tile_px, unit, k)
            assert who == ref, (full, tile_px)
            assert len(org) <= n_ref and len(org) == -(-(full - n) // (n - 2 * k)) + 1


def test_walk_counts_of_the_documented_cases(E):
    # the 32 x 32 latent at 64-px tiles: ceil(32 / 8) = 4 tiles per dimension in the reference (16 decodes), 2 distinct origins (4 decodes)
    assert reference_last_writers(32, 64, 8, 8)[1] == 4 and E.vae_tile_walk(32, 64, 8, 8)[1] == [0, 8]
    assert E.vae_tile_walk(40, 64, 8, 8)[1:] == ([0, 8, 16], [0, 8, 8], [16, 16, 16])
    assert E.vae_tile_walk(28, 64, 8, 8)[1] == [0, 4]                               # clamped: not a multiple of the step
    assert E.vae_tile_walk(40, 128, 8, 8) == E.vae_tile_walk(40, 65, 8, 8) == (32, [0, 8], [0, 8], [24, 24])
    # one tile covers the dimension: 17 .. 24 lost their last 8 in the reference, 16 divided by zero, below 16 nothing ran
    for full in (24, 17, 16, 15, 8, 1):
        assert E.vae_tile_walk(full, 64, 8, 8) == (full, [0], [0], [full])
    # 512 x 768 at vae_tile 512: the width is one tile of 64, the height three of 80 at {0, 16, 32}
    assert E.vae_tile_walk(64, 512, 8, 8)[1] == [0] and E.vae_tile_walk(96, 512, 8, 8)[:2] == (80, [0, 16])
    for bad in ((0, 64, 8, 8), (10, 0, 8, 8), (10, 64, 0, 8), (10, 64, 8, -1), (300, 64, 128, 8)):
        from mlimgsynth_amd import _lib
        with pytest.raises(_lib.MlsdError):
            E.vae_tile_walk(*bad)


def check_capacities(g, B):
    d, e = g.vae_tile_info(), g.vae_tile_info(encoder=True)
    for info, cin, cout, up in ((d, 4, 3, 8 * 8), (e, 3, 8, 1.0 / 64)):
        if info is None:
            continue
        n0, n1 = info["tile"]
        assert info["in_bytes"] >= B * cin * n0 * n1 * 4, info
        assert info["out_bytes"] >= B * cout * n0 * n1 * up * 4, info
    return (d["tile"] if d else None), (e["tile"] if e else None)


@pytest.mark.parametrize("B", [1, 2])
def test_tile_buffers_follow_the_tile_size(dry, B):
    """vae_tile 64 -> 128 -> 192 -> 64 on one engine at 320 x 320 (40 x 40 latent): tiles of 24, 32, none (40 covers all: disabled), 24 latent pixels; the buffers of the
    24-tile must not serve the 32-tile (4 x 24 x 24 floats against 4 x 32 x 32)"""
    g = dry.Generator("tiny", 320, 320, B, defer_weights=True)
    try:
        assert g.vae_tile_info() is None and g.vae_tile_info(encoder=True) is None
        seen = []
        for tile_px, lat in ((64, 24), (128, 32), (192, None), (64, 24)):
            g.set_vae_tile(tile_px)
            assert g.vae_tile_info() is None and g.vae_tile_info(encoder=True) is None          # the old plans are gone with the old tile
            assert g.vae_tile_prepare() == (lat is not None) and g.vae_tile_prepare(encoder=True) == (lat is not None)
            dt, et = check_capacities(g, B)
            assert dt == ((lat, lat) if lat else None) and et == ((lat * 8, lat * 8) if lat else None)
            assert (g.ctx_at(3) is not None) == (lat is not None) == (g.ctx_at(4) is not None)
            if lat:
                i = g.vae_tile_info()
                assert i["in_bytes"] == B * 4 * lat * lat * 4 and i["out_bytes"] == B * 3 * lat * lat * 64 * 4        # exactly the tile: nothing kept from a larger one
                # the tile plans take one image at any batch size: the batch walks them image by image (an image's tiles do not depend on B)
                for which in (3, 4):
                    gather = [r for r in g.ctx_at(which).op_records() if r[0] == "n2h"]
                    assert len(gather) == 1 and (gather[0][5].n_src, gather[0][5].n_dst) == (1, 1)
                n = len(R.walk(40, tile_px, 8, 8)[1]) ** 2
                assert i["n_tiles"] == n == g.vae_tile_info(encoder=True)["n_tiles"] and i["n_evals"] == 0
                seen.append(n)
        assert seen == [9, 4, 9]
    finally:
        g.destroy()


@pytest.mark.parametrize("W,H,tile,tiles", [(128, 256, (16, 24), 2), (64, 256, (8, 24), 2), (256, 128, (24, 16), 2), (256, 64, (24, 8), 2), (192, 256, (24, 24), 2)],
                         ids=lambda v: str(v))
def test_narrow_dimension_prepares_and_walks(dry, W, H, tile, tiles):
    """a dimension of 16 latent pixels gave step 0 and a division by zero, one below 16 a negative step and no tile at all (src/vae.c:353-356 with n == full in one
    dimension only); 17 .. 24 ran but left 8 columns unwritten.  Each is one tile across that dimension now."""
    g = dry.Generator("tiny", W, H, 1, defer_weights=True)
    try:
        g.set_vae_tile(64)
        assert g.vae_tile_prepare() and g.vae_tile_prepare(encoder=True)
        dt, et = check_capacities(g, 1)
        assert dt == tile and et == (tile[0] * 8, tile[1] * 8)
        assert g.vae_tile_info()["n_tiles"] == tiles == g.vae_tile_info(encoder=True)["n_tiles"]
        _, _, wins = R.windows(W // 8, H // 8, 64, 8, 8)
        cover = np.zeros((H // 8, W // 8), int)
        for _, (x0, x1), (y0, y1) in wins:
            cover[y0:y1, x0:x1] += 1
        assert (cover == 1).all() and len(wins) == tiles          # two tiles, abutting: every latent pixel written once
    finally:
        g.destroy()


def test_ref_equals_the_oracles_tiled_codec_where_both_dimensions_are_tiled():
    """vae_tile_ref pastes the oracle's UNTILED results by its own walk; orc_vae_decode_tiled / orc_vae_encode_moments_tiled restate the loops of src/vae.c with every
    repeat.  28 x 32 latent, 64-px tiles: origins {0, 4} x {0, 8}.  (Never called where one tile covers a dimension: they carry the reference's division by zero.)"""
    import oracle_lib as O
    orc = R.Oracle("tiny")
    rng = np.random.default_rng(21)
    z = (rng.standard_normal((1, 4, 32, 28)) * 0.5).astype(np.float32)
    got, wins, n = R.decode_ref(orc, z, 64)
    want = O.from_ot(O.L().orc_vae_decode_tiled(orc.P.h, b"vae", orc.V, O.to_ot(z), 64))
    assert n == 4 and len(wins) == 4 and got.shape == want.shape == (1, 3, 256, 224)
    assert got.tobytes() == want.tobytes()
    img = rng.random((1, 3, 256, 224)).astype(np.float32)
    got, wins, n = R.encode_moments_ref(orc, img, 64)
    want = O.from_ot(O.L().orc_vae_encode_moments_tiled(orc.P.h, b"vae", orc.V, O.to_ot(img), 64))
    assert n == 4 and got.shape == want.shape == (1, 8, 32, 28)
    assert got.tobytes() == want.tobytes()
    assert wins == [((0, 16), (0, 16)), ((12, 28), (0, 16)), ((0, 16), (16, 32)), ((12, 28), (16, 32))]
