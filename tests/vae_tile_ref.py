"""What a tiled KL-VAE decode / encode has to give, without the engine's walk: the tile size, margin and clamp from their definitions
(src/vae.c:238-244, 333-339: n = min(round_up(tile_px, 64) / unit + 2 k, full); :269-289, 365-384: origin min(t step, full - n) with step = n - 2 k,
tile 0 pastes [0, n - k), every other tile [i0 + k, i0 + n)), and the oracle's UNTILED codec on every tile slice.

Two rules are this project's, not the reference's (include/mlimgsynth_amd.h at mlis_amd_set_vae_tile):
  - a dimension that one tile covers (n == full) is one tile at 0 pasted whole.  The reference gives it the paste [0, n - k) and leaves the rest
    unwritten (and divides by zero at full == 2 k); on [0, n - k) both read the same tile at the same origin;
  - an origin is visited once.  The reference's count ceil(full / step) repeats the clamped last origin; a repeat pastes the same values again.

Lengths are in units of `unit` image pixels: decode walks the latent (unit f = 8, k = 8), encode the image (unit 1, k = 64)."""
import numpy as np

import oracle_lib as O

F_DOWN = 8


def tile_len(full, tile_px, unit, k):
    return min((tile_px + 63) // 64 * 64 // unit + 2 * k, full)


def walk(full, tile_px, unit, k):
    """(n, [(origin, lo, hi)]): tile length and, per tile in paste order, where it starts and the half-open window [lo, hi) of the OUTPUT it writes"""
    n = tile_len(full, tile_px, unit, k)
    if n == full:
        return n, [(0, 0, full)]
    step, last = n - 2 * k, full - n
    out, t = [(0, 0, n - k)], 1
    while out[-1][0] != last:
        i0 = min(t * step, last)
        out.append((i0, i0 + k, i0 + n))
        t += 1
    return n, out


def walk_records(full, tile_px, unit, k):
    """the same as (n, origins, source offsets, paste widths): the form mlis_amd_vae_tile_walk reports"""
    n, w = walk(full, tile_px, unit, k)
    return n, [o for o, _, _ in w], [lo - o for o, lo, _ in w], [hi - lo for _, lo, hi in w]


def windows(w_full, h_full, tile_px, unit, k):
    """(n0, n1, [((i0, i1), (x_lo, x_hi), (y_lo, y_hi))]) of a 2-D walk, rows outermost like the reference's loops"""
    n0, w0 = walk(w_full, tile_px, unit, k)
    n1, w1 = walk(h_full, tile_px, unit, k)
    return n0, n1, [((a[0], b[0]), a[1:], b[1:]) for b in w1 for a in w0]


def compose(out, tiles, wins, scale_num=1, scale_den=1):
    """paste tiles[(i0, i1)] ([..., n1', n0'] arrays) into out by the windows; window coordinates times scale_num / scale_den are out's pixels"""
    s = lambda v: v * scale_num // scale_den
    for (i0, i1), (x0, x1), (y0, y1) in wins:
        t = tiles[(i0, i1)]
        out[..., s(y0):s(y1), s(x0):s(x1)] = t[..., s(y0 - i1):s(y1 - i1), s(x0 - i0):s(x1 - i0)]
    return out


class Oracle:
    """the oracle's untiled VAE of one model with its synthetic weights; results of tile slices are kept by (content, origin)"""

    def __init__(self, model="tiny", seed=1234):
        self.P, self.V = O.Params(seed), O.vae_params(model)
        self.cache = {}

    def _run(self, f, x):
        t = O.to_ot(x[None])
        try:
            return O.from_ot(f(self.P.h, b"vae", self.V, t))[0]
        finally:
            O.L().ot_free(t)

    def decode(self, z):                   # [4][h][w] -> [3][8h][8w]
        return self._run(O.L().orc_vae_decode, z)

    def moments(self, img):                # [3][H][W] -> [8][H/8][W/8]
        return self._run(O.L().orc_vae_encode_moments, img)

    def tile(self, what, full, n0, n1, i0, i1):
        key = (what, full.shape, hash(full.tobytes()), n0, n1, i0, i1)
        if key not in self.cache:
            f = self.decode if what == "dec" else self.moments
            self.cache[key] = f(np.ascontiguousarray(full[:, i1:i1 + n1, i0:i0 + n0]))
        return self.cache[key]


def decode_ref(orc, z, tile_px):
    """z [B][4][lh][lw] -> (image [B][3][8 lh][8 lw], the paste windows in IMAGE pixels [((x_lo, x_hi), (y_lo, y_hi))], distinct tiles)"""
    B, _, lh, lw = z.shape
    n0, n1, wins = windows(lw, lh, tile_px, F_DOWN, 8)
    img = np.full((B, 3, lh * F_DOWN, lw * F_DOWN), np.nan, np.float32)
    for b in range(B):
        tiles = {o: orc.tile("dec", z[b], n0, n1, *o) for o, _, _ in wins}
        compose(img[b], tiles, wins, F_DOWN, 1)
    return img, [tuple((lo * F_DOWN, hi * F_DOWN) for lo, hi in w[1:]) for w in wins], len({w[0] for w in wins})


def encode_moments_ref(orc, img, tile_px):
    """img [B][3][H][W] in [0, 1] -> (moments [B][8][H/8][W/8], the paste windows in LATENT pixels, distinct tiles)"""
    B, _, H, W = img.shape
    n0, n1, wins = windows(W, H, tile_px, 1, 8 * F_DOWN)
    mom = np.full((B, 8, H // F_DOWN, W // F_DOWN), np.nan, np.float32)
    for b in range(B):
        tiles = {o: orc.tile("enc", img[b], n0, n1, *o) for o, _, _ in wins}
        compose(mom[b], tiles, wins, 1, F_DOWN)
    return mom, [tuple((lo // F_DOWN, hi // F_DOWN) for lo, hi in w[1:]) for w in wins], len({w[0] for w in wins})


def latent_sample(orc, mom, rnd=None):
    """orc_latent_sample per image: moments [B][8][h][w] (+ rnd [B][4 h w]) -> latent [B][4][h][w]; rnd None: the mean"""
    out = []
    for b in range(mom.shape[0]):
        m = O.to_ot(mom[b][None])
        out.append(O.from_ot(O.L().orc_latent_sample(m, orc.V, O.fptr(np.ascontiguousarray(rnd[b], np.float32)) if rnd is not None else None))[0])
        O.L().ot_free(m)
    return np.stack(out)
