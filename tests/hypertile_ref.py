"""HyperTile restated for the tests: the tile rule in Python, the row permutation in numpy, and the torch reference -- tools/torch_ref.Net with every UNet
self-attention computed inside tiles of its token map, as the published code does around attn1:

    'b (nh th) (nw tw) c -> (b nh nw) (th tw) c'   before the self-attention, and back after it.

Nothing else changes: the convolutions, norms, Linear layers and the cross-attention see the whole map.  The subclass works wherever a Net does
(controlnet_ref.controlnet / unet_controlled, freeu_ref.unet_freeu), so the compositions have references too.

The rule (include/mlimgsynth_amd.h, mlis_amd_hypertile_side): m = min(max(tile_px // px_per_token, 4), side); the smallest divisor of side that is >= m.  A level
of h x w tokens at UNet downscale ds (px_per_token = 8 ds) is tiled when (side(h), side(w)) != (h, w) and log2(ds) <= depth."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import controlnet_ref as CR         # noqa: E402
from tools import torch_ref as TR   # noqa: E402

eps_rows, unmix, rel_l2, UNET = CR.eps_rows, CR.unmix, CR.rel_l2, CR.UNET


def side(n, px_per_token, tile_px):
    m = min(max(tile_px // px_per_token, 4), n)
    while n % m:
        m += 1
    return m


def level_tile(h, w, ds, tile_px, depth):
    """(th, tw) of a map of h x w tokens at downscale ds, or None when the level is not tiled"""
    lvl = ds.bit_length() - 1
    if not tile_px or lvl > depth:
        return None
    th, tw = side(h, 8 * ds, tile_px), side(w, 8 * ds, tile_px)
    return None if (th, tw) == (h, w) else (th, tw)


def plan_info(model, w, h, tile_px, depth):
    """what mlis_amd_hypertile_info reports for a UNet plan of w x h latent pixels: (n_tiled, n_untiled, [(th, tw, nh, nw)] * 4), from the walk of the UNet: per
    level n_res_blk encoder and n_res_blk + 1 decoder transformers where ds is in attn_res, and the middle block's at the deepest level"""
    P = UNET[model]
    n_tiled = n_untiled = 0
    tiles = [(0, 0, 0, 0)] * 4
    top = len(P["ch_mult"]) - 1
    for level in range(top + 1):
        ds = 1 << level
        count = (2 * P["n_res_blk"] + 1 if ds in P["attn_res"] else 0) + (1 if level == top else 0)
        t = level_tile(h, w, ds, tile_px, depth)
        if t and count:
            tiles[level] = (t[0], t[1], h // t[0], w // t[1])
            n_tiled += count
        else:
            n_untiled += count
        h, w = (h + 1) // 2, (w + 1) // 2
    return n_tiled, n_untiled, tiles


def permute_rows(x, n_img, H, W, th, tw, inverse=False):
    """mlsd_tile_permute on an array of n_img H W rows (any trailing shape): image order -> tile-major order, or back"""
    x = np.asarray(x)
    rest = x.shape[1:]
    nh, nw = H // th, W // tw
    if not inverse:
        return np.ascontiguousarray(x.reshape((n_img, nh, th, nw, tw) + rest).swapaxes(2, 3)).reshape(x.shape)
    return np.ascontiguousarray(x.reshape((n_img, nh, nw, th, tw) + rest).swapaxes(2, 3)).reshape(x.shape)


class HyperNet(TR.Net):
    """Net with HyperTile around the self-attention of every spatial transformer.  The downscale of a level is found from the size of the map that entered the
    network's first convolution ("<prefix>.in.conv": the UNet's and the ControlNet's alike)."""

    def __init__(self, weights, tile_px, depth=3, **kw):
        super().__init__(weights, **kw)
        self.tile_px, self.depth, self.root, self.cur, self.log = tile_px, depth, None, None, []

    def conv(self, x, name, ch_out, k=3, stride=1, pad=1, bias=True):
        if name.endswith(".in.conv"):
            self.root = (x.shape[2], x.shape[3])
        return super().conv(x, name, ch_out, k, stride, pad, bias)

    def spatial_transformer(self, x, ctx, name, n_head, depth):
        H, W = x.shape[2], x.shape[3]
        ds, h = 1, self.root[0]
        while h != H:
            h, ds = (h + 1) // 2, ds * 2
        t = level_tile(H, W, ds, self.tile_px, self.depth)
        self.cur = (H, W) + t if t else None
        self.log.append((name, ds, t))
        try:
            return super().spatial_transformer(x, ctx, name, n_head, depth)
        finally:
            self.cur = None

    def mha(self, xq, xkv, name, d_out, d_embed, n_head, causal=False, bias=False, bias_out=True):
        if xq is not xkv or self.cur is None:
            return super().mha(xq, xkv, name, d_out, d_embed, n_head, causal, bias, bias_out)
        H, W, th, tw = self.cur
        B, T, Cn = xq.shape
        assert T == H * W
        nh, nw = H // th, W // tw
        x = xq.reshape(B, nh, th, nw, tw, Cn).permute(0, 1, 3, 2, 4, 5).reshape(B * nh * nw, th * tw, Cn)
        y = super().mha(x, x, name, d_out, d_embed, n_head, causal, bias, bias_out)
        return y.reshape(B, nh, nw, th, tw, d_out).permute(0, 1, 3, 2, 4, 5).reshape(B, T, d_out)


def make_net(tile_px, depth=3):
    return HyperNet(TR.Weights(CR.synth), tile_px, depth, f16_ops=True)
