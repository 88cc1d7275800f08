"""Perturbed-attention guidance restated for the tests, on tools/torch_ref.Net (f16_ops=True):

    perturbed evaluation   the UNet on the cond row's inputs with, in the self-attentions of the MIDDLE block's spatial transformer
                           ("<prefix>.mid.1.transf.<i>.attn1"), softmax(q k^T) v replaced by v:  attn1(x) = out_proj(v_proj(x))
    mix                    dx = g + s (c - p),  g = c f + u (1 - f)  (or c at f <= 1),  on the rows after the v-prediction rescale

The rule is the one include/mlimgsynth_amd.h states, as recalled from the publication ("Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance",
2024): parity with the published code is not pinned.  The perturbation is a mixin over Net.mha, so it composes with the other subclasses
(hypertile_ref.HyperNet: the identity inside a tile is the identity) and works wherever a Net does (controlnet_ref, freeu_ref)."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import controlnet_ref as CR         # noqa: E402
import hypertile_ref as HR          # noqa: E402
from tools import torch_ref as TR   # noqa: E402

rel_l2, UNET = CR.rel_l2, CR.UNET
N_ATTN = {"sd1": 1, "sd2": 1, "sdxl": 10, "tiny": 1, "tinyv": 1, "tinyxl": 2}      # transf_depth of the deepest level: the self-attentions of mid.1


class _Perturb:
    """mha of names matching <prefix>.mid.1.transf.*.attn1 returns out_proj(v_proj(x)) while `perturb` is on"""
    perturb, pag_prefix, pag_hits = False, "unet", 0

    def mha(self, xq, xkv, name, d_out, d_embed, n_head, causal=False, bias=False, bias_out=True):
        if self.perturb and xq is xkv and re.fullmatch(re.escape(self.pag_prefix) + r"\.mid\.1\.transf\.\d+\.attn1", name):
            self.pag_hits += 1
            return self.linear(self.linear(xkv, name + ".v_proj", d_embed, bias), name + ".out_proj", d_out, bias_out)
        return super().mha(xq, xkv, name, d_out, d_embed, n_head, causal, bias, bias_out)


class PagNet(_Perturb, TR.Net):
    pass


class PagHyperNet(_Perturb, HR.HyperNet):
    """(the perturbed branch is per token, so it does not matter that HyperNet hands it tile-shaped batches)"""


def make_net(tile_px=0, depth=3):
    if tile_px:
        return PagHyperNet(TR.Weights(CR.synth), tile_px, depth, f16_ops=True)
    return PagNet(TR.Weights(CR.synth), f16_ops=True)


def eps_rows(net, model, x, sigma, cond, label, uncond, unlabel, cfg=2.0, hint=None, gain=1.0, rows_fn=None):
    """the rows of one evaluation of a PAG engine with batch B = len(x): controlnet_ref.eps_rows ([cond B | uncond B]; only [cond B] at cfg <= 1) with the perturbed
    group appended -- the cond rows evaluated again with the switch on (the control, where there is one, on them as well).  rows_fn: another eps_rows with the
    signature of controlnet_ref's (freeu_ref's with its factors bound).  Returns [N,4,h,w] float32."""
    B = x.shape[0]
    rows_fn = rows_fn or CR.eps_rows
    kw = dict(hint=hint, gain=gain) if hint is not None else {}
    net.perturb = False
    plain = rows_fn(net, model, x, sigma, cond, label, uncond, unlabel, **kw)
    net.perturb, net.pag_hits = True, 0
    try:
        pert = rows_fn(net, model, x, sigma, cond, label, cond, label, **kw)[:B]
    finally:
        net.perturb = False
    assert net.pag_hits == 2 * N_ATTN[model] or net.pag_hits == N_ATTN[model], net.pag_hits      # (rows_fn evaluates 2B rows in one batch, or in two)
    return np.concatenate([plain if cfg > 1 else plain[:B], pert]).astype(np.float32)


def mix(eps, cfg, s):
    """mlsd_dxdt_pag on rows that already carry the v-prediction rescale: numpy fp32, every operation rounded once, in the kernel's order"""
    eps = np.asarray(eps, np.float32)
    f, s = np.float32(cfg), np.float32(s)
    B = len(eps) // (3 if cfg > 1 else 2)
    c, p = eps[:B], eps[-B:]
    g = (c * f + eps[B:2 * B] * (np.float32(1) - f)).astype(np.float32) if cfg > 1 else c
    if s == 0:
        return g.astype(np.float32)
    return (g + s * (c - p)).astype(np.float32)


def unmix(d, cfg):
    """The rows behind mlis_amd_dxdt, in float64.  cfg > 1: d = its answers at (cfg, s) = (2, 1), (3, 1), (2, 2):  e = d3 - d1 = c - p,  c = 2 (d1 - e) - (d2 - e),
    u = 3 (d1 - e) - 2 (d2 - e),  p = c - e.  cfg <= 1: d = its answers at s = 1 and 2:  e = d2 - d1,  c = d1 - e,  p = c - e.  The evaluations are deterministic, so
    every answer mixes the same rows: the un-mixing adds a few fp32 roundings of the mix, not a multiple of the evaluations' error."""
    d = [np.asarray(a, np.float64) for a in d]
    if cfg > 1:
        d1, d2, d3 = d
        e = d3 - d1
        c = 2 * (d1 - e) - (d2 - e)
        u = 3 * (d1 - e) - 2 * (d2 - e)
        return np.concatenate([c, u, c - e])
    d1, d2 = d
    e = d2 - d1
    c = d1 - e
    return np.concatenate([c, c - e])
