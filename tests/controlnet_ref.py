"""fp32 CPU restatement of the ControlNet and of the UNet it controls, on tools/torch_ref.Net (f16_ops=True: ggml's F16 operand rounding), written from the
published cldm.py (ControlNet.forward, ControlledUnetModel.forward):

    controlnet(net, P, x, t, ctx, label, hint)      -> [r_0 .. r_{k-1}, r_mid]: zero_convs on what the UNet pushes on its skip stack, middle_block_out last
    unet_controlled(net, P, x, t, ctx, label, residuals, gain)
                                                    -> the UNet with h = mid(h) + gain r_mid and every popped skip tensor + gain r_i before the concat
    dxdt(...)                                       -> what mlis_amd_dxdt returns: c_in scaling, sigma -> t, cond and uncond rows, v-prediction rescale, CFG mix

Shared with the engine: DATA only -- the parameter names ("control.<...>", as tnconv_controlnet produces them) and the synthetic weight rule keyed by
(seed, name, shape) (oracle orc_synth_rule / orc_synth_fill == mlctx_params_synth).  No ControlNet checkpoint exists on the machines the tests run on."""
import ctypes
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import golden_cases as G            # noqa: E402
import oracle_lib as O              # noqa: E402
from tools import torch_ref as TR   # noqa: E402

HINT_WIDTHS = (16, 16, 32, 32, 96, 96, 256)          # cldm.py input_hint_block, then model_channels
HINT_STRIDES = (1, 1, 2, 1, 2, 1, 2, 1)

UNET = dict(G.UNET)
UNET["tinyv"] = dict(G.UNET["tiny"], n_head=0, d_head=32, vparam=1)      # unet_params_get("tinyv"): tiny with v-prediction


def synth(name, shape, f16, seed=G.WEIGHT_SEED):
    """the synthetic weight rule (tools/make_torch_golden.py:30): DATA"""
    ne = (ctypes.c_int64 * 4)(*(list(shape)[::-1] + [1] * (4 - len(shape))))
    off, sc = ctypes.c_float(), ctypes.c_float()
    O.L().orc_synth_rule(name.encode(), 1 if f16 else 0, ctypes.byref(ne), ctypes.byref(off), ctypes.byref(sc))
    out = np.empty(int(np.prod(shape)), np.float32)
    O.L().orc_synth_fill(O.fptr(out), out.size, seed, name.encode(), off.value, sc.value, 1 if f16 else 0)
    return out.reshape(shape)


def make_net():
    return TR.Net(TR.Weights(synth), f16_ops=True)


def _emb(net, P, t, label, p):
    half = P["n_ch"] // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    temb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    emb = net.linear(F.silu(net.linear(temb, p + "time_embed.0", P["n_te"])), p + "time_embed.2", P["n_te"])
    if P.get("ch_adm_in") and label is not None:
        emb = emb + net.linear(F.silu(net.linear(label, p + "label_embed.0", P["n_te"])), p + "label_embed.2", P["n_te"])
    return emb


def _heads(P, ch):
    return P["n_head"] if P.get("n_head") else ch // P["d_head"]


def hint_block(net, P, hint, prefix="control"):
    """input_hint_block: conv, SiLU, ... conv (no SiLU after the last): hint [1,3,H,W] -> [1,n_ch,H/8,W/8]"""
    h = hint
    for i in range(8):
        h = net.conv(h, f"{prefix}.hint.{2 * i}", HINT_WIDTHS[i] if i < 7 else P["n_ch"], stride=HINT_STRIDES[i])
        if i < 7:
            h = F.silu(h)
    return h


def controlnet(net, P, x, t, ctx, label, hint, prefix="control", guided=None):
    """ControlNet.forward.  hint: the control image [1,3,8h,8w] shared by the batch, or `guided` = its embedding [1 or N, n_ch, h, w] (a tiled engine's crop)"""
    p = prefix + "."
    emb = _emb(net, P, t, label, p)
    g = hint_block(net, P, hint, prefix) if guided is None else guided
    outs = []

    def zero(h):
        outs.append(net.conv(h, f"{p}zero.{len(outs)}", h.shape[1], k=1, pad=0))

    h = net.conv(x, p + "in.conv", P["n_ch"]) + g              # guided_hint is added after the first input block only
    zero(h)
    blk, ds = 0, 1
    for level, mult in enumerate(P["ch_mult"]):
        if level:
            ds *= 2
            blk += 1
            h = net.conv(h, f"{p}in.{blk}.0.conv", h.shape[1], stride=2)
            zero(h)
        for _ in range(P["n_res_blk"]):
            blk += 1
            ch = P["n_ch"] * mult
            h = net.resblock(h, emb, f"{p}in.{blk}.0", ch)
            if ds in P["attn_res"]:
                h = net.spatial_transformer(h, ctx, f"{p}in.{blk}.1", _heads(P, ch), P["transf_depth"][level])
            zero(h)
    ch = P["n_ch"] * P["ch_mult"][-1]
    top = len(P["ch_mult"]) - 1
    h = net.resblock(h, emb, p + "mid.0", ch)
    h = net.spatial_transformer(h, ctx, p + "mid.1", _heads(P, ch), P["transf_depth"][top])
    h = net.resblock(h, emb, p + "mid.2", ch)
    outs.append(net.conv(h, p + "mid_out", ch, k=1, pad=0))
    return outs


def unet_controlled(net, P, x, t, ctx, label, residuals, gain, prefix="unet"):
    """ControlledUnetModel.forward: Net.unet with  h = middle(h) + gain control.pop()  and  cat([h, hs.pop() + gain control.pop()])"""
    p = prefix + "."
    emb = _emb(net, P, t, label, p)
    ctl = list(residuals)
    gain = float(gain)
    hs = []
    h = net.conv(x, p + "in.conv", P["n_ch"])
    hs.append(h)
    blk, ds = 0, 1
    for level, mult in enumerate(P["ch_mult"]):
        if level:
            ds *= 2
            blk += 1
            h = net.conv(h, f"{p}in.{blk}.0.conv", h.shape[1], stride=2)
            hs.append(h)
        for _ in range(P["n_res_blk"]):
            blk += 1
            ch = P["n_ch"] * mult
            h = net.resblock(h, emb, f"{p}in.{blk}.0", ch)
            if ds in P["attn_res"]:
                h = net.spatial_transformer(h, ctx, f"{p}in.{blk}.1", _heads(P, ch), P["transf_depth"][level])
            hs.append(h)
    assert len(ctl) == len(hs) + 1
    ch = P["n_ch"] * P["ch_mult"][-1]
    top = len(P["ch_mult"]) - 1
    h = net.resblock(h, emb, p + "mid.0", ch)
    h = net.spatial_transformer(h, ctx, p + "mid.1", _heads(P, ch), P["transf_depth"][top])
    h = net.resblock(h, emb, p + "mid.2", ch)
    h = h + gain * ctl.pop()
    ob = 0
    for level in range(top, -1, -1):
        ch = P["n_ch"] * P["ch_mult"][level]
        for j in range(P["n_res_blk"] + 1):
            h = torch.cat([h, hs.pop() + gain * ctl.pop()], dim=1)
            sub = 0
            h = net.resblock(h, emb, f"{p}out.{ob}.{sub}", ch)
            sub += 1
            if ds in P["attn_res"]:
                h = net.spatial_transformer(h, ctx, f"{p}out.{ob}.{sub}", _heads(P, ch), P["transf_depth"][level])
                sub += 1
            if level and j == P["n_res_blk"]:
                h = F.interpolate(h, scale_factor=2, mode="nearest")
                h = net.conv(h, f"{p}out.{ob}.{sub}.conv", ch)
                ds //= 2
            ob += 1
    assert not hs and not ctl
    return net.conv(F.silu(net.gn(h, p + "out.norm")), p + "out.conv", P["n_ch_out"])


def eps_rows(net, model, x, sigma, cond, label, uncond, unlabel, hint=None, gain=1.0, guided=None):
    """the N = 2B evaluations behind one mlis_amd_dxdt of an engine with batch B = len(x) and guidance on: c_in scaling, sigma -> t, the cond rows of every
    image then the uncond rows, the control on both halves, the v-prediction rescale.  hint None and guided None: the uncontrolled UNet (Net.unet).
    Returns [2B,4,h,w] float32."""
    P = UNET[model]
    B = x.shape[0]
    s = np.float32(sigma)
    t = O.L().orc_sigma_to_t(float(s))
    c_in = np.float32(1) / np.sqrt(s * s + np.float32(1), dtype=np.float32)
    with torch.no_grad():
        xs = torch.from_numpy(np.concatenate([x, x]) * c_in)
        ts = torch.full((2 * B,), float(t))
        cs = torch.from_numpy(np.stack([cond] * B + [uncond] * B))
        ls = torch.from_numpy(np.stack([label] * B + [unlabel] * B)) if P.get("ch_adm_in") else None
        if hint is None and guided is None:
            eps = net.unet(P, xs, ts, cs, ls)
        else:
            res = controlnet(net, P, xs, ts, cs, ls, torch.from_numpy(hint) if hint is not None else None, guided=guided)
            eps = unet_controlled(net, P, xs, ts, cs, ls, res, gain)
        eps = eps.numpy()
    if P.get("vparam"):
        c_out, c_skip = np.float32(1) / np.sqrt(s * s + 1, dtype=np.float32), s / (s * s + np.float32(1))
        eps = eps * c_out + np.concatenate([x, x]) * c_skip
    return eps.astype(np.float32)


def mix(eps, cfg):
    """the CFG mix of mlis_amd_dxdt: dx = cond cfg + uncond (1 - cfg)"""
    B = len(eps) // 2
    return (eps[:B] * np.float32(cfg) + eps[B:] * (np.float32(1) - np.float32(cfg))).astype(np.float32)


def dxdt(net, model, x, sigma, cond, label, uncond, unlabel, cfg, hint=None, gain=1.0, guided=None):
    """what mlis_amd_dxdt returns: dx [B,4,h,w] float32"""
    return mix(eps_rows(net, model, x, sigma, cond, label, uncond, unlabel, hint, gain, guided), cfg)


def unmix(dx2, dx3):
    """The two halves behind mlis_amd_dxdt, from its answers at cfg 2 and cfg 3 on the same inputs: dx2 = 2 c - u and dx3 = 3 c - 2 u give c = 2 dx2 - dx3 and
    u = 3 dx2 - 2 dx3 (float64).  The engine's evaluations are deterministic, so both answers mix the SAME c and u: the un-mixing adds a few fp32 roundings of the
    mix (1e-6 relative), not a multiple of the evaluations' error, which a comparison of the mixed dx at cfg 7 would (by cfg + |1 - cfg| = 13)."""
    a, b = np.asarray(dx2, np.float64), np.asarray(dx3, np.float64)
    return np.concatenate([2 * a - b, 3 * a - 2 * b])


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
