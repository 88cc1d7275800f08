"""float64 restatement of FreeU (version 2 of the published code) and the UNet that carries it, for the FreeU tests:

    fourier_filter64(x, scale)          the published Fourier_filter with threshold 1 on [.., H, W]: fftn, fftshift, mask, ifftshift, ifftn, .real
    fourier_closed64(x, scale)          the closed form the kernel computes: x + (s - 1) / (H W) sum x' (1 + cos t + cos f + cos(t + f)); equal for H, W >= 2
    backbone64(x, b)                    x [N, C, H, W]: the first C / 2 channels times (b - 1) x the per-image normalised channel mean + 1
    unet_freeu(net, P, x, t, ctx, label, b1, b2, s1, s2, residuals=None, gain=0)
                                        controlnet_ref.unet_controlled with the two hooks in front of every decoder concatenation
    eps_rows(...)                       the N = 2B evaluations behind one mlis_amd_dxdt, as controlnet_ref.eps_rows, with FreeU

The stage follows the backbone's channel count, as the published forward does: n_ch x the top multiplier is stage 1 (b1, s1), half of it stage 2 (b2, s2).
Where a channel-mean map is constant (max == min) the published code divides by zero; here, as in the engine, the factor is 1."""
import numpy as np
import torch

import controlnet_ref as R
import oracle_lib as O

# decoder concatenations treated per model: (stage 1, stage 2); from the walk of the decoder (backbone channels at every concatenation)
COUNTS = {"sd1": (7, 3), "sd2": (7, 3), "sdxl": (4, 3), "tiny": (3, 1), "tinyv": (3, 1), "tinyxl": (4, 2)}


def fourier_filter64(x, scale):
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    f = np.fft.fftshift(np.fft.fftn(x, axes=(-2, -1)), axes=(-2, -1))
    mask = np.ones(x.shape, np.float64)
    crow, ccol = H // 2, W // 2
    mask[..., crow - 1:crow + 1, ccol - 1:ccol + 1] = scale
    f = np.fft.ifftshift(f * mask, axes=(-2, -1))
    return np.fft.ifftn(f, axes=(-2, -1)).real


def fourier_closed64(x, scale):
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2:]
    y, xx = np.arange(H), np.arange(W)
    th = 2 * np.pi * (y[:, None] - y[None, :]) / H          # [y', y]
    ph = 2 * np.pi * (xx[:, None] - xx[None, :]) / W        # [x', x]
    k = 1 + np.cos(th)[:, None, :, None] + np.cos(ph)[None, :, None, :] + np.cos(th[:, None, :, None] + ph[None, :, None, :])      # [y', x', y, x]
    return x + (scale - 1.0) / (H * W) * np.einsum("...ab,abyx->...yx", x, k)


def backbone64(x, b):
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    m = x.mean(axis=1, keepdims=True)
    mn, mx = m.min(axis=(2, 3), keepdims=True), m.max(axis=(2, 3), keepdims=True)
    span = mx - mn
    mh = np.where(span > 0, (m - mn) / np.where(span > 0, span, 1.0), 0.0)
    out = x.copy()
    out[:, :C // 2] = x[:, :C // 2] * np.where(span > 0, (b - 1.0) * mh + 1.0, 1.0)
    return out


def _hooks(P, h, hsk, b1, b2, s1, s2):
    top = P["n_ch"] * P["ch_mult"][-1]
    if h.shape[1] == top:
        b, s = b1, s1
    elif 2 * h.shape[1] == top:
        b, s = b2, s2
    else:
        return h, hsk, 0
    h = torch.from_numpy(backbone64(h.numpy(), float(np.float32(b))).astype(np.float32))
    hsk = torch.from_numpy(fourier_filter64(hsk.numpy(), float(np.float32(s))).astype(np.float32))
    return h, hsk, 1 if h.shape[1] == top else 2


def unet_freeu(net, P, x, t, ctx, label, b1, b2, s1, s2, residuals=None, gain=0, prefix="unet", stages=None):
    """controlnet_ref.unet_controlled (residuals None: no control sums at all) with FreeU in front of every decoder concatenation; `stages`, a list, receives
    the stage of every concatenation (0: untouched)"""
    import torch.nn.functional as F
    p = prefix + "."
    emb = R._emb(net, P, t, label, p)
    ctl = list(residuals) if residuals is not None else None
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
                h = net.spatial_transformer(h, ctx, f"{p}in.{blk}.1", R._heads(P, ch), P["transf_depth"][level])
            hs.append(h)
    ch = P["n_ch"] * P["ch_mult"][-1]
    top = len(P["ch_mult"]) - 1
    h = net.resblock(h, emb, p + "mid.0", ch)
    h = net.spatial_transformer(h, ctx, p + "mid.1", R._heads(P, ch), P["transf_depth"][top])
    h = net.resblock(h, emb, p + "mid.2", ch)
    if ctl is not None:
        assert len(ctl) == len(hs) + 1
        h = h + gain * ctl.pop()
    ob = 0
    for level in range(top, -1, -1):
        ch = P["n_ch"] * P["ch_mult"][level]
        for j in range(P["n_res_blk"] + 1):
            hsk = hs.pop()
            if ctl is not None:
                hsk = hsk + gain * ctl.pop()
            h, hsk, stage = _hooks(P, h, hsk, b1, b2, s1, s2)
            if stages is not None:
                stages.append(stage)
            h = torch.cat([h, hsk], dim=1)
            sub = 0
            h = net.resblock(h, emb, f"{p}out.{ob}.{sub}", ch)
            sub += 1
            if ds in P["attn_res"]:
                h = net.spatial_transformer(h, ctx, f"{p}out.{ob}.{sub}", R._heads(P, ch), P["transf_depth"][level])
                sub += 1
            if level and j == P["n_res_blk"]:
                h = F.interpolate(h, scale_factor=2, mode="nearest")
                h = net.conv(h, f"{p}out.{ob}.{sub}.conv", ch)
                ds //= 2
            ob += 1
    assert not hs and not ctl
    return net.conv(F.silu(net.gn(h, p + "out.norm")), p + "out.conv", P["n_ch_out"])


def eps_rows(net, model, x, sigma, cond, label, uncond, unlabel, factors, hint=None, gain=1.0):
    """controlnet_ref.eps_rows with FreeU (factors = (b1, b2, s1, s2)); hint given: with the ControlNet's residuals as well.  Returns [2B,4,h,w] float32."""
    P = R.UNET[model]
    B = x.shape[0]
    s = np.float32(sigma)
    t = O.L().orc_sigma_to_t(float(s))
    c_in = np.float32(1) / np.sqrt(s * s + np.float32(1), dtype=np.float32)
    with torch.no_grad():
        xs = torch.from_numpy(np.concatenate([x, x]) * c_in)
        ts = torch.full((2 * B,), float(t))
        cs = torch.from_numpy(np.stack([cond] * B + [uncond] * B))
        ls = torch.from_numpy(np.stack([label] * B + [unlabel] * B)) if P.get("ch_adm_in") else None
        res = R.controlnet(net, P, xs, ts, cs, ls, torch.from_numpy(hint)) if hint is not None else None
        eps = unet_freeu(net, P, xs, ts, cs, ls, *factors, residuals=res, gain=gain).numpy()
    if P.get("vparam"):
        c_out, c_skip = np.float32(1) / np.sqrt(s * s + 1, dtype=np.float32), s / (s * s + np.float32(1))
        eps = eps * c_out + np.concatenate([x, x]) * c_skip
    return eps.astype(np.float32)
