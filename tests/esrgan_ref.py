"""The yardstick of the upscaler tests: RRDBNet x4 (ESRGAN / Real-ESRGAN as published with BasicSR, AS RECALLED: no publication and no weight file were at hand) restated twice
in float64, independently of each other and of the engine --

    forward_numpy   on ref64.im2col64 / ref64.gemm64 (channels-last, the arithmetic the kernel tests use)
    forward_torch   on torch.nn.functional.conv2d / interpolate (planar)

tests/test_upscale_cpu.py holds the two to each other at 1e-12.  The reference project has no upscaler, and no ESRGAN file exists on the machines the tests run on.

    fea   = conv_first(x)                      3 -> 64
    trunk = conv_body(RRDB^nb(fea));  fea = fea + trunk
    fea   = lrelu(conv_up1(nearest2x(fea)));   fea = lrelu(conv_up2(nearest2x(fea)))
    out   = conv_last(lrelu(conv_hr(fea)))     64 -> 64 -> 3
    RDB : x1 = lrelu(conv1(x)); ... x4 = lrelu(conv4(x|x1|x2|x3)); out = 0.2 conv5(x|x1|x2|x3|x4) + x
    RRDB: out = 0.2 rdb3(rdb2(rdb1(x))) + x

Shared with the engine: DATA only -- the tensor names (BasicSR's) and the synthetic weight rule keyed by (seed, name), oracle orc_synth_fill with standard deviation
0.1 sqrt(2 / fan_in) for the dense blocks' weights, sqrt(2 / fan_in) for the other convolutions and 0.05 for biases.  `knobs` breaks the net on purpose (the discrimination test): rdb / rrdb = the two residual scales, slope = the
LeakyReLU slope, skip = whether fea + trunk is added."""
import math

import numpy as np

import ref64

FEAT, GROW = 64, 32
KNOBS = dict(rdb=0.2, rrdb=0.2, slope=0.2, skip=True)


def conv_names(n_block):
    """(name, cin, cout) of every convolution, in the file's naming"""
    out = [("conv_first", 3, FEAT)]
    for i in range(n_block):
        for j in range(1, 4):
            for k in range(1, 6):
                out.append((f"body.{i}.rdb{j}.conv{k}", FEAT + GROW * (k - 1), GROW if k < 5 else FEAT))
    out += [("conv_body", FEAT, FEAT), ("conv_up1", FEAT, FEAT), ("conv_up2", FEAT, FEAT), ("conv_hr", FEAT, FEAT), ("conv_last", FEAT, 3)]
    return out


def synth_weights(seed=1234, n_block=2):
    """{name.weight: float32 [cout, cin, 3, 3] holding fp16 values, name.bias: float32 [cout]} of the model "synth:<seed>:<n_block>" """
    import oracle_lib as O
    w = {}
    for name, cin, cout in conv_names(n_block):
        a = np.empty(cout * cin * 9, np.float32)
        O.L().orc_synth_fill(O.fptr(a), a.size, seed, (name + ".weight").encode(), 0.0, float(np.float32((0.1 if name.startswith("body.") else 1.0) * math.sqrt(2.0 / (9.0 * cin)))), 1)
        b = np.empty(cout, np.float32)
        O.L().orc_synth_fill(O.fptr(b), b.size, seed, (name + ".bias").encode(), 0.0, float(np.float32(0.05)), 0)
        w[name + ".weight"], w[name + ".bias"] = a.reshape(cout, cin, 3, 3), b
    return w


def n_blocks(w):
    n = 0
    while f"body.{n}.rdb1.conv1.weight" in w:
        n += 1
    return n


# ------------------------------------------------------------------ numpy, channels-last
def _conv_np(w, name, x, ups=False):
    n, H, W, C = x.shape
    OH, OW = (2 * H, 2 * W) if ups else (H, W)
    A = ref64.im2col64(x.reshape(-1, C), n, H, W, C, 3, 3, 1, 1, 1 if ups else 0, OH, OW)
    Wt = np.asarray(w[name + ".weight"], np.float64).transpose(0, 2, 3, 1).reshape(-1, 9 * C)          # [cout][kh][kw][cin]
    acc, _ = ref64.gemm64(A, Wt)
    return (acc + np.asarray(w[name + ".bias"], np.float64)[None, :]).reshape(n, OH, OW, -1)


def forward_numpy(w, x, **knobs):
    """x [n, 3, h, w] -> [n, 3, 4h, 4w], float64"""
    k = dict(KNOBS, **knobs)
    lrelu = lambda v: np.where(v >= 0, v, k["slope"] * v)
    fea = _conv_np(w, "conv_first", np.asarray(x, np.float64).transpose(0, 2, 3, 1))
    t = fea
    for i in range(n_blocks(w)):
        t_in = t
        for j in range(1, 4):
            p = f"body.{i}.rdb{j}."
            d = t
            for c in range(1, 5):
                d = np.concatenate([d, lrelu(_conv_np(w, p + f"conv{c}", d))], axis=-1)
            t = k["rdb"] * _conv_np(w, p + "conv5", d) + t
        t = k["rrdb"] * t + t_in
    trunk = _conv_np(w, "conv_body", t)
    fea = fea + trunk if k["skip"] else trunk
    fea = lrelu(_conv_np(w, "conv_up1", fea, ups=True))
    fea = lrelu(_conv_np(w, "conv_up2", fea, ups=True))
    return _conv_np(w, "conv_last", lrelu(_conv_np(w, "conv_hr", fea))).transpose(0, 3, 1, 2)


# ------------------------------------------------------------------ torch, planar
def forward_torch(w, x, **knobs):
    import torch
    import torch.nn.functional as TF
    k = dict(KNOBS, **knobs)
    T = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    conv = lambda name, v: TF.conv2d(v, T(w[name + ".weight"]), T(w[name + ".bias"]), stride=1, padding=1)
    lrelu = lambda v: TF.leaky_relu(v, negative_slope=k["slope"])
    up = lambda v: TF.interpolate(v, scale_factor=2, mode="nearest")
    fea = conv("conv_first", T(x))
    t = fea
    for i in range(n_blocks(w)):
        rrdb_in = t
        for j in range(1, 4):
            p = f"body.{i}.rdb{j}."
            x1 = lrelu(conv(p + "conv1", t))
            x2 = lrelu(conv(p + "conv2", torch.cat((t, x1), 1)))
            x3 = lrelu(conv(p + "conv3", torch.cat((t, x1, x2), 1)))
            x4 = lrelu(conv(p + "conv4", torch.cat((t, x1, x2, x3), 1)))
            t = conv(p + "conv5", torch.cat((t, x1, x2, x3, x4), 1)) * k["rdb"] + t
        t = t * k["rrdb"] + rrdb_in
    trunk = conv("conv_body", t)
    fea = fea + trunk if k["skip"] else trunk
    fea = lrelu(conv("conv_up1", up(fea)))
    fea = lrelu(conv("conv_up2", up(fea)))
    return conv("conv_last", lrelu(conv("conv_hr", fea))).numpy()


def rel_l2(got, want):
    """per image"""
    g, r = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ax = tuple(range(1, g.ndim))
    return np.sqrt(((g - r) ** 2).sum(axis=ax) / (r ** 2).sum(axis=ax))


def test_input(n, h, w, seed=5):
    """planar images in 0..1 with structure at every scale (smooth ramps + noise), different per image"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.empty((n, 3, h, w), np.float32)
    for b in range(n):
        for c in range(3):
            out[b, c] = 0.5 + 0.3 * np.sin(0.9 * xx + 0.7 * c + b) * np.cos(0.6 * yy - 0.4 * b) + 0.2 * (rng.random((h, w)) - 0.5)
    return np.clip(out, 0, 1)


test_input.__test__ = False


def old_name(key, n_block):
    """the first ESRGAN release's naming (an nn.Sequential), as recalled and unverified: conv_first model.0, the blocks model.1.sub.{i}.RDB{j}.conv{k}.0, conv_body
    model.1.sub.{n_block}, conv_up1 model.3, conv_up2 model.6, conv_hr model.8, conv_last model.10"""
    import re
    name, suffix = key.rsplit(".", 1)
    m = re.fullmatch(r"body\.(\d+)\.rdb(\d)\.conv(\d)", name)
    if m:
        return f"model.1.sub.{m.group(1)}.RDB{m.group(2)}.conv{m.group(3)}.0.{suffix}"
    fixed = dict(conv_first="model.0", conv_body=f"model.1.sub.{n_block}", conv_up1="model.3", conv_up2="model.6", conv_hr="model.8", conv_last="model.10")
    return f"{fixed[name]}.{suffix}"


def save_safetensors(path, w, prefix="", f16=True, old_names=False):
    from safetensors.numpy import save_file
    if old_names:
        nb = n_blocks(w)
        w = {old_name(k, nb): v for k, v in w.items()}
    save_file({prefix + k: np.ascontiguousarray(v.astype(np.float16) if (f16 and k.endswith(".weight")) else v.astype(np.float32)) for k, v in w.items()}, path)
