"""The yardstick of the compact-upscaler tests: one layer of SRVGGNetCompact (3x3 convolution, PReLU; for the tail the pixel shuffle and the added input) and the net built
on it, restated in float64 on ref64.im2col64 / ref64.gemm64, independently of the engine.  The network is the one include/mlsd_kernels.h states at mlsd_conv3x3_compact
(Real-ESRGAN / BasicSR srvgg_arch.py AS RECALLED: no weight file and no publication was at hand):

    body.0 conv 3 -> 64, body.1 PReLU;  N x (body.2k conv 64 -> 64, body.2k+1 PReLU);  body.(2N+2) conv 64 -> 3 s^2;  out = pixel_shuffle(body(x), s) + nearest_s(x)

Shared with the engine: DATA only -- BasicSR's tensor names and the synthetic rule of "synth-compact:seed:convs:scale" keyed by (seed, name): oracle orc_synth_fill with
deviation sqrt(2 / fan_in) for the convolutions (rounded to fp16), 0.05 for biases, and slopes 0.1 + deviation 0.1."""
import math

import numpy as np

import esrgan_ref as E
import ref64

FEAT = 64


def shuffle64(z, n, H, W, s):
    """[n H W][3 s s] -> planar [n][3][s H][s W]: channel c s^2 + dy s + dx of pixel (y, x) -> channel c of pixel (s y + dy, s x + dx)"""
    return z.reshape(n, H, W, 3, s, s).transpose(0, 3, 1, 4, 2, 5).reshape(n, 3, s * H, s * W)


def layer64(A, n, H, W, Wt, bias, slope=None, x=None, s=0):
    """A [n H W][Cin], Wt [Cout][3][3][Cin], bias [Cout] -> (y, z, S): z = conv + bias and S the sum of the products' magnitudes, both [n H W][Cout];
    y = PReLU(z) (slope [Cout] or None), or with s the planar [n][3][sH][sW] shuffle of z plus the nearest upsample of x [n][3][H][W]"""
    Cin = A.shape[1]
    acc, S = ref64.gemm64(ref64.im2col64(A, n, H, W, Cin, 3, 3, 1, 1, 0, H, W), np.asarray(Wt, np.float64).reshape(len(Wt), 9 * Cin))
    z = acc + np.asarray(bias, np.float64)[None, :]
    if s:
        return shuffle64(z, n, H, W, s) + np.repeat(np.repeat(np.asarray(x, np.float64), s, axis=2), s, axis=3), z, S
    return (z if slope is None else np.where(z >= 0, z, np.asarray(slope, np.float64)[None, :] * z)), z, S


def n_conv(w):
    t = 0
    while f"body.{2 * t}.weight" in w:
        t += 1
    return t - 2


def forward64(w, x, round16=False):
    """x [n][3][h][w] -> [n][3][s h][s w] in float64; round16: the activations between layers (and the input of the head) rounded to fp16, as the engine stores them"""
    r16 = (lambda v: ref64.fp16_rne(v)) if round16 else (lambda v: v)
    n, _, H, W = x.shape
    N = n_conv(w)
    s = math.isqrt(w[f"body.{2 * N + 2}.weight"].shape[0] // 3)
    a = r16(np.asarray(x, np.float64).transpose(0, 2, 3, 1).reshape(-1, 3))
    for i in range(N + 2):
        Wt = np.asarray(w[f"body.{2 * i}.weight"], np.float64).transpose(0, 2, 3, 1)
        if i == N + 1:
            return layer64(a, n, H, W, Wt, w[f"body.{2 * i}.bias"], x=x, s=s)[0]
        a = r16(layer64(a, n, H, W, Wt, w[f"body.{2 * i}.bias"], w[f"body.{2 * i + 1}.weight"])[0])


def synth_weights(seed, convs, scale):
    """the tensors of "synth-compact:<seed>:<convs>:<scale>" in BasicSR's names: convolutions [cout][cin][3][3] float32 holding fp16 values, biases and slopes float32"""
    import oracle_lib as O

    def fill(name, count, offset, dev, f16):
        a = np.empty(count, np.float32)
        O.L().orc_synth_fill(O.fptr(a), a.size, seed, name.encode(), offset, float(np.float32(dev)), f16)
        return a

    w = {}
    for i in range(convs + 2):
        cin, cout = (FEAT if i else 3), (3 * scale * scale if i == convs + 1 else FEAT)
        w[f"body.{2 * i}.weight"] = fill(f"body.{2 * i}.weight", cout * cin * 9, 0.0, math.sqrt(2.0 / (9.0 * cin)), 1).reshape(cout, cin, 3, 3)
        w[f"body.{2 * i}.bias"] = fill(f"body.{2 * i}.bias", cout, 0.0, 0.05, 0)
        if i <= convs:
            w[f"body.{2 * i + 1}.weight"] = fill(f"body.{2 * i + 1}.weight", FEAT, float(np.float32(0.1)), 0.1, 0)
    return w


def save_safetensors(path, w, prefix=""):
    """in float32 throughout: the convolutions hold fp16 values already, and the slopes (".weight" too) must not be rounded"""
    E.save_safetensors(path, w, prefix=prefix, f16=False)
