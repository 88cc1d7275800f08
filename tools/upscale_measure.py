"""ESRGAN upscaler: the dense-block convolution (hip/upscale.hip) against the existing implicit-GEMM route on the same operands, and a whole 23-block upscale.

  - the five convolution shapes of an RDB (Cin 64, 96, 128, 160 -> 32 and 192 -> 64) on one 512 x 512 image: mlsd_conv3x3_dense with the net's epilogue
    (LeakyReLU into an fp16 slice; conv5: 0.2 conv + fp32 residual, fp32 and fp16 out) and mlsd_gemm with act none and fp16 output, the tile its own rule picks.
    The GEMM row does LESS epilogue work: it is a lower bound on what a GEMM-routed net would cost.
  - synth:1:23 on a 512 x 512 input (2048 x 2048 out), host to host.

Every figure is the median of `rounds` timed windows of `reps` launches after a warm-up, with the spread (min .. max) beside it; device events around the window.
usage: python3 tools/upscale_measure.py [reps [rounds [size]]]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlimgsynth_amd import _lib, kernels as K      # noqa: E402

L = _lib.lib()
vp = _lib.vp
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
size = int(sys.argv[3]) if len(sys.argv) > 3 else 512
ev = [vp(), vp()]
for e in ev:
    L.mlsd_event_create(ctypes.byref(e))


def window(fn):
    L.mlsd_event_record(ev[0], None)
    for _ in range(reps):
        fn()
    L.mlsd_event_record(ev[1], None)
    L.mlsd_event_sync(ev[1])
    ms = ctypes.c_float()
    L.mlsd_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms))
    return ms.value * 1e3 / reps


def measure(fns):
    """the candidates alternate window by window; -> [(median, min, max)] in us"""
    for fn in fns:
        for _ in range(3):
            fn()
    K.sync()
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(window(fn))
    return [(float(np.median(x)), min(x), max(x)) for x in t]


rng = np.random.default_rng(0)
H = W = size
M = H * W
print(f"# mlsd_conv3x3_dense vs mlsd_gemm, one {H} x {W} image, {reps} launches per window, {rounds} windows, median (min .. max) in us")
print("| Cin -> N | dense conv | variant | GEMM route | tile | dense / GEMM | dense TFLOP/s |")
print("|---|---|---|---|---|---|---|")
dense = _lib.from_numpy((rng.standard_normal((M, 192)) * 0.5).astype(np.float16))
other = _lib.DeviceBuffer(M * 192 * 2)
trunk = _lib.from_numpy(rng.standard_normal((M, 64)).astype(np.float32))
out32 = _lib.DeviceBuffer(M * 64 * 4)
out16 = _lib.DeviceBuffer(M * 64 * 2)
for cin, n in [(64, 32), (96, 32), (128, 32), (160, 32), (192, 64)]:
    wt = _lib.from_numpy((rng.standard_normal((n, 9 * cin)) / np.sqrt(9 * cin)).astype(np.float16))
    bias = _lib.from_numpy(rng.standard_normal(n).astype(np.float32))
    if n == 32:       # conv1..4: LeakyReLU into the slice of the buffer it reads
        d = K.DconvArgs(A=dense.ptr, lda=192, n_img=1, H=H, W=W, Cin=cin, W_=wt.ptr, N=n, bias=bias.ptr, lrelu=1, scale=1.0, C16=dense.ptr + 2 * cin, ldc16=192)
    else:             # conv5: 0.2 conv + trunk, fp32 and fp16 out
        d = K.DconvArgs(A=dense.ptr, lda=192, n_img=1, H=H, W=W, Cin=cin, W_=wt.ptr, N=n, bias=bias.ptr, lrelu=0, scale=0.2, resid=trunk.ptr, ldr=64,
                        C32=out32.ptr, ldc32=64, C16=other.ptr, ldc16=192)
    g = K.GemmArgs(A=dense.ptr, lda=192, conv=1, n_img=1, H=H, W=W, Cin=cin, OH=H, OW=W, KH=3, KW=3, stride=1, pad=1, upsample=0, W_=wt.ptr, ldb=9 * cin,
                   M=M, N=n, K=9 * cin, bias=bias.ptr, rows_per_batch=M, ldrb=n, act=K.ACT_NONE, C16=out16.ptr, ldc16=n)
    (td, tg) = measure([lambda: K.conv3x3_dense(d), lambda: K.gemm(g)])
    fl = 2.0 * M * n * 9 * cin
    print(f"| {cin} -> {n} | {td[0]:.1f} ({td[1]:.1f} .. {td[2]:.1f}) | {K.dconv_variant(d)} | {tg[0]:.1f} ({tg[1]:.1f} .. {tg[2]:.1f}) | {K.gemm_variant(g)} | "
          f"{td[0] / tg[0]:.2f} | {fl / td[0] * 1e-6:.0f} |", flush=True)

# ---- the whole net
L.mlis_amd_upscaler_create.restype = vp
L.mlis_amd_upscaler_create.argtypes = [ctypes.c_char_p]
L.mlis_amd_upscaler_run.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
L.mlis_amd_upscaler_destroy.argtypes = [vp]
for o in (dense, other, trunk, out32, out16):
    o.free()
up = L.mlis_amd_upscaler_create(b"synth:1:23")
assert up, _lib.last_error()
x = rng.random((1, 3, H, W)).astype(np.float32)
y = np.empty((1, 3, 4 * H, 4 * W), np.float32)
ts = []
for i in range(2 + max(rounds, 3)):
    t0 = time.perf_counter()
    r = L.mlis_amd_upscaler_run(up, x.ctypes.data_as(vp), W, H, 1, y.ctypes.data_as(vp))      # ends in a device synchronise
    assert r == 1, _lib.last_error()
    if i >= 2:
        ts.append((time.perf_counter() - t0) * 1e3)
fl = 2.0 * 9 * M * (23 * 3 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64) + 32 * 64 + 64 * 64 + 4 * 64 * 64 + 16 * 64 * 64 + 16 * 64 * 64 + 16 * 64 * 3)
print(f"\n# synth:1:23, {H} x {W} -> {4 * H} x {4 * W}, host to host (upload, 350 launches, download): median {np.median(ts):.1f} ms ({min(ts):.1f} .. {max(ts):.1f}), "
      f"{fl * 1e-12:.2f} TFLOP = {fl / np.median(ts) * 1e-9:.0f} TFLOP/s end to end; finite: {bool(np.isfinite(y).all())}")
L.mlis_amd_upscaler_destroy(up)
