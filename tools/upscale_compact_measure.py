"""Compact (SRVGG) upscaler: the body form of mlsd_conv3x3_compact (hip/upscale_compact.hip, weights resident in LDS) against mlsd_conv3x3_dense 64 -> 64 on the same
operands (its LeakyReLU standing in for the PReLU: the existing route a composition would have used), a device copy of the layer's bytes, and a whole 32-convolution x4
net beside the 23-block RRDBNet, host to host.

Every kernel figure is the median of `rounds` timed windows of `reps` launches after a warm-up, with the spread (min .. max) beside it; the candidates alternate window by
window; device events around the window.  MFMA rate: 1.9 PFLOP/s, what profiles/r4_mfma_rate.txt measured for v_mfma_f32_16x16x32_f16 on random operands.
usage: python3 tools/upscale_compact_measure.py [reps [rounds [size]]]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlimgsynth_amd import _lib, kernels as K      # noqa: E402

L = _lib.lib()
vp = _lib.vp
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
size = int(sys.argv[3]) if len(sys.argv) > 3 else 512
MFMA_RATE = 1.9e15
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


def fmt(t):
    return f"{t[0]:.1f} ({t[1]:.1f} .. {t[2]:.1f})"


rng = np.random.default_rng(0)
H = W = size
M = H * W
src = _lib.from_numpy((rng.standard_normal((M, 64)) * 0.5).astype(np.float16))
dst = _lib.DeviceBuffer(M * 64 * 2)
wt = _lib.from_numpy((rng.standard_normal((64, 9 * 64)) / 24.0).astype(np.float16))
bias = _lib.from_numpy(rng.standard_normal(64).astype(np.float32))
slope = _lib.from_numpy(np.full(64, 0.2, np.float32))
c = K.CconvArgs(A=src.ptr, lda=64, n_img=1, H=H, W=W, Cin=64, Cout=64, W_=wt.ptr, bias=bias.ptr, slope=slope.ptr, C16=dst.ptr, ldc16=64)
d = K.DconvArgs(A=src.ptr, lda=64, n_img=1, H=H, W=W, Cin=64, W_=wt.ptr, N=64, bias=bias.ptr, lrelu=1, scale=1.0, C16=dst.ptr, ldc16=64)
L.mlsd_memcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
tc, td, tm = measure([lambda: K.conv3x3_compact(c), lambda: K.conv3x3_dense(d), lambda: L.mlsd_memcpy(dst.ptr, src.ptr, M * 128, 2, None)])
K.conv3x3_compact(c)
a = dst.download((M, 64), np.float16)
K.conv3x3_dense(d)
same = a.tobytes() == dst.download((M, 64), np.float16).tobytes()      # slope 0.2 everywhere: the same arithmetic up to the order of the sum
fl, by = 2.0 * M * 64 * 9 * 64, 2.0 * M * 128
print(f"# 64 -> 64 at {H} x {W}, {reps} launches per window, {rounds} windows, median (min .. max) in us")
print("| kernel | us | TFLOP/s | of the MFMA rate | of the device copy's rate |")
print("|---|---|---|---|---|")
for name, t in ((K.cconv_variant(c), tc), (K.dconv_variant(d), td)):
    print(f"| {name} | {fmt(t)} | {fl / t[0] * 1e-6:.0f} | {fl / t[0] * 1e6 / MFMA_RATE:.2f} | {tm[0] / t[0]:.2f} |")
print(f"| device copy of {by / 2e6:.1f} MB | {fmt(tm)} | | | {by / tm[0] * 1e-6:.2f} TB/s read + written |")
print(f"\ncompact / dense = {tc[0] / td[0]:.2f}; the two outputs are {'the same bits' if same else 'not the same bits (another order of the sum)'}", flush=True)
for o in (src, dst):
    o.free()

# ---- the whole nets, host to host
L.mlis_amd_upscaler_create.restype = vp
L.mlis_amd_upscaler_create.argtypes = [ctypes.c_char_p]
L.mlis_amd_upscaler_run.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp]
L.mlis_amd_upscaler_destroy.argtypes = [vp]
x = rng.random((1, 3, H, W)).astype(np.float32)
y = np.empty((1, 3, 4 * H, 4 * W), np.float32)
print(f"\n# {H} x {W} -> {4 * H} x {4 * W}, host to host (upload, launches, download), median (min .. max) in ms")
for spec, fl in ((b"synth-compact:1:32:4", 2.0 * 9 * M * (32 * 64 + 32 * 64 * 64 + 64 * 48)),
                 (b"synth:1:23", 2.0 * 9 * M * (23 * 3 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64) + 32 * 64 + 64 * 64 + 4 * 64 * 64 + 32 * 64 * 64 + 16 * 64 * 3))):
    up = L.mlis_amd_upscaler_create(spec)
    assert up, _lib.last_error()
    ts = []
    for i in range(2 + max(rounds, 3)):
        t0 = time.perf_counter()
        r = L.mlis_amd_upscaler_run(up, x.ctypes.data_as(vp), W, H, 1, y.ctypes.data_as(vp))      # ends in a device synchronise
        assert r == 1, _lib.last_error()
        if i >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    print(f"{spec.decode()}: {np.median(ts):.2f} ({min(ts):.2f} .. {max(ts):.2f}), {fl * 1e-12:.3f} TFLOP = {fl / np.median(ts) * 1e-9:.0f} TFLOP/s end to end; "
          f"finite: {bool(np.isfinite(y).all())}", flush=True)
    L.mlis_amd_upscaler_destroy(up)
