"""The measurements of profiles/colorfix.md: one JSON line per size and mode (appended to --out when given), and the table itself with --md.

  The three colour fixes on one image of 3 channels at 1024 x 1024 and 2048 x 2048, the target of the content's size (content uniform in 0 .. 1, target =
  content x 0.8 + 0.1 plus noise), each in two ways:
    device       : mlsd_colorfix_* on buffers that live on the device, --reps calls enqueued back to back and one wait for the device, the time per call; the
                   least of --calls such windows after a warm-up.  The launch overhead of a call overlaps the call before it, so this is the kernels' time.
                   (Per kernel: `rocprofv3 --kernel-trace --stats -- python tools/colorfix_measure.py --sides N`, a run of its own per size: the
                   statistics kernels have the same grid at both sizes, so one trace of both could not tell them apart.)
    host to host : mlis_amd_tensor_color_fix on host tensors -- allocation, upload, the kernels, download --, a clock around the call, the least of --calls.
  Beside them a device copy of the same bytes (mlsd_probe_copy of the content's bytes, timed the same way as `device`) and of 1 GiB, and for the wavelet the read
  amplification of its tile: the floats a workgroup stages per float it writes, ((64 + 2 (2^levels - 1)) / 64)^2, for each of its two inputs.
  bytes = what the algorithm needs: wavelet and the two maps read content and target once and write dst once (12 per pixel and channel; the statistics of adain
  and histogram read content a second time: 16)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Tensor(C.Structure):          # MLIS_Tensor
    _fields_ = [("d", C.POINTER(C.c_float)), ("n", C.c_int * 4), ("flags", C.c_int)]


def pictures(side, seed=0):
    """content [1][3][side][side] uniform in 0 .. 1, target = content x 0.8 + 0.1 plus noise"""
    rng = np.random.default_rng(seed + side)
    content = rng.random((1, 3, side, side), dtype=np.float32)
    noise = np.float32(0.02) * rng.standard_normal(content.shape).astype(np.float32)
    return content, (content * np.float32(0.8) + np.float32(0.1) + noise).astype(np.float32)


def main(args):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    vp = C.c_void_p
    TP = C.POINTER(Tensor)
    L.mlis_ctx_create_i.restype, L.mlis_ctx_create_i.argtypes = vp, [C.c_int]
    L.mlis_ctx_destroy.argtypes = [C.POINTER(vp)]
    L.mlis_errstr_get.restype, L.mlis_errstr_get.argtypes = C.c_char_p, [vp]
    L.mlis_amd_tensor_color_fix.restype, L.mlis_amd_tensor_color_fix.argtypes = C.c_int, [vp, TP, TP, TP, C.c_int, C.c_int]
    L.mlis_tensor_free.argtypes = [TP]

    def as_tensor(x):
        b, c, h, w = x.shape
        return Tensor(x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_int * 4)(w, h, c, b), 0)

    def window_us(call, reps, n, warm=2):
        for _ in range(warm):
            call()
        K.sync()
        best = None
        for _ in range(n):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            K.sync()
            dt = (time.perf_counter() - t0) * 1e6 / reps
            best = dt if best is None else min(best, dt)
        return best

    def copy_gbs(nbytes, reps):
        a, b = _lib.DeviceBuffer(nbytes), _lib.DeviceBuffer(nbytes)
        us = window_us(lambda: _lib.check(L.mlsd_probe_copy(vp(a.ptr), vp(b.ptr), C.c_size_t(nbytes), None)), reps, args.calls)
        a.free(), b.free()
        return us, 2 * nbytes / us / 1e3

    ctx = vp(L.mlis_ctx_create_i(0x000400))
    assert ctx.value, "no library context"
    _, big_gbs = copy_gbs(1 << 30, 3)
    tile, levels = K.colorfix_tile(0), K.colorfix_tile(1)
    amp = ((tile + 2 * ((1 << levels) - 1)) / tile) ** 2
    rows = []
    for side in args.sides:
        content, target = pictures(side)
        t_content, t_target = as_tensor(content), as_tensor(target)
        nbytes = content.nbytes
        same_us, same_gbs = copy_gbs(nbytes, args.reps)
        dc, dt, dst = _lib.from_numpy(content), _lib.from_numpy(target), _lib.DeviceBuffer(nbytes)
        for mode, name in ((K.COLORFIX_WAVELET, "wavelet"), (K.COLORFIX_ADAIN, "adain"), (K.COLORFIX_HISTOGRAM, "histogram")):
            ws = _lib.DeviceBuffer(K.colorfix_ws_bytes(mode, side, side, side, side, 3, 1, 1))
            call = {K.COLORFIX_WAVELET: lambda: K.colorfix_wavelet(dc.ptr, dt.ptr, dst.ptr, side, side, 3, 1, 1, levels),
                    K.COLORFIX_ADAIN: lambda: K.colorfix_adain(dc.ptr, side, side, dt.ptr, side, side, dst.ptr, 3, 1, 1, ws.ptr),
                    K.COLORFIX_HISTOGRAM: lambda: K.colorfix_histogram(dc.ptr, side, side, dt.ptr, side, side, dst.ptr, 3, 1, 1, ws.ptr)}[mode]
            dev_us = window_us(call, args.reps, args.calls)

            def host_call():
                out = Tensor()
                r = L.mlis_amd_tensor_color_fix(ctx, C.byref(t_content), C.byref(t_target), C.byref(out), mode, 0)
                L.mlis_tensor_free(C.byref(out))
                assert r == 1, L.mlis_errstr_get(ctx)
            host_us = window_us(host_call, 1, args.calls, warm=1)
            moved = nbytes * (3 if mode == K.COLORFIX_WAVELET else 4)
            rec = dict(what="colorfix", side=side, mode=name, device_us=round(dev_us, 1), host_to_host_us=round(host_us, 1), bytes=moved,
                       gbs=round(moved / dev_us / 1e3, 1), copy_same_bytes_us=round(same_us, 1), copy_same_bytes_gbs=round(same_gbs, 1), copy_1gib_gbs=round(big_gbs, 1),
                       device_over_copy=round(dev_us / same_us, 2), tile=tile, levels=levels, read_amplification=round(amp, 2) if mode == K.COLORFIX_WAVELET else None)
            rows.append(rec)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
            ws.free()
        for buf in (dc, dt, dst):
            buf.free()
    L.mlis_ctx_destroy(C.byref(ctx))
    if args.md:
        with open(args.md, "w") as fh:
            fh.write("| side | mode | device, per call | host to host | bytes needed | GB/s (device) | device copy of the content's bytes | call / that copy | "
                     "copy of 1 GiB | read amplification |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write(f"| {r['side']} | {r['mode']} | {r['device_us']:.0f} us | {r['host_to_host_us']:.0f} us | {r['bytes'] / 1e6:.1f} MB | {r['gbs']:.0f} | "
                         f"{r['copy_same_bytes_us']:.0f} us ({r['copy_same_bytes_gbs']:.0f} GB/s) | {r['device_over_copy']:.1f} x | {r['copy_1gib_gbs']:.0f} GB/s | "
                         f"{r['read_amplification'] if r['read_amplification'] else '-'} |\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sides", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    main(ap.parse_args())
