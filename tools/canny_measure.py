"""The measurements of profiles/canny.md: one JSON line per shape and input (appended to --out when given), and the table itself with --md.

  mlsd_canny, 3 planes in, 3 planes out, thresholds 100 / 200 (L1), no wrap, at 512 x 512, 1024 x 1024 and 2048 x 2048 on
    natural : white noise through a Gaussian low-pass (sigma 3 pixels), stretched to 0 .. 1 -- the edge density of a photograph, long connected edges;
    noise   : white uint8 noise -- nearly every pixel is a candidate, the worst case for the classification's stores and the best for the hysteresis.
  Beside it the resample control_apply runs before it in the same pass: mlsd_resample2d, bilinear, 3 planes, from a source 1.5 x the side, and a device copy
  (mlsd_probe_copy of 1 GiB, the copy of tests/test_hw_probe.py) as the bandwidth the bytes are held against.

Times are host to host: a clock around the call and the wait for the device, the least of --calls repeats after a warm-up.  mlsd_canny waits for the stream
itself once per group of sweeps (it reads their flags), so this is what a caller pays.  The kernels' own durations come from a run of their own:
`rocprofv3 --kernel-trace --stats -- python tools/canny_measure.py`.  bytes = src read (12 per pixel) + class map written (1) + per launched sweep one map read
and one written (2) + the map read and dst written (1 + 12)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = (512, 1024, 2048)


def make_input(kind, side, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (rng.integers(0, 256, (3, side, side), dtype=np.uint8).astype(np.float32) / np.float32(255)).astype(np.float32)
    from scipy import ndimage as ndi
    x = np.stack([ndi.gaussian_filter(rng.standard_normal((side, side)), 3.0, mode="wrap") for _ in range(3)])
    x = (x - x.min()) / (x.max() - x.min())
    return (np.rint(x * 255).astype(np.float32) / np.float32(255)).astype(np.float32)


def main(args):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    vp = C.c_void_p

    def host_us(call, n, warm=2):
        for _ in range(warm):
            call()
        K.sync()
        best = None
        for _ in range(n):
            t0 = time.perf_counter()
            call()
            K.sync()
            dt = (time.perf_counter() - t0) * 1e6
            best = dt if best is None else min(best, dt)
        return best

    n = 1 << 30
    a, b = _lib.DeviceBuffer(n), _lib.DeviceBuffer(n)
    copy_us = host_us(lambda: _lib.check(L.mlsd_probe_copy(vp(a.ptr), vp(b.ptr), C.c_size_t(n), None)), 5)
    copy_gbs = 2 * n / copy_us / 1e3
    a.free(), b.free()
    group = K.canny_tile(4)
    rows = []
    for side in SIDES:
        for kind in ("natural", "noise"):
            x = make_input(kind, side)
            px = side * side
            src, dst, ws = _lib.from_numpy(x), _lib.DeviceBuffer(3 * px * 4), _lib.DeviceBuffer(K.canny_ws_bytes(side, side))
            lo, hi = K.canny_thresholds(100, 200, False)
            sweeps = K.canny(src.ptr, side, side, 3, lo, hi, 0, 0, dst.ptr, 3, ws.ptr)
            K.sync()
            edges = float(dst.download((3, side, side), np.float32)[0].mean())
            launched = -(-sweeps // group) * group
            us = host_us(lambda: K.canny(src.ptr, side, side, 3, lo, hi, 0, 0, dst.ptr, 3, ws.ptr), args.calls)
            moved = px * (12 + 1 + 2 * launched + 1 + 12)
            s_side = side * 3 // 2
            big = _lib.from_numpy(np.random.default_rng(1).random((3, s_side, s_side), np.float32))
            rs_us = host_us(lambda: K.resample2d(big.ptr, s_side, s_side, src.ptr, side, side, 3, K.RESAMPLE_BILINEAR), args.calls)
            rec = dict(what="canny", side=side, input=kind, edge_share=round(edges, 4), sweeps=sweeps, sweeps_launched=launched, canny_us=round(us, 1), bytes=moved,
                       gbs=round(moved / us / 1e3, 1), copy_gbs=round(copy_gbs, 1), share_of_copy=round(moved / us / 1e3 / copy_gbs, 4),
                       resample_us=round(rs_us, 1), canny_over_resample=round(us / rs_us, 2), tile=[K.canny_tile(i) for i in range(4)])
            rows.append(rec)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
            for buf in (src, dst, ws, big):
                buf.free()
    if args.md:
        with open(args.md, "w") as fh:
            fh.write("| side | input | edge pixels | sweeps needed (launched) | mlsd_canny, host to host | bytes moved | GB/s | share of the device copy | "
                     "resample before it | canny / resample |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write(f"| {r['side']} | {r['input']} | {100 * r['edge_share']:.1f} % | {r['sweeps']} ({r['sweeps_launched']}) | {r['canny_us']:.0f} us | "
                         f"{r['bytes'] / 1e6:.1f} MB | {r['gbs']:.0f} | {100 * r['share_of_copy']:.1f} % of {r['copy_gbs']:.0f} GB/s | {r['resample_us']:.0f} us | "
                         f"{r['canny_over_resample']:.1f} x |\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    main(ap.parse_args())
