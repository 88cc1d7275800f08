"""The measurements of profiles/inpaint.md: one JSON line per kernel and shape (appended to --out when given), the tables with --md, and with --e2e one end-to-end
figure.

  mlsd_gauss_blur   one plane (a mask) at 1024 x 1024, 2048 x 2048 and 4096 x 4096 with sigma 4, 16 and 64 (radius 10, 40, 160), with the LDS row pass and, beside
                    it, with the row pass reading global memory directly (mlsd_gauss_blur_lds_limit(0)); bytes = src read, intermediate written and read, dst written
                    (16 per pixel)
  mlsd_mask_grow    one plane, radius 8 and 64; the same 16 bytes per pixel
  mlsd_composite    3 planes, one image, the rectangle being the whole image: orig, patch and p read, dst written (12 + 12 + 4 + 12 = 40 bytes per pixel)
  each against a device copy (mlsd_probe_copy of 1 GiB, the yardstick of profiles/canny.md) timed in the same run: `x copy` is the call's time over the time the copy
  would need for the same bytes.

Times are host to host: a clock around the call and the wait for the device, the least of --calls repeats after a warm-up.  mlsd_gauss_blur uploads its taps and waits
for the stream once per call, so this is what a caller pays.

--e2e: synth:sdxl, a 2048 x 2048 picture with a 300 x 300 repaint rectangle, 8 steps at f_t_ini 0.6, inpaint_area whole against masked at 1024 x 1024 (mask_blur 4,
padding 32): wall time of the second of two mlis_generate calls each, and the engine builds."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDES = (1024, 2048, 4096)


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def kernels(args):
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
    rows = []

    def record(what, side, param, us, moved, **more):
        rec = dict(what=what, side=side, param=param, us=round(us, 1), bytes=moved, gbs=round(moved / us / 1e3, 1), copy_gbs=round(copy_gbs, 1),
                   x_copy=round(us / (moved / copy_gbs / 1e3), 1), **more)
        rows.append(rec)
        emit(args, rec)

    rng = np.random.default_rng(0)
    for side in SIDES:
        px = side * side
        mask = (rng.random((side, side)) < 0.2).astype(np.float32)
        src, dst = _lib.from_numpy(mask), _lib.DeviceBuffer(px * 4)
        ws = _lib.DeviceBuffer(K.gauss_blur_ws_bytes(side, side, 1))
        for sigma in (4.0, 16.0, 64.0):
            us = host_us(lambda: K.gauss_blur(src.ptr, dst.ptr, side, side, 1, sigma, 0, ws.ptr), args.calls)
            was = K.gauss_blur_lds_limit(0)
            try:
                us_direct = host_us(lambda: K.gauss_blur(src.ptr, dst.ptr, side, side, 1, sigma, 0, ws.ptr), args.calls)
            finally:
                K.gauss_blur_lds_limit(was)
            record("gauss_blur", side, sigma, us, 16 * px, radius=len(K.gauss_taps(sigma)) // 2, direct_rows_us=round(us_direct, 1))
        for radius in (8, 64):
            us = host_us(lambda: K.mask_grow(src.ptr, dst.ptr, side, side, radius, 0, ws.ptr), args.calls)
            record("mask_grow", side, radius, us, 16 * px)
        orig, patch = _lib.from_numpy(rng.random((3, side, side), np.float32)), _lib.from_numpy(rng.random((3, side, side), np.float32))
        out = _lib.DeviceBuffer(3 * px * 4)
        us = host_us(lambda: K.composite(out.ptr, orig.ptr, 1, patch.ptr, src.ptr, side, side, 3, 1, 0, 0, side, side), args.calls)
        record("composite", side, "", us, 40 * px)
        for buf in (src, dst, ws, orig, patch, out):
            buf.free()
    return rows


def e2e(args):
    from mlimgsynth_amd import mlimgsynth as M
    side, rect = 2048, (900, 700, 1200, 1000)
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    mask = np.full((side, side, 1), 255, np.uint8)
    mask[rect[1]:rect[3], rect[0]:rect[2]] = 0
    rows = []
    for area in ("masked", "whole"):
        s = M.MLImgSynth()
        try:
            s.option_set("model", "synth:sdxl"), s.option_set("image_dim", 1024, 1024), s.option_set("steps", 8), s.option_set("seed", 1), s.option_set("cfg_scale", 7.0)
            s.inpaint_set(area=area, padding=32, mask_blur=4.0, composite=True)
            times = []
            for _ in range(2):
                for arr, oid, c in ((img, M.MLIS_OPT_IMAGE, 3), (mask, M.MLIS_OPT_IMAGE_MASK, 1)):
                    im = M.MLIS_Image_C(arr.ctypes.data_as(C.POINTER(C.c_uint8)), arr.size, side, side, c, 0)
                    if s._lib.mlis_option_set(s._ctx, oid, C.byref(im)) < 0:
                        raise RuntimeError(s.errstr_get())
                s.option_set("f_t_ini", 0.6)
                toks = (C.c_int32 * 5)(5, 17, 300, 42, 7)
                s._lib.mlis_amd_prompt_tokens_set(s._ctx, toks, None, 5, 0)
                s._lib.mlis_amd_prompt_tokens_set(s._ctx, toks, None, 2, 1)
                t0 = time.perf_counter()
                s.generate()
                times.append(time.perf_counter() - t0)
            rec = dict(what="e2e", model="synth:sdxl", picture=side, rect=rect, area=area, info=s.inpaint_info(), first_s=round(times[0], 2), second_s=round(times[1], 3),
                       engine_builds=s.engine_builds())
            rows.append(rec)
            emit(args, rec)
        finally:
            s.close()
    return rows


def main(args):
    rows = [] if args.only_e2e else kernels(args)
    if args.e2e or args.only_e2e:
        rows += e2e(args)
    if args.md:
        with open(args.md, "w") as fh:
            fh.write("| kernel | side | sigma / radius | host to host | bytes moved | GB/s | x the copy of the same bytes | row pass direct |\n|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                if r["what"] == "e2e":
                    continue
                p = f"{r['param']} (r {r['radius']})" if r["what"] == "gauss_blur" else r["param"]
                d = f"{r['direct_rows_us']:.0f} us" if "direct_rows_us" in r else ""
                fh.write(f"| {r['what']} | {r['side']} | {p} | {r['us']:.0f} us | {r['bytes'] / 1e6:.0f} MB | {r['gbs']:.0f} | {r['x_copy']:.1f} x at {r['copy_gbs']:.0f} GB/s | {d} |\n")
            for r in rows:
                if r["what"] == "e2e":
                    fh.write(f"\ne2e {r['area']}: region and pass size {r['info']}, first call {r['first_s']} s, second call {r['second_s']} s, {r['engine_builds']} engine build(s)\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--e2e", action="store_true", help="also the end-to-end figure (builds synth:sdxl engines at 1024 x 1024 and 2048 x 2048)")
    ap.add_argument("--only-e2e", action="store_true")
    main(ap.parse_args())
