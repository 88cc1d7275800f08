"""The measurements of profiles/resample_aa.md, one JSON line per shape (appended to --out when given).

  mlsd_resample2d_aa, 3 planes:  4096 x 4096 -> 2048 x 2048 (lanczos and bilinear),  4096 x 4096 -> 1536 x 1536 (lanczos),  2048 x 2048 -> 512 x 512 (lanczos),
  each with the horizontal pass staged in LDS (the default) and reading global memory directly (mlsd_resample2d_aa_lds_limit(0)), beside mlsd_resample2d
  bicubic (16 point-sampled taps, no antialiasing) on the same operands as the yardstick, and a device copy (mlsd_probe_copy of 1 GiB, the copy of
  tests/test_hw_probe.py) as the bandwidth the bytes are held against.

Time per call of a train of back-to-back calls between two device events.  A call of mlsd_resample2d_aa builds its tap tables on the host, uploads them
and waits for the stream once, so its figure is what a caller pays, not the two kernels' durations: those come from
`rocprofv3 --kernel-trace --stats -- python tools/resample_aa_measure.py`.  bytes = src read + intermediate written and read + dst written."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 2048, ("lanczos3", "triangle")), (4096, 1536, ("lanczos3",)), (2048, 512, ("lanczos3",))]
FILTERS = ["box", "triangle", "cubic", "lanczos3"]
PLANES = 3


def main(args):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    vp = C.c_void_p
    e0, e1 = vp(), vp()
    _lib.check(L.mlsd_event_create(C.byref(e0))); _lib.check(L.mlsd_event_create(C.byref(e1)))

    def train(launch, n, warm=3):
        for _ in range(warm):
            launch()
        K.sync()
        _lib.check(L.mlsd_event_record(e0, None))
        for _ in range(n):
            launch()
        _lib.check(L.mlsd_event_record(e1, None))
        _lib.check(L.mlsd_event_sync(e1))
        ms = C.c_float()
        _lib.check(L.mlsd_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e3 / n

    n = 1 << 30
    a, b = _lib.DeviceBuffer(n), _lib.DeviceBuffer(n)
    copy_us = min(train(lambda: _lib.check(L.mlsd_probe_copy(vp(a.ptr), vp(b.ptr), C.c_size_t(n), None)), 5, 2) for _ in range(3))
    copy_gbs = 2 * n / copy_us / 1e3
    a.free(), b.free()

    for s, d, filters in SHAPES:
        x = np.random.default_rng(0).standard_normal((PLANES, s, s)).astype(np.float32)
        src, dst = _lib.from_numpy(x), _lib.DeviceBuffer(PLANES * d * d * 4)
        moved = 4 * PLANES * (s * s + 2 * s * d + d * d)
        rec = dict(what="resample_aa", src=f"{PLANES}x{s}x{s}", dst=f"{PLANES}x{d}x{d}", bytes_aa=moved, bytes_plain=4 * PLANES * (s * s + d * d), calls=args.calls,
                   copy_gbs=round(copy_gbs, 1), us_per_call={}, gbs={}, share_of_copy={})

        def note(name, us, nbytes):
            rec["us_per_call"][name] = [round(u, 2) for u in us]
            rec["gbs"][name] = round(nbytes / min(us) / 1e3, 1)
            rec["share_of_copy"][name] = round(nbytes / min(us) / 1e3 / copy_gbs, 3)

        for f in filters:
            fi = FILTERS.index(f)
            ws = _lib.DeviceBuffer(K.resample2d_aa_ws_bytes(s, s, d, d, PLANES, fi))
            outs = {}
            for how, limit in (("lds", 32 * 1024), ("direct", 0)):
                L.mlsd_resample2d_aa_lds_limit(limit)
                note(f"aa_{f}_{how}", [train(lambda: K.resample2d_aa(src.ptr, s, s, dst.ptr, d, d, PLANES, fi, 0, ws.ptr), args.calls) for _ in range(3)], moved)
                outs[how] = dst.download((PLANES, d, d), np.float32)
            L.mlsd_resample2d_aa_lds_limit(32 * 1024)
            rec.setdefault("lds_equals_direct", {})[f] = outs["lds"].tobytes() == outs["direct"].tobytes()
            ws.free()
        note("plain_bicubic", [train(lambda: K.resample2d(src.ptr, s, s, dst.ptr, d, d, PLANES, K.RESAMPLE_BICUBIC), args.calls) for _ in range(3)], rec["bytes_plain"])
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        src.free(), dst.free()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
