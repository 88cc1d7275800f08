"""The measurements of profiles/hires.md, one JSON line per run (appended to --out when given).

  kernel                       mlsd_resample2d, 4 x 4 planes of 128 x 128 -> 192 x 192 and -> 256 x 256, every mode, beside a device-to-device copy of
                               the output's bytes: time per launch in a train of back-to-back launches between two device events (what a caller
                               pays), to be read beside the kernel durations of `rocprofv3 --kernel-trace --stats -- python tools/hires_measure.py kernel`
  pipeline --batch B           this library: device memory the second engine takes, then steady-state time of one hires generation
                               (SDXL synthetic weights, 1024 x 1024 -> 1536 x 1536, 20 + 20 steps at denoise 0.7, Euler-a, cfg 7, decoded)
  baseline --batch B --lib SO  a library without the hires options (the parent commit's build): txt2img at 1024 x 1024 (not decoded, as the first
                               pass) and img2img from a latent at 1536 x 1536 with the same f_t_ini, each in its own warm context; then one context
                               alternating the two, which rebuilds its engine at every call -- what the second slot saves

Times are host clocks around mlis_generate, which ends with the latent and the image on the host."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
BASE, SCALE, STEPS, DENOISE = 1024, 1.5, 20, 0.7


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def stats(ts):
    ts = sorted(ts)
    return dict(n=len(ts), min=round(ts[0], 4), median=round(ts[len(ts) // 2], 4), max=round(ts[-1], 4))


# ------------------------------------------------------------------ kernel
def kernel(args):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    vp = C.c_void_p
    e0, e1 = vp(), vp()
    _lib.check(L.mlsd_event_create(C.byref(e0))); _lib.check(L.mlsd_event_create(C.byref(e1)))

    def train(launch, n):
        for _ in range(20):
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

    planes, s = 16, 128
    x = np.random.default_rng(0).standard_normal((planes, s, s)).astype(np.float32)
    src = _lib.from_numpy(x)
    for d in (192, 256):
        nbytes = planes * d * d * 4
        dst, other = _lib.DeviceBuffer(nbytes), _lib.DeviceBuffer(nbytes)
        rec = dict(what="kernel", src=f"{planes}x{s}x{s}", dst=f"{planes}x{d}x{d}", bytes_read=x.nbytes, bytes_written=nbytes, launches=args.launches, us_per_launch={})
        for mode, name in enumerate(("nearest", "bilinear", "bicubic")):
            rec["us_per_launch"][name] = [round(train(lambda: K.resample2d(src.ptr, s, s, dst.ptr, d, d, planes, mode), args.launches), 3) for _ in range(3)]
        copy = lambda: _lib.check(L.mlsd_memcpy(vp(other.ptr), vp(dst.ptr), C.c_size_t(nbytes), 2, None))
        rec["us_per_launch"]["device_copy"] = [round(train(copy, args.launches), 3) for _ in range(3)]
        emit(args, rec)


# ------------------------------------------------------------------ pipeline
def bind(path):
    import torch  # noqa: F401     (first, as mlimgsynth_amd._lib does: one HIP runtime in the process)
    import mlis_ffi as F
    lib = F.bind(path)
    return F, lib


def context(F, lib, batch, dim):
    m = F.Mlis(lib)
    m.set("model", "synth:sdxl")
    m.set("image_dim", dim, dim)
    m.set("steps", STEPS)
    m.set("seed", 42)
    m.set("cfg_scale", 7.0)
    m.set("method", "euler_a")
    m.set("batch_size", batch)
    return m


def prompt(m):
    m.tokens(TOKS)
    m.tokens(NTOKS, negative=True)


def timed(fn, warm, reps):
    ts = []
    for i in range(warm + reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts[:warm], ts[warm:]


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def pipeline(args):
    F, lib = bind(args.lib)
    lib.mlis_amd_engine_builds.restype, lib.mlis_amd_engine_builds.argtypes = C.c_int, [C.c_void_p]
    m = context(F, lib, args.batch, BASE)
    f0 = free_bytes()

    def plain():
        prompt(m)
        m.set("no_decode", 1)
        m.generate()
    t = time.perf_counter(); plain(); t_first_plain = time.perf_counter() - t
    f1 = free_bytes()                       # text towers, the 1024 x 1024 engine
    m.set("no_decode", 0)
    m.set("hires_scale", SCALE)
    m.set("hires_denoise", DENOISE)

    def hires():
        prompt(m)
        m.generate()
    t = time.perf_counter(); hires(); t_first_hires = time.perf_counter() - t
    f2 = free_bytes()                       # + the 1536 x 1536 engine and its decoder plan
    _, ts = timed(hires, 1, args.reps)
    builds = lib.mlis_amd_engine_builds(m.ctx)
    info = lib.mlis_infotext_get(m.ctx, 0).decode()
    m.close()
    emit(args, dict(what="hires", batch=args.batch, first_plain_s=round(t_first_plain, 3), first_hires_s=round(t_first_hires, 3), hires_s=stats(ts), all_s=[round(x, 4) for x in ts],
                    engine_builds=builds, first_engine_and_text_bytes=f0 - f1, second_engine_bytes=f1 - f2, infotext=info))


def baseline(args):
    F, lib = bind(args.lib)
    lat = int(BASE * SCALE) // 8
    z = np.random.default_rng(1).standard_normal((args.batch, 4, lat, lat)).astype(np.float32)

    def txt2img(m):
        prompt(m)
        m.set("no_decode", 1)
        m.generate()

    def img2img(m):
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["LATENT"])
        lib.mlis_tensor_resize(t, lat, lat, 4, args.batch)
        C.memmove(t.contents.d, z.ctypes.data, z.nbytes)
        prompt(m)
        m.set("no_decode", 0)
        m.set("tensor_use_flags", F.TUF["LATENT"])
        m.set("f_t_ini", DENOISE)
        m.generate()

    a = context(F, lib, args.batch, BASE)
    first_a, ta = timed(lambda: txt2img(a), 2, args.reps)
    a.close()
    b = context(F, lib, args.batch, int(BASE * SCALE))
    first_b, tb = timed(lambda: img2img(b), 2, args.reps)
    info = lib.mlis_infotext_get(b.ctx, 0).decode()
    b.close()
    # one context, two sizes: a library with one engine slot rebuilds at every call
    c = context(F, lib, args.batch, BASE)
    alt_a, alt_b = [], []
    for i in range(3):
        c.set("image_dim", BASE, BASE)
        t = time.perf_counter(); txt2img(c); alt_a.append(time.perf_counter() - t)
        c.set("image_dim", int(BASE * SCALE), int(BASE * SCALE))
        t = time.perf_counter(); img2img(c); alt_b.append(time.perf_counter() - t)
    c.close()
    emit(args, dict(what="baseline", batch=args.batch, txt2img_1024_s=stats(ta), img2img_1536_s=stats(tb), sum_median_s=round(stats(ta)["median"] + stats(tb)["median"], 4),
                    all_txt2img_s=[round(x, 4) for x in ta], all_img2img_s=[round(x, 4) for x in tb], first_calls_s=[round(x, 3) for x in first_a + first_b],
                    alternating_txt2img_s=[round(x, 3) for x in alt_a], alternating_img2img_s=[round(x, 3) for x in alt_b], infotext=info))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "pipeline", "baseline"])
    ap.add_argument("--lib", default=os.path.join(ROOT, "mlimgsynth_amd", "lib", "libmlimgsynth_amd.so"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=500)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dict(kernel=kernel, pipeline=pipeline, baseline=baseline)[args.what](args)
