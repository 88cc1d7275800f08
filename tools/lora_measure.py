"""The measurements of the device-side LoRA path (DESIGN.md "LoRA on resident engines", profiles/NOTES.md), one JSON line per run (appended to --out).

  kernel               mlsd_lora_apply on SDXL-shaped F16 weights -- a 1280 x 1280 linear, the GEGLU 10240 x 1280, a 1280 x 1280 x 3 x 3 conv -- at ranks
                       16 / 64 / 128, beside a device-to-device copy of the same weight bytes in the same process (the floor of one read plus one write):
                       time per launch in a train of back-to-back launches between two device events, three trains each
  context [--lib SO]   the tiny checkpoint of the tests through the C-ABI: a generation with lora=style,0.6, then the wall time of the generations after
                       the multiplier changes to 0.8 and back, with the engine builds and (where the library exports them) the LoRA counters.  With the
                       parent commit's build as --lib this is the rebuild it replaces.

Times of `context` are host clocks around mlis_generate, which ends with the latent and the image on the host."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def emit(args, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def kernel(args):
    import torch
    import lora_ffi as LF
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    lib = LF.bind(_lib.LIB_PATH)
    vp = C.c_void_p
    e0, e1 = vp(), vp()
    _lib.check(L.mlsd_event_create(C.byref(e0))); _lib.check(L.mlsd_event_create(C.byref(e1)))

    def train(launch, n):
        for _ in range(10):
            launch()
        _lib.check(L.mlsd_device_sync())
        _lib.check(L.mlsd_event_record(e0, None))
        for _ in range(n):
            launch()
        _lib.check(L.mlsd_event_record(e1, None))
        _lib.check(L.mlsd_event_sync(e1))
        ms = C.c_float()
        _lib.check(L.mlsd_event_elapsed_ms(e0, e1, C.byref(ms)))
        return ms.value * 1e3 / n

    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for name, layout, shape in (("linear 1280x1280", 0, (1280, 1280)), ("geglu 10240x1280", 2, (10240, 1280)), ("conv 1280x1280x3x3", 1, (1280, 1280, 3, 3))):
        lp, n_dev = LF.layout_params(layout, shape)
        n1, n0 = shape[0], int(np.prod(shape[1:]))
        W, other = torch.zeros(n_dev, dtype=torch.float16, device="cuda"), torch.zeros(n_dev, dtype=torch.float16, device="cuda")
        rec = dict(what="kernel", weight=name, weight_bytes=n_dev * 2, launches=args.launches, us_per_launch={})
        copy = lambda: _lib.check(L.mlsd_memcpy(vp(other.data_ptr()), vp(W.data_ptr()), C.c_size_t(n_dev * 2), 2, None))
        rec["us_per_launch"]["device_copy"] = [round(train(copy, args.launches), 2) for _ in range(3)]
        for r in (16, 64, 128):
            up = (torch.randn(n1, r, device="cuda") * 0.01).half().float()
            down = (torch.randn(r, n0, device="cuda") * 0.01).half().float()
            # scale 0 keeps the weights finite over a train of launches; the kernel does the same work for any scale
            run = lambda: _lib.check(lib.mlsd_lora_apply(W.data_ptr(), 1, n0, n1, up.data_ptr(), down.data_ptr(), r, 0.0, layout, *lp, flag.data_ptr(), None))
            rec["us_per_launch"]["rank%d" % r] = [round(train(run, args.launches), 2) for _ in range(3)]
            rec["valu_flop_rank%d" % r] = 2 * r * n0 * n1
        assert flag.item() == 0
        emit(args, rec)


def context(args):
    import torch  # noqa: F401     (first, as mlimgsynth_amd._lib does: one HIP runtime in the process)
    import loader_cases as LC
    import mlis_ffi as F
    import test_lora_gpu as G
    lib = F.bind(args.lib)
    lib.mlis_amd_engine_builds.restype, lib.mlis_amd_engine_builds.argtypes = C.c_int, [C.c_void_p]
    have_stats = hasattr(lib, "mlis_amd_lora_stats")
    d = tempfile.mkdtemp()
    LC.write_checkpoint(os.path.join(d, "tiny.safetensors"), "tiny", "F16")
    G.write_model_adapter(os.path.join(d, "style.safetensors"), "tiny", 21)
    m = F.Mlis(lib)
    m.set("model_type", "tiny"); m.set("lora_dir", d); m.set("model", os.path.join(d, "tiny.safetensors"))
    m.set("image_dim", 64, 64); m.set("steps", 4); m.set("method", "euler_a"); m.set("cfg_scale", 7.0)

    def gen(mult):
        m.set("lora_clear", "")
        m.set("lora", "style", mult)
        m.set("seed", 42)
        m.tokens(G.TOKS); m.tokens(G.NEG, negative=True)
        t = time.perf_counter()
        m.generate()
        return round(time.perf_counter() - t, 4)
    first = gen(0.6)
    same = [gen(0.6) for _ in range(args.reps)]
    changed = [gen(0.8 if i % 2 == 0 else 0.6) for i in range(args.reps)]
    rec = dict(what="context", lib=os.path.basename(os.path.dirname(os.path.dirname(args.lib))) or args.lib, first_s=first, same_multiplier_s=same,
               changed_multiplier_s=changed, engine_builds=lib.mlis_amd_engine_builds(m.ctx))
    if have_stats:
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        lib.mlis_amd_lora_stats(m.ctx, C.byref(a), C.byref(b), C.byref(c))
        rec["lora_stats"] = dict(restored=a.value, patched=b.value, cold_merges=c.value)
    m.close()
    emit(args, rec)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "context"])
    ap.add_argument("--lib", default=os.path.join(ROOT, "mlimgsynth_amd", "lib", "libmlimgsynth_amd.so"))
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dict(kernel=kernel, context=context)[args.what](args)
