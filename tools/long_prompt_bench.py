"""Windowed text context (prompts of more than 75 tokens): timings of the cross attention over 77 W keys and of whole UNet evaluations.

  python3 tools/long_prompt_bench.py kernels [reps]     device-event times per launch; run it under `rocprofv3 --kernel-trace --stats -- python3 ...`
                                                        in a run of its own for the per-kernel table
  python3 tools/long_prompt_bench.py unet [rounds]      UNet evaluation times (device events) at W = 1..4, W alternating inside each round

kernels: mlsd_attention_ctx (keys resident in LDS / one restaged 96-key slot, mlsd_attention_ctx_mode) against mlsd_attention on the same
arguments (Tk > 96: the 64-key tile loop), with the one-pass Tk <= 96 kernel at 77 keys as the anchor.  Shapes: SDXL b4 with CFG
(8 images) 1024 x Tk x 20 heads and 4096 x Tk x 10 heads at d 64; SD1.5 b1 with CFG (2 images) at d 40 / 80 / 160.  q / k / v are
column slices of fused buffers as in the plan.
unet: SDXL 1024x1024 b4 (128 x 128 latent, 8 images with CFG) and SD1.5 512x512 b1 (64 x 64, 2 images), synthetic weights."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlimgsynth_amd import _lib, kernels  # noqa: E402

L = _lib.lib()
vp = _lib.vp
EV = [vp(), vp()]
for e in EV:
    L.mlsd_event_create(ctypes.byref(e))


def timeit(fn, reps):
    for _ in range(3):
        fn()
    L.mlsd_event_record(EV[0], None)
    for _ in range(reps):
        fn()
    L.mlsd_event_record(EV[1], None)
    L.mlsd_event_sync(EV[1])
    ms = ctypes.c_float()
    L.mlsd_event_elapsed_ms(EV[0], EV[1], ctypes.byref(ms))
    return ms.value / reps


KERNEL_SHAPES = [   # (label, images, heads, d_head, Tq)
    ("sdxl b4 1024", 8, 20, 64, 1024), ("sdxl b4 4096", 8, 10, 64, 4096),
    ("sd15 b1 4096", 2, 8, 40, 4096), ("sd15 b1 1024", 2, 8, 80, 1024), ("sd15 b1 256", 2, 8, 160, 256),
]


def kernels_main(reps):
    rng = np.random.default_rng(0)
    L.mlsd_attention_ctx_mode.argtypes = [ctypes.c_int]
    for label, nb, heads, dh, tq in KERNEL_SHAPES:
        D = heads * dh
        for tk in (77, 154, 231, 308):
            q = rng.standard_normal((nb, tq, D)).astype(np.float16)
            kv = rng.standard_normal((nb, tk, 2 * D)).astype(np.float16)
            dq, dkv = _lib.from_numpy(q), _lib.from_numpy(kv)
            do = _lib.DeviceBuffer(nb * tq * D * 2)
            a = kernels.AttnArgs(q=dq.ptr, k=dkv.ptr, v=dkv.ptr + 2 * D, out=do.ptr, ldq=D, ldk=2 * D, ldv=2 * D, ldo=D, bsq=tq * D,
                                 bsk=tk * 2 * D, bsv=tk * 2 * D, bso=tq * D, n_batch=nb, n_head=heads, d_head=dh, Tq=tq, Tk=tk, causal=0)
            runs = [("mlsd_attention (tk96 one pass)" if tk <= 96 else "mlsd_attention (tile loop)", None, kernels.attention)]
            if tk > 96:
                runs += [("mlsd_attention_ctx resident" if dh <= 80 else "mlsd_attention_ctx slot", 0, kernels.attention_ctx)]
                if dh <= 80:
                    runs += [("mlsd_attention_ctx slot", 1, kernels.attention_ctx)]
            res = {}
            for name, mode, fn in runs:
                if mode is not None:
                    L.mlsd_attention_ctx_mode(mode)
                res[name] = timeit(lambda: fn(a), reps)
                L.mlsd_attention_ctx_mode(0)
            base = [v for k, v in res.items() if k.startswith("mlsd_attention (")][0]
            for name, ms in res.items():
                print(f"{label} h{heads} d{dh} {tq}x{tk:3d}  {name:32s} {ms * 1e3:8.1f} us  {4.0 * nb * heads * tq * tk * dh / ms / 1e9:7.1f} TFLOP/s"
                      f"  x{ms / base:.3f} of mlsd_attention", flush=True)


def unet_main(rounds):
    from mlimgsynth_amd import engine
    for model, lat, n in (("sdxl", 128, 8), ("sd1", 64, 2)):
        rng = np.random.default_rng(1)
        us = {}
        for W in (1, 2, 3, 4):
            u = engine.Unet(model, lat, lat, n, n_ctx_tok=77 * W)
            P = u.P
            x = rng.standard_normal((n, 4, lat, lat)).astype(np.float32)
            c = (rng.standard_normal((n, 77 * W, P.n_ctx)) * 0.5).astype(np.float32)
            lab = rng.standard_normal((n, P.ch_adm_in)).astype(np.float32) if P.ch_adm_in else None
            u.run(x, c, lab, np.full(n, 2.0, np.float32))           # inputs set, first evaluation (tuning)
            us[W] = u
        t = {W: [] for W in us}
        for r in range(rounds):
            for W in ((1, 2, 3, 4) if r % 2 == 0 else (4, 3, 2, 1)):
                u = us[W]
                t[W].append(timeit(lambda: u.ctx.compute(), 5))
        for W in us:
            a = np.array(t[W])
            print(f"{model} {lat}x{lat} n{n} W={W} ({77 * W} context rows): UNet evaluation {np.median(a):.3f} ms median, "
                  f"{a.min():.3f} - {a.max():.3f} over {rounds} rounds; x{np.median(a) / np.median(t[1]):.4f} of W=1", flush=True)
        for u in us.values():
            u.ctx.destroy()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    arg = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    if what == "kernels":
        kernels_main(arg or 20)
    elif what == "unet":
        unet_main(arg or 3)
    else:
        sys.exit(__doc__)
