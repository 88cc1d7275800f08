"""The measurements of profiles/cfg_rescale.md, one JSON line per run (appended to --out when given).  Synthetic data, cfg 7, phi 0.7.

ONE process, per case (model, size, batch): buffers of the mix's shapes (eps NHWC [2B][HW][ld] with the plan's dense ld = 4, x and dx NCHW [B][4][HW]) and, after a
warm-up of every kernel, --repeats rounds that alternate four timed windows of --launches launches each, a device event on either side:
  plain      mlsd_dxdt_cfg, the mix without the rescale (the guided mix with pag 0 and no factor)
  rescaled   mlsd_guidance_stats (statistics + factor) + mlsd_dxdt_rescaled: the three launches of a rescaled mix
  stats      mlsd_guidance_stats alone
  copy       a device-to-device copy of the bytes the statistics kernel reads (the cond and uncond groups)
Reported per launch (window time / launches), mean and spread of the rounds, with the statistics kernel's rate (bytes read / time) beside the copy's (bytes read,
the same number, / time).  Then one engine of the case runs a warm-up and a timed --steps Euler generation for the time of a UNet evaluation from the engine's
device events: the mix's share of an evaluation is the mix's time over that."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

stat = lambda v: dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)))
CASES = {"sdxl": ("sdxl", 1024, 4), "sd1": ("sd1", 512, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="sdxl,sd1")
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--ld", type=int, default=4)
    ap.add_argument("--no-engine", action="store_true", help="kernels only: no UNet evaluation time, no share")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "cfg_rescale_measure needs a GPU"
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    l = _lib.lib()
    vp, cf, ci, i64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    l.mlsd_dxdt_cfg.argtypes = [vp, i64, vp, vp, ci, ci, ci, cf, ci, cf, cf, vp]
    l.mlsd_event_create.argtypes = [ctypes.POINTER(vp)]
    l.mlsd_event_record.argtypes = [vp, vp]
    l.mlsd_event_sync.argtypes = [vp]
    l.mlsd_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(cf)]
    l.mlsd_memcpy.argtypes = [vp, vp, ctypes.c_size_t, ci, vp]
    ev = [vp(), vp()]
    for e in ev:
        _lib.check(l.mlsd_event_create(ctypes.byref(e)))

    def window(fn, n):
        _lib.check(l.mlsd_event_record(ev[0], None))
        for _ in range(n):
            fn()
        _lib.check(l.mlsd_event_record(ev[1], None))
        _lib.check(l.mlsd_event_sync(ev[1]))
        ms = cf()
        _lib.check(l.mlsd_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)))
        return ms.value / n

    recs = []
    for name in a.cases.split(","):
        model, size, B = CASES[name]
        HW, ld, cfg, phi = (size // 8) ** 2, a.ld, 7.0, 0.7
        rng = np.random.default_rng(0)
        eps = _lib.from_numpy(rng.standard_normal((2 * B, HW, ld)).astype(np.float32))
        x = _lib.from_numpy(rng.standard_normal((B, 4, HW)).astype(np.float32))
        dx = _lib.from_numpy(np.zeros((B, 4, HW), np.float32))
        cp = _lib.from_numpy(np.zeros((2 * B, HW, ld), np.float32))
        nb = K.guidance_scratch_bytes(B, HW)
        scratch, fac = _lib.from_numpy(np.zeros(nb // 8, np.float64)), _lib.from_numpy(np.ones(B, np.float32))
        read_bytes = 2 * B * HW * ld * 4
        fns = dict(
            plain=lambda: _lib.check(l.mlsd_dxdt_cfg(eps.ptr, ld, x.ptr, dx.ptr, B, 4, HW, cfg, 0, 1.0, 0.0, None)),
            rescaled=lambda: (K.guidance_stats(eps.ptr, ld, B, 4, HW, cfg, 0.0, phi, scratch.ptr, nb, fac.ptr),
                              K.dxdt_rescaled(eps.ptr, ld, x.ptr, dx.ptr, B, 4, HW, cfg, 0.0, fac.ptr)),
            stats=lambda: K.guidance_stats(eps.ptr, ld, B, 4, HW, cfg, 0.0, phi, scratch.ptr, nb, fac.ptr),
            copy=lambda: _lib.check(l.mlsd_memcpy(cp.ptr, eps.ptr, read_bytes, 2, None)))
        ms = {k: [] for k in fns}
        for r in range(a.repeats + 1):                   # round 0 warms every kernel up
            for k, fn in fns.items():
                t = window(fn, a.launches)
                if r:
                    ms[k].append(t)
        rec = dict(case=name, model=model, size=size, batch=B, HW=HW, ld=ld, cfg=cfg, phi=phi, launches=a.launches, repeats=a.repeats,
                   stats_blocks_per_image=K.guidance_blocks(HW), stats_read_bytes=read_bytes, ms_per_launch={k: stat(v) for k, v in ms.items()},
                   ms_per_launch_all=ms, stats_gb_per_s=read_bytes / (np.mean(ms["stats"]) * 1e-3) / 1e9, copy_read_gb_per_s=read_bytes / (np.mean(ms["copy"]) * 1e-3) / 1e9)
        if not a.no_engine:
            P = E.unet_params(model)
            c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.5).astype(np.float32)
            lab = (lambda: (rng.standard_normal(P.ch_adm_in) * 0.5).astype(np.float32)) if P.ch_adm_in else (lambda: None)
            g = E.Generator(model, size, size, B, n_step=a.steps, cfg_scale=cfg, s_ancestral=0.0)
            g.set_cond(c(), lab(), c(), lab())
            ev_ms = []
            for r in range(2):
                g.generate([100 + i for i in range(B)], want_latents=True, want_images=False)
                ev_ms.append(g.last_unet_ms() / g.last_n_step())
            g.destroy()
            rec.update(unet_eval_ms=ev_ms[1], mix_share_plain=float(np.mean(ms["plain"])) / ev_ms[1], mix_share_rescaled=float(np.mean(ms["rescaled"])) / ev_ms[1])
        recs.append(rec)
    line = json.dumps(dict(cases=recs))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
