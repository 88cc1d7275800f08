"""The measurements of profiles/guidance_limit.md, one JSON line per run (appended to --out when given).  Synthetic data, cfg 12, mimic 7, percentile 0.995, APG
eta 0 and norm 15.

ONE process, per case (model, size, batch): buffers of the mix's shapes (eps NHWC [2B][HW][ld] with the plan's dense ld = 4, x and dx NCHW [B][4][HW]) and, after a
warm-up of every kernel, --repeats rounds that alternate timed windows of --launches launches each, a device event on either side:
  plain        mlsd_dxdt_guided without a factor: the parent commit's mix
  dynthresh    mlsd_guidance_plane_means + mlsd_guidance_plane_select + mlsd_dxdt_limited: the four launches of a thresholded mix
  apg          mlsd_guidance_apg_coef + mlsd_dxdt_limited: the three launches of an APG mix
  means        mlsd_guidance_plane_means alone (two launches)
  select_lds   mlsd_guidance_plane_select alone, keys in LDS (left out where the plane does not fit)
  select_mem   the same launch with mlsd_guidance_select_lds_limit(0): every pass forms the keys from global memory
  copy         a device-to-device copy of the bytes the statistics read (the cond and uncond groups)
Reported per window launch (window time / launches), mean and spread of the rounds.  A window of back-to-back launches on one stream gives a kernel's own time once
that exceeds the rate at which launches can be issued (4 .. 6 microseconds each from Python); below it, it gives that rate.  Then, for the cases with a model, one
engine runs a warm-up and a timed --steps Euler generation for the time of a UNet evaluation from the engine's device events."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

stat = lambda v: dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)))
CASES = {"sdxl": ("sdxl", 1024, 4), "sd1": ("sd1", 512, 1), "big": (None, 2048, 1)}      # big: HW 65536, above the LDS limit of the selection


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="sdxl,sd1,big")
    ap.add_argument("--launches", type=int, default=4000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-engine", action="store_true", help="kernels only: no UNet evaluation time, no share")
    ap.add_argument("--out")
    a = ap.parse_args()
    import ctypes
    import torch
    assert torch.cuda.is_available(), "guidance_limit_measure needs a GPU"
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    l = _lib.lib()
    vp, cf = ctypes.c_void_p, ctypes.c_float
    l.mlsd_event_create.argtypes = [ctypes.POINTER(vp)]
    l.mlsd_event_record.argtypes = [vp, vp]
    l.mlsd_event_sync.argtypes = [vp]
    l.mlsd_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(cf)]
    l.mlsd_memcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int, vp]
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

    limit = K.guidance_select_lds_limit()
    recs = []
    for name in a.cases.split(","):
        model, size, B = CASES[name]
        HW, ld, cfg, mimic, pct, eta, norm = (size // 8) ** 2, 4, 12.0, 7.0, 0.995, 0.0, 15.0
        rng = np.random.default_rng(0)
        eps = _lib.from_numpy(rng.standard_normal((2 * B, HW, ld)).astype(np.float32))
        x = _lib.from_numpy(rng.standard_normal((B, 4, HW)).astype(np.float32))
        dx = _lib.from_numpy(np.zeros((B, 4, HW), np.float32))
        cp = _lib.from_numpy(np.zeros((2 * B, HW, ld), np.float32))
        nb = K.guidance_limit_scratch_bytes(B, 4, HW)
        scratch = _lib.from_numpy(np.zeros(nb // 8, np.float64))
        means, lim = _lib.from_numpy(np.zeros((B, 4, 2), np.float32)), _lib.from_numpy(np.zeros((B, 4, 3), np.float32))
        read_bytes = 2 * B * HW * ld * 4
        sel = lambda: K.guidance_plane_select(eps.ptr, ld, B, 4, HW, cfg, mimic, pct, means.ptr, lim.ptr)

        def sel_mem():
            K.guidance_select_lds_limit(0)
            sel()
            K.guidance_select_lds_limit(limit)
        mean_fn = lambda: K.guidance_plane_means(eps.ptr, ld, B, 4, HW, cfg, mimic, scratch.ptr, nb, means.ptr)
        fns = dict(
            plain=lambda: K.dxdt_guided(eps.ptr, ld, x.ptr, dx.ptr, B, 4, HW, cfg),
            dynthresh=lambda: (mean_fn(), sel(), K.dxdt_limited(eps.ptr, ld, x.ptr, dx.ptr, B, 4, HW, 1, cfg, 0.0, lim.ptr)),
            apg=lambda: (K.guidance_apg_coef(eps.ptr, ld, B, 4, HW, cfg, eta, norm, scratch.ptr, nb, lim.ptr),
                         K.dxdt_limited(eps.ptr, ld, x.ptr, dx.ptr, B, 4, HW, 2, cfg, 0.0, lim.ptr)),
            means=mean_fn, select_lds=sel, select_mem=sel_mem,
            copy=lambda: _lib.check(l.mlsd_memcpy(cp.ptr, eps.ptr, read_bytes, 2, None)))
        if HW * 4 > limit:
            del fns["select_lds"]
        ms = {k: [] for k in fns}
        for r in range(a.repeats + 1):                   # round 0 warms every kernel up
            for k, fn in fns.items():
                t = window(fn, a.launches)
                if r:
                    ms[k].append(t)
        rec = dict(case=name, model=model, size=size, batch=B, HW=HW, ld=ld, cfg=cfg, mimic=mimic, percentile=pct, eta=eta, norm=norm, launches=a.launches,
                   repeats=a.repeats, select_lds_limit=limit, read_bytes=read_bytes, ms_per_launch={k: stat(v) for k, v in ms.items()}, ms_per_launch_all=ms)
        if model and not a.no_engine:
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
            rec.update(unet_eval_ms=ev_ms[1], **{"mix_share_" + k: float(np.mean(ms[k])) / ev_ms[1] for k in ("plain", "dynthresh", "apg")})
        recs.append(rec)
    line = json.dumps(dict(cases=recs))
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
