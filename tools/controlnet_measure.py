"""The measurements of profiles/controlnet.md, one JSON line per run (appended to --out when given).  Synthetic weights, cfg 7, a random control image.

  flops                 FLOP counts of the UNet, ControlNet and hint plans and their ratio, from dry plans (no GPU)
  eval [--evals K]      K controlled evaluations through mlis_amd_dxdt after a warm-up: the run to put under
                        `rocprofv3 --kernel-trace --stats -- python tools/controlnet_measure.py eval ...` for the share of the ControlNet plan and of
                        the ctrl_add launches in one evaluation (a run of its own: no counters, no other tracing)
  generate              one warm-up and --repeats timed 20-step Euler-a generations (not decoded), and the free device memory before and after the
                        engine was built.  Run it alternating --control 0 and --control 1, two rounds, on one box; report every time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def free_bytes():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def conditioning(E, model, rng):
    P = E.unet_params(model)
    c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P.ch_adm_in) * 0.5).astype(np.float32)) if P.ch_adm_in else (lambda: None)
    return c(), l(), c(), l()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["flops", "eval", "generate"])
    ap.add_argument("--model", default="sdxl")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--control", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    rec = dict(what=a.what, model=a.model, size=a.size, batch=a.batch, control=a.control)
    if a.what == "flops":
        _lib.lib().mlsd_runtime_dry(1)
        g = E.Generator(a.model, a.size, a.size, a.batch, defer_weights=True, control=True)
        f = [g.ctx_at(i).info().flops for i in (0, 5, 6)]
        rec.update(unet_flops=f[0], controlnet_flops=f[1], hint_flops=f[2], ratio=f[1] / f[0], unet_ops=g.ctx_at(0).info().n_ops, controlnet_ops=g.ctx_at(5).info().n_ops)
        g.destroy()
    else:
        rng = np.random.default_rng(0)
        before = free_bytes()
        g = E.Generator(a.model, a.size, a.size, a.batch, n_step=a.steps, cfg_scale=7.0, control=bool(a.control))
        g.set_cond(*conditioning(E, a.model, rng))
        if a.control:
            g.set_control_image(rng.random((3, a.size, a.size)).astype(np.float32))
        rec.update(free_before=before, free_after=free_bytes())
        if a.what == "eval":
            x = (rng.standard_normal((a.batch, 4, a.size // 8, a.size // 8)) * 3).astype(np.float32)
            g.dxdt(x, 3.0)
            t0 = time.time()
            for _ in range(a.evals):
                g.dxdt(x, 3.0)
            rec.update(evals=a.evals, seconds=time.time() - t0)
        else:
            times = []
            for r in range(a.repeats + 1):
                t0 = time.time()
                g.generate([100 + i for i in range(a.batch)], want_latents=True, want_images=False)
                times.append(time.time() - t0)
            rec.update(warmup_s=times[0], seconds=times[1:], unet_ms=g.last_unet_ms(), evals_controlled=g.control_info()[1])
        g.destroy()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
