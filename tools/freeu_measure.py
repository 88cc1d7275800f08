"""The measurements of profiles/freeu.md, one JSON line per run (appended to --out when given).  Synthetic weights, cfg 7.

  bytes                 the FreeU passes of the UNet plan and the bytes they move (mlctx_op_bytes), from a dry plan (no GPU)
  eval                  ONE process holds an engine without and one with FreeU (factors 1.3 1.4 0.9 0.2) of the same model, size and batch.  After a warm-up of
                        both, --repeats rounds alternate them: each round runs one --steps Euler generation per engine (not decoded) and records the mean
                        plan-evaluation time from the engine's device events (mlis_amd_last_unet_ms / steps; cond and uncond rows are one evaluation).  Then, per round, the in-plan timing of the FreeU
                        engine's plan (mlctx_profile_ops: an event pair around every op) summed over its freeu_backbone and its freeu_skip ops.  The spread of
                        the rounds is reported with the means; the difference of the two engines is the cost of the feature, the per-op sums say where it goes.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FACTORS = (1.3, 1.4, 0.9, 0.2)


def conditioning(E, model, rng):
    P = E.unet_params(model)
    c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P.ch_adm_in) * 0.5).astype(np.float32)) if P.ch_adm_in else (lambda: None)
    return c(), l(), c(), l()


def freeu_ops(ctx):
    labels = [lab for lab, _ in ctx.op_list()]
    return {k: [i for i, lab in enumerate(labels) if lab == k] for k in ("freeu_backbone", "freeu_skip")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["bytes", "eval"])
    ap.add_argument("--model", default="sdxl")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    rec = dict(what=a.what, model=a.model, size=a.size, batch=a.batch)
    if a.what == "bytes":
        _lib.lib().mlsd_runtime_dry(1)
        g = E.Generator(a.model, a.size, a.size, a.batch, defer_weights=True, freeu=True)
        u = g.unet_ctx()
        idx, by = freeu_ops(u), u.op_bytes()
        rec.update(stages=g.freeu_info(), backbone_ops=len(idx["freeu_backbone"]), skip_ops=len(idx["freeu_skip"]),
                   backbone_bytes=sum(by[i] for i in idx["freeu_backbone"]), skip_bytes=sum(by[i] for i in idx["freeu_skip"]))
        g.destroy()
    else:
        import torch
        assert torch.cuda.is_available(), "freeu_measure eval needs a GPU"
        rng = np.random.default_rng(0)
        cond = conditioning(E, a.model, rng)
        eng = {}
        for on in (0, 1):
            eng[on] = E.Generator(a.model, a.size, a.size, a.batch, n_step=a.steps, cfg_scale=7.0, s_ancestral=0.0, freeu=bool(on))
            eng[on].set_cond(*cond)
        eng[1].set_freeu(*FACTORS)
        seeds = [100 + i for i in range(a.batch)]
        ms = {0: [], 1: []}
        for r in range(a.repeats + 1):                   # round 0 warms both engines up
            for on in (0, 1):
                eng[on].generate(seeds, want_latents=True, want_images=False)
                if r:
                    ms[on].append(eng[on].last_unet_ms() / eng[on].last_n_step())      # Euler without noise: one plan evaluation (cond and uncond rows together) per step
        u = eng[1].unet_ctx()
        idx = freeu_ops(u)
        per_op = {k: [] for k in idx}
        total = []
        for r in range(a.repeats + 1):
            t = u.profile_ops()
            if r:
                for k in idx:
                    per_op[k].append(float(sum(t[i] for i in idx[k])))
                total.append(float(t.sum()))
        stat = lambda v: dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)))
        rec.update(steps=a.steps, repeats=a.repeats, stages=eng[1].freeu_info(), eval_ms_off=stat(ms[0]), eval_ms_on=stat(ms[1]),
                   eval_ms_off_all=ms[0], eval_ms_on_all=ms[1], in_plan_ms={k: stat(v) for k, v in per_op.items()}, in_plan_ms_all_ops=stat(total),
                   n_ops={k: len(v) for k, v in idx.items()}, bytes={k: float(sum(u.op_bytes()[i] for i in idx[k])) for k in idx})
        for g in eng.values():
            g.destroy()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
