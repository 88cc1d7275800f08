"""The measurements of profiles/pag.md, one JSON line per run (appended to --out when given).  Synthetic weights, cfg 7.

ONE process holds three engines of the same model and size on the same library:
  pag      batch B with perturbed-attention guidance: 3B rows per evaluation, the last B without the middle block's q, k projections and attention
  plain    batch B without it: 2B rows (what a generation costs today)
  rows     a plain engine with as many rows as `pag`: batch 3B / 2 at cfg 7 when 3B is even, else batch 3B at cfg 1 (the same plan either way)
After a warm-up round, --repeats rounds alternate them: each round runs one --steps Euler generation per engine (not decoded) and records the mean
plan-evaluation time from the engine's device events (mlis_amd_last_unet_ms / steps).  Then, per engine, --repeats in-plan timings (mlctx_profile_ops: an event
pair around every op) give the summed time of all ops and, for `pag`, of the added GEMMs, with the shape of each launch of the middle block's self-attentions.
Means with the spread (min, max) of the rounds."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

stat = lambda v: dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)))


def conditioning(E, model, rng):
    P = E.unet_params(model)
    c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P.ch_adm_in) * 0.5).astype(np.float32)) if P.ch_adm_in else (lambda: None)
    return c(), l(), c(), l()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sdxl")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "pag_measure needs a GPU"
    from mlimgsynth_amd import engine as E
    cond = conditioning(E, a.model, np.random.default_rng(0))
    B, N = a.batch, 3 * a.batch
    mk = lambda batch, cfg, **kw: E.Generator(a.model, a.size, a.size, batch, n_step=a.steps, cfg_scale=cfg, s_ancestral=0.0, **kw)
    eng = dict(pag=(mk(B, 7.0, pag=True), B, 7.0), plain=(mk(B, 7.0), B, 7.0), rows=(mk(N // 2, 7.0), N // 2, 7.0) if N % 2 == 0 else (mk(N, 1.0), N, 1.0))
    for g, _, cfg in eng.values():
        g.set_cond(*cond) if cfg > 1 else g.set_cond(cond[0], cond[1])
    eng["pag"][0].set_pag(3.0)
    ms = {k: [] for k in eng}
    for r in range(a.repeats + 1):                       # round 0 warms every engine up
        for k, (g, batch, _) in eng.items():
            g.generate([100 + i for i in range(batch)], want_latents=True, want_images=False)
            if r:
                ms[k].append(g.last_unet_ms() / g.last_n_step())      # Euler without noise: one plan evaluation per step
    rec = dict(model=a.model, size=a.size, batch=B, steps=a.steps, repeats=a.repeats, engines=[])
    for k, (g, batch, cfg) in eng.items():
        u = g.unet_ctx()
        ops = u.op_records()
        extra = [i for i, o in enumerate(ops) if o[1] == "pag_v_proj"]
        mid = [dict(op=i, kind=ops[i][0], M=getattr(ops[i][5], "M", None), N=getattr(ops[i][5], "N", None), n_batch=getattr(ops[i][5], "n_batch", None))
               for j in extra for i in (j - 2, j - 1, j)]
        times = []
        for r in range(a.repeats + 1):
            tm = u.profile_ops()
            if r:
                times.append(tm)
        rec["engines"].append(dict(engine=k, batch=batch, cfg=cfg, rows=g.pag_info()[1], perturbed_attentions=g.pag_info()[0], eval_ms=stat(ms[k]), eval_ms_all=ms[k],
                                   in_plan_ms_all_ops=stat([float(tm.sum()) for tm in times]),
                                   pag_gemm_ms=stat([float(sum(tm[i] for i in extra)) for tm in times]) if extra else None, middle_launches=mid))
    for g, _, _ in eng.values():
        g.destroy()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
