"""The measurements of profiles/tome.md, one JSON line per run (appended to --out when given).  Synthetic weights, cfg 7.

ONE process holds an engine without token merging and one with --ratio, same model, size and batch, on the same library.  After a warm-up round, --repeats rounds
alternate them: each round runs one --steps Euler generation per engine (not decoded) and records the mean plan-evaluation time from the engine's device events
(mlis_amd_last_unet_ms / steps; cond and uncond rows are one evaluation).  Then, per engine, --repeats in-plan timings (mlctx_profile_ops: an event pair around
every op) give the summed time of the self-attention launches and, for the merged engine, of each of the four token-merging kernels.  Means with the spread
(min, max) of the rounds.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

stat = lambda v: dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)))
FORMS = {1: "tome_match", 2: "tome_select", 3: "tome_merge", 4: "tome_unmerge"}


def conditioning(E, model, rng):
    P = E.unet_params(model)
    c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.5).astype(np.float32)
    l = (lambda: (rng.standard_normal(P.ch_adm_in) * 0.5).astype(np.float32)) if P.ch_adm_in else (lambda: None)
    return c(), l(), c(), l()


def plan_groups(ctx):
    """op indices of the plan's self-attention launches, of its separate LayerNorm launches, and of each token-merging kernel"""
    g = dict(self_attention=[], layernorm=[], **{n: [] for n in FORMS.values()})
    for i, (kind, label, fused, once, _, a) in enumerate(ctx.op_records()):
        if kind == "copy" and a.tome:
            g[FORMS[a.tome]].append(i)
        elif kind == "attn" and a.Tq == a.Tk:
            g["self_attention"].append(i)
        elif kind == "ln" and not fused:
            g["layernorm"].append(i)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="sdxl")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--max-ds", type=int, default=0)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tome_measure needs a GPU"
    from mlimgsynth_amd import engine as E
    rng = np.random.default_rng(0)
    cond = conditioning(E, a.model, rng)
    eng = {}
    for ratio in (0.0, a.ratio):
        eng[ratio] = E.Generator(a.model, a.size, a.size, a.batch, n_step=a.steps, cfg_scale=7.0, s_ancestral=0.0, tome=ratio, tome_max_ds=a.max_ds)
        eng[ratio].set_cond(*cond)
    seeds = [100 + i for i in range(a.batch)]
    ms = {t: [] for t in eng}
    for r in range(a.repeats + 1):                       # round 0 warms every engine up
        for t, g in eng.items():
            g.generate(seeds, want_latents=True, want_images=False)
            if r:
                ms[t].append(g.last_unet_ms() / g.last_n_step())      # Euler without noise: one plan evaluation per step
    rec = dict(what="tome", model=a.model, size=a.size, batch=a.batch, steps=a.steps, repeats=a.repeats, engines=[])
    for t, g in eng.items():
        u = g.unet_ctx()
        groups = plan_groups(u)
        times = [u.profile_ops() for _ in range(a.repeats + 1)][1:]
        rec["engines"].append(dict(ratio=t, info=g.tome_info(), eval_ms=stat(ms[t]), eval_ms_all=ms[t], in_plan_ms_all_ops=stat([float(tm.sum()) for tm in times]),
                                   **{k: dict(launches=len(ix), ms=stat([float(sum(tm[i] for i in ix)) for tm in times])) for k, ix in groups.items()}))
    for g in eng.values():
        g.destroy()
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
