"""The measurements of profiles/hypertile.md, one JSON line per run (appended to --out when given).  Synthetic weights, cfg 7.

  eval     ONE process holds an engine without HyperTile and one per --tile value, same model, size and batch, on the same library.  After a warm-up round,
           --repeats rounds alternate them: each round runs one --steps Euler generation per engine (not decoded) and records the mean plan-evaluation time from
           the engine's device events (mlis_amd_last_unet_ms / steps; cond and uncond rows are one evaluation).  Then, per engine, --repeats in-plan timings
           (mlctx_profile_ops: an event pair around every op) give, per self-attention shape, the launches, their route label (mlsd_attention_variant) and their
           summed time, and the summed time of the permuting copies.  Means with the spread (min, max) of the rounds.
  kernel   mlsd_tile_permute alone on the two tiled SDXL 1024 x 1024 batch-4 shapes, against mlsd_memcpy (device to device) of the same bytes: --repeats rounds
           of --iters back-to-back launches between two events, after a warm-up round; microseconds per launch and the permutation's rate as a share of the copy's.
"""
import argparse
import ctypes
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


def plan_groups(K, ctx):
    """{("attn", shape, label): [op indices]} of the plan's self-attention launches, and the indices of its permuting copies"""
    groups, copies = {}, []
    for i, (kind, label, fused, once, _, a) in enumerate(ctx.op_records()):
        if kind == "copy" and a.th > 0:
            copies.append(i)
        elif kind == "attn" and a.Tq == a.Tk:
            key = (f"b{a.n_batch} h{a.n_head} d{a.d_head} {a.Tq}x{a.Tk}", K.attention_variant(a))
            groups.setdefault(key, []).append(i)
    return groups, copies


def measure_eval(a, rec):
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    rng = np.random.default_rng(0)
    cond = conditioning(E, a.model, rng)
    eng = {}
    for tile in [0] + a.tile:
        eng[tile] = E.Generator(a.model, a.size, a.size, a.batch, n_step=a.steps, cfg_scale=7.0, s_ancestral=0.0, hypertile=tile, hypertile_depth=a.depth)
        eng[tile].set_cond(*cond)
    seeds = [100 + i for i in range(a.batch)]
    ms = {t: [] for t in eng}
    for r in range(a.repeats + 1):                       # round 0 warms every engine up
        for t, g in eng.items():
            g.generate(seeds, want_latents=True, want_images=False)
            if r:
                ms[t].append(g.last_unet_ms() / g.last_n_step())      # Euler without noise: one plan evaluation per step
    rec.update(steps=a.steps, repeats=a.repeats, depth=a.depth, engines=[])
    for t, g in eng.items():
        u = g.unet_ctx()
        groups, copies = plan_groups(K, u)
        by = u.op_bytes()
        times = []
        for r in range(a.repeats + 1):
            tm = u.profile_ops()
            if r:
                times.append(tm)
        attn = [dict(shape=s, route=lab, launches=len(ix), ms=stat([float(sum(tm[i] for i in ix)) for tm in times])) for (s, lab), ix in groups.items()]
        rec["engines"].append(dict(tile=t, info=g.hypertile_info(), eval_ms=stat(ms[t]), eval_ms_all=ms[t], self_attention=attn,
                                   self_attention_ms=stat([float(sum(tm[i] for ix in groups.values() for i in ix)) for tm in times]),
                                   copies=len(copies), copy_bytes=float(sum(by[i] for i in copies)), copy_ms=stat([float(sum(tm[i] for i in copies)) for tm in times]),
                                   in_plan_ms_all_ops=stat([float(tm.sum()) for tm in times])))
    for g in eng.values():
        g.destroy()


def measure_kernel(a, rec):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    vp = ctypes.c_void_p
    L.mlsd_event_elapsed_ms.argtypes = [vp, vp, ctypes.POINTER(ctypes.c_float)]
    ev = [vp(), vp()]
    for e in ev:
        _lib.check(L.mlsd_event_create(ctypes.byref(e)))
    rec.update(iters=a.iters, repeats=a.repeats, shapes=[])
    # SDXL 1024 x 1024 batch 4 (N = 8) with tile 512: 64 x 64 tokens of 640 halfs in tiles of 32 x 32, 32 x 32 tokens of 1280 halfs in tiles of 16 x 16
    for n, H, W, th, tw, rb in ((8, 64, 64, 32, 32, 1280), (8, 32, 32, 16, 16, 2560)):
        nbytes = n * H * W * rb
        src = _lib.from_numpy(np.random.default_rng(1).integers(0, 256, nbytes, dtype=np.uint8))
        dst = _lib.DeviceBuffer(nbytes)

        def timed(launch):
            out = []
            for r in range(a.repeats + 1):
                _lib.check(L.mlsd_event_record(ev[0], None))
                for _ in range(a.iters):
                    launch()
                _lib.check(L.mlsd_event_record(ev[1], None))
                _lib.check(L.mlsd_event_sync(ev[1]))
                t = ctypes.c_float()
                _lib.check(L.mlsd_event_elapsed_ms(ev[0], ev[1], ctypes.byref(t)))
                if r:
                    out.append(1e3 * t.value / a.iters)
            return out
        fwd = timed(lambda: K.tile_permute(src.ptr, dst.ptr, n, H, W, th, tw, rb))
        inv = timed(lambda: K.tile_permute(src.ptr, dst.ptr, n, H, W, th, tw, rb, inverse=True))
        cpy = timed(lambda: _lib.check(L.mlsd_memcpy(vp(dst.ptr), vp(src.ptr), ctypes.c_size_t(nbytes), 2, None)))
        rec["shapes"].append(dict(shape=[n, H, W, th, tw, rb], bytes=nbytes, permute_us=stat(fwd), inverse_us=stat(inv), memcpy_us=stat(cpy),
                                  rate_share_of_memcpy=float(np.mean(cpy) / np.mean(fwd)), gb_per_s=2e-3 * nbytes / float(np.mean(fwd))))
        src.free(), dst.free()
    for e in ev:
        L.mlsd_event_destroy(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["eval", "kernel"])
    ap.add_argument("--model", default="sdxl")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--tile", type=int, nargs="+", default=[512])
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "hypertile_measure needs a GPU"
    rec = dict(what=a.what)
    if a.what == "eval":
        rec.update(model=a.model, size=a.size, batch=a.batch)
        measure_eval(a, rec)
    else:
        measure_kernel(a, rec)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
