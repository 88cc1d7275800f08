"""The measurements of profiles/unet_tile.md, one JSON line per run (appended to --out when given).  SDXL, synthetic weights, batch 1, cfg 7,
a 2048 x 2048 canvas; tiled = 1024 tile, 256 overlap.

  count [--tile-batch P]    window count, windows per plan evaluation and plan evaluations per step for that configuration (mlis_amd_tile_pack;
                            geometry only: no GPU)
  eval [--evals K]          K tiled evaluations through mlis_amd_dxdt after a warm-up: the run to put under
                            `rocprofv3 --kernel-trace --stats -- python tools/unet_tile_measure.py eval` for the share of the
                            window_gather / window_blend launches in one evaluation (a run of its own: no counters, no other tracing)
  generate --tile PX        one warm-up and --repeats timed 20-step Euler-a generations (not decoded) with unet_tile PX (0 = untiled, the
                            parent commit's behaviour), and the free device memory before and after the engine was built.  Run it alternating
                            --tile 1024 and --tile 0, two rounds, on one box; report every time, not a ratio alone.
  --tile-batch P            (eval, generate) unet_tile_batch: at most P windows per plan evaluation; 1 is the behaviour of the commit before packing
  --unet-split              (generate) stream the UNet's weights: one pass over them per plan evaluation

Times are host clocks around mlis_generate, which ends with the latent on the host."""
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
CANVAS, TILE, OVERLAP, STEPS = 2048, 1024, 256, 20


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


def count(args):
    from mlimgsynth_amd import kernels as K
    s = K.window_starts(CANVAS // 8, TILE // 8, OVERLAP // 8)
    P, n_eval = K.tile_pack(len(s) ** 2, 1, args.tile_batch)
    emit(args, dict(what="count", canvas=CANVAS, tile=TILE, overlap=OVERLAP, starts_per_axis=s, windows=len(s) ** 2, tile_batch=args.tile_batch,
                    windows_per_plan_evaluation=P, plan_evaluations_per_step=n_eval,
                    note=f"euler: one canvas evaluation per step; each plan evaluation is batch {2 * P} (cond + uncond of {P} windows)"))


def evaluate(args):
    from mlimgsynth_amd import engine as E
    g = E.Generator("sdxl", CANVAS, CANVAS, 1, cfg_scale=7.0, unet_tile=TILE, unet_tile_overlap=OVERLAP, unet_tile_batch=args.tile_batch)
    rng = np.random.default_rng(0)
    P = g.P
    c = lambda: (rng.standard_normal((77, P.n_ctx)) * 0.1).astype(np.float32)
    l = lambda: (rng.standard_normal(P.ch_adm_in) * 0.1).astype(np.float32)
    g.set_cond(c(), l(), c(), l())
    x = (rng.standard_normal((1, 4, CANVAS // 8, CANVAS // 8)) * 5).astype(np.float32)
    g.dxdt(x, 5.0)                                           # warm-up: first-touch, plan tuning
    ts = []
    for _ in range(args.evals):
        t = time.perf_counter()
        g.dxdt(x, 5.0)
        ts.append(time.perf_counter() - t)
    emit(args, dict(what="eval", windows=g.tile_info()[0], tile_pack=g.tile_pack_info(), seconds_per_evaluation_incl_host_copies=stats(ts)))
    g.destroy()


def free_bytes():
    import torch
    return int(torch.cuda.mem_get_info()[0])


def generate(args):
    import mlis_ffi as F
    from mlimgsynth_amd import _lib
    _lib.lib()
    lib = F.bind(_lib.LIB_PATH)
    lib.mlis_amd_engine_builds.argtypes = [C.c_void_p]
    m = F.Mlis(lib)
    try:
        m.set("model", "synth:sdxl"), m.set("image_dim", CANVAS, CANVAS), m.set("steps", STEPS), m.set("seed", 42), m.set("cfg_scale", 7.0)
        m.set("method", "euler_a"), m.set("no_decode", 1)
        m.set("unet_tile", args.tile), m.set("unet_tile_overlap", OVERLAP), m.set("unet_tile_batch", args.tile_batch)
        if args.unet_split:
            m.set("unet_split", 1)
        before = free_bytes()
        ts = []
        for i in range(args.repeats + 1):
            m.tokens(TOKS), m.tokens(NTOKS, negative=True)
            t = time.perf_counter()
            m.generate()
            dt = time.perf_counter() - t
            if i == 0:
                after = free_bytes()                         # the first call builds the engine
            else:
                ts.append(dt)
        emit(args, dict(what="generate", tile=args.tile, overlap=OVERLAP if args.tile else 0, tile_batch=args.tile_batch, unet_split=bool(args.unet_split), steps=STEPS, seconds=stats(ts),
                        free_gib_before=round(before / 2**30, 2), free_gib_after_build=round(after / 2**30, 2),
                        builds=lib.mlis_amd_engine_builds(m.ctx), info=lib.mlis_infotext_get(m.ctx, 0).decode().splitlines()[-1]))
    finally:
        m.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["count", "eval", "generate"])
    ap.add_argument("--tile", type=int, default=TILE)
    ap.add_argument("--tile-batch", type=int, default=1)
    ap.add_argument("--unet-split", action="store_true")
    ap.add_argument("--evals", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    dict(count=count, eval=evaluate, generate=generate)[a.what](a)
