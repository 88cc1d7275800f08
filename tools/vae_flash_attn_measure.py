"""The KL-VAE decoder with its mid-block attention over a score matrix in memory (`scores`) against the flash launch (`flash`), in one process on one GPU.

usage: python3 tools/vae_flash_attn_measure.py [out.md]          (default profiles/vae_flash_attn.md)

Per size: both plans are built with the same synthetic weights and fed the same latent; after two warm-up evaluations each, the whole decode (host clock around
mlctx_compute + stream synchronise) is timed REPS times per plan, the two plans alternating; then every op of each plan is timed by event pairs (mlctx_profile_ops)
and the four launches of the scores path (V^T, QK^T, row softmax, P.V, per image) are added up against the one flash launch.  Plan device bytes are mem_compute.
The outputs of the two plans are compared (rel-L2 of the image).  A size whose plan cannot be built (device memory) is reported as such, not skipped silently."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlimgsynth_amd import engine as E  # noqa: E402

REPS = 7
SIZES = [("SD1.5 512 x 512, batch 1", "sd1", 64, 1), ("SDXL 1024 x 1024, batch 4", "sdxl", 128, 4), ("SD1.5 2048 x 2048, batch 1", "sd1", 256, 1)]
OLD = ("vae_attn_vT", "vae_attn_qk", "softmax_rows", "vae_attn_pv")


class Plan:
    def __init__(self, model, lat, nb, mode):
        l = E._proto2()
        self.ctx, self.t, self.P, self.lat, self.nb = E.MLCtx(), E.vp(), E.VaeParams(), lat, nb
        E.set_vae_attn(self.ctx, mode)
        E.check1(l.vae_params_get(model.encode(), ctypes.byref(self.P)), "vae_params_get")
        E.check1(l.sdvae_decode_init(self.ctx.h, ctypes.byref(self.P), lat, lat, nb, ctypes.byref(self.t)), "sdvae_decode_init")
        E.check1(l.sdvae_decode_build(self.ctx.h, ctypes.byref(self.P), self.t), "sdvae_decode_build")
        self.ctx.params_synth(1234)

    def run(self, z):
        img = np.empty((self.nb, 3, self.lat * 8, self.lat * 8), np.float32)
        E.check1(E._proto2().sdvae_decode_run(self.ctx.h, self.t, E.fptr(z), E.fptr(img)), "sdvae_decode_run")
        return img

    def timed(self):
        t0 = time.perf_counter()
        self.ctx.compute()
        self.ctx.sync()
        return (time.perf_counter() - t0) * 1e3


def spread(v):
    return f"{np.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f})"


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "vae_flash_attn.md")
    lines = ["# KL-VAE decode: mid-block attention as `scores` against `flash`", "",
             f"One process, one MI355X, synthetic weights; whole-decode times are medians of {REPS} evaluations per plan, the plans alternating (min and max = the spread);",
             "launch times are event pairs around every op of the plan (mlctx_profile_ops), one pass.  Produced by tools/vae_flash_attn_measure.py.", ""]
    for title, model, lat, nb in SIZES:
        T = lat * lat
        lines += [f"## {title} (latent {lat} x {lat}, T = {T})", ""]
        try:
            plans = {name: Plan(model, lat, nb, mode) for name, mode in (("scores", 0), ("flash", 1))}
        except Exception as e:
            lines += [f"not measured: the plans could not be built ({e})", ""]
            continue
        z = (np.random.default_rng(lat).standard_normal((nb, 4, lat, lat)) * 0.5).astype(np.float32)
        img = {n: p.run(z) for n, p in plans.items()}
        d = np.linalg.norm(img["flash"].astype(np.float64) - img["scores"]) / np.linalg.norm(img["scores"].astype(np.float64))
        for p in plans.values():
            p.timed()
        t = {n: [] for n in plans}
        for _ in range(REPS):
            for n, p in plans.items():
                t[n].append(p.timed())
        ops = {n: (p.ctx.op_list(), p.ctx.profile_ops()) for n, p in plans.items()}
        old = {lab: sum(ms for (l, _), ms in zip(*ops["scores"]) if l.split(" ")[0] == lab) for lab in OLD}
        labs, ms_f = ops["flash"]
        i_f = [i for i, (l, _) in enumerate(labs) if l.startswith("vae_attn_flash")][0]
        new, vconv = float(ms_f[i_f]), float(ms_f[i_f - 1])      # (the op recorded before it is the v projection, which vae_attn_vT is in the scores plan)
        flops = 4.0 * nb * T * T * 512
        lines += ["| | scores | flash |", "|---|---|---|",
                  f"| whole decode | {spread(t['scores'])} | {spread(t['flash'])} |",
                  f"| plan device bytes (activations) | {plans['scores'].ctx.info().mem_compute / 2**20:.0f} MiB | {plans['flash'].ctx.info().mem_compute / 2**20:.0f} MiB |",
                  f"| attention launches | {' + '.join(f'{old[k]:.3f}' for k in OLD)} = {sum(old.values()):.3f} ms ({', '.join(OLD)}; {nb} image(s)) | {new:.3f} ms (one launch, "
                  f"{flops / new / 1e9:.0f} TFLOP/s of its 4 n T^2 d FLOP) + v projection {vconv:.3f} ms = {new + vconv:.3f} ms |",
                  "", f"image of the flash plan against the scores plan: rel-L2 {d:.2e}", ""]
        for p in plans.values():
            p.ctx.destroy()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
