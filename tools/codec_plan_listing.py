"""Lists the codec plans of dry engines, op for op without addresses (tests/plan_audit.py op_signature), to compare two builds of the library:

    python tools/codec_plan_listing.py a.txt        (build A; MLSD_LIB_PATH picks a library elsewhere)
    python tools/codec_plan_listing.py b.txt        (build B)
    cmp a.txt b.txt

Decoder, encoder, tile decoder and tile encoder (mlis_amd_ctx_at 1 .. 4) of "tinyw" engines (a mid block the flash kernel takes) at 384 x 320 (latent 48 x 40: both dimensions tile at vae_tile 64 and 128), two images, for vae_attn 0 / 1
(1: the decoder rebuilt by mlis_amd_set_vae_attn), vae_tile 0 / 64 / 128, seamless tiling 0 / 3, KL-VAE / TAESD; once more after the tile size and the attention
changed on the live engine; and what a decoder that fails to build leaves.  Needs no GPU."""
import itertools
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import plan_audit as PA  # noqa: E402
from mlimgsynth_amd import _lib, engine  # noqa: E402


def plans(g, out, head):
    l = engine._proto2()
    l.mlis_amd_encoder_prepare.restype, l.mlis_amd_encoder_prepare.argtypes = engine.vp, [engine.vp]
    assert l.mlis_amd_encoder_prepare(g.h)
    tiled = (g.vae_tile_prepare(), g.vae_tile_prepare(encoder=True))
    out.append(f"== {head} tile plans {tiled} info {g.vae_tile_info()} {g.vae_tile_info(encoder=True)}")
    for i in (1, 2, 3, 4):
        c = g.ctx_at(i)
        out.append(f"-- plan {i}: {'none' if c is None else ''}")
        for o in (PA.Plan(c).ops if c is not None else ()):
            out.append(repr(PA.op_signature(o)))


def main(path):
    _lib.lib().mlsd_runtime_dry(1)
    out = []
    for tae, tiling, attn, tile in itertools.product((0, 1), (0, 3), (0, 1), (0, 64, 128)):
        g = engine.Generator("tinyw", 384, 320, 2, defer_weights=True, use_tae=bool(tae), tiling=tiling, vae_attn=attn)
        g.set_vae_tile(tile)
        plans(g, out, f"tae {tae} tiling {tiling} vae_attn {attn} vae_tile {tile}")
        if tile == 64:      # the drop and rebuild paths of a live engine
            g.set_vae_tile(128)
            g.set_vae_attn(1 - attn)
            plans(g, out, "... then vae_tile 128 and the other vae_attn")
        g.destroy()
    g = engine.Generator("tiny", 384, 320, 2, defer_weights=True)      # its mid block is 256 wide: the flash decoder does not build, and stays in place
    try:
        g.set_vae_attn(1)
    except _lib.MlsdError as e:
        out.append(f"== tiny, vae_attn 1: {e}; mode {g.vae_attn()}, decoder of {g.ctx_at(1).info().n_ops} ops, encoder {g.ctx_at(2)}")
    g.destroy()
    open(path, "w").write("\n".join(out) + "\n")
    print(f"{len(out)} lines -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
