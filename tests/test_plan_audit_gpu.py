"""Prepared plans on the device, audited launch by launch (tests/plan_audit.py).

Every plan is built with MLB_F_KEEP (no block is lent out twice, so every operand is still in memory when the evaluation ends) and the synthetic
weights, computed once, and then EVERY launch is recomputed in float64 from the operands it actually read -- folded residuals and row biases,
column views, producer statistics, LayerNorm endings, hoisted ops -- and held to the per-element / per-row bounds of tests/ref64.py.  With -s the
worst ratio per (kind, path) is printed.  The second test compares the default (recycling) plan with the kept plan bit for bit: the arena must
not change a result.

The option plans are audited the same way (tests/plan_audit.py has their rules): a UNet with the control sums of a ControlNet plan of fewer images, the same at
gain 0 with poisoned residuals, the ControlNet plan and its hint block, FreeU, control + PAG (the third row group reads the cond group's residuals), HyperTile with
and without PAG (permuting copies bit for bit, per-tile attention, pag_v_proj in tile-major order), and the forced phase form of the upsampling convolution, plain
and with seamless tiling, on a poisoned map.  What those plans read from outside themselves is declared by the builder; an undeclared range fails the coverage check.

Measured on MI355X, worst ratio to the bound over these plans: control sum 0.982 (the bound is attained where the base vanishes; gain 0: bit-equal), freeu_backbone
0.063 (the kept half bit-equal), freeu_skip 0.210, tile / untile copies bit-equal, phase launches against their own operands 0.021, the assembled map against
upsample + 3x3 with the loaded weight 0.131 (0.069 with seamless tiling), no pixel of another parity or of the poison left.

Two censuses close the file.  The first holds every op form of the bench plans (SD1.5 64x64 N = 2, SDXL 128x128 N = 8, their KL-VAE decoders).  The second holds the
plans of PA.SIZE_PLANS, sizes nobody tuned: SD1.5 at 64x64 with N = 1, 3, 4, 6, 8, at 64x96, 96x64, 96x96, 72x88, 88x72 and 40x40; SDXL at 128x128 with N = 1, 2, 3,
4, 6, at 104x152 (N = 2 and 8), 152x104, 112x144, 168x96, 96x96, 64x64, 120x136, 100x100 and at the bench size with a 154-token context; the KL-VAE decoders at 96
(sd1), 128, 96 x 2 images and 100 (sdxl), the encoders at 128 (sdxl) and 64 (sd1), TAESD both ways at 64.  Each form must be met in an audited plan or a bench plan
or be listed in COVERED_ELSEWHERE with the float64 case of exactly that form; tests/test_size_census_cpu.py runs the same rule in the dry runtime.

Measured on MI355X: the 35 size plans have 10 to 54 op forms each, 5 to 38 of them met in audited plans; 34 GEMM forms and attn<64x2> are held by the entries added
for them.  Five of those only the device meets (the dry runtime has no device to ask for its CUs and plans the fall-back of a stream-K tile): 256x256x64ppsk with a
row bias, 128x320x64ppsk with a residual, 128x320x64pp with (colstats, row bias), 256x256x64pp with (colstats) and (colstats, residual).  Worst ratio over the cases
written for these forms (tests/gemm64_cases.py): C32 0.204 (s29_conv_rowbias), C16 0.999 (g16_c16; C16 == fp16_rne(C32) bit for bit everywhere), column statistics
0.059 (g9_stats_res), LayerNorm ending 0.983 (sk0_ln, sk0_ln_res).  Every census parameter builds in under half a second.
"""
import contextlib
import os
import re

import numpy as np
import pytest

import plan_audit as PA
import test_hypertile_cpu as THC
import test_pag_cpu as TPC

pytestmark = pytest.mark.gpu

KEEP = PA.MLB_F_OPSHAPES | PA.MLB_F_KEEP

# (spec, xattn mode while the plan is built, kinds the plan must contain)
AUDITED = [
    (("unet", "tiny", 16, 2), None, {"gemm", "attn", "gn", "ln", "act", "temb", "n2h"}),
    (("unet", "tinyxl", 16, 2), None, {"gemm", "attn", "gn", "ln"}),
    (("unet", "sd1", 16, 2), None, {"gemm", "attn", "gn", "ln"}),                # 512 x 320 rows: the 128x160 LayerNorm ending; 8-row levels: split-K, skinny tiles
    (("vae_dec", "tiny", 8, 1), None, {"gemm", "gn", "smax", "n2h"}),
    (("vae_enc", "tiny", 8, 1), None, {"gemm", "gn", "smax", "n2h"}),
    (("tae_dec", "tiny", 8, 1), None, {"gemm", "n2h"}),
    (("clip", "tiny", 2), None, {"gemm", "attn", "ln", "cemb"}),                  # causal attention, quick-GELU, clip_embed
    # mlsd_gemm_set_xattn(2): the cross attention ends its q projection wherever the kernel takes the launch.  It takes 320-column projections (5 heads of 64) of
    # K >= 192 on 128-row blocks: tinyxl's 64 / 128 channels never qualify, so the configuration is run at 320 channels on both levels (n_ch = 320, ch_mult 1, 1;
    # 16 x 8 = 128 tokens at the attention level): K / V as column views of the batched context projection, the hoisted V^T pack, a q projection that stores no C16
    (("unet", "tinyxl", (32, 16), 2, dict(params=dict(n_ch=320, ch_mult=(1, 1, 0, 0, 0)))), 2, {"gemm", "attn", "xavt"}),
    (("unet", "sd1", 8, 2, dict(n_ctx_tok=154)), None, {"attn_ctx"}),             # windowed context: OP_ATTN_CTX
    # ---- the option plans.  ControlNet: the UNet's control sums on the residuals of a ControlNet plan of ONE image (image n reads residual image n % 1), the same
    # with gain 0 (the sums are bit copies and the residuals, poisoned, are never read), the ControlNet plan itself and its hint block
    (("unet", "tinyxl", 16, 2, dict(control=1)), None, {"cadd"}),
    (("unet", "tinyxl", 16, 2, dict(control=1, gain=0.0)), None, {"cadd"}),
    (("controlnet", "tinyxl", 16, 1), None, {"gemm", "gn", "attn"}),
    (("control_hint", "tinyxl", 16), None, {"gemm", "n2h"}),
    (("unet", "tinyxl", 16, 2, dict(freeu=True)), None, {"freeu_backbone", "freeu_skip"}),      # both stages; the half kept; the padding
    (("unet", "tinyxl", 16, 3, dict(control=2, pag=1)), None, {"cadd"}),          # pag_tail: row group 3 reads the cond residuals; the pag_v_proj GEMM
    # HyperTile (non-square tiles at 20 x 12 and 16 x 24) and PAG inside tiles: pag_v_proj's rows in tile-major order.  The permuting copies, the per-tile attention
    # (n_batch = images x tiles, batch strides of a tile) and pag_v_proj (a GEMM on a row slice of the fused q | k | v weight into the tail rows of the attention
    # output) are judged by the copy rule above and by the unchanged GEMM and attention verifiers, from their raw arguments: the audit needed no code for them
    (THC.AUDITED[0], None, {"copy", "attn"}), (THC.AUDITED[1], None, {"copy", "attn"}), (THC.AUDITED[2], None, {"copy", "attn"}),
    (TPC.AUDITED[2], None, {"copy", "attn"}),
    # the phase form of the upsampling convolution, forced (320 channels on both levels: a form the ping-pong tiles take), plain and with seamless tiling
    (("unet", "tinyxl", (32, 16), 2, dict(params=dict(n_ch=320, ch_mult=(1, 1, 0, 0, 0)), ups_phases=2)), None, {"gemm"}),
    (("unet", "tinyxl", (32, 16), 2, dict(params=dict(n_ch=320, ch_mult=(1, 1, 0, 0, 0)), ups_phases=2, tiling=3)), None, {"gemm"}),
]
assert THC.AUDITED[2] == ("unet", "sd1", (16, 24), 2, dict(hypertile=64)) and TPC.AUDITED[2] == ("unet", "tiny", 16, 6, dict(pag=2, hypertile=32))
# + the SDXL real configuration at the smallest latent its three levels accept, for the bit comparison only
BITWISE = [(s, x) for s, x, _ in AUDITED] + [(("unet", "sdxl", 4, 2), None)]


@contextlib.contextmanager
def _built(E, spec, xattn, flags, synth):
    """the plan, built AND used under the xattn mode (the launcher asks the mode again at every launch), closed and the mode restored afterwards"""
    engine, _lib = E
    L = _lib.lib()
    b = None
    try:
        if xattn is not None:
            L.mlsd_gemm_set_xattn(xattn)
        b = PA.build(engine, spec, flags, synth=synth)
        yield b
    finally:
        if b is not None:
            b.close()
        if xattn is not None:
            L.mlsd_gemm_set_xattn(-1)


@pytest.fixture(scope="module")
def E():
    from mlimgsynth_amd import _lib, engine
    yield engine, _lib


@pytest.mark.parametrize("spec,xattn,kinds", AUDITED, ids=[PA.plan_id(s) + ("-xattn2" if x else "") for s, x, _ in AUDITED])
def test_every_launch_against_float64(E, spec, xattn, kinds):
    engine, _lib = E
    with _built(E, spec, xattn, KEEP, True) as b:
        out = b.run(1)
        assert np.isfinite(out).all()
        mem = PA.DeviceMemory(_lib)
        plan = PA.Plan(b.ctx, PA.plan_id(spec), external=b.external, mem=mem)
        assert kinds <= {o.kind for o in plan.ops}, sorted({o.kind for o in plan.ops})
        gone = PA.clobbered_operands(plan)
        assert not gone, [f"{w} ({wn}) overwrites operand {rn} of {r}" for w, wn, r, rn in gone[:8]]
        uncovered = PA.uncovered_reads(plan)      # (what the plan reads from outside itself -- residuals, gain, FreeU factors, hint embedding -- is declared by the builder)
        assert not uncovered, [why for _, _, why in uncovered[:6]]
        worst, bad = {}, []
        for i, op in enumerate(plan.ops):
            if op.fused:      # checked as the ending of its producer, which must carry it
                prod = plan.ops[i - 1]
                assert prod.kind == "gemm" and (prod.a.ln_y16 == op.a.y16 if op.kind == "ln" else prod.a.gn_y16 == op.a.y16), (op, prod)
            key, ratios = PA.verify_op(mem, plan, i)
            for name, r in ratios.items():
                k = key + (name,)
                worst[k] = max(worst.get(k, 0.0), r)
                if not r <= 1.0:
                    bad.append(f"{op} output {name}: ratio {r:.4g}")
        n_xa = sum(1 for o in plan.ops if o.kind == "gemm" and o.a.xa_k)
        print(f"\n[plan audit] {PA.plan_id(spec)}{' xattn(2)' if xattn else ''}: {len(plan.ops)} ops, {n_xa} q projections end with their attention; worst ratio per (kind, path, output):")
        for k, r in sorted(worst.items(), key=str):
            print(f"  {k[0]:9s} {str(k[1]):44s} {k[2]:14s} {r:8.3f}")
        assert not bad, bad[:12]
        _option_forms(spec, plan, worst, b)
        if xattn:      # the plan is here for the ending: it must have been taken, checked and fed by the hoisted pack
            assert n_xa > 0 and any(k[2] == "xa_out" for k in worst) and any(k[0] == "xavt" for k in worst), (n_xa, sorted(worst, key=str))
            assert all(not any(w.name == "C16" for w in o.writes) for o in plan.ops if o.kind == "gemm" and o.a.xa_k)


def _option_forms(spec, plan, worst, b):
    """the forms an option plan is in AUDITED for: present, and judged by their own rule"""
    opt = spec[4] if len(spec) > 4 and isinstance(spec[4], dict) else {}
    seen = {k[:2] for k in worst}
    cadd = [o for o in plan.ops if o.kind == "cadd"]
    if opt.get("control"):
        assert cadd and all(o.a.n_ctrl == opt["control"] < o.a.n_img == spec[3] for o in cadd)
        zero = opt.get("gain") == 0.0
        assert (("cadd", "gain 0") in seen) == zero and (("cadd", "") in seen) != zero
        assert all(("ctrl" in [r.name for r in o.reads]) != zero for o in cadd)
        assert all(np.isnan(PA._mat(PA.DeviceMemory(b.info["control"]._lib), o.a.ctrl, 1, o.a.C, o.a.C, np.float32)).all() == zero for o in cadd)
    if opt.get("pag"):
        assert any(o.kind == "gemm" and o.label == "pag_v_proj" for o in plan.ops)
        if opt.get("control"):      # pag_tail: the third row group adds the cond group's residuals
            assert all(o.a.n_img == o.a.n_ctrl + opt["pag"] for o in cadd)
    if opt.get("freeu"):
        n1, n2 = b.info["freeu_stages"]
        assert n1 > 0 and n2 > 0 and ("freeu_backbone", "") in seen and ("freeu_skip", "") in seen and any(k[2] == "kept half" for k in worst)
        assert sum(1 for o in plan.ops if o.kind == "freeu_skip") == n1 + n2 == sum(1 for o in plan.ops if o.kind == "freeu_backbone")
    if opt.get("hypertile"):
        cp = [o for o in plan.ops if o.kind == "copy" and o.a.th > 0]
        assert ("copy", "tile") in seen and ("copy", "untile") in seen and len(cp) % 2 == 0
        for c in cp:      # every tiled level has self-attentions over its tiles: n_batch = images x tiles, a tile's tokens each
            nt = (c.a.H // c.a.th) * (c.a.W // c.a.tw)
            assert any(o.kind == "attn" and o.a.Tq == o.a.Tk == c.a.th * c.a.tw and o.a.n_batch % nt == 0 and 0 < o.a.n_batch // nt <= c.a.n_img for o in plan.ops), c
        if isinstance(spec[2], tuple):      # maps that are not square; at 20 x 12 the second level (10 x 6 tokens) is cut into tiles that are not square either
            assert all(c.a.H != c.a.W for c in cp) and (spec[2] != (20, 12) or any(c.a.th != c.a.tw for c in cp))
    if opt.get("ups_phases"):
        ph = [o for o in plan.ops if o.kind == "gemm" and o.a.out_phase]
        assert [o.a.out_phase for o in ph] == [1, 2, 3, 4] and all(bool(o.a.wrap) == bool(opt.get("tiling")) for o in ph)
        assert {k[2] for k in worst if k[0] == "gemm" and str(k[1]).endswith("phase")} == {"C32", "other parities", "assembled"}


def _two_evaluations(E, spec, xattn, flags):
    with _built(E, spec, xattn, flags, True) as b:
        sig = [PA.op_signature(o) for o in PA.Plan(b.ctx).ops]
        return [b.run(1), b.run(5), b.run(1)], sig      # changed inputs, then the first ones again: hoisted ops and hand-off scratch are reused


@pytest.mark.parametrize("spec,xattn", BITWISE, ids=[PA.plan_id(s) + ("-xattn2" if x else "") for s, x in BITWISE])
def test_recycling_plan_equals_kept_plan_bit_for_bit(E, spec, xattn):
    env = os.environ.get("MLSD_NO_LN_FOLD")
    try:
        rec, sig_r = _two_evaluations(E, spec, xattn, PA.MLB_F_OPSHAPES)
        kept, sig_k = _two_evaluations(E, spec, xattn, KEEP)
        if sig_r != sig_k:      # a LayerNorm fold the alias rule refuses only in the recycling plan: compare the unfolded plans
            print(f"\n[plan audit] {PA.plan_id(spec)}: op lists differ in {sum(a != b for a, b in zip(sig_r, sig_k))} ops; compared with MLSD_NO_LN_FOLD=1")
            os.environ["MLSD_NO_LN_FOLD"] = "1"
            rec, sig_r = _two_evaluations(E, spec, xattn, PA.MLB_F_OPSHAPES)
            kept, sig_k = _two_evaluations(E, spec, xattn, KEEP)
            assert sig_r == sig_k
    finally:
        if env is None:
            os.environ.pop("MLSD_NO_LN_FOLD", None)
        else:
            os.environ["MLSD_NO_LN_FOLD"] = env
    for n, (a, b) in enumerate(zip(rec, kept)):
        assert np.isfinite(a).all() and a.tobytes() == b.tobytes(), f"evaluation {n}: {int((a != b).sum())} of {a.size} values differ"
    assert rec[0].tobytes() == rec[2].tobytes() and rec[0].tobytes() != rec[1].tobytes()


# ------------------------------------------------------------------ census
def _case_features(c):
    return {name for name, on in (("row bias", c["rowbias"]), ("residual", c["resid"]), ("act_after_resid", c["post"]), ("GEGLU", c["act"] == 5),
                                  ("C16 + C32", c["c16"] and c["c32"]), ("colstats", c["stats"]), ("LN ending", c["ln"]), ("upsample", c.get("ups"))) if on}


# Op forms of the bench plans that the audited plans above do not contain, and the kernel-level float64 test that holds EXACTLY that form: a GEMM case on the same
# tile and split form with the same set of epilogue features, no more and no fewer (each combination selects its own epilogue body); an attention case with the
# same kernel label.  `once` only says when a launch runs (the later evaluations of the bit comparison above exercise it): the case is the form without it.
# A form that a bench plan newly takes fails the census until its case is written and listed here.
COVERED_ELSEWHERE = {
    ('attn', 'attn<64x2s,d40>', ()): "test_attention_float64_gpu.py::test_attention_float64[x2s_d40_tk192_sigma1]",
    ('attn', 'attn<64x2s,d64>', ()): "test_attention_float64_gpu.py::test_attention_float64[x2s_tk128_sigma1]",
    ('attn', 'attn<tile,d160>', ()): "test_attention_float64_gpu.py::test_attention_float64[tile_d160_tk200_sigma1]",
    ('attn', 'attn<tile,d80>', ()): "test_attention_float64_gpu.py::test_attention_float64[tile_d80_tk200_sigma1]",
    ('gemm', ('128x128x64s2', 'splitk'), ('C16 + C32', 'colstats')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_c16_stats]",
    ('gemm', ('128x128x64s2', 'splitk'), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_unequal]",
    ('gemm', ('128x128x64s2', 'splitk'), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_stats_res]",
    ('gemm', ('128x128x64s2', 'splitk'), ('colstats', 'row bias')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_stats_rowbias]",
    ('gemm', ('128x128x64s2', 'splitk'), ('colstats', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_stats_ups]",
    ('gemm', ('128x128x64s2', 'splitk'), ('colstats',)): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_stats]",
    ('gemm', ('128x160x64tt', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[t30_res]",
    ('gemm', ('128x160x64tt', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[t30_f32]",
    ('gemm', ('128x320x64pp', ''), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p18_generic_silu]",
    ('gemm', ('128x320x64pp', ''), ('C16 + C32',)): "test_gemm_float64_gpu.py::test_gemm_float64[p18_subnormal]",
    ('gemm', ('128x320x64pp', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p18_conv_stats_res]",
    ('gemm', ('128x320x64pp', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[p18_f32_res]",
    ('gemm', ('128x320x64pp', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[p18_f16_bigout]",
    ('gemm', ('128x320x64pp', 'layernorm'), ('LN ending', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p18_ln]",
    ('gemm', ('128x320x64pp', 'linear+attention'), ('xattn ending',)): "test_conditioning_gpu.py::test_attention_fused_into_the_q_projection",
    ('gemm', ('128x320x64pp2', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p20_stats_res]",
    ('gemm', ('128x320x64pp2', ''), ('colstats', 'row bias')): "test_gemm_float64_gpu.py::test_gemm_float64[p20_stats_rowbias]",
    ('gemm', ('128x320x64pp2', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[p20_res]",
    ('gemm', ('128x320x64ppsk', ''), ('C16 + C32',)): "test_gemm_float64_gpu.py::test_gemm_float64[p28_sk18_c16]",
    ('gemm', ('128x320x64ppsk', ''), ('row bias',)): "test_gemm_float64_gpu.py::test_gemm_float64[p28_conv_rowbias]",
    ('gemm', ('256x128x32s3', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g4_stats_res]",
    ('gemm', ('256x128x32s3', ''), ('colstats',)): "test_gemm_float64_gpu.py::test_gemm_float64[g4_stats]",
    ('gemm', ('256x128x32s3', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[g4_plain]",
    ('gemm', ('256x128x64s2', ''), ('colstats', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[g3_stats_ups]",
    ('gemm', ('256x256x64pp', ''), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p17_generic_gelu]",
    ('gemm', ('256x256x64pp', ''), ('GEGLU',)): "test_gemm_float64_gpu.py::test_gemm_float64[p17_geglu16]",
    ('gemm', ('256x256x64pp', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[p17_f16]",
    ('gemm', ('256x256x64pp2', ''), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p21_c16_res]",
    ('gemm', ('256x256x64pp2', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p21_stats_res]",
    ('gemm', ('256x256x64pp2', ''), ('colstats',)): "test_gemm_float64_gpu.py::test_gemm_float64[p21_stats]",
    ('gemm', ('256x256x64pp2', ''), ('upsample',)): "test_gemm_float64_gpu.py::test_gemm_float64[p21_ups]",
    ('gemm', ('256x256x64ppsk', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[p19_sk16]",
    ('gemm', ('256x256x64ppsk', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[p19_sk64]",
    ('gemm', ('256x256x64s2w16', ''), ('C16 + C32', 'colstats', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[g9_c16_stats_ups]",
    ('gemm', ('256x256x64s2w16', ''), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g9_c16_res]",
    ('gemm', ('256x256x64s2w16', ''), ('colstats', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[g9_stats_ups]",
    ('gemm', ('256x256x64s2w16', ''), ('colstats',)): "test_gemm_float64_gpu.py::test_gemm_float64[g9_stats]",
    ('gemm', ('256x256x64s2w16', ''), ('once',)): "test_gemm_float64_gpu.py::test_gemm_float64[g9_plain]",
    ('gemm', ('256x256x64s2w16', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[g9_plain]",
    ('gemm', ('64x128x64s2', ''), ('colstats', 'row bias')): "test_gemm_float64_gpu.py::test_gemm_float64[g1_stats_rowbias]",
    ('gemm', ('64x128x64s2', ''), ('colstats', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[g1_stats_ups]",
    ('gemm', ('64x128x64s2', 'splitk'), ('C16 + C32', 'colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[sk1_c16_stats_res]",
    ('gemm', ('conv3x3n16', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[n31_vae_out]",
    ('gemm', ('skinny128x64', ''), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[s29_m8_c16]",
    ('xavt', '', ('once',)): "test_conditioning_gpu.py::test_attention_fused_into_the_q_projection",
    # the phase launches of the SDXL UNet's upsampling convolutions (128 x 128 latent, N = 8) run on the 128x320 ping-pong tile; the audited plans above meet the form
    # on the 256x256 tile, which is the one the KL-VAE decoders' phase launches take
    ('gemm', ('128x320x64pp', ''), ('phase',)): "test_upsample_phases_gpu.py::test_phase_launches_and_assembled_output_float64[t18_b1_w0_h4]",
    # ---- forms that only sizes other than the bench's take (PA.SIZE_PLANS, the census at the end of this file and tests/test_size_census_cpu.py).  Small N and SD1.5
    # with guidance off: split-K whose reduce pass ends with the LayerNorm, a row bias alone on split-K and on the skinny-M kernel
    ('gemm', ('128x128x64s2', 'layernorm+splitk'), ('LN ending', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_ln_res]",
    ('gemm', ('128x128x64s2', 'layernorm+splitk'), ('LN ending',)): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_ln]",
    ('gemm', ('128x128x64s2', 'splitk'), ('row bias',)): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_rowbias]",
    ('gemm', ('128x128x64s2', 'splitk'), ('C16 + C32', 'colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_c16_stats_res]",
    ('gemm', ('128x128x64s2', 'splitk'), ('upsample',)): "test_gemm_float64_gpu.py::test_gemm_float64[sk0_ups]",
    ('gemm', ('64x128x64s2', 'splitk'), ('colstats',)): "test_gemm_float64_gpu.py::test_gemm_float64[sk1_stats]",
    ('gemm', ('skinny128x64', ''), ('row bias',)): "test_gemm_float64_gpu.py::test_gemm_float64[s29_conv_rowbias]",
    # latents that are not square (and 100 x 100): rows that fill no ping-pong wave slab run on the general tiles of the same shape
    ('gemm', ('128x320x64s2', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[g16_plain]",
    ('gemm', ('128x320x64s2', ''), ('upsample',)): "test_gemm_float64_gpu.py::test_gemm_float64[g16_ups]",
    ('gemm', ('128x320x64s2', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[g16_res]",
    ('gemm', ('128x320x64s2', ''), ('row bias',)): "test_gemm_float64_gpu.py::test_gemm_float64[g16_rowbias]",
    ('gemm', ('128x320x64s2', ''), ('C16 + C32',)): "test_gemm_float64_gpu.py::test_gemm_float64[g16_c16]",
    ('gemm', ('128x320x64s2', ''), ('C16 + C32', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g16_c16_res]",
    ('gemm', ('256x256x64s2w16', ''), ('GEGLU',)): "test_gemm_float64_gpu.py::test_gemm_float64[g9_geglu16]",
    ('gemm', ('256x256x64s2w16', ''), ('row bias',)): "test_gemm_float64_gpu.py::test_gemm_float64[g9_rowbias]",
    ('gemm', ('256x256x64s2w16', ''), ('colstats', 'row bias')): "test_gemm_float64_gpu.py::test_gemm_float64[g9_stats_rowbias]",
    ('gemm', ('256x256x64s2w16', ''), ('upsample',)): "test_gemm_float64_gpu.py::test_gemm_float64[g9_ups]",
    ('gemm', ('256x256x64s2w16', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[g9_res]",
    ('gemm', ('256x256x64s2w16', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g9_stats_res]",
    ('gemm', ('256x256x64pp', ''), ('colstats', 'row bias')): "test_gemm_float64_gpu.py::test_gemm_float64[p17_stats_rowbias]",
    ('gemm', ('256x256x64pp2', ''), ('colstats', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[p21_stats_ups]",
    ('gemm', ('256x256x64pp2', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[p21_plain]",
    # the KL-VAE decoders and encoders at other sizes, and TAESD (relu after the residual; fp16 beside fp32 on the upsampled source)
    ('gemm', ('256x128x64s2', ''), ()): "test_gemm_float64_gpu.py::test_gemm_float64[g3_plain]",
    ('gemm', ('256x128x64s2', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g3_stats_res]",
    ('gemm', ('256x128x64s2', ''), ('C16 + C32', 'act_after_resid', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g3_c16_relu_post]",
    ('gemm', ('256x128x64s2', ''), ('C16 + C32', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[g3_c16_ups]",
    ('gemm', ('256x128x32s3', ''), ('upsample',)): "test_gemm_float64_gpu.py::test_gemm_float64[g4_ups]",
    ('gemm', ('256x128x32s3', ''), ('C16 + C32', 'upsample')): "test_gemm_float64_gpu.py::test_gemm_float64[g4_c16_ups]",
    ('gemm', ('256x128x32s3', ''), ('act_after_resid', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[g4_relu_post16]",
    # forms only the device census meets: where the dry runtime (no device to ask for its CUs) plans the ping-pong fall-back of a stream-K tile, the device runs
    # stream-K, and the launches around it take other tiles
    ('gemm', ('256x256x64ppsk', ''), ('row bias',)): "test_gemm_float64_gpu.py::test_gemm_float64[p19_conv_rowbias]",
    ('gemm', ('128x320x64ppsk', ''), ('residual',)): "test_gemm_float64_gpu.py::test_gemm_float64[p28_conv]",
    ('gemm', ('128x320x64pp', ''), ('colstats', 'row bias')): "test_gemm_float64_gpu.py::test_gemm_float64[p18_stats_rowbias]",
    ('gemm', ('256x256x64pp', ''), ('colstats', 'residual')): "test_gemm_float64_gpu.py::test_gemm_float64[p17_stats_res]",
    ('gemm', ('256x256x64pp', ''), ('colstats',)): "test_gemm_float64_gpu.py::test_gemm_float64[p17_conv_stats]",
    # the SDXL cross attention over two context windows (154 keys: two full key tiles and a ragged one, as the case's 333 are five and one)
    ('attn', 'attn<64x2>', ()): "test_attention_float64_gpu.py::test_attention_float64[cond_x2_lds_dma_64row]",
}


def test_covered_elsewhere_names_cases_of_exactly_that_form():
    import attn64_cases as AC
    import gemm64_cases as GC
    for (kind, path, feats), where in COVERED_ELSEWHERE.items():
        cid = where[where.index("[") + 1:-1] if where.endswith("]") else None
        if kind == "gemm" and where.startswith("test_gemm_float64_gpu.py"):
            c = GC.BY_ID[cid]
            assert not c["exp"] and PA.gemm_path(c["variant"])[:2] == path and _case_features(c) == set(feats) - {"once"}, (kind, path, feats, cid)
        elif kind == "gemm" and where.startswith("test_upsample_phases_gpu.py::test_phase_launches_and_assembled_output_float64["):
            # a phase form: the case's own launch arguments (all four) must have exactly this key -- the tile the launcher routes them to, out_phase set, wrap or not
            import test_upsample_phases_gpu as UP
            from mlimgsynth_amd import kernels
            tile, bias_on, wrap, H = map(int, re.fullmatch(r"t(\d+)_b(\d)_w(\d)_h(\d+)", cid).groups())
            assert (tile, bias_on, wrap, H) in UP.CASES and "phase" in feats, cid
            for ph in range(4):
                a = UP.phase_launch_args(kernels, 0x10000, (UP.N_IMG, H, UP.W_SRC, UP.CIN), 0x20000, 0x30000 if bias_on else None, UP.TILES[tile][1], tile, wrap, 0x40000, ph)
                assert a.out_phase == 1 + ph and PA.census_key(PA.Op(0, "gemm", "", 0, 0, (-1, -1), a)) == (kind, path, tuple(sorted(set(feats) - {"once"}))), (cid, ph)
        elif kind in ("attn", "attn_ctx") and where.startswith("test_attention_float64_gpu.py"):
            assert any(c["id"] == cid and c["variant"] == path for c in AC.CASES), (path, cid)
        else:
            assert where.startswith("test_conditioning_gpu.py::test_attention_fused_into_the_q_projection") and (kind == "xavt" or "xattn ending" in feats), (kind, path, feats)


def test_every_op_form_of_the_bench_plans_is_audited_or_covered(E):
    """SD1.5 64x64 N = 2, SDXL 128x128 N = 8 and their KL-VAE decoders, built on the device as bench.py builds them (not computed): the key of every
    op -- kind, GEMM tile and split form or attention kernel, and the epilogue / wiring features it uses -- must occur in an audited plan above or
    in COVERED_ELSEWHERE."""
    def keys(spec, xattn=None):
        with _built(E, spec, xattn, PA.MLB_F_OPSHAPES, False) as b:
            return {PA.census_key(o) for o in PA.Plan(b.ctx).ops}
    audited = set()
    for spec, xattn, _ in AUDITED:
        audited |= keys(spec, xattn)
    need = {}
    for spec in PA.BENCH_PLANS:
        for k in keys(spec):
            need.setdefault(k, []).append(PA.plan_id(spec))
    others = sorted((k for k in need if k not in audited), key=str)
    print(f"\n[plan audit] census: {len(need)} op forms in the bench plans, {len(need) - len(others)} met in audited plans, the others:")
    for k in others:
        print(f"  {k} ({', '.join(need[k])}): {COVERED_ELSEWHERE.get(k)}")
    missing = [k for k in others if k not in COVERED_ELSEWHERE]
    assert not missing, f"op forms of the bench plans that no audited plan contains and COVERED_ELSEWHERE does not list: {missing}"
    # the forms of the option plans are met, and the census sees the phase form the bench plans run (it has a key of its own, not a plain convolution's)
    for want in (("cadd", "", ()), ("freeu_backbone", "", ()), ("freeu_skip", "", ()), ("copy", "tile", ()), ("copy", "untile", ())):
        assert want in audited, want
    phase = sorted((k for k in need if k[0] == "gemm" and "phase" in k[2]), key=str)
    print(f"[plan audit] census: phase forms of the bench plans: {[(k, need[k]) for k in phase]}")
    assert phase and any("unet-sdxl" in p for k in phase for p in need[k]) and any(k[0] == "gemm" and "phase" in k[2] for k in audited)
    assert all(k in audited or COVERED_ELSEWHERE[k].startswith("test_upsample_phases_gpu.py") for k in phase)


# ------------------------------------------------------------------ census beyond the bench sizes
def _device_keys(E, spec, xattn=None):
    with _built(E, spec, xattn, PA.MLB_F_OPSHAPES, False) as b:
        return {PA.census_key(o) for o in PA.Plan(b.ctx, external=b.external).ops}


@pytest.fixture(scope="module")
def audited_keys(E):
    """(census keys met in the AUDITED plans, built on the device under their xattn mode; census keys of the bench plans, whose forms the census above holds)"""
    met, bench = set(), set()
    for spec, xattn, _ in AUDITED:
        met |= _device_keys(E, spec, xattn)
    for spec in PA.BENCH_PLANS:
        bench |= _device_keys(E, spec)
    return met, bench


@pytest.mark.parametrize("spec", PA.SIZE_PLANS, ids=[PA.plan_id(s) for s in PA.SIZE_PLANS])
def test_every_op_form_at_sizes_other_than_the_bench_is_held(E, audited_keys, spec):
    """PA.SIZE_PLANS: SD1.5 at 64x64 with N = 1, 3, 4, 6, 8, at 64x96, 96x64, 96x96, 72x88, 88x72, 40x40; SDXL at 128x128 with N = 1, 2, 3, 4, 6, at 104x152 (N = 2, 8),
    152x104, 112x144, 168x96, 96x96, 64x64, 120x136, 100x100 and at the bench size with a 154-token context; the KL-VAE decoders and encoders and TAESD at other sizes.
    Built on the device (the device answers for its CUs), not computed: every op form must be met in an audited plan or a bench plan, or be listed in
    COVERED_ELSEWHERE with the float64 case of exactly that form.  A plan that cannot be built fails."""
    met, bench = audited_keys
    pid = PA.plan_id(spec)
    keys = _device_keys(E, spec)
    assert keys
    others = sorted((k for k in keys if k not in met), key=str)
    print(f"\n[size census] {pid}: {len(keys)} op forms, {len(keys) - len(others)} met in audited plans, the others:")
    for k in others:
        print(f"  {k}: {COVERED_ELSEWHERE.get(k) or ('a bench plan' if k in bench else None)}")
    missing = PA.unheld_forms({pid: keys}, met | bench | set(COVERED_ELSEWHERE))
    assert not missing, "op forms that no audited plan, no bench plan and no COVERED_ELSEWHERE entry holds: " + "; ".join(f"{k} in {', '.join(p)}" for k, p in missing.items())
