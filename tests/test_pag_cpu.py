"""Perturbed-attention guidance without a GPU: dry UNet plans with and without the flag (op records field for field, the pointers of the one added GEMM against
its siblings'), the unmodified plan audit's dataflow checks on PAG plans, the row-count function, the option, the CLI flag and the reference's own mix.

What needs a device is in tests/test_pag_gpu.py: the engine key (on / off builds one more engine, the value builds nothing) needs generations, and tiled engines
compute their blend weights with a launch while they are created.  The plan audit does not know the ControlNet's sums (its extents() refuses the kind "cadd"
by name), so the ControlNet + FreeU composition is checked here on its records -- the sums read control image n % 4 of a 6-row plan -- and on the GPU against
the reference."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mlis_ffi as F
import plan_audit as PA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAG_SCALE = 201


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return F.bind(_lib.LIB_PATH)


@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


def records(ctx):
    """(kind, label, fused, once, gn_src, {field: value} of every field that is not a pointer, the argument record itself)"""
    out = []
    for kind, label, fused, once, gn_src, a in ctx.op_records():
        out.append((kind, label, fused, once, tuple(gn_src), {n: getattr(a, n) for n, t in a._fields_ if t is not C.c_void_p}, a))
    return out


def gen(model, lat, B, **kw):
    from mlimgsynth_amd import engine as E
    return E.Generator(model, 8 * lat, 8 * lat, B, defer_weights=True, cfg_scale=2.0, **kw)


def mid_self_attentions(model):
    """(index of the first self-attention of mid.1 among the plan's self-attentions, how many it has): the walk of the UNet builder"""
    from mlimgsynth_amd import engine as E
    P = E.unet_params(model)
    mult = [m for m in P.ch_mult if m]
    before = sum(P.n_res_blk * P.transf_depth[i] for i in range(len(mult)) if (1 << i) in list(P.attn_res))
    return before, P.transf_depth[len(mult) - 1]


# ------------------------------------------------------------------ plans
@pytest.mark.parametrize("model", ["tinyxl", "sd1"])
def test_pag_plan_is_the_plain_plan_of_as_many_rows_but_for_mid1_attn1(dry, model):
    """B = 2 with the flag (6 rows) against the plain plan of B = 3 (6 rows) at a 16 x 16 latent"""
    from mlimgsynth_amd import engine as E
    g0, g1 = gen(model, 16, 3), gen(model, 16, 2, pag=True)
    try:
        plain, pag = records(g0.ctx_at(0)), records(g1.ctx_at(0))
        first, depth = mid_self_attentions(model)
        assert g1.pag_info() == (depth, 6) and g0.pag_info() == (0, 6) and depth == {"tinyxl": 2, "sd1": 1}[model]
        assert len(pag) == len(plain) + depth
        extra = [i for i, r in enumerate(pag) if r[1] == "pag_v_proj"]
        assert len(extra) == depth
        rest = [r for r in pag if r[1] != "pag_v_proj"]
        unshift = lambda t: tuple(v - sum(1 for k in extra if k < v) if v >= 0 else v for v in t)      # producer indices, counted without the added ops
        # the self-attentions of the plain plan, in order: a fused q|k|v GEMM (N = 3 K) directly in front of an attention with Tq == Tk
        selfs = [i for i, r in enumerate(plain) if r[0] == "attn" and r[5]["Tq"] == r[5]["Tk"] and plain[i - 1][0] == "gemm" and plain[i - 1][5]["N"] == 3 * plain[i - 1][5]["K"]]
        inside = {i for s in selfs[first:first + depth] for i in (s - 1, s)}
        assert len(inside) == 2 * depth
        for i, (a, b) in enumerate(zip(rest, plain)):
            a5 = (a[0], a[1], a[2], a[3], unshift(a[4]), a[5])
            if i in inside:
                continue
            if a[0] == "n2h" and a5 != b[:6]:          # the latent's gather: 2 source images behind 6 rows, not 3 (row n reads image n % n_src: the cond group again)
                assert {k for k in a[5] if a[5][k] != b[5][k]} == {"n_src"} and (a[5]["n_src"], b[5]["n_src"]) == (2, 3)
                continue
            assert a5 == b[:6], (i, a5, b[:6])
        # inside mid.1.transf.*.attn1
        T = None
        for k, s in enumerate(selfs[first:first + depth]):
            qkv0, at0 = plain[s - 1], plain[s]
            j = extra[k]
            qkv1, at1, ex = pag[j - 2], pag[j - 1], pag[j]
            assert (qkv1[0], at1[0], ex[0]) == ("gemm", "attn", "gemm")
            T = at0[5]["Tq"] * at0[5]["n_batch"] // 6
            d = at0[5]["n_head"] * at0[5]["d_head"]
            assert qkv0[5]["M"] == 6 * T and qkv1[5]["M"] == 4 * T and {n for n in qkv0[5] if qkv0[5][n] != qkv1[5][n]} == {"M"}
            assert at0[5]["n_batch"] == 6 * at1[5]["n_batch"] // 4 and {n for n in at0[5] if at0[5][n] != at1[5][n]} == {"n_batch"}
            assert (ex[5]["M"], ex[5]["N"], ex[5]["K"]) == (2 * T, d, qkv1[5]["K"]) and ex[5]["lda"] == qkv1[5]["lda"] and ex[5]["ldb"] == qkv1[5]["ldb"]
            assert ex[5]["ldc16"] == at1[5]["ldo"] == d and (ex[2], ex[3]) == (0, 0)
            # its operands: the rows of the last 2 images of the same LayerNorm output, the v_proj slice of the fused weight, the last 2 images of the buffer
            # out_proj reads; nothing else is bound
            qa, xa, ata = qkv1[6], ex[6], at1[6]
            assert xa.A == qa.A + 4 * T * qa.lda * 2
            assert xa.W_ == qa.W_ + 2 * d * qa.K * 2
            assert xa.C16 == ata.out + 4 * T * d * 2 and not xa.C32 and not xa.resid and not xa.bias and not qa.bias
            out_proj = pag[j + 1]
            assert out_proj[0] == "gemm" and out_proj[6].A == ata.out and out_proj[5]["M"] == 6 * T
        assert T == 64 if model == "tinyxl" else T == 4
        # no new parameter: checkpoint loading, LoRA patching and weight streaming see what they saw
        assert g1.ctx_at(0).param_list() == g0.ctx_at(0).param_list()
    finally:
        g0.destroy(), g1.destroy()


def test_flag_off_records_the_plain_plan(dry):
    from mlimgsynth_amd import engine as E
    for model in ("tinyxl", "sd1"):
        g0, g1 = gen(model, 16, 3), gen(model, 16, 3, pag=False)
        un = E.Unet(model, 16, 16, 6, synth=False, pag=0)
        try:
            r0 = [r[:6] for r in records(g0.ctx_at(0))]
            assert [r[:6] for r in records(g1.ctx_at(0))] == r0 and g1.cfg.control == 0
            assert g1.ctx_at(0).op_list() == g0.ctx_at(0).op_list()
            assert not [r for r in records(un.ctx) if r[1] == "pag_v_proj"]
        finally:
            g0.destroy(), g1.destroy(), un.ctx.destroy()


def test_cfg_at_most_one_has_two_groups_and_the_controlnet_is_never_perturbed(dry):
    from mlimgsynth_amd import engine as E
    g = gen("tiny", 8, 2, pag=True)
    g1 = E.Generator("tiny", 64, 64, 2, defer_weights=True, cfg_scale=1.0, pag=True)
    gc = gen("tiny", 8, 2, pag=True, control=True, freeu=True)
    gc1 = E.Generator("tiny", 64, 64, 2, defer_weights=True, cfg_scale=1.0, pag=True, control=True)
    try:
        assert g.pag_info() == (1, 6) and g1.pag_info() == (1, 4) and gc.cfg.control == 1 | 2 | 8
        for e, rows, crows in ((gc, 6, 4), (gc1, 4, 2)):
            sums = [r for r in records(e.ctx_at(0)) if r[0] == "cadd"]
            assert sums and all((r[5]["n_img"], r[5]["n_ctrl"]) == (rows, crows) for r in sums)      # image n reads control image n % crows: the last 2 read 0, 1
            ctl = records(e.ctx_at(5))
            assert not [r for r in ctl if r[1] == "pag_v_proj"]
            assert [r[5]["n_src"] for r in ctl if r[0] == "n2h"] == [2] and [r[5]["n"] for r in ctl if r[0] == "temb"] == [crows]
        assert gc.freeu_info() == (3, 1)
    finally:
        g.destroy(), g1.destroy(), gc.destroy(), gc1.destroy()


def test_engine_refuses_more_rows_than_a_plain_engine_holds(dry):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    assert E.Generator("tiny", 64, 64, 42, defer_weights=True, cfg_scale=2.0, pag=True).destroy() is None      # 126 rows
    with pytest.raises(_lib.MlsdError, match="PAG: 129 rows"):
        E.Generator("tiny", 64, 64, 43, defer_weights=True, cfg_scale=2.0, pag=True)
    assert E.Generator("tiny", 64, 64, 64, defer_weights=True, cfg_scale=1.0, pag=True).destroy() is None      # 128 rows
    g = gen("tiny", 8, 1)
    try:
        with pytest.raises(_lib.MlsdError, match="without PAG"):
            g.set_pag(1.0)
    finally:
        g.destroy()
    g = gen("tiny", 8, 1, pag=True)
    try:
        for bad in (-0.5, 20.5, float("nan")):
            with pytest.raises(_lib.MlsdError, match="PAG scale"):
                g.set_pag(bad)
        g.set_pag(0), g.set_pag(20), g.set_pag()
    finally:
        g.destroy()


AUDITED = [("unet", "tinyxl", 16, 6, dict(pag=2)), ("unet", "sd1", 16, 6, dict(pag=2)), ("unet", "tiny", 16, 6, dict(pag=2, hypertile=32)),
           ("unet", "tinyxl", 16, 4, dict(pag=2, hypertile=32)), ("unet", "tinyxl", 16, 6, dict(pag=2, stream_weights_mib=1))]


@pytest.mark.parametrize("spec", AUDITED, ids=[PA.plan_id(s) for s in AUDITED])
def test_dataflow_of_pag_plans(spec):
    """the unmodified plan audit on PAG plans, the recycling arena and the kept one: every read has a writer (the rows out_proj reads come from two launches),
    no launch writes onto its own operand but the LayerNorm ending's sound form, and recycling never changes who wrote what a launch reads.  hypertile 32 cuts
    the middle level (8 x 8 tokens at downscale 2 into 4 x 4 tiles)."""
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    try:
        b0, b1 = PA.build(engine, spec, PA.MLB_F_OPSHAPES), PA.build(engine, spec, PA.MLB_F_OPSHAPES | PA.MLB_F_KEEP)
        try:
            rec, kept = PA.Plan(b0.ctx, PA.plan_id(spec)), PA.Plan(b1.ctx, PA.plan_id(spec) + " kept")
            extra = [o for o in rec.ops if o.label == "pag_v_proj"]
            assert len(extra) == (2 if spec[1] == "tinyxl" else 1) and all(o.kind == "gemm" for o in extra)
            if "hypertile" in spec[4]:      # the perturbed GEMM sits between the pair of permuting copies of the middle block
                cp = [o.i for o in rec.ops if o.kind == "copy" and o.a.th > 0]
                assert any(a < extra[0].i < b for a, b in zip(cp[0::2], cp[1::2]))
            for plan in (rec, kept):
                bad = PA.uncovered_reads(plan)
                assert not bad, [why for _, _, why in bad[:6]]
                own = PA.own_operand_overwrites(plan)
                assert not own, [f"{o}: {w} lands on its own operand {r}" for o, w, r in own[:6]]
            assert not PA.clobbered_operands(kept)
            if [PA.op_signature(o) for o in rec.ops] == [PA.op_signature(o) for o in kept.ops]:
                bad = PA.lifetime_diffs(rec, kept)
                assert not bad, bad[:6]
            else:
                assert all({o.kind, p.kind} <= {"gemm", "ln"} for o, p in zip(rec.ops, kept.ops) if PA.op_signature(o) != PA.op_signature(p))
        finally:
            b0.close(), b1.close()
    finally:
        L.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ the host function
def test_eval_rows(lib):
    from mlimgsynth_amd import engine as E
    for B in (1, 2, 3, 16, 64):
        for cfg, groups in ((0.5, 1), (1.0, 1), (1.0000001, 2), (2.0, 2), (7.0, 2)):
            for pag in (0, 1):
                assert E.eval_rows(B, cfg, pag) == (groups + pag) * B, (B, cfg, pag)
    assert E.eval_rows(0, 7.0, 1) == -1 and E.eval_rows(-3, 7.0, 0) == -1


# ------------------------------------------------------------------ option, wrapper, CLI
def test_option_symbols_wrapper_and_cli(lib):
    assert lib.mlis_option_str(PAG_SCALE).decode() == "pag_scale" and lib.mlis_option_fromz(b"pag_scale") == PAG_SCALE == lib.mlis_option_fromz(b"pag-scale")
    assert lib.mlis_option_str(200) == b"???" and lib.mlis_option_str(202) == b"???"
    m = F.Mlis(lib)
    try:
        f = C.c_float(-1)
        get = lambda: (lib.mlis_option_get(m.ctx, PAG_SCALE, C.byref(f)), f.value)
        assert get() == (1, 0.0)                                 # default: off
        for v in (3, 0.5, 20, 0):
            m.set("pag_scale", v)
            assert get() == (1, float(v))
        lib.mlis_option_set.argtypes = None
        assert lib.mlis_option_set(m.ctx, PAG_SCALE, C.c_double(1.5)) == 1 and get() == (1, 1.5)
        for bad in (-0.1, 20.5):
            assert lib.mlis_option_set(m.ctx, PAG_SCALE, C.c_double(bad)) == -4, bad
            assert lib.mlis_option_set_str(m.ctx, b"pag_scale", str(bad).encode()) == -4, bad
        assert lib.mlis_option_set_str(m.ctx, b"pag_scale", b"3x") == -4 and get() == (1, 1.5)      # a refused value changes nothing
    finally:
        m.close()
    for name in ("mlsd_dxdt_pag", "mlsd_euler_pag_update", "mlis_amd_eval_rows", "mlis_amd_set_pag", "mlis_amd_pag_info", "mlctx_set_pag", "mlctx_pag_info"):
        assert hasattr(lib, name), name
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert M.MLIS_OPT_AMD_PAG_SCALE == 201 and E.CONTROL_PAG == 8
    assert callable(M.MLImgSynth.pag_set) and callable(M.MLImgSynth.pag_info) and callable(K.dxdt_pag) and callable(K.euler_pag_update)
    assert callable(E.Generator.set_pag) and callable(E.Generator.pag_info)
    mm = M.MLImgSynth()
    mm.pag_set()
    v = C.c_float()
    mm.option_get(M.MLIS_OPT_AMD_PAG_SCALE, v)
    assert v.value == 3.0 and mm.pag_info() is None              # front ends' default when switched on; no engine yet
    with pytest.raises(RuntimeError):
        mm.pag_set(scale=21)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--pag-scale F" in out
    r = subprocess.run([exe, "generate", "--pag-scale", "21"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "pag-scale" in r.stderr


# ------------------------------------------------------------------ the reference's own mix
def test_reference_mix():
    import controlnet_ref as CR
    import pag_ref as R
    rng = np.random.default_rng(5)
    eps = (rng.standard_normal((6, 4, 5, 7)) * 3).astype(np.float32)
    for cfg in (1.5, 2.0, 7.0):
        assert R.mix(eps, cfg, 0).tobytes() == CR.mix(eps[:4], cfg).tobytes()              # s = 0: the plain mix, bit for bit; the third group is not looked at
        nan = eps.copy()
        nan[4:] = np.nan
        assert R.mix(nan, cfg, 0).tobytes() == CR.mix(eps[:4], cfg).tobytes()
    assert R.mix(eps[:4], 1.0, 0).tobytes() == eps[:2].tobytes() and R.mix(eps[:4], 0.5, 0).tobytes() == eps[:2].tobytes()
    # the three rounded operations, against float64 rounded once per operation
    c, u, p = (eps[2 * i:2 * i + 2].astype(np.float64) for i in range(3))
    f, s = np.float32(7.0), np.float32(3.0)
    g = ((c * f).astype(np.float32).astype(np.float64) + (u * np.float64(np.float32(1) - f)).astype(np.float32)).astype(np.float32)
    want = (g.astype(np.float64) + (np.float64(s) * (c - p).astype(np.float32)).astype(np.float32)).astype(np.float32)
    assert R.mix(eps, 7.0, 3.0).tobytes() == want.tobytes()
    # unmix inverts mix up to the roundings of the mix
    d = [R.mix(eps, a, b) for a, b in ((2, 1), (3, 1), (2, 2))]
    assert np.abs(R.unmix(d, 2.0) - eps).max() < 2e-5 * np.abs(eps).max() * 13
    d = [R.mix(eps[:4], 1.0, b) for b in (1, 2)]
    assert np.abs(R.unmix(d, 1.0) - eps[:4]).max() < 2e-5 * np.abs(eps).max() * 13


def test_reference_perturbation_is_where_the_rule_says():
    """the subclass perturbs attn1 of unet.mid.1 only, while the switch is on; elsewhere and with the switch off it is tools/torch_ref.Net"""
    import torch
    import pag_ref as R
    net = R.make_net()
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 16, 64)).astype(np.float32))
    args = (64, 64, 2)
    plain = net.mha(x, x, "unet.mid.1.transf.0.attn1", *args)
    net.perturb = True
    same = [net.mha(x, x, n, *args) for n in ("unet.in.1.1.transf.0.attn1", "control.mid.1.transf.0.attn1", "unet.out.2.1.transf.0.attn1")]
    other = [type(net).__mro__[2].mha(net, x, x, n, *args) for n in ("unet.in.1.1.transf.0.attn1", "control.mid.1.transf.0.attn1", "unet.out.2.1.transf.0.attn1")]
    assert all(torch.equal(a, b) for a, b in zip(same, other))
    cross = net.mha(x, x.clone(), "unet.mid.1.transf.0.attn1", *args)          # q and k/v are different tensors: a cross-attention is never perturbed
    assert torch.equal(cross, plain)
    got = net.mha(x, x, "unet.mid.1.transf.0.attn1", *args)
    want = net.linear(net.linear(x, "unet.mid.1.transf.0.attn1.v_proj", 64, False), "unet.mid.1.transf.0.attn1.out_proj", 64, True)
    assert torch.equal(got, want) and not torch.equal(got, plain) and net.pag_hits == 1
    net.perturb = False
    assert torch.equal(net.mha(x, x, "unet.mid.1.transf.0.attn1", *args), plain)
