"""ControlNet without a GPU: the option table, the exported symbols, the wrapper and the CLI, the step-window rule, the tensor-name converter against the
parameter keys of dry ControlNet plans, their parameter counts, the plain UNet plan untouched, and the torch restatement's self-check.

No ControlNet checkpoint exists on the machines these tests run on: names and counts are checked against the published layout (cldm.py) and the published
file sizes, the arithmetic on synthetic weights."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import controlnet_ffi as CF
import mlis_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return CF.bind(_lib.LIB_PATH)


@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ options, symbols, wrapper, CLI
def test_option_table_round_trips(lib):
    for oid, name in CF.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid).decode() == name and lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(136) == b"???" and lib.mlis_option_str(130) == b"???"


def test_options_set_get_and_refusals(lib):
    m = F.Mlis(lib)
    try:
        f, s = C.c_float(-1), C.c_char_p()
        for oid, want in ((CF.CONTROL_STRENGTH, 1.0), (CF.CONTROL_START, 0.0), (CF.CONTROL_END, 1.0)):     # defaults
            assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1 and f.value == want
        assert lib.mlis_option_get(m.ctx, CF.CONTROL_MODEL, C.byref(s)) == 1 and s.value == b""
        m.set("control_model", "some/dir/net.safetensors")
        m.set("control_strength", 0.75)
        assert lib.mlis_option_set(m.ctx, CF.CONTROL_START, C.c_double(0.25)) == 1 and lib.mlis_option_set(m.ctx, CF.CONTROL_END, C.c_double(0.5)) == 1
        assert lib.mlis_option_get(m.ctx, CF.CONTROL_MODEL, C.byref(s)) == 1 and s.value == b"some/dir/net.safetensors"
        for oid, want in ((CF.CONTROL_STRENGTH, 0.75), (CF.CONTROL_START, 0.25), (CF.CONTROL_END, 0.5)):
            assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1 and f.value == want
        for name, bad in (("control_strength", "-0.1"), ("control_strength", "2.5"), ("control_strength", "x"), ("control_start", "1.5"), ("control_end", "-1"),
                          ("control_end", "0.5x")):
            assert lib.mlis_option_set_str(m.ctx, name.encode(), bad.encode()) == -4, (name, bad)        # MLIS_E_OPT_VALUE
        assert lib.mlis_option_set_str(m.ctx, b"control_image", b"x.png") == -4                          # an image cannot travel as text
        px = (C.c_uint8 * 12)()
        img = F.Image(C.cast(px, C.POINTER(C.c_uint8)), 12, 2, 2, 3, 0)
        has = C.c_int(-1)
        assert lib.mlis_option_get(m.ctx, CF.CONTROL_IMAGE, C.byref(has)) == 1 and has.value == 0
        assert lib.mlis_option_set(m.ctx, CF.CONTROL_IMAGE, C.byref(img)) == 1
        assert lib.mlis_option_get(m.ctx, CF.CONTROL_IMAGE, C.byref(has)) == 1 and has.value == 1      # whether one is set
        img4 = F.Image(C.cast(px, C.POINTER(C.c_uint8)), 12, 3, 1, 4, 0)
        assert lib.mlis_option_set(m.ctx, CF.CONTROL_IMAGE, C.byref(img4)) < 0 and "channels" in m.err()
        assert lib.mlis_option_set(m.ctx, CF.CONTROL_IMAGE, C.c_void_p(None)) == 1
        assert lib.mlis_option_get(m.ctx, CF.CONTROL_IMAGE, C.byref(has)) == 1 and has.value == 0
        m.set("control_model", "")
        assert lib.mlis_option_get(m.ctx, CF.CONTROL_MODEL, C.byref(s)) == 1 and s.value == b""
    finally:
        m.close()


def test_generate_refuses_half_a_control_setup(dry):
    m = F.Mlis(dry)
    try:
        m.set("model", "synth:tiny")
        m.set("image_dim", 64, 64)
        m.set("prompt", "a")
        m.set("control_model", "synth")
        assert dry.mlis_generate(m.ctx) == -4 and "control_image" in m.err()
        m.set("control_model", "")
        px = (C.c_uint8 * 12)()
        img = F.Image(C.cast(px, C.POINTER(C.c_uint8)), 12, 2, 2, 3, 0)
        assert dry.mlis_option_set(m.ctx, CF.CONTROL_IMAGE, C.byref(img)) == 1
        assert dry.mlis_generate(m.ctx) == -4 and "control_model" in m.err()
        m.set("control_model", "synth")
        m.set("control_start", 0.8)
        m.set("control_end", 0.3)
        assert dry.mlis_generate(m.ctx) == -4 and "control_start" in m.err()
    finally:
        m.close()


def test_symbols_wrapper_and_cli(lib):
    for name in CF.EXPORTS + ["mlts_open_controlnet", "mlis_amd_control_tag_set"]:
        assert hasattr(lib, name), name
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert [f[0] for f in E.AmdControlConfig._fields_][-1] == "control" and C.sizeof(E.AmdControlConfig) == C.sizeof(E.AmdConfig)      # the field took tail padding
    assert E.AmdControlConfig.control.offset == E.AmdConfig.n_ctx_tok.offset + 4
    assert (M.MLIS_OPT_AMD_CONTROL_MODEL, M.MLIS_OPT_AMD_CONTROL_IMAGE, M.MLIS_OPT_AMD_CONTROL_STRENGTH, M.MLIS_OPT_AMD_CONTROL_START,
            M.MLIS_OPT_AMD_CONTROL_END) == (131, 132, 133, 134, 135)
    assert callable(M.MLImgSynth.control_set) and callable(K.ctrl_add) and callable(K.window_gather_nhwc) and callable(E.Generator.set_control_image)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--control-model", "--control-image", "--control-strength", "--control-start", "--control-end"):
        assert flag in out, flag
    r = subprocess.run([exe, "generate", "--control-strength", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "control-strength" in r.stderr


def test_zeroed_config_is_an_engine_without_control(dry):
    from mlimgsynth_amd import engine as E
    g = E.Generator("tiny", 64, 64, 1, defer_weights=True)
    try:
        assert g.cfg.control == 0 and g.ctx_at(5) is None and g.ctx_at(6) is None and g.control_info() == (0, 0)
        with pytest.raises(Exception):
            g.set_control(1.0)
        with pytest.raises(Exception):
            g.set_control_image(np.zeros((3, 64, 64), np.float32))
    finally:
        g.destroy()


# ------------------------------------------------------------------ the step window
def test_control_active_is_the_python_rule(lib):
    grid = [0.0, 0.1, 0.2, 0.25, 1 / 3, 0.5, 0.7, 0.75, 0.9, 1.0]
    n = 0
    for n_step in range(1, 51):
        for a in grid:
            for b in grid:
                fa, fb = float(np.float32(a)), float(np.float32(b))          # the values the C function receives
                for i in range(n_step):
                    assert bool(lib.mlis_amd_control_active(i, n_step, a, b)) == CF.active(i, n_step, fa, fb), (i, n_step, a, b)
                    n += 1
    assert n > 100000
    assert [i for i in range(10) if lib.mlis_amd_control_active(i, 10, 0.2, 0.7)] == [2, 3, 4, 5, 6]
    assert not any(lib.mlis_amd_control_active(i, 10, 0.0, 0.0) for i in range(10)) and all(lib.mlis_amd_control_active(i, 10, 0.0, 1.0) for i in range(10))


# ------------------------------------------------------------------ dry plans: names and counts
def dry_plans(lib, model, lat=16):
    """(keys and element counts of the dry ControlNet plan + hint plan) for `model`"""
    from mlimgsynth_amd import engine as E
    P = E.unet_params(model)
    ctl, hint, S, t = E.MLCtx(), E.MLCtx(), CF.ControlState(), C.c_void_p()
    assert lib.controlnet_init_nc(C.byref(S), ctl.h, C.addressof(P), lat, lat, 2, 77) > 0
    assert lib.controlnet_build(C.byref(S)) > 0
    assert lib.control_hint_init(hint.h, C.addressof(P), 8 * lat, 8 * lat, C.byref(t)) > 0
    assert lib.control_hint_build(hint.h, C.addressof(P), t) > 0
    out = {k: int(np.prod(ne)) for k, _, ne in ctl.param_list() + hint.param_list()}
    n_res = S.n_res
    ctl.destroy(), hint.destroy()
    return out, n_res


# (parameters, residuals): the published files are 723 MB (SD1.5) and 2.5 GB (SDXL) in fp16, i.e. about 361 M and 1251 M parameters; the plans hold
# 361 279 120 and 1 251 014 160 -- 0.08 % and 0.001 % from those figures.  No ControlNet checkpoint exists on this machine to compare tensor by tensor.
COUNTS = {"sd1": (361279120, 13), "sdxl": (1251014160, 10), "tiny": (2459344, 5), "tinyxl": (4283792, 7)}


@pytest.mark.parametrize("model", ["sd1", "sdxl"])
def test_name_converter_maps_the_original_layout_onto_the_plan(dry, model):
    params, n_res = dry_plans(dry, model)
    assert (sum(params.values()), n_res) == COUNTS[model]
    published = {"sd1": 361e6, "sdxl": 1251e6}[model]
    assert abs(sum(params.values()) - published) / published < 0.01
    names = [CF.original_name(k) for k in params]
    assert len(set(names)) == len(names)
    for prefix in ("", "control_model."):
        got = {}
        for nm in names:
            r, key = CF.tnconv(dry, prefix + nm)
            assert r == 1, nm
            got[key] = nm
        assert set(got) == set(params), sorted(set(got) ^ set(params))[:5]
    for nm in ("output_blocks.0.0.in_layers.0.weight", "out.0.weight", "out.2.bias", "control_model.output_blocks.3.1.norm.weight",
               "down_blocks.0.resnets.0.conv1.weight", "controlnet_cond_embedding.conv_in.weight", "controlnet_down_blocks.0.weight", "mid_block.attentions.0.norm.weight",
               "zero_convs.3.1.weight", "model.diffusion_model.input_blocks.0.0.weight"):
        assert CF.tnconv(dry, nm)[0] == 0, nm
    assert CF.tnconv(dry, "input_hint_block.14.bias") == (1, "control.hint.14.bias")
    assert CF.tnconv(dry, "control_model.zero_convs.11.0.weight") == (1, "control.zero.11.weight")
    assert CF.tnconv(dry, "middle_block_out.0.bias") == (1, "control.mid_out.bias")


@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
def test_small_plans_have_the_counts_the_layout_gives(dry, model):
    params, n_res = dry_plans(dry, model, lat=8)
    assert (sum(params.values()), n_res) == COUNTS[model]
    assert all(k.startswith("control.") for k in params)
    hint = sorted(k for k in params if k.startswith("control.hint."))
    assert hint == sorted(f"control.hint.{2 * i}.{w}" for i in range(8) for w in ("weight", "bias"))
    assert ("control.label_embed.0.weight" in params) == (model == "tinyxl")


# The plain UNet plan of a dry engine, as the parent commit builds it.  Readable part: launches by kind (convolution and linear GEMMs whatever their tile, the
# other ops by label), parameters, algorithmic FLOPs.  Then an md5 of repr((op labels with tiles and flops, parameter list)): the order and every tile; when
# only the hash differs the failure prints the labels' histogram.
PLAIN = {
    "tiny": (dict(attention=14, conv=39, f32_to_f16=1, groupnorm=7, groupnorm_silu=17, layernorm=21, linear=46, nchw_to_nhwc_f16=1, silu_f16=1, timestep_embedding=1),
             286, 435159040.0, "5bae9a2fa1"),
    "tinyxl": (dict(attention=24, conv=47, f32_to_f16=2, groupnorm=6, groupnorm_silu=25, layernorm=36, linear=78, nchw_to_nhwc_f16=1, silu_f16=1, timestep_embedding=1),
               428, 718438400.0, "3bb2ccbb37"),
    "sd1": (dict(attention=32, conv=88, f32_to_f16=1, groupnorm=16, groupnorm_silu=45, layernorm=48, linear=110, nchw_to_nhwc_f16=1, silu_f16=1, timestep_embedding=1),
            686, 1606546882560.0, "2699d1a59f"),
    "sdxl": (dict(attention=140, conv=62, f32_to_f16=2, groupnorm=11, groupnorm_silu=35, layernorm=210, linear=437, nchw_to_nhwc_f16=1, silu_f16=1, timestep_embedding=1),
             1680, 13522472796160.0, "e6b13b084e"),
}


def op_kinds(ops):
    from collections import Counter
    kind = lambda lab: ("conv" if ",conv" in lab else "linear") if lab.startswith("gemm<") else lab
    return dict(Counter(kind(lab) for lab, _ in ops)), dict(sorted(Counter(lab for lab, _ in ops).items()))


@pytest.mark.parametrize("model,px", [("tiny", 64), ("tinyxl", 64), ("sd1", 512), ("sdxl", 1024)])
def test_plain_unet_plan_is_the_parents_and_control_adds_only_the_sums(dry, model, px):
    from mlimgsynth_amd import engine as E
    sig = {}
    for control in (False, True):
        g = E.Generator(model, px, px, 1, defer_weights=True, control=control)
        try:
            u = g.unet_ctx()
            ops, pl = u.op_list(), u.param_list()
            sig[control] = (ops, pl)
            if not control:
                kinds, labels = op_kinds(ops)
                want_kinds, want_params, want_flops, want_md5 = PLAIN[model]
                assert kinds == want_kinds and len(pl) == want_params and sum(f for _, f in ops) == want_flops
                assert hashlib.md5(repr((ops, pl)).encode()).hexdigest()[:10] == want_md5, f"same launches by kind, another order, tile or parameter: {labels}"
            else:
                assert g.control_info()[0] == COUNTS[model][1] and g.ctx_at(5) is not None and g.ctx_at(6) is not None
        finally:
            g.destroy()
    plain_ops, ctl_ops = sig[False][0], sig[True][0]
    assert [o for o in ctl_ops if o[0] != "ctrl_add"] == plain_ops and len(ctl_ops) - len(plain_ops) == COUNTS[model][1]
    assert sig[True][1] == sig[False][1]                                   # the UNet's parameters are the same: the ControlNet's live in its own plans


# ------------------------------------------------------------------ the reference's self-check
def test_reference_with_gain_zero_is_the_plain_unet_bit_for_bit():
    torch = pytest.importorskip("torch")
    import controlnet_ref as R
    from tools import torch_ref as TR
    for model, B in (("tiny", 2), ("tinyxl", 1)):
        P = R.UNET[model]
        rng = np.random.default_rng(1)
        x = torch.from_numpy(rng.standard_normal((B, 4, 8, 8)).astype(np.float32))
        ctx = torch.from_numpy(rng.standard_normal((B, 77, P["n_ctx"])).astype(np.float32))
        lab = torch.from_numpy(rng.standard_normal((B, P["ch_adm_in"])).astype(np.float32)) if P["ch_adm_in"] else None
        hint = torch.from_numpy(rng.random((1, 3, 64, 64)).astype(np.float32))
        t = torch.full((B,), 500.0)
        net = R.make_net()
        with torch.no_grad():
            res = R.controlnet(net, P, x, t, ctx, lab, hint)
            assert len(res) == COUNTS[model][1] and all(float(r.abs().max()) > 0 for r in res)
            plain = net.unet(P, x, t, ctx, lab)
            assert torch.equal(R.unet_controlled(net, P, x, t, ctx, lab, res, 0.0), plain)
            assert not torch.equal(R.unet_controlled(net, P, x, t, ctx, lab, res, 1.0), plain)
        assert isinstance(net, TR.Net)
