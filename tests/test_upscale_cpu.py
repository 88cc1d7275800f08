"""ESRGAN upscaler, the parts that need no GPU: the yardstick of the GPU tests (two independent float64 restatements of RRDBNet agree, and each of the net's constants moves
the output by far more than the GPU test's bound), the two options (ids 151, 152), the entry points' argument checks, the safetensors loader under the dry runtime, and
the CLI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import esrgan_ref as E
import mlis_ffi as F
import tolerances
import upscale_ffi as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
E_OPT_VALUE = -4
CASES = [(2, 12, 20), (1, 1, 1), (1, 7, 70)]          # (n_img, h, w) of tests/test_upscale_gpu.py's network test


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return U.bind(_lib.LIB_PATH)


@pytest.fixture()
def m(lib):
    m = F.Mlis(lib)
    yield m
    m.close()


@pytest.fixture(scope="module")
def weights():
    return E.synth_weights(1234, 2)


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d" % c)
def test_the_two_restatements_agree(weights, case):
    n, h, w = case
    x = E.test_input(n, h, w)
    a, b = E.forward_numpy(weights, x), E.forward_torch(weights, x)
    assert a.shape == b.shape == (n, 3, 4 * h, 4 * w)
    err = E.rel_l2(a, b)
    print("numpy vs torch rel-L2", err)
    assert (err <= 1e-12).all(), err


@pytest.mark.parametrize("knob", [dict(rdb=1.0), dict(rrdb=1.0), dict(slope=0.0), dict(skip=False)], ids=["rdb_scale", "rrdb_scale", "lrelu_slope", "long_skip"])
def test_every_constant_of_the_net_shows_in_the_output(weights, knob):
    """so that the GPU network test (rel-L2 <= tolerances.EVAL on these inputs) cannot pass with one of them wrong"""
    n, h, w = CASES[0]
    x = E.test_input(n, h, w)
    moved = E.rel_l2(E.forward_torch(weights, x, **knob), E.forward_torch(weights, x))
    print(knob, "moves the output by rel-L2", moved)
    assert (moved > 10 * tolerances.EVAL).all(), (knob, moved)


def test_synthetic_activations_stay_of_order_one(weights):
    """the scaled initialisation keeps the trunk from growing or dying with depth: the output of 2 and of 6 blocks have the same magnitude"""
    x = E.test_input(1, 6, 6)
    a, b = E.forward_torch(weights, x), E.forward_torch(E.synth_weights(1234, 6), x)
    ra, rb = np.sqrt((a ** 2).mean()), np.sqrt((b ** 2).mean())
    assert np.isfinite(b).all() and 0.25 < rb / ra < 4, (ra, rb)


# ------------------------------------------------------------------ options
def get(lib, m, opt):
    if opt == U.UPSCALE_MODEL:
        v = C.c_char_p()
        assert lib.mlis_option_get(m.ctx, opt, C.byref(v)) == 1, m.err()
        return v.value.decode()
    v = C.c_int(-7)
    assert lib.mlis_option_get(m.ctx, opt, C.byref(v)) == 1, m.err()
    return v.value


def test_option_table_round_trips(lib):
    for oid, name in U.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid) == name.encode()
        assert lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.upper().replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(153) == b"???" and lib.mlis_option_str(150) == b"???"
    assert lib.mlis_option_str(145) == b"freeu_s2" and lib.mlis_option_str(105) == b"hires_upscaler"       # no existing id or name moved


def test_defaults_and_round_trips(lib, m):
    assert get(lib, m, U.UPSCALE_MODEL) == "" and get(lib, m, U.HIRES_USE_MODEL) == 0
    for val in ("synth", "synth:7:3", "/some/where/RealESRGAN_x4plus.safetensors", ""):
        m.set("upscale_model", val)
        assert get(lib, m, U.UPSCALE_MODEL) == val
        assert lib.mlis_option_set(m.ctx, U.UPSCALE_MODEL, C.c_char_p(val.encode())) == 1
        assert get(lib, m, U.UPSCALE_MODEL) == val
    for val, want in (("1", 1), ("0", 0), ("y", 1), ("n", 0), ("true", 1)):
        m.set("hires-use-model", val)
        assert get(lib, m, U.HIRES_USE_MODEL) == want
    assert lib.mlis_option_set(m.ctx, U.HIRES_USE_MODEL, 1) == 1 and get(lib, m, U.HIRES_USE_MODEL) == 1
    assert lib.mlis_option_set(m.ctx, U.HIRES_USE_MODEL, 2) == E_OPT_VALUE and get(lib, m, U.HIRES_USE_MODEL) == 1
    assert lib.mlis_option_set_str(m.ctx, b"hires_use_model", b"maybe") == E_OPT_VALUE and "hires_use_model" in m.err()
    # hires_upscaler keeps exactly its three values
    assert lib.mlis_option_set_str(m.ctx, b"hires_upscaler", b"3") == E_OPT_VALUE


def test_hires_use_model_needs_a_model(lib, m):
    m.set("model", "synth:tiny")
    m.set("hires_scale", 2)
    m.set("hires_use_model", 1)
    assert lib.mlis_generate(m.ctx) == E_OPT_VALUE
    assert "hires_use_model" in m.err() and "upscale_model" in m.err()


def test_tensor_upscale_checks_its_arguments(lib, m):
    x = np.zeros((1, 3, 4, 4), np.float32)
    out = F.Tensor()
    assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(U.as_tensor(x)), C.byref(out)) == E_OPT_VALUE
    assert "upscale_model" in m.err()
    m.set("upscale_model", "synth")
    x4 = np.zeros((1, 4, 4, 4), np.float32)
    assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(U.as_tensor(x4)), C.byref(out)) == E_OPT_VALUE            # 4 channels
    assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(F.Tensor()), C.byref(out)) == E_OPT_VALUE
    res = C.c_int(-1)
    assert lib.mlis_amd_upscaler_builds(m.ctx, C.byref(res)) == 0 and res.value == 0


def test_symbols_are_exported():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    for name in ("mlsd_conv3x3_dense", "mlsd_dconv_variant", "mlis_amd_tensor_upscale", "mlis_amd_upscaler_builds", "mlis_amd_upscaler_create",
                 "mlis_amd_upscaler_run", "mlis_amd_upscaler_info", "mlis_amd_upscaler_destroy"):
        assert hasattr(L, name), name


def test_python_mirrors():
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as W
    assert (W.MLIS_OPT_AMD_UPSCALE_MODEL, W.MLIS_OPT_AMD_HIRES_USE_MODEL) == (151, 152)
    assert callable(K.conv3x3_dense) and callable(K.dconv_variant) and callable(W.MLImgSynth.upscale)
    assert C.sizeof(K.DconvArgs) == 144                 # mlsd_dconv_args on LP64
    a = K.DconvArgs(Cin=96, N=32)
    assert K.dconv_variant(a) == "dconv3x3<refused>"    # no pointers
    with W.MLImgSynth() as s:
        s.hires_set(2, use_model=True)
        s.option_set("upscale_model", "synth:3")
        v, p = C.c_int(), C.c_char_p()
        s.option_get(W.MLIS_OPT_AMD_HIRES_USE_MODEL, v)
        s.option_get(W.MLIS_OPT_AMD_UPSCALE_MODEL, p)
        assert v.value == 1 and p.value == b"synth:3"
        s.hires_set(2, use_model=False)
        s.option_get(W.MLIS_OPT_AMD_HIRES_USE_MODEL, v)
        assert v.value == 0


# ------------------------------------------------------------------ loader (dry runtime: device memory is host memory, no kernel runs)
@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


def load(lib, path):
    h = lib.mlis_amd_upscaler_create(str(path).encode())
    if not h:
        return None, lib.mlsd_last_error().decode()
    nb = C.c_int()
    assert lib.mlis_amd_upscaler_info(h, C.byref(nb), None) == 1
    lib.mlis_amd_upscaler_destroy(h)
    return nb.value, ""


@pytest.mark.parametrize("prefix,f16", [("", True), ("params_ema.", False), ("params.", True)])
def test_loader_reads_the_new_arch_names(dry, tmp_path, prefix, f16):
    w = E.synth_weights(3, 1)
    E.save_safetensors(str(tmp_path / "m.safetensors"), w, prefix=prefix, f16=f16)
    assert load(dry, tmp_path / "m.safetensors") == (1, "")


def test_loader_maps_the_older_names(dry, tmp_path):
    w = E.synth_weights(3, 1)
    p = str(tmp_path / "old.safetensors")
    E.save_safetensors(p, w, old_names=True)
    assert load(dry, p) == (1, "")
    E.save_safetensors(p, {k: v for k, v in w.items() if k != "conv_body.bias"}, old_names=True)
    nb, err = load(dry, p)
    assert nb is None and "model.1.sub.1.bias" in err and "missing" in err


def test_loader_names_what_is_wrong(dry, tmp_path):
    w = E.synth_weights(3, 1)
    p = str(tmp_path / "m.safetensors")
    x2 = dict(w, **{"conv_first.weight": np.zeros((64, 12, 3, 3), np.float32)})
    E.save_safetensors(p, x2)
    nb, err = load(dry, p)
    assert nb is None and "conv_first.weight" in err and "pixel-unshuffle" in err and "12" in err
    E.save_safetensors(p, {k: v for k, v in w.items() if k != "body.0.rdb2.conv3.bias"})
    nb, err = load(dry, p)
    assert nb is None and "body.0.rdb2.conv3.bias" in err and "missing" in err
    E.save_safetensors(p, dict(w, **{"body.0.rdb1.conv2.weight": np.zeros((32, 64, 3, 3), np.float32)}))
    nb, err = load(dry, p)
    assert nb is None and "body.0.rdb1.conv2.weight" in err and "[32, 96, 3, 3]" in err
    E.save_safetensors(p, dict(w, **{"conv_hr.bias": np.zeros(32, np.float32)}))
    nb, err = load(dry, p)
    assert nb is None and "conv_hr.bias" in err
    E.save_safetensors(p, {"something.weight": np.zeros((4, 4), np.float32)})
    nb, err = load(dry, p)
    assert nb is None and "conv_first.weight" in err
    nb, err = load(dry, tmp_path / "absent.safetensors")
    assert nb is None and err
    for bad in ("synth:x", "synth:1:0", "synth:1:65", "synth:1:2:3"):
        nb, err = load(dry, bad)
        assert nb is None and bad in err, (bad, err)


# ------------------------------------------------------------------ CLI
def test_cli_upscale_needs_a_model():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--upscale-model PATH", "--hires-use-model y|n", "upscale"):
        assert flag in r.stdout, flag
    r = subprocess.run([CLI, "upscale", "-i", "in.png", "-o", "out.png"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--upscale-model" in r.stderr
    r = subprocess.run([CLI, "generate", "--hires-use-model", "perhaps"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "hires_use_model" in r.stderr
