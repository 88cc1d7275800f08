"""Real-ESRGAN compact (SRVGG) upscaler, the parts that need no GPU: the loader under the dry runtime (device memory is host memory, no kernel runs) reads N and s from
a file and names what is wrong, the "synth-compact" grammar, the exported symbols and the ctypes mirror."""
import ctypes as C

import numpy as np
import pytest

import upscale_compact_ref as R
import upscale_ffi as U


@pytest.fixture()
def dry():
    from mlimgsynth_amd import _lib
    _lib.lib()
    lib = U.bind(_lib.LIB_PATH)
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


def load(lib, spec):
    """(N, s) of the model and "", or None and the error"""
    h = lib.mlis_amd_upscaler_create(str(spec).encode())
    if not h:
        return None, lib.mlsd_last_error().decode()
    nb, sc = C.c_int(), C.c_int()
    assert lib.mlis_amd_upscaler_info(h, C.byref(nb), C.byref(sc)) == 1
    lib.mlis_amd_upscaler_destroy(h)
    return (nb.value, sc.value), ""


@pytest.mark.parametrize("prefix,convs,scale", [("", 1, 4), ("params_ema.", 3, 2), ("params.", 2, 1), ("", 2, 3)])
def test_loader_reads_convolutions_and_scale(dry, tmp_path, prefix, convs, scale):
    p = tmp_path / "m.safetensors"
    R.save_safetensors(str(p), R.synth_weights(3, convs, scale), prefix=prefix)
    assert load(dry, p) == ((convs, scale), "")


def test_loader_names_what_is_wrong(dry, tmp_path):
    w = R.synth_weights(3, 2, 2)
    p = str(tmp_path / "m.safetensors")
    wrong = {
        "missing_slopes": ({k: v for k, v in w.items() if k != "body.3.weight"}, ("body.3.weight", "missing")),
        "missing_bias": ({k: v for k, v in w.items() if k != "body.4.bias"}, ("body.4.bias", "missing")),
        "num_feat_32": (dict(w, **{"body.0.weight": np.zeros((32, 3, 3, 3), np.float32)}), ("body.0.weight", "[32, 3, 3, 3]", "[64, 3, 3, 3]")),
        "body_conv_shape": (dict(w, **{"body.2.weight": np.zeros((64, 32, 3, 3), np.float32)}), ("body.2.weight", "[64, 64, 3, 3]")),
        "slopes_of_32": (dict(w, **{"body.1.weight": np.zeros(32, np.float32)}), ("body.1.weight", "32", "64")),
        "last_conv_of_5": (dict(w, **{"body.6.weight": np.zeros((5, 64, 3, 3), np.float32)}), ("body.6.weight", "5 output channels")),
        "scale_5": (dict(w, **{"body.6.weight": np.zeros((75, 64, 3, 3), np.float32)}), ("body.6.weight", "75 output channels", "1 .. 4")),
        "two_convolutions": ({k: v for k, v in w.items() if k[5] in "01"}, ("body.2.weight", "missing")),
    }
    for name, (tensors, words) in wrong.items():
        R.save_safetensors(p, tensors)
        got, err = load(dry, p)
        assert got is None and all(word in err for word in words), (name, err)
    R.save_safetensors(p, {"body.0.weight": np.zeros(64, np.float32)})          # no four-dimensional body.0.weight: not a compact net, and no RRDBNet either
    got, err = load(dry, p)
    assert got is None and "conv_first.weight" in err


def test_synthetic_spec_grammar(dry):
    for good in ("synth-compact", "synth-compact:5", "synth-compact:5:16", "synth-compact:5:1:1", "synth-compact:5:64:4", "synth:1:2"):
        got, err = load(dry, good)          # read as a synthetic model: the dry runtime then refuses the fill kernel (the GPU tests build these)
        assert got is None and "no GPU" in err and "invalid" not in err, (good, err)
    for bad in ("synth-compact:", "synth-compact:x", "synth-compact:1:0", "synth-compact:1:65", "synth-compact:1:2:0", "synth-compact:1:2:5", "synth-compact:1:2:3:4",
                "synth-compact:-1", "synth-compact:1:2:", "synth:1:2:3"):
        got, err = load(dry, bad)
        assert got is None and bad in err, (bad, err)
    got, err = load(dry, "synth-compactx")          # not the word: a path, which does not exist
    assert got is None and err


def test_symbols_and_mirror():
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    L = _lib.lib()
    for name in ("mlsd_conv3x3_compact", "mlsd_cconv_variant"):
        assert hasattr(L, name), name
    assert C.sizeof(K.CconvArgs) == 104             # mlsd_cconv_args on LP64
    assert K.CconvArgs.Cout.offset == 32 and K.CconvArgs.W_.offset == 40 and K.CconvArgs.grid.offset == 96
    assert K.cconv_variant(K.CconvArgs(Cin=64, Cout=64)) == "cconv3x3<refused>"          # no pointers
    assert callable(K.conv3x3_compact)
