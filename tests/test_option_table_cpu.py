"""The public option surface (mlis_option_str / _fromz / _set / _set_str / _get of csrc/host/mlis_api.c) derives from one table.
Coverage: every MLIS_Option enumerator of include/mlis_abi.h has a name that maps back to it, no other id has one, and the map
below names every enumerator's argument kind.  Characterisation: what every option answers to a fixed list of values
(option_probe.py) equals tests/golden/option_matrix.json, recorded from the library as it was before the table existed."""
import json
import os

import pytest

import mlis_ffi as F
import option_probe as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# option name -> what mlis_option_set takes after the id.  int, double, uint64 and str are probed in both forms; the others
# (two arguments, pointers, nothing) in string form only.  A new option has to be entered here before the suite passes.
ARG_KIND = {
    "none": "void", "backend": "str2", "model": "str", "tae": "str", "lora_dir": "str", "lora": "str_double", "lora_clear": "void",
    "prompt": "str", "nprompt": "str", "image_dim": "int2", "batch_size": "int", "clip_skip": "int", "cfg_scale": "double",
    "method": "int", "scheduler": "int", "steps": "int", "f_t_ini": "double", "f_t_end": "double", "s_noise": "double",
    "s_ancestral": "double", "image": "ptr", "image_mask": "ptr", "no_decode": "int", "tensor_use_flags": "int", "seed": "uint64",
    "vae_tile": "int", "unet_split": "int", "threads": "int", "dump_flags": "int", "aux_dir": "str", "callback": "ptr",
    "error_handler": "ptr", "log_level": "int", "model_type": "int", "weight_type": "int", "no_prompt_parse": "int",
    "tiling": "int", "hires_scale": "double", "hires_denoise": "double", "hires_steps": "int", "hires_upscaler": "int",
    "unet_tile": "int", "unet_tile_overlap": "int", "unet_tile_batch": "int",
    "control_model": "str", "control_image": "ptr", "control_strength": "double", "control_start": "double", "control_end": "double",
    "freeu": "int", "freeu_b1": "double", "freeu_b2": "double", "freeu_s1": "double", "freeu_s2": "double",
    "upscale_model": "str", "hires_use_model": "int", "downscale_filter": "int",
    "control_preprocess": "int", "canny_low": "double", "canny_high": "double", "canny_l2": "int",
    "inpaint_area": "int", "inpaint_padding": "int", "mask_blur": "double", "mask_grow": "int", "mask_invert": "int", "inpaint_composite": "int",
    "hypertile": "int", "hypertile_depth": "int", "pag_scale": "double", "cfg_rescale": "double", "prediction": "int", "zsnr": "int",
}


@pytest.fixture(scope="module")
def lib_path():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return _lib.LIB_PATH


def test_every_enumerator_has_a_name_and_a_kind(lib_path):
    lib = F.bind(lib_path)
    opts = P.header_options()
    assert len(opts) >= 73 and opts["none"] == 0 and opts["no_prompt_parse"] == 35 and opts["tiling"] == 101
    assert set(ARG_KIND) == set(opts)                       # a new enumerator is probed, a removed one leaves the map
    for name, oid in opts.items():
        got = lib.mlis_option_str(oid)
        assert got != b"???" and got == name.encode(), (name, oid, got)
        assert lib.mlis_option_fromz(got) == oid, (name, oid)
    for oid in set(range(256)) - set(opts.values()):
        assert lib.mlis_option_str(oid) == b"???", oid
    assert lib.mlis_option_fromz(b"nosuchoption") == -1 and lib.mlis_option_fromz(b"???") == -1


def test_option_matrix_equals_the_recorded_one(lib_path):
    with open(os.path.join(ROOT, "tests", "golden", "option_matrix.json")) as f:
        want = json.load(f)
    got = json.loads(json.dumps(P.probe(lib_path, ARG_KIND), allow_nan=False))
    assert set(got) == set(want)
    for part in ("get_rc", "set_unknown"):
        assert got[part] == want[part], part
    for part in ("set_str", "set"):
        assert set(got[part]) == set(want[part]), part
        for name in want[part]:         # outcome: rc, errstr, handler calls, get rc, get value (option_probe.py on "{}", None and "=")
            g, w = got[part][name], want[part][name]
            assert g["first"] == w["first"] and g["else"] == w["else"], (part, name)
            for v in sorted(set(g["values"]) | set(w["values"])):
                assert g["values"].get(v, g["else"]) == w["values"].get(v, w["else"]), (part, name, v)
