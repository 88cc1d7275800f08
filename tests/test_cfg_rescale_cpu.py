"""v-prediction / zero-terminal-SNR / guidance rescale, the parts that need no device: the second sigma table against a float64 restatement of its rule, sigma <-> t
and the schedule on it, the plain table's schedule against the sigmas recorded from the commit before this feature, the three options, the `auto` resolution against
synthetic checkpoints, and the structure sizes."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import mlis_ffi as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_RESCALE, PREDICTION, ZSNR = 211, 212, 213
ABAR_LAST = 4.8973451890853435e-08


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return F.bind(_lib.LIB_PATH)


def tables64():
    """float64 log sigmas of the scaled-linear table and of its zero-terminal-SNR rescale (Algorithm 1 of the paper, last entry clamped)"""
    n = 1000
    b, e = np.sqrt(0.00085), np.sqrt(0.0120)
    beta = b + (e - b) / (n - 1) * np.arange(n, dtype=np.float64)
    abar = np.cumprod(1.0 - beta * beta)
    s = np.sqrt(abar)
    sz = (s - s[-1]) * s[0] / (s[0] - s[-1])
    az = sz * sz
    az[-1] = ABAR_LAST
    return np.log(np.sqrt((1 - abar) / abar)), np.log(np.sqrt((1 - az) / az))


# ------------------------------------------------------------------ the table
def test_ztsnr_table_against_float64(lib):
    from mlimgsynth_amd import engine as E
    plain64, z64 = tables64()
    plain, z = E.log_sigmas(False), E.log_sigmas(True)
    assert plain.dtype == np.float32 and z.shape == (1000,)
    # 1 float ulp of the stored log (np.spacing of the float32 nearest the float64 value)
    ulp = np.spacing(np.abs(z64).astype(np.float32)).astype(np.float64)
    err = np.abs(z.astype(np.float64) - z64)
    print("ztsnr table: max error in ulps of the stored log", float((err / ulp).max()))
    assert (err <= ulp).all()
    assert (np.abs(plain.astype(np.float64) - plain64) <= np.spacing(np.abs(plain64).astype(np.float32))).all()
    assert z[0] == plain[0]                                                  # first entry: the plain table's
    assert z[999] == np.float32(np.log(np.sqrt((1 - ABAR_LAST) / ABAR_LAST)))   # last entry: the clamp constant's sigma
    assert (np.diff(z.astype(np.float64)) > 0).all()                         # strictly increasing
    sig = np.exp(z.astype(np.float64))
    assert abs(sig[0] - 0.029167158) < 1e-8 and abs(sig[997] - 1124.55) < 0.01 and abs(sig[998] - 2254.24) < 0.01 and abs(sig[999] - 4518.76) < 0.01
    P = E.unet_params("sdxl", zsnr=True)
    assert P.zsnr == 1 and P.sigma_max == np.float32(np.exp(np.float32(z[999]).astype(np.float64))) and P.sigma_min == np.float32(0.029167158)
    P0 = E.unet_params("sdxl")
    assert P0.zsnr == 0 and P0.sigma_max == np.float32(14.614641)


def test_sigma_t_round_trip_on_both_tables(lib):
    """unet_sigma_to_t(unet_t_to_sigma(t)) at integer and half-integer t.  The estimator reads the slope of the FOLLOWING interval (the reference's quirk), so at
    t in [i, i + 1] it is off by at most |1 - m_i / m_(i+1)|, m the table's log slopes, on top of the 0.02 the plain table meets in test_oracle_host.  Both tables
    are curved at small t (the term is 0.08 at t = 10 and below 0.01 from t = 100); the rescaled table's log sigma goes like -log(999 - t) at its end, where the term
    grows again, to 1/3 at t = 996.  The slopes come from the float64 restatement, not from the library."""
    from mlimgsynth_amd import engine as E
    l = E.L()
    for zsnr, t64 in zip((False, True), tables64()):
        P = E.unet_params("sd1", zsnr)
        m = np.diff(t64)
        worst = 0.0
        for t in list(np.arange(10, 997.6, 0.5)):
            i = int(t)
            bound = 0.02 + abs(1 - m[i] / m[i + 1])
            got = l.unet_sigma_to_t(C.byref(P), l.unet_t_to_sigma(C.byref(P), float(t)))
            worst = max(worst, abs(got - t) - abs(1 - m[i] / m[i + 1]))
            assert abs(got - t) <= bound, (zsnr, t, got, bound)
        print("round trip, zsnr", zsnr, ": worst error beyond the slope term", worst)
        assert l.unet_sigma_to_t(C.byref(P), l.unet_t_to_sigma(C.byref(P), 999.0)) == 999.0
    Pz = E.unet_params("sd1", True)
    assert abs(l.unet_t_to_sigma(C.byref(Pz), 999.0) - 4518.76) < 0.01 and l.unet_t_to_sigma(C.byref(Pz), 0.0) == l.unet_t_to_sigma(C.byref(E.unet_params("sd1")), 0.0)


def test_schedule_with_zsnr(lib):
    from mlimgsynth_amd import engine as E
    z = E.log_sigmas(True)
    s = E.schedule("sdxl", 20, 1, zsnr=True)
    assert s.shape == (21,) and s[0] == np.float32(np.exp(np.float32(z[999]))) and s[-1] == 0
    assert (np.diff(s.astype(np.float64)) < 0).all()
    assert (np.abs(s[:4].astype(np.float64) - [4518.76, 38.195, 17.055, 10.207]) <= [0.005, 0.0005, 0.0005, 0.0005]).all()      # (half a unit of the quoted digits)
    k = E.schedule("sdxl", 20, 2, zsnr=True)                              # Karras between the table's ends: allowed, the user's choice
    assert abs(k[0] - s[0]) / s[0] < 1e-5 and k[-1] == 0 and (np.diff(k.astype(np.float64)) < 0).all()


def test_plain_schedule_is_the_recorded_one(lib):
    """with the flag off, bit for bit the sigmas of the commit before the second table existed (tests/golden/schedule_sd1_parent.json)"""
    from mlimgsynth_amd import engine as E
    with open(os.path.join(ROOT, "tests", "golden", "schedule_sd1_parent.json")) as f:
        gold = json.load(f)
    for name, sched in (("uniform", 1), ("karras", 2)):
        s = E.schedule("sd1", gold["n_step"], sched, gold["f_t_ini"], gold["f_t_end"])
        assert [int(v) for v in s.view(np.uint32)] == gold[name]["bits"], name
        assert s.tolist() == [np.float32(v) for v in gold[name]["sigmas"]]


# ------------------------------------------------------------------ options
def test_options_defaults_ranges_names_and_forms(lib):
    for oid, name in ((CFG_RESCALE, "cfg_rescale"), (PREDICTION, "prediction"), (ZSNR, "zsnr")):
        assert lib.mlis_option_str(oid).decode() == name and lib.mlis_option_fromz(name.encode()) == oid == lib.mlis_option_fromz(name.replace("_", "-").encode())
    assert lib.mlis_option_str(210) == b"???" and lib.mlis_option_str(214) == b"???"
    m = F.Mlis(lib)
    try:
        f, i = C.c_float(-1), C.c_int(-1)
        getf = lambda: (lib.mlis_option_get(m.ctx, CFG_RESCALE, C.byref(f)), f.value)
        geti = lambda oid: (lib.mlis_option_get(m.ctx, oid, C.byref(i)), i.value)
        assert getf() == (1, 0.0) and geti(PREDICTION) == (1, 0) and geti(ZSNR) == (1, 0)        # defaults: off, auto, auto
        for v in (0.7, 1, 0.25, 0):
            m.set("cfg_rescale", v)
            assert getf() == (1, float(np.float32(v)))
        lib.mlis_option_set.argtypes = None
        assert lib.mlis_option_set(m.ctx, CFG_RESCALE, C.c_double(0.5)) == 1 and getf() == (1, 0.5)
        for bad in (-0.1, 1.01, 7):
            assert lib.mlis_option_set(m.ctx, CFG_RESCALE, C.c_double(bad)) == -4, bad
            assert lib.mlis_option_set_str(m.ctx, b"cfg_rescale", str(bad).encode()) == -4, bad
        assert lib.mlis_option_set_str(m.ctx, b"cfg_rescale", b"0.7x") == -4 and getf() == (1, 0.5)    # a refused value changes nothing
        for k, s in enumerate(("auto", "eps", "v")):
            m.set("prediction", s)
            assert geti(PREDICTION) == (1, k)
            m.set("prediction", (k + 1) % 3)
            assert geti(PREDICTION) == (1, (k + 1) % 3)
            assert lib.mlis_option_set(m.ctx, PREDICTION, C.c_int(k)) == 1 and geti(PREDICTION) == (1, k)
        for s, k in (("auto", 0), ("off", 1), ("on", 2), ("n", 1), ("y", 2), ("0", 0), ("2", 2)):
            m.set("zsnr", s)
            assert geti(ZSNR) == (1, k), s
        assert lib.mlis_option_set(m.ctx, ZSNR, C.c_int(1)) == 1 and geti(ZSNR) == (1, 1)
        for oid, name in ((PREDICTION, b"prediction"), (ZSNR, b"zsnr")):
            before = geti(oid)
            for bad in (b"3", b"-1", b"vv", b"maybe"):
                assert lib.mlis_option_set_str(m.ctx, name, bad) == -4, (name, bad)
            assert lib.mlis_option_set(m.ctx, oid, C.c_int(3)) == -4 and lib.mlis_option_set(m.ctx, oid, C.c_int(-1)) == -4
            assert geti(oid) == before
    finally:
        m.close()


def test_symbols_wrappers_and_cli(lib):
    for name in ("mlsd_guidance_stats", "mlsd_guidance_blocks", "mlsd_guidance_scratch_bytes", "mlsd_dxdt_rescaled", "mlsd_euler_rescaled_update",
                 "mlis_amd_set_prediction", "mlis_amd_set_cfg_rescale", "mlis_amd_guidance_info", "mlis_amd_prediction_resolve", "mlts_markers", "unet_log_sigmas",
                 "unet_params_set_zsnr", "unet_params_sizeof"):
        assert hasattr(lib, name), name
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert (M.MLIS_OPT_AMD_CFG_RESCALE, M.MLIS_OPT_AMD_PREDICTION, M.MLIS_OPT_AMD_ZSNR) == (211, 212, 213)
    assert callable(K.guidance_stats) and callable(K.dxdt_rescaled) and callable(K.euler_rescaled_update)
    assert callable(E.Generator.set_prediction) and callable(E.Generator.set_cfg_rescale) and callable(E.Generator.guidance_info)
    assert [K.guidance_blocks(hw) for hw in (1, 63, 1024, 1025, 1030, 4096, 16384, 66001, 1 << 20)] == [1, 1, 1, 2, 2, 4, 16, 64, 64]
    assert K.guidance_scratch_bytes(3, 1030) == 3 * 2 * 32 and K.guidance_scratch_bytes(0, 64) == 0
    mm = M.MLImgSynth()
    mm.guidance_set(cfg_rescale=0.7, prediction="v", zsnr=True)
    f, i, j = C.c_float(), C.c_int(), C.c_int()
    mm.option_get(M.MLIS_OPT_AMD_CFG_RESCALE, f), mm.option_get(M.MLIS_OPT_AMD_PREDICTION, i), mm.option_get(M.MLIS_OPT_AMD_ZSNR, j)
    assert (f.value, i.value, j.value) == (np.float32(0.7), 2, 2) and mm.guidance_info() is None        # no engine yet
    mm.guidance_set(zsnr="auto")
    mm.option_get(M.MLIS_OPT_AMD_ZSNR, j), mm.option_get(M.MLIS_OPT_AMD_PREDICTION, i)
    assert (i.value, j.value) == (2, 0)                                    # arguments left out keep their value
    with pytest.raises(RuntimeError):
        mm.guidance_set(cfg_rescale=1.5)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--cfg-rescale F" in out and "--prediction auto|eps|v" in out and "--zsnr auto|y|n" in out
    r = subprocess.run([exe, "generate", "--cfg-rescale", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "cfg-rescale" in r.stderr
    r = subprocess.run([exe, "generate", "--prediction", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "prediction" in r.stderr


# ------------------------------------------------------------------ `auto` against synthetic checkpoints
PROBE = "model.diffusion_model.input_blocks.4.1.transformer_blocks.0.attn2.to_k.weight"      # what identifies an SDXL file


def markers_of(lib, path):
    lib.mlts_open_safetensors.restype = C.c_void_p
    lib.mlts_open_safetensors.argtypes = [C.c_char_p, C.c_int]
    lib.mlts_markers.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mlts_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.mlts_find.restype = C.c_void_p
    lib.mlts_find.argtypes = [C.c_void_p, C.c_char_p]
    lib.mlts_count.argtypes = [C.c_void_p]
    lib.mlts_close.argtypes = [C.c_void_p]
    lib.mlts_model_identify.restype = C.c_char_p
    lib.mlts_model_identify.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    S = lib.mlts_open_safetensors(path.encode(), 1)
    assert S
    v, z, un, sp = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.mlts_markers(S, C.byref(v), C.byref(z)) == 1 and lib.mlts_stats(S, C.byref(un), C.byref(sp)) == 1
    assert lib.mlts_model_identify(S, None) == b"sdxl"
    assert not lib.mlts_find(S, b"v_pred") and not lib.mlts_find(S, b"ztsnr") and not lib.mlts_find(S, b"unet.v_pred")      # markers are never parameters
    n = lib.mlts_count(S)
    lib.mlts_close(S)
    return v.value, z.value, un.value, n


def test_auto_resolution_from_checkpoint_markers(lib, tmp_path):
    from safetensors.numpy import save_file
    from mlimgsynth_amd import engine as E
    probe = {PROBE: np.zeros((640, 2048), np.float16)}
    cases = [("plain", {}, (0, 0)),
             ("v", {"v_pred": np.zeros((), np.float32)}, (1, 0)),
             ("vz", {"v_pred": np.zeros((), np.float32), "ztsnr": np.zeros((), np.float32)}, (1, 1)),
             ("vz_prefixed", {"model.diffusion_model.v_pred": np.zeros((1,), np.float16), "model.diffusion_model.ztsnr": np.zeros((2, 3), np.float32)}, (1, 1))]
    for name, extra, want in cases:
        p = str(tmp_path / f"{name}.safetensors")
        save_file(dict(probe, **extra), p)
        v, z, unused, n = markers_of(lib, p)
        assert (v, z) == want, name
        assert unused == 0 and n == 1, name                               # the markers do not count as unknown tensors and are not entries
        assert E.prediction_resolve("sdxl", v, z) == want                 # auto: what the checkpoint says
        for pred, wv in ((1, 0), (2, 1)):                                 # explicit options always win
            for zo, wz in ((1, 0), (2, 1)):
                assert E.prediction_resolve("sdxl", v, z, pred, zo) == (wv, wz), (name, pred, zo)
        assert E.prediction_resolve("sdxl", v, z, 1, 0) == (0, want[1]) and E.prediction_resolve("sdxl", v, z, 0, 1) == (want[0], 0)
    # the model type under auto: sd2 and tinyv are v-prediction, everything else eps; no table but the plain one without a marker
    for model, v in (("sd1", 0), ("sd2", 1), ("sdxl", 0), ("tiny", 0), ("tinyv", 1), ("tinyxl", 0)):
        assert E.prediction_resolve(model) == (v, 0), model
        assert E.prediction_resolve(model, prediction=1) == (0, 0) and E.prediction_resolve(model, prediction=2, zsnr=2) == (1, 1)
    with pytest.raises(RuntimeError):
        E.prediction_resolve("nope")
    with pytest.raises(RuntimeError):
        E.prediction_resolve("sdxl", prediction=3)


# ------------------------------------------------------------------ structure sizes
def test_structure_sizes(lib):
    from mlimgsynth_amd import engine as E
    import oracle_lib as O
    assert C.sizeof(E.AmdConfig) == 88 == C.sizeof(E.AmdControlConfig) and E.AmdControlConfig.control.offset == E.AmdConfig.n_ctx_tok.offset + 4      # MLIS_AmdConfig: as before
    assert C.sizeof(E.UnetParams) == E.L().unet_params_sizeof() == C.sizeof(O.UnetParams) + 4      # zsnr appended; the oracle's structure is the reference's
    assert E.UnetParams.zsnr.offset == C.sizeof(O.UnetParams)
