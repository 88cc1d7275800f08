"""FreeU without a GPU: the closed form of the Fourier filter against numpy.fft, dry UNet plans with and without the flag, the configuration word, the option
table, the wrapper and the CLI, and what the two kernels refuse before any launch."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import freeu_ffi as FF
import mlis_ffi as F
import tolerances as TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return FF.bind(_lib.LIB_PATH)


@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("H,W", [(2, 2), (2, 3), (3, 5), (4, 4), (8, 8), (7, 12), (16, 8)])
def test_closed_form_is_the_published_fourier_filter(H, W):
    """Both sides are float64; an FFT pair of H W points carries a few log2(H W) roundings of 2^-53 relative to the plane's largest value, the closed form's sum
    of H W terms at most H W of them: 1e-13 x max|x| is orders above either and orders below any wrong term."""
    import freeu_ref as R
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((2, 3, H, W)) + 1.5
    for s in (0.2, 0.9, 1.0, 1.4):
        a, b = R.fourier_filter64(x, s), R.fourier_closed64(x, s)
        err = np.abs(a - b).max()
        print(f"{H}x{W} s {s}: closed form vs numpy.fft {err:.2e}")
        assert err <= 1e-13 * np.abs(x).max()
    assert np.abs(R.fourier_filter64(x, 0.2) - x).max() > 0.1


def test_closed_form_fails_for_a_side_of_one():
    """why the kernel refuses H or W = 1: the mask of a length-1 axis selects its only bin once, the closed form counts it twice"""
    import freeu_ref as R
    x = np.random.default_rng(0).standard_normal((1, 1, 1, 6)) + 1.5
    assert np.abs(R.fourier_filter64(x, 0.2) - R.fourier_closed64(x, 0.2)).max() > 1e-3


def test_backbone_reference_properties():
    import freeu_ref as R
    rng = np.random.default_rng(1)
    x = rng.standard_normal((2, 8, 3, 5)) + 1.5
    y = R.backbone64(x, 1.4)
    assert np.array_equal(y[:, 4:], x[:, 4:]) and not np.array_equal(y[:, :4], x[:, :4])
    m = x.mean(1)
    for n in range(2):
        lo, hi = np.unravel_index(m[n].argmin(), m[n].shape), np.unravel_index(m[n].argmax(), m[n].shape)
        assert np.array_equal(y[n, :4, lo[0], lo[1]], x[n, :4, lo[0], lo[1]])                     # factor 1 at the minimum of the mean map
        assert np.allclose(y[n, :4, hi[0], hi[1]], 1.4 * x[n, :4, hi[0], hi[1]], rtol=1e-15)      # factor b at its maximum
    flat = np.ones((1, 8, 2, 2))
    assert np.array_equal(R.backbone64(flat, 1.4), flat)                                            # max == min: the factor is defined as 1


def test_depth_and_workspace_are_pure_functions(lib):
    assert [lib.mlsd_freeu_depth(n) for n in (1, 8, 256, 257, 640, 1280, 4096, 16384)] == [8, 8, 8, 9, 10, 12, 23, 71]
    assert lib.mlsd_freeu_depth(0) == 0
    for n, H, W, Cn in ((1, 2, 2, 8), (3, 64, 64, 128), (8, 128, 128, 640)):
        b = lib.mlsd_freeu_ws_bytes(n, H, W, Cn)
        assert b % 256 == 0 and b >= 4 * max(n * H * W + n * 512, n * 17 * 7 * Cn)
    assert lib.mlsd_freeu_ws_bytes(0, 2, 2, 8) == 0


# ------------------------------------------------------------------ dry plans
# md5 of repr((op labels with tiles and flops, parameter list)) of the plain UNet plan of a dry engine, as tests/test_controlnet_cpu.py pins it (PLAIN)
PLAIN_MD5 = {"tiny": "5bae9a2fa1", "tinyxl": "3bb2ccbb37", "sd1": "2699d1a59f", "sdxl": "e6b13b084e"}
SPECIAL = ("ctrl_add", "freeu_backbone", "freeu_skip")


def plan(model, px, **kw):
    from mlimgsynth_amd import engine as E
    g = E.Generator(model, px, px, 1, defer_weights=True, **kw)
    try:
        u = g.unet_ctx()
        return u.op_list(), u.param_list(), g.freeu_info(), g.control_info()[0]
    finally:
        g.destroy()


@pytest.mark.parametrize("model,px", [("tiny", 64), ("tinyv", 64), ("tinyxl", 64), ("sd1", 512), ("sd2", 512), ("sdxl", 1024)])
def test_plan_without_the_flag_is_todays_and_the_flag_adds_only_the_passes(dry, model, px):
    import freeu_ref as R
    ops0, pl0, info0, _ = plan(model, px)
    assert info0 == (0, 0) and not [o for o in ops0 if o[0] in SPECIAL]
    if model in PLAIN_MD5:
        assert hashlib.md5(repr((ops0, pl0)).encode()).hexdigest()[:10] == PLAIN_MD5[model]
    ops1, pl1, info1, _ = plan(model, px, freeu=True)
    n1, n2 = R.COUNTS[model]
    assert info1 == (n1, n2)
    labels = [o[0] for o in ops1]
    assert labels.count("freeu_backbone") == labels.count("freeu_skip") == n1 + n2 and "ctrl_add" not in labels
    assert [o for o in ops1 if o[0] not in SPECIAL] == ops0 and pl1 == pl0        # everything else, tiles and parameters included, is the plain plan
    special = [l for l in labels if l in SPECIAL]
    assert special == ["freeu_backbone", "freeu_skip"] * (n1 + n2)


@pytest.mark.parametrize("model,px", [("tiny", 64), ("tinyxl", 64), ("sdxl", 1024)])
def test_with_a_controlnet_the_order_is_control_sum_filter_concat(dry, model, px):
    import freeu_ref as R
    ops, _, info, n_res = plan(model, px, freeu=True, control=True)
    ops_c, _, info_c, n_res_c = plan(model, px, control=True)
    assert info == R.COUNTS[model] and info_c == (0, 0) and n_res == n_res_c > 0      # control = 1 alone is a ControlNet and nothing else
    assert [o for o in ops if not o[0].startswith("freeu_")] == ops_c
    labels = [o[0] for o in ops]
    n_skip = 0
    for i, l in enumerate(labels):
        if l == "freeu_skip":                             # the control sum of the popped tensor, the filter on that sum, then the first op that reads the concatenation
            assert labels[i - 1] == "ctrl_add" and labels[i - 2] == "freeu_backbone" and labels[i + 1] not in SPECIAL
            n_skip += 1
    assert n_skip == sum(R.COUNTS[model])
    # the decoder pops one skip tensor per concatenation: the treated ones are the first n1 + n2 whose backbone is wide enough, in decoder order
    seq = [l for l in labels if l in SPECIAL]
    first = seq.index("freeu_backbone")
    assert seq[first - 1] == "ctrl_add" and seq[:first] == ["ctrl_add"] * first      # only the middle block's sum comes before the first treated concatenation


def test_reference_walks_the_same_stages():
    """the torch restatement treats the same concatenations (stage by stage) as COUNTS says the plan does"""
    torch = pytest.importorskip("torch")
    import controlnet_ref as CR
    import freeu_ref as R
    for model in ("tiny", "tinyxl"):
        P = CR.UNET[model]
        rng = np.random.default_rng(2)
        x = torch.from_numpy(rng.standard_normal((1, 4, 8, 8)).astype(np.float32))
        ctx = torch.from_numpy(rng.standard_normal((1, 77, P["n_ctx"])).astype(np.float32))
        lab = torch.from_numpy(rng.standard_normal((1, P["ch_adm_in"])).astype(np.float32)) if P["ch_adm_in"] else None
        t = torch.full((1,), 500.0)
        net = CR.make_net()
        stages = []
        with torch.no_grad():
            on = R.unet_freeu(net, P, x, t, ctx, lab, 1.4, 1.6, 0.9, 0.2, stages=stages)
            off = R.unet_freeu(net, P, x, t, ctx, lab, 1, 1, 1, 1)
            plain = net.unet(P, x, t, ctx, lab)
        assert (stages.count(1), stages.count(2)) == R.COUNTS[model]
        assert not torch.equal(on, plain)
        # factors of 1: the float64 hooks return their inputs up to an FFT's rounding, i.e. last-bit changes of fp32 values; the net rounds GEMM operands to fp16,
        # where such a change can flip a rounding -- the scatter tolerances.EVAL_SMALL is stated for
        assert CR.rel_l2(off.numpy(), plain.numpy()) <= TOL.EVAL_SMALL


# ------------------------------------------------------------------ the configuration word
def test_config_keeps_its_size_and_control_is_a_flags_word(dry):
    from mlimgsynth_amd import engine as E
    assert C.sizeof(E.AmdControlConfig) == C.sizeof(E.AmdConfig) and E.AmdControlConfig.control.offset == E.AmdConfig.n_ctx_tok.offset + 4
    assert (E.CONTROL_NET, E.CONTROL_FREEU) == (FF.CONTROL_NET, FF.CONTROL_FREEU) == (1, 2)
    for kw, word, has_ctl, has_fu in ((dict(), 0, False, False), (dict(control=True), 1, True, False), (dict(freeu=True), 2, False, True),
                                      (dict(control=True, freeu=True), 3, True, True)):
        g = E.Generator("tiny", 64, 64, 1, defer_weights=True, **kw)
        try:
            assert g.cfg.control == word and (g.ctx_at(5) is not None) == has_ctl and (g.control_info()[0] > 0) == has_ctl
            assert (g.freeu_info() != (0, 0)) == has_fu
            if has_fu:
                g.set_freeu(1.3, 1.4, 0.9, 0.2)
                for bad in ((-0.1, 1, 1, 1), (1, 4.5, 1, 1), (1, 1, float("nan"), 1), (1, 1, 1, float("inf"))):
                    with pytest.raises(Exception):
                        g.set_freeu(*bad)
            else:
                with pytest.raises(Exception):
                    g.set_freeu(1.3, 1.4, 0.9, 0.2)
        finally:
            g.destroy()
    cfg = E.AmdControlConfig(b"tiny", 64, 64, 1, 20, 7.0, 1.0, 1, 0, 0, 1234, 0, 0.0, 1.0, 0.0, 1, 0, 77, 4)
    assert not dry.mlis_amd_create(C.byref(cfg), None)                       # an unknown bit is refused, not ignored


# ------------------------------------------------------------------ options, symbols, wrapper, CLI
def test_option_table_round_trips(lib):
    for oid, name in FF.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid).decode() == name and lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(140) == b"???" and lib.mlis_option_str(146) == b"???"


def test_options_defaults_ranges_and_refusals(lib):
    m = F.Mlis(lib)
    try:
        f, i = C.c_float(-1), C.c_int(-1)
        assert lib.mlis_option_get(m.ctx, FF.FREEU, C.byref(i)) == 1 and i.value == 0
        for oid, want in FF.DEFAULTS.items():
            assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1 and f.value == np.float32(want)
        m.set("freeu", 1)
        assert lib.mlis_option_get(m.ctx, FF.FREEU, C.byref(i)) == 1 and i.value == 1
        m.set("freeu", "n")
        assert lib.mlis_option_get(m.ctx, FF.FREEU, C.byref(i)) == 1 and i.value == 0
        assert lib.mlis_option_set(m.ctx, FF.FREEU, 1) == 1 and lib.mlis_option_get(m.ctx, FF.FREEU, C.byref(i)) == 1 and i.value == 1
        assert lib.mlis_option_set(m.ctx, FF.FREEU, 2) == -4 and lib.mlis_option_set(m.ctx, FF.FREEU, -1) == -4          # MLIS_E_OPT_VALUE
        for oid, name in list(FF.OPTION_NAMES.items())[1:]:
            m.set(name, 0), m.set(name, 4), m.set(name, 1.25)
            assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1 and f.value == 1.25
            assert lib.mlis_option_set(m.ctx, oid, C.c_double(2.5)) == 1 and lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1 and f.value == 2.5
            for bad in ("-0.1", "4.1", "x", "1.5x", "nan"):
                assert lib.mlis_option_set_str(m.ctx, name.encode(), bad.encode()) == -4, (name, bad)
            assert lib.mlis_option_set(m.ctx, oid, C.c_double(-1.0)) == -4 and lib.mlis_option_set(m.ctx, oid, C.c_double(4.5)) == -4
            assert lib.mlis_option_get(m.ctx, oid, C.byref(f)) == 1 and f.value == 2.5                                   # a refused value changes nothing
        for bad in ("2", "maybe", "-1"):
            assert lib.mlis_option_set_str(m.ctx, b"freeu", bad.encode()) == -4, bad
    finally:
        m.close()


def test_symbols_wrapper_and_cli(lib):
    for name in FF.EXPORTS:
        assert hasattr(lib, name), name
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert (M.MLIS_OPT_AMD_FREEU, M.MLIS_OPT_AMD_FREEU_B1, M.MLIS_OPT_AMD_FREEU_B2, M.MLIS_OPT_AMD_FREEU_S1, M.MLIS_OPT_AMD_FREEU_S2) == (141, 142, 143, 144, 145)
    assert callable(M.MLImgSynth.freeu_set) and callable(K.freeu_backbone) and callable(K.freeu_skip) and callable(E.Generator.set_freeu)
    assert K.freeu_depth(4096) == lib.mlsd_freeu_depth(4096) and K.freeu_ws_bytes(3, 64, 64, 128) == lib.mlsd_freeu_ws_bytes(3, 64, 64, 128)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    for flag in ("--freeu ", "--freeu-b1", "--freeu-b2", "--freeu-s1", "--freeu-s2"):
        assert flag in out, flag
    r = subprocess.run([exe, "generate", "--freeu", "y", "--freeu-b1", "5"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "freeu-b1" in r.stderr


def test_python_wrapper_sets_the_options(lib):
    from mlimgsynth_amd import mlimgsynth as M
    m = M.MLImgSynth()
    m.freeu_set(on=True, b1=1.1, s2=0.5)
    i, f = C.c_int(), C.c_float()
    m.option_get(M.MLIS_OPT_AMD_FREEU, i)
    assert i.value == 1
    for oid, want in ((M.MLIS_OPT_AMD_FREEU_B1, 1.1), (M.MLIS_OPT_AMD_FREEU_B2, 1.4), (M.MLIS_OPT_AMD_FREEU_S1, 0.9), (M.MLIS_OPT_AMD_FREEU_S2, 0.5)):
        m.option_get(oid, f)
        assert f.value == np.float32(want)
    m.freeu_set(on=False)
    m.option_get(M.MLIS_OPT_AMD_FREEU, i)
    assert i.value == 0
    with pytest.raises(RuntimeError):
        m.freeu_set(b2=7)


# ------------------------------------------------------------------ what the kernels refuse (before any launch: the dry runtime's buffers are host memory)
def test_kernels_refuse_bad_arguments(dry):
    n, H, W, Cn = 2, 4, 6, 16
    sz = n * H * W * 32                                    # room for strides up to 32
    buf = np.zeros(2 * sz + 64 + dry.mlsd_freeu_ws_bytes(n, H, W, Cn) // 4 + 64, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data % 256)
    d, s, f, w = base, base + sz * 4, base + 2 * sz * 4, base + 2 * sz * 4 + 256
    bb = lambda dst=d, ldd=16, src=s, lds=16, n_=n, rows=H * W, C_=Cn, ws=w, fd=f: dry.mlsd_freeu_backbone(dst, ldd, src, lds, n_, rows, C_, ws, fd, None)
    sk = lambda dst=d, ldd=16, src=s, lds=16, n_=n, H_=H, W_=W, C_=Cn, ws=w, fd=f: dry.mlsd_freeu_skip(dst, ldd, src, lds, n_, H_, W_, C_, ws, fd, None)
    OK = -2                                                # arguments accepted: the dry runtime then declines the launch (-2); a refused argument is -1
    assert bb() == OK and sk() == OK and bb(ldd=32, lds=24) == OK and sk(ldd=32, lds=24) == OK
    assert bb(rows=1) == OK                                # one pixel: max == min, the factor is 1
    common = (dict(C_=12), dict(C_=4), dict(C_=0), dict(ldd=18), dict(lds=12), dict(ldd=8), dict(dst=d + 4), dict(src=s + 8), dict(ws=w + 4), dict(fd=f + 2),
              dict(dst=None), dict(src=None), dict(ws=None), dict(fd=None), dict(n_=0), dict(dst=s), dict(dst=s + 16 * 4), dict(ws=d), dict(ws=s + 64), dict(fd=d + 16),
              dict(fd=w + 16), dict(src=d + 16 * 8))
    for kw in common:
        assert bb(**kw) == -1, kw
        assert sk(**kw) == -1, kw
    for kw in (dict(H_=1), dict(W_=1), dict(H_=1, W_=1), dict(H_=0), dict(W_=1025), dict(H_=2048)):
        assert sk(**kw) == -1, kw
    assert bb(rows=0) == -1
