"""Seamless tiling (circular padding of the UNet / codec convolutions), the parts that need no GPU: the public option (MLIS_OPT_AMD_TILING =
101, "tiling"), the Python mirrors, the CLI flag, and the launcher's route for wrap launches in the dry runtime: a wrap launch only runs on a
tile that implements the wrap, and a launch none of whose taps can leave the image routes exactly as without it."""
import ctypes as C
import os
import subprocess

import pytest

import mlis_ffi as F
from gemm_route_cases import addr, shape_args, with_epilogue
from mlimgsynth_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
TILING = 101

# product tiles that carry the wrap in their convolution gather
WRAP_TILES = {K.TILE_128x128, K.TILE_64x128, K.TILE_256x128, K.TILE_256x128_S3, K.TILE_256x256, K.TILE_128x320, K.TILE_PP_256x256, K.TILE_PP_128x320,
              K.TILE_PPSK_256x256, K.TILE_PP2_128x320, K.TILE_PP2_256x256, K.TILE_PPSK_128x320, K.TILE_SKINNY, K.TILE_CONV_SMALLN}
EXPERIMENTS_ONLY = {K.TILE_PPB_128x320, K.TILE_PP2_256x128, K.TILE_W4_256x256, K.TILE_W4_128x320}
PP_TILES = {K.TILE_PP_256x256, K.TILE_PP_128x320, K.TILE_PP2_128x320, K.TILE_PP2_256x256}
SK_TILES = {K.TILE_PPSK_256x256, K.TILE_PPSK_128x320}
# epilogue forms of conv_cases() whose ping-pong epilogue has a wrap build (gemm_conv.hip launch_pp): F32 (rowbias rides on it), F32_RES, F32_STATS,
# F32_RES_STATS; through the upsample F32 and F32_STATS; stream-K F32 and F32_RES
PP_WRAP_FORMS = {"f32", "rowbias", "resid", "colstats", "resid+colstats"}
PP_UPS_WRAP_FORMS = {"f32", "rowbias", "colstats"}
SK_WRAP_FORMS = {"f32", "rowbias", "resid"}


def test_gemm_args_have_the_wrap_field():
    # (a ctypes Structure takes an unknown attribute silently: every test below would route zero-padded launches without this)
    assert "wrap" in dict(K.GemmArgs._fields_)
    assert K.GemmArgs.wrap.offset == K.GemmArgs.colstats_shift.offset + 4


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return F.bind(_lib.LIB_PATH)


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield L
    L.mlsd_runtime_dry(0)


def get_tiling(lib, m):
    v = C.c_int(-7)
    assert lib.mlis_option_get(m.ctx, TILING, C.byref(v)) == 1, m.err()
    return v.value


def test_option_by_id_and_by_string(lib):
    m = F.Mlis(lib)
    try:
        assert get_tiling(lib, m) == 0
        for name in ("tiling", "TILING"):
            for val, want in (("none", 0), ("x", 1), ("y", 2), ("xy", 3), ("XY", 3), ("0", 0), ("1", 1), ("2", 2), ("3", 3)):
                assert lib.mlis_option_set_str(m.ctx, name.encode(), val.encode()) == 1, (name, val, m.err())
                assert get_tiling(lib, m) == want, (name, val)
        for i in range(4):
            assert lib.mlis_option_set(m.ctx, TILING, i) == 1
            assert get_tiling(lib, m) == i
        lib.mlis_option_set(m.ctx, TILING, 2)
        for bad in ("z", "4", "-1", "", "x y", "1.0"):
            assert lib.mlis_option_set_str(m.ctx, b"tiling", bad.encode()) == -4, bad
            assert get_tiling(lib, m) == 2, bad             # a refused value leaves the mode alone
        for bad in (4, -1, 101):
            assert lib.mlis_option_set(m.ctx, TILING, bad) == -4, bad
        assert lib.mlis_option_str(TILING) == b"tiling"
        assert lib.mlis_option_fromz(b"tiling") == TILING and lib.mlis_option_fromz(lib.mlis_option_str(TILING)) == TILING
        assert lib.mlis_option_set(m.ctx, 99, 1) == -3     # (no id between the reference's options and the extensions)
        assert lib.mlis_option_str(35) == b"no_prompt_parse" and lib.mlis_option_str(36) == b"???"
    finally:
        m.close()


def test_python_wrapper_knows_the_option():
    from mlimgsynth_amd import mlimgsynth as W
    assert W.MLIS_OPT_AMD_TILING == TILING and W.MLIS_OPT__LAST == 35


def test_mirrors():
    assert K.GemmArgs._fields_[-1][0] == "wrap" and K.GemmArgs._fields_[-2][0] == "colstats_shift"
    import inspect
    from mlimgsynth_amd import engine
    for cls in (engine.Unet, engine.Decoder, engine.Generator):
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == "tiling" and p["tiling"].default == 0, cls
    assert engine.AmdConfig._fields_[-1][0] == "n_ctx_tok"      # (the mode is an argument of mlis_amd_create_ex, not a config field)


def conv_cases():
    """(description, args) of convolutions whose taps leave the image, over epilogues and K splits"""
    shapes = [(1, 64, 64, 320, 320, 3, 1, 0), (2, 32, 32, 640, 640, 3, 1, 0), (1, 16, 16, 1280, 1280, 3, 1, 0), (1, 8, 8, 1280, 1280, 3, 1, 0),
              (1, 32, 32, 320, 320, 3, 2, 0), (1, 32, 32, 1280, 1280, 3, 1, 1), (1, 128, 128, 128, 3, 3, 1, 0), (1, 128, 128, 64, 16, 3, 1, 0),
              (2, 128, 128, 512, 512, 3, 1, 0), (1, 256, 256, 256, 128, 3, 1, 0), (2, 3, 5, 64, 64, 3, 1, 0)]
    for shape in shapes:
        for epi in ("f32", "f16", "resid", "colstats", "resid+colstats", "silu", "rowbias"):
            for ksplit in (1, 4):
                a = with_epilogue(shape_args(shape), "resid" if epi == "resid+colstats" else epi)
                if epi == "resid+colstats":
                    a.colstats, a.colstats_shift = addr(), 1
                a.ksplit, a.ws, a.ws_bytes, a.sk_flags = ksplit, addr(), 1 << 28, addr()
                yield f"{shape} {epi} ksplit={ksplit}", epi, a


def test_wrap_launches_run_only_on_tiles_that_wrap(dry):
    assert "wrap" in dict(K.GemmArgs._fields_)
    n, pp = 0, 0
    for v in sorted(K.TILE_LABELS):
        dry.mlsd_gemm_force_variant(v)
        try:
            for desc, epi, a in conv_cases():
                a0 = K.gemm_route(a)
                for wrap in (1, 2, 3):
                    a.wrap = wrap
                    r = K.gemm_route(a)
                    assert r.variant in WRAP_TILES and r.variant not in EXPERIMENTS_ONLY, (v, desc, wrap, r.variant)
                    assert r.asked == (r.variant == v), (v, desc, wrap, r.variant, r.asked)
                    if v not in WRAP_TILES:
                        assert not r.asked, (v, desc, wrap)
                    assert K.gemm_variant(a).startswith(f"gemm<{K.TILE_LABELS[r.variant]},"), (v, desc, wrap)
                    # a ping-pong / stream-K wrap route has a kernel built for its epilogue (launch_pp would fail otherwise)
                    if r.variant in PP_TILES:
                        assert epi in (PP_UPS_WRAP_FORMS if a.upsample else PP_WRAP_FORMS), (v, desc, wrap, r.variant)
                        pp += 1
                    if r.variant in SK_TILES:
                        assert epi in SK_WRAP_FORMS, (v, desc, wrap, r.variant)
                    n += 1
                a.wrap = 0
                assert K.gemm_route(a).variant == a0.variant
        finally:
            dry.mlsd_gemm_force_variant(-1)
    assert n > 2000 and pp > 200


def test_a_ping_pong_conv_without_a_wrap_build_falls_back(dry):
    """the fp16-output conv runs on the ping-pong tile's generic epilogue, which has no wrap build: the wrap launch takes the general tile"""
    a = with_epilogue(shape_args((2, 32, 32, 640, 640, 3, 1, 0)), "f16")
    a.tile_variant = K.tile_arg(K.TILE_PP_256x256)
    r0 = K.gemm_route(a)
    assert r0.variant == K.TILE_PP_256x256 and r0.asked
    a.wrap = 3
    r = K.gemm_route(a)
    assert r.variant == K.TILE_256x256 and not r.asked


def route_tuple(r):
    return tuple(getattr(r, f) for f, _ in K.GemmRouteInfo._fields_)


def test_wrap_launches_whose_taps_stay_inside_route_as_zero_padding(dry):
    shapes = [(2, 64, 64, 640, 320, 1, 1, 0), (1, 32, 32, 1280, 1280, 1, 1, 0), (1, 16, 16, 320, 640, 1, 2, 0), (8192, 1280, 1280), (128, 1280, 1280)]
    n = 0
    for v in [-1] + sorted(K.TILE_LABELS):
        dry.mlsd_gemm_force_variant(v)
        try:
            for shape in shapes:
                for epi in ("f32", "f16", "resid", "colstats", "ln"):
                    a = with_epilogue(shape_args(shape), epi)
                    if a is None:
                        continue
                    a.ws, a.ws_bytes, a.sk_flags = addr(), 1 << 28, addr()
                    if len(shape) == 8:
                        a.pad = 0
                        a.OH, a.OW = (a.H - 1) // a.stride + 1, (a.W - 1) // a.stride + 1
                        a.M = a.n_img * a.OH * a.OW
                    want, label = route_tuple(K.gemm_route(a)), K.gemm_variant(a)
                    for wrap in (1, 2, 3):
                        a.wrap = wrap
                        assert route_tuple(K.gemm_route(a)) == want and K.gemm_variant(a) == label, (v, shape, epi, wrap)
                        n += 1
                    a.wrap = 0
        finally:
            dry.mlsd_gemm_force_variant(-1)
    assert n > 300


def test_tt_tile_takes_a_pointwise_wrap_launch(dry):
    """the 128x160 tile (30) has no convolution gather: a 1x1 pad-0 convolution with a wrap mode still runs on it"""
    a = with_epilogue(shape_args((2, 64, 64, 1280, 1280, 1, 1, 0)), "f32")
    a.pad, a.OH, a.OW = 0, 64, 64
    a.M = 2 * 64 * 64
    a.tile_variant = K.tile_arg(K.TILE_TT)
    r0 = route_tuple(K.gemm_route(a))
    a.wrap = 3
    assert route_tuple(K.gemm_route(a)) == r0


def test_cli_lists_and_checks_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--tiling none|x|y|xy" in r.stdout
    r = subprocess.run([CLI, "generate", "--tiling", "diagonal"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "tiling" in r.stderr
