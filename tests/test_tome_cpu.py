"""Token merging without a GPU (dry runtime): the r and level rule, the refusals, the plan's records, and tome_ref's partition against a second statement of it."""
import pytest

import tome_ref as TR


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield engine
    L.mlsd_runtime_dry(0)


@pytest.mark.parametrize("H,W", [(8, 8), (9, 7), (12, 20), (2, 2), (5, 2), (64, 64)])
def test_partition_against_a_second_statement(H, W):
    src, dst = TR.partition(H, W)
    want_dst = [y * W + x for y in range(0, H - 1, 2) for x in range(0, W - 1, 2)]      # the corner of every whole 2 x 2 cell
    assert dst.tolist() == want_dst and src.tolist() == sorted(set(range(H * W)) - set(want_dst))


@pytest.mark.parametrize("H,W,ratio,r", [(64, 64, 0.5, 2048), (128, 128, 0.5, 8192), (64, 64, 0.75, 3072), (8, 8, 0.5, 32), (8, 8, 0.2, 0), (9, 7, 0.75, 32),
                                          (12, 8, 0.3, 16), (64, 64, 0.0, 0)])
def test_r_rule(dry, H, W, ratio, r):
    from mlimgsynth_amd import kernels as K
    assert K.tome_r(H, W, ratio) == TR.r_of(H, W, ratio) == r


def test_levels_for_sd15_and_sdxl(dry):
    z = (0, 0, 0)
    # SD1.5 512 x 512: 5 transformer layers at each of downscale 1, 2, 4 (the middle block's never counts); SDXL 1024 x 1024: 10 at downscale 2, 50 at 4
    assert dry.tome_levels("sd1", 64, 64, 0.5, 0) == (5, [(4096, 2048, 2048), z, z, z])
    assert dry.tome_levels("sd1", 64, 64, 0.5, 2) == (10, [(4096, 2048, 2048), (1024, 512, 512), z, z])
    assert dry.tome_levels("sd1", 64, 64, 0.5, 8) == (15, [(4096, 2048, 2048), (1024, 512, 512), (256, 128, 128), z])
    assert dry.tome_levels("sdxl", 128, 128, 0.5, 0) == (10, [z, (4096, 2048, 2048), z, z])
    assert dry.tome_levels("sdxl", 128, 128, 0.5, 1) == (0, [z] * 4)
    assert dry.tome_levels("sdxl", 128, 128, 0.3, 4) == (60, [z, (4096, 1216, 2880), (1024, 304, 720), z])


BUILT = [("sd1", 24, 16, 0.5, 8), ("sd1", 24, 16, 0.3, 0), ("sdxl", 28, 20, 0.5, 4), ("sdxl", 24, 16, 0.75, 0), ("tinyxl", 18, 14, 0.5, 0), ("tinyxl", 16, 16, 0.1, 0)]


@pytest.mark.parametrize("model,lw,lh,ratio,ds", BUILT)
def test_the_key_rule_agrees_with_what_built_plans_report(dry, model, lw, lh, ratio, ds):
    """unet_tome_levels decides the engine key before an engine exists; sdxl 28 x 20 and tinyxl 18 x 14 merge odd maps (7 x 5, 9 x 7), the last case has r = 0"""
    g = dry.Generator(model, 8 * lw, 8 * lh, 1, defer_weights=True, tome=ratio, tome_max_ds=ds)
    try:
        want = dry.tome_levels(model, lw, lh, ratio, ds)
        assert g.tome_info()[2:] == want and (want[0] > 0) == ((model, lw, ratio) != ("tinyxl", 16, 0.1))
    finally:
        g.destroy()


def test_refusals(dry):
    from mlimgsynth_amd._lib import MlsdError
    g = dry.Generator("tinyxl", 512, 512, 1, defer_weights=True, hypertile=64, hypertile_depth=3)
    try:
        g.set_tome(0.5, 1)                       # tinyxl has no transformers at downscale 1: nothing to merge, nothing clashes
        for bad in ((0.8, 0), (-0.1, 0), (float("nan"), 0), (0.5, 3), (0.5, 16)):
            with pytest.raises(MlsdError):
                g.set_tome(*bad)
        assert g.tome_info()[:3] == (0.5, 1, 0) and g.hypertile_info()[0] > 0
        g.set_tome(0.0, 0)
        with pytest.raises(MlsdError, match="HyperTile"):
            g.set_tome(0.5, 0)                   # both on the downscale-2 level
        assert g.tome_info()[:3] == (0.0, 2, 0) and g.hypertile_info()[0] > 0      # the engine as it was
    finally:
        g.destroy()
    with pytest.raises(MlsdError, match="HyperTile"):
        dry.Unet("tinyxl", 64, 64, 1, synth=False, hypertile=64, tome=0.5)


def test_public_setting_and_info(dry):
    import ctypes as C
    import mlis_ffi as F
    from mlimgsynth_amd import _lib
    lib = F.bind(_lib.LIB_PATH)
    lib.mlis_amd_tome.argtypes = [C.c_void_p, C.c_float, C.c_int]
    lib.mlis_amd_tome_info.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    m, ratio, ds, lv = F.Mlis(lib), C.c_float(-1), C.c_int(-1), (C.c_int * 12)()
    try:
        assert lib.mlis_amd_tome_info(m.ctx, ratio, ds, lv) == 1 and (ratio.value, ds.value, list(lv)) == (0.0, 0, [0] * 12)      # the default: off
        assert all(lib.mlis_amd_tome(m.ctx, *bad) < 0 and "token merging" in m.err() for bad in ((0.76, 0), (-1.0, 0), (0.5, 5)))
        assert lib.mlis_amd_tome(m.ctx, 0.5, 4) == 1
        assert lib.mlis_amd_tome_info(m.ctx, ratio, ds, None) == 1 and (ratio.value, ds.value) == (0.5, 4)
    finally:
        m.close()
