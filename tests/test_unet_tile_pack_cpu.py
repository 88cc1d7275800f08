"""Packed tiled diffusion, the parts that need no GPU: the pack rule (mlis_amd_tile_pack) on the worked values and over a sweep, option 121 by id
and by name with its refusals, the exported symbols, the CLI usage text and the Python mirrors."""
import ctypes as C
import os
import subprocess

import pytest

import mlis_ffi as F
import unet_tile_ffi as U
import unet_tile_pack_ffi as UP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
E_OPT_VALUE = -4


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return UP.bind(_lib.LIB_PATH)


@pytest.fixture()
def m(lib):
    m = F.Mlis(lib)
    yield m
    m.close()


# ------------------------------------------------------------------ the pack rule
WORKED = [(9, 1, 4, 3, 3), (9, 1, 8, 5, 2), (9, 1, 9, 9, 1), (9, 1, 100, 9, 1), (4, 2, 3, 2, 2), (3, 2, 2, 2, 2), (7, 1, 3, 3, 3), (20, 1, 16, 10, 2),
          (9, 16, 8, 3, 3), (9, 64, 4, 1, 9)]


@pytest.mark.parametrize("n_win,B,pack,P,n_eval", WORKED)
def test_worked_values(lib, n_win, B, pack, P, n_eval):
    assert UP.c_pack(lib, n_win, B, pack) == (P, n_eval)
    assert UP.pack_rule(n_win, B, pack)[:2] == (P, n_eval)          # (the tests' own restatement)


def test_pack_one_is_one_window_per_evaluation(lib):
    for n in (1, 2, 9, 40):
        for B in (1, 2, 64):
            assert UP.c_pack(lib, n, B, 1) == (1, n)


def test_refusals_and_null(lib):
    for n_win, B, pack in ((9, 1, 0), (9, 1, -1), (0, 1, 4), (-3, 1, 4), (9, 0, 4), (9, -2, 4)):
        assert UP.c_pack(lib, n_win, B, pack) is None, (n_win, B, pack)
    assert lib.mlis_amd_tile_pack(9, 1, 4, None) == 3               # the evaluation count is optional


def test_sweep(lib):
    n_cases = 0
    for n_win in range(1, 41):
        for B in (1, 2, 16, 64):
            for pack in range(1, 21):
                got = UP.c_pack(lib, n_win, B, pack)
                want_p, want_n, p0 = UP.pack_rule(n_win, B, pack)
                assert got == (want_p, want_n), (n_win, B, pack, got)
                P, n_eval = got
                assert 1 <= P <= min(pack, n_win, 16, 64 // B)
                assert n_eval * P >= n_win > (n_eval - 1) * P
                assert n_eval * P - n_win < n_eval                 # fewer padded slots than evaluations
                assert n_eval == -(-n_win // p0)
                gs = UP.groups(n_win, B, pack)
                assert len(gs) == n_eval and all(len(s) == P for s, _ in gs)
                assert [j for s, u in gs for j in s[:u]] == list(range(n_win))          # every window once, in order
                assert all(u == P for _, u in gs[:-1]) and all(j == s[u - 1] for s, u in gs for j in s[u:])
                n_cases += 1
    assert n_cases == 40 * 4 * 20


# ------------------------------------------------------------------ option 121
def test_option_table(lib):
    for oid, name in UP.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid) == name.encode()
        assert lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.upper().replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(120) == b"???" and lib.mlis_option_str(122) == b"???"
    assert lib.mlis_option_str(111) == b"unet_tile" and lib.mlis_option_str(112) == b"unet_tile_overlap"      # no existing id moved
    assert lib.mlis_option_str(105) == b"hires_upscaler" and lib.mlis_option_str(101) == b"tiling" and lib.mlis_option_str(35) == b"no_prompt_parse"


def test_default_and_round_trip(lib, m):
    assert U.get(lib, m, UP.UNET_TILE_BATCH) == 1
    for val in (2, 16, 9, 1):
        m.set("unet_tile_batch", val)
        assert U.get(lib, m, UP.UNET_TILE_BATCH) == val
        m.set("UNET-TILE-BATCH", val)
        assert U.get(lib, m, UP.UNET_TILE_BATCH) == val
        assert lib.mlis_option_set(m.ctx, UP.UNET_TILE_BATCH, val) == 1 and U.get(lib, m, UP.UNET_TILE_BATCH) == val
    assert U.get(lib, m, U.UNET_TILE) == 0 and U.get(lib, m, U.UNET_TILE_OVERLAP) == -1         # the neighbours are untouched


@pytest.mark.parametrize("bad", ["0", "-1", "17", "2x", "1.5"])
def test_value_refusals(lib, m, bad):
    m.set("unet_tile_batch", 3)
    assert lib.mlis_option_set_str(m.ctx, b"unet_tile_batch", bad.encode()) == E_OPT_VALUE, bad
    assert "unet_tile_batch" in m.err()
    assert U.get(lib, m, UP.UNET_TILE_BATCH) == 3
    if bad.lstrip("-").isdigit():
        assert lib.mlis_option_set(m.ctx, UP.UNET_TILE_BATCH, int(bad)) == E_OPT_VALUE
        assert "unet_tile_batch" in m.err() and U.get(lib, m, UP.UNET_TILE_BATCH) == 3


def test_symbols_are_exported():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    for name in UP.EXPORTS:
        assert hasattr(L, name), name


def test_cli_lists_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--unet-tile-batch N", "--unet-tile PX", "--unet-tile-overlap PX"):
        assert flag in r.stdout, flag
    r = subprocess.run([CLI, "generate", "--unet-tile-batch", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "unet_tile_batch" in r.stderr


def test_python_mirrors():
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as W
    assert W.MLIS_OPT_AMD_UNET_TILE_BATCH == 121 and (W.MLIS_OPT_AMD_UNET_TILE, W.MLIS_OPT_AMD_UNET_TILE_OVERLAP) == (111, 112)
    for f in (K.window_gather_packed, K.window_blend_packed, K.tile_pack, E.Generator.tile_pack_info):
        assert callable(f)
    assert K.WINDOW_MAX_PACK == 16
    assert K.tile_pack(9, 1, 4) == (3, 3) and K.tile_pack(20, 1, 16) == (10, 2) and K.tile_pack(9, 1, 0) is None
    with W.MLImgSynth() as s:
        s.unet_tile_set(64, overlap=32, batch=2)
        t, o, b = C.c_int(), C.c_int(), C.c_int()
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE, t)
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE_OVERLAP, o)
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE_BATCH, b)
        assert (t.value, o.value, b.value) == (64, 32, 2)
        s.unet_tile_set(0)
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE_BATCH, b)
        assert b.value == 2                                # None keeps the batch
        with pytest.raises(RuntimeError, match="unet_tile_batch"):
            s.unet_tile_set(64, batch=17)
