"""Tiled diffusion, the parts that need no GPU: the window geometry (mlis_amd_window_starts) on the worked values and over a sweep, the two options
(ids 111 and 112) by id and by name with their refusals, the exported symbols, the CLI usage text and the Python mirrors."""
import ctypes as C
import os
import subprocess

import pytest

import mlis_ffi as F
import unet_tile_ffi as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
E_OPT_VALUE = -4


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


# ------------------------------------------------------------------ geometry
WORKED = [(12, 8, 4, 0, [0, 4]), (16, 8, 4, 0, [0, 4, 8]), (20, 8, 2, 0, [0, 6, 12]), (17, 8, 4, 0, [0, 3, 6, 9]),
          (12, 8, 4, 1, [0, 4, 8]), (16, 8, 4, 1, [0, 4, 8, 12])]


@pytest.mark.parametrize("L,T,O,wrap,want", WORKED)
def test_worked_values(lib, L, T, O, wrap, want):
    assert U.c_starts(lib, L, T, O, wrap) == want
    assert U.starts(L, T, O, wrap) == want                  # (the tests' own restatement)


def test_sweep_covers_and_overlaps(lib):
    n_cases = 0
    for L in range(1, 41):
        for T in range(1, 17):
            for O in range(0, T // 2 + 1):
                for wrap in (0, 1):
                    s = U.c_starts(lib, L, T, O, wrap)
                    assert s is not None and s == U.starts(L, T, O, wrap), (L, T, O, wrap, s)
                    n_cases += 1
                    if T >= L:
                        assert s == [0]
                        continue
                    assert s[0] == 0 and s == sorted(set(s)) and len(s) >= 2
                    cover = [0] * L
                    for a in s:
                        for k in range(T):
                            if not wrap:
                                assert a + k < L, (L, T, O, s)       # inside [0, L]
                            cover[(a + k) % L] += 1
                    assert min(cover) >= 1, (L, T, O, wrap, s)
                    if not wrap:
                        assert s[-1] + T == L
                        gaps = [b - a for a, b in zip(s, s[1:])]
                    else:
                        gaps = [b - a for a, b in zip(s, s[1:])] + [s[0] + L - s[-1]]
                    assert max(gaps) <= T - O, (L, T, O, wrap, s)    # neighbours share at least O pixels
    assert n_cases > 5000


def test_bad_arguments(lib):
    out = (C.c_int * 8)()
    for L, T, O, wrap, cap in ((12, 8, -1, 0, 8), (12, 8, 5, 0, 8), (12, 0, 0, 0, 8), (12, -3, 0, 1, 8), (0, 8, 4, 0, 8), (-5, 8, 4, 1, 8),
                               (12, 8, 4, 0, 1), (12, 8, 4, 1, 2), (40, 1, 0, 0, 8)):
        assert lib.mlis_amd_window_starts(L, T, O, wrap, out, cap) == -1, (L, T, O, wrap, cap)
    assert lib.mlis_amd_window_starts(12, 8, 4, 0, out, 2) == 2                # exactly the capacity
    assert lib.mlis_amd_window_starts(12, 8, 4, 0, None, 2) == -1


def test_weight_restatement():
    """linear over the overlap, 1 inside, 1 everywhere without overlap"""
    assert U.ramp(8, 4).tolist() == [0.2, 0.4, 0.6, 0.8, 0.8, 0.6, 0.4, 0.2]
    assert U.ramp(12, 2).tolist() == [1 / 3, 2 / 3] + [1.0] * 8 + [2 / 3, 1 / 3]
    assert (U.weight(5, 3, 0, 0) == 1).all()


# ------------------------------------------------------------------ options
def test_option_table_round_trips(lib):
    for oid, name in U.OPTION_NAMES.items():
        assert lib.mlis_option_str(oid) == name.encode()
        assert lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.upper().replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(105) == b"hires_upscaler" and lib.mlis_option_str(101) == b"tiling"      # no existing id moved
    assert lib.mlis_option_str(110) == b"???" and lib.mlis_option_str(113) == b"???"
    assert lib.mlis_option_str(35) == b"no_prompt_parse" and lib.mlis_option_str(36) == b"???"


def test_defaults_and_round_trip(lib, m):
    assert U.get(lib, m, U.UNET_TILE) == 0 and U.get(lib, m, U.UNET_TILE_OVERLAP) == -1
    for val in (64, 512, 1024, 0):
        m.set("unet_tile", val)
        assert U.get(lib, m, U.UNET_TILE) == val
        assert lib.mlis_option_set(m.ctx, U.UNET_TILE, val) == 1 and U.get(lib, m, U.UNET_TILE) == val
    for val in (0, 32, 256, -1):
        m.set("unet-tile-overlap", val)
        assert U.get(lib, m, U.UNET_TILE_OVERLAP) == val
        assert lib.mlis_option_set(m.ctx, U.UNET_TILE_OVERLAP, val) == 1 and U.get(lib, m, U.UNET_TILE_OVERLAP) == val
    m.set("unet_tile_overlap", "")                         # empty: auto
    assert U.get(lib, m, U.UNET_TILE_OVERLAP) == -1


@pytest.mark.parametrize("name,bad", [("unet_tile", "60"), ("unet_tile", "-8"), ("unet_tile", "7"), ("unet_tile", "64x"), ("unet_tile", "70000"),
                                      ("unet_tile_overlap", "12"), ("unet_tile_overlap", "-2"), ("unet_tile_overlap", "4"), ("unet_tile_overlap", "8.5")])
def test_value_refusals(lib, m, name, bad):
    oid = lib.mlis_option_fromz(name.encode())
    m.set("unet_tile", 64), m.set("unet_tile_overlap", 16)
    before = U.get(lib, m, oid)
    assert lib.mlis_option_set_str(m.ctx, name.encode(), bad.encode()) == E_OPT_VALUE, (name, bad)
    assert name in m.err()
    assert U.get(lib, m, oid) == before
    if "." not in bad and "x" not in bad:
        assert lib.mlis_option_set(m.ctx, oid, int(bad)) == E_OPT_VALUE


def test_symbols_are_exported():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    for name in U.EXPORTS:
        assert hasattr(L, name), name


def test_cli_lists_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--unet-tile PX", "--unet-tile-overlap PX", "--vae-tile N"):
        assert flag in r.stdout, flag
    r = subprocess.run([CLI, "generate", "--unet-tile", "60"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "unet_tile" in r.stderr


def test_python_mirrors():
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as W
    assert (W.MLIS_OPT_AMD_UNET_TILE, W.MLIS_OPT_AMD_UNET_TILE_OVERLAP) == (111, 112)
    assert W.MLIS_OPT__LAST == 35 and W.MLIS_OPT_AMD_HIRES_UPSCALER == 105
    for f in (K.window_gather, K.window_blend, K.window_wsum, K.window_starts):
        assert callable(f)
    assert K.window_starts(17, 8, 4) == [0, 3, 6, 9] and K.window_starts(12, 8, 4, wrap=True) == [0, 4, 8] and K.window_starts(12, 8, 5) is None
    with W.MLImgSynth() as s:
        s.unet_tile_set(64, overlap=32)
        t, o = C.c_int(), C.c_int()
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE, t)
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE_OVERLAP, o)
        assert (t.value, o.value) == (64, 32)
        s.unet_tile_set(0)
        s.option_get(W.MLIS_OPT_AMD_UNET_TILE_OVERLAP, o)
        assert o.value == 32                               # None keeps the overlap
        with pytest.raises(RuntimeError, match="unet_tile"):
            s.unet_tile_set(60)
