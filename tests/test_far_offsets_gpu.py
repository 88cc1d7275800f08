"""The kernels of 2048x2048 decodes across 2 GiB and 4 GiB offsets, on the device (tests/far_offsets.py: the census, the cases, the arena rule, the sampled rows).

One test per case of FAR_CASES: the operands are carved from one allocation (the far ones 2 GiB + 64 KiB into it, their extent rounded up to 4 GiB behind them), the
inputs tiled from blocks that differ on the two sides of every boundary, the outputs filled with 0xFF bytes; after the launch mlsd_count_nonfinite over every output
(as fp32 words) must be 0 and the sampled rows -- first, last, around 2^31 and 2^32 bytes of every far operand, the ends of their tiles, 300 seeded others -- must
hold the bounds of tests/ref64.py.  Each test prints its worst ratio, its arena and its wall time.  A test skips only where the arena cannot be allocated.

The last test bounds, on the device, the workspace of every split-K launch that adds its slices itself (EXPERIMENTS builds): its kernels keep 32-bit offsets.
"""
import ctypes
import time

import numpy as np
import pytest

import far_offsets as FO

pytestmark = pytest.mark.gpu


def _arena(_lib, nbytes):
    try:
        return FO.DeviceMemory(_lib, nbytes)
    except _lib.MlsdError as e:
        pytest.skip(f"an arena of {nbytes} bytes ({nbytes / 2 ** 30:.2f} GiB) cannot be allocated: {e}")


@pytest.mark.parametrize("cid", FO.ALL_IDS)
def test_far_case(cid):
    from mlimgsynth_amd import _lib
    t0 = time.time()
    c = FO.build_case(cid)
    mem = _arena(_lib, c.arena)
    try:
        FO.fill(c, mem)
        label = FO.launch(c, mem)
        t1 = time.time()
        holes = FO.unwritten(c, mem)
        worst = FO.check(c, mem)
    finally:
        mem.free()
    cls = FO.case_classes(c)
    print(f"\n[far offsets] {cid:20s} {label:28s} arena {c.arena / 2 ** 30:6.2f} GiB  " + ", ".join(f"{n} {k}" for n, k in cls.items()) +
          "  worst " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()) + f"  rows {len(FO.sample_rows(c))}  fill+launch {t1 - t0:.1f} s, all {time.time() - t0:.1f} s")
    assert all(n == 0 for n in holes.values()), f"{cid} ({label}): fp32 words of the outputs still 0xFF after the launch: {holes}"
    assert worst and all(r <= 1.0 for r in worst.values()), f"{cid} ({label}): worst ratio to the bound {worst}"


def test_count_nonfinite_beyond_4_gib():
    """the counter the cases rely on, at 2^30 + 5 elements (4 GiB + 20 bytes): three planted NaNs, one below 2^31 bytes, one above, one in the last element"""
    from mlimgsynth_amd import _lib
    n = 2 ** 30 + 5
    mem = _arena(_lib, 4 * n)
    try:
        mem.memset(0, 0, 4 * n)
        assert mem.count_nonfinite(0, n) == 0
        nan = np.array([np.nan], np.float32).view(np.uint8)
        for i in (12345, 2 ** 29 + 7, n - 1):
            mem.write(4 * i, nan)
        assert mem.count_nonfinite(0, n) == 3
        assert mem.count_nonfinite(0, n - 1) == 2 and mem.count_nonfinite(4 * (2 ** 29 + 8), n - 2 ** 29 - 8) == 1
    finally:
        mem.free()


def _has_experiments():
    from mlimgsynth_amd import _lib
    return bool(_lib.lib().mlsd_has_experiments())


needs_experiments = pytest.mark.skipif(not _has_experiments(), reason="variant not in the product build (make EXPERIMENTS=1)")


@needs_experiments
def test_in_launch_split_k_never_gets_a_workspace_of_2_gib():
    """gemm_kernel PAR stores and merges its slices through a buffer resource of 0x7fffffff bytes with (int) byte offsets: wherever the route picks it (the whole grid
    resident: at most 2047 tiles and tiles x slices <= 3 x CUs), slices x M x N x 4 bytes must stay below 2^31; and the shapes that reach 2^31 must not get it"""
    import test_far_offsets_cpu as TC
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    took = 0
    try:
        L.mlsd_gemm_set_splitk_parallel(1)
        for M, N, K, ks in TC.SPLITK_SHAPES + [(m, n, 4096, ks) for m in (64, 128, 1000, 4096, 32768) for n in (128, 640, 1280, 4096) for ks in (2, 4, 8, 16)]:
            par = L.mlsd_gemm_splitk_parallel(ctypes.byref(TC._splitk_args(M, N, K, ks)))
            took += par
            assert not par or ks * M * N * 4 < 2 ** 31, (M, N, K, ks)
    finally:
        L.mlsd_gemm_set_splitk_parallel(0)
    assert took, "no shape took the in-launch split-K: the sweep bounds nothing"
