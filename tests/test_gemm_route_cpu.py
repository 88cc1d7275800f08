"""mlsd_gemm_route in the dry runtime (no device: no stream-K, no LayerNorm ending on the 128x320 tile): it agrees with the six routing queries and
the variant label on a grid of launches, and the MLSD_TILE_* names are the tiles that mlsd_gemm_variant names."""
import pytest

from gemm_route_cases import cases, check_route, forced_cases, tile_label_when_forced
from mlimgsynth_amd import kernels as K


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield L
    L.mlsd_runtime_dry(0)


def test_route_agrees_with_the_queries(dry):
    n = sum(1 for desc, a in cases() if check_route(desc, a))
    assert n > 10000


def test_route_agrees_with_the_queries_on_forced_variants(dry):
    for desc, v, a in forced_cases():
        dry.mlsd_gemm_force_variant(v)
        try:
            check_route(desc, a, forced=v)
        finally:
            dry.mlsd_gemm_force_variant(-1)


def test_tile_names_are_the_launcher_labels(dry):
    experiments = dry.mlsd_has_experiments()
    for v, name in K.TILE_LABELS.items():
        if v in (K.TILE_PPSK_256x256, K.TILE_PPSK_128x320):
            continue           # (stream-K needs the device: tests/test_gemm_route_gpu.py)
        if v in (K.TILE_PPB_128x320, K.TILE_PP2_256x128, K.TILE_W4_256x256, K.TILE_W4_128x320) and not experiments:
            continue
        label, r = tile_label_when_forced(v)
        assert label.startswith(f"gemm<{name},") and r.variant == v and r.asked, (v, name, label)
