"""mlsd_gemm_route on an MI355X, queries only (nothing is launched): the LayerNorm endings of the 128x320 tile and the stream-K tiles that the dry
runtime cannot reach agree with the six routing queries and the variant label too, and the stream-K names are the launcher's labels."""
import pytest

from gemm_route_cases import cases, check_route, forced_cases, tile_label_when_forced
from mlimgsynth_amd import kernels as K


@pytest.mark.gpu
def test_route_agrees_with_the_queries_on_the_device():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    seen = {"ln1": 0, "ppsk": 0}
    for desc, a in cases():
        r = check_route(desc, a)
        seen["ln1"] += r.ln == 1
        seen["ppsk"] += r.variant in (K.TILE_PPSK_256x256, K.TILE_PPSK_128x320)
    for desc, v, a in forced_cases():
        L.mlsd_gemm_force_variant(v)
        try:
            check_route(desc, a, forced=v)
        finally:
            L.mlsd_gemm_force_variant(-1)
    assert seen["ln1"] > 0 and seen["ppsk"] > 0, seen


@pytest.mark.gpu
@pytest.mark.parametrize("v", [K.TILE_PPSK_256x256, K.TILE_PPSK_128x320])
def test_stream_k_tile_names_are_the_launcher_labels(v):
    label, r = tile_label_when_forced(v)
    assert label.startswith(f"gemm<{K.TILE_LABELS[v]},") and r.variant == v and r.asked and r.handoff, label
