"""Prompts longer than 75 tokens, host side: the split into 75-token windows (mlis_amd_prompt_windows), the engine
configuration's trailing context length (MLIS_AmdConfig.n_ctx_tok) and the Python mirrors of both."""
import ctypes

import pytest


def windows(n):
    from mlimgsynth_amd import text
    return text.prompt_windows(n)


@pytest.mark.parametrize("n,want", [
    (0, [(0, 0)]),                                       # an empty prompt is one (empty) window
    (1, [(0, 1)]),
    (75, [(0, 75)]),
    (76, [(0, 75), (75, 1)]),
    (150, [(0, 75), (75, 75)]),
    (151, [(0, 75), (75, 75), (150, 1)]),
    (300, [(0, 75), (75, 75), (150, 75), (225, 75)]),
])
def test_window_split(n, want):
    assert windows(n) == want


def test_window_split_above_300_tokens_is_an_error():
    from mlimgsynth_amd._lib import MlsdError, last_error
    with pytest.raises(MlsdError):
        windows(301)
    assert "max: 300" in last_error()


def test_window_split_covers_the_tokens_in_order():
    for n in range(1, 301):
        w = windows(n)
        assert len(w) == (n + 74) // 75
        assert [s for s, _ in w] == [75 * i for i in range(len(w))]
        assert sum(ln for _, ln in w) == n and all(0 < ln <= 75 for _, ln in w)


def test_amd_config_mirror_has_the_context_length_last():
    from mlimgsynth_amd import engine
    names = [f[0] for f in engine.AmdConfig._fields_]
    assert names[-1] == "n_ctx_tok" and names[-2] == "unet_split"
    off = engine.AmdConfig.n_ctx_tok.offset
    assert off == engine.AmdConfig.unet_split.offset + ctypes.sizeof(ctypes.c_int)
    assert ctypes.sizeof(engine.AmdConfig) >= off + ctypes.sizeof(ctypes.c_int)


def test_generator_defaults_to_77_context_rows():
    import inspect
    from mlimgsynth_amd import engine
    assert inspect.signature(engine.Generator.__init__).parameters["n_ctx_tok"].default == 77
    assert inspect.signature(engine.Unet.__init__).parameters["n_ctx_tok"].default == 77


def test_kernel_entry_and_profile_label():
    from mlimgsynth_amd import _lib, kernels
    assert hasattr(_lib.lib(), "mlsd_attention_ctx") and callable(kernels.attention_ctx)
    from tools.kernel_labels import known
    assert known("void (anonymous namespace)::attn_ctx_kernel<64, 3, true>((anonymous namespace)::AttnP, int)") == ("attention<64,key groups>", "keys in LDS")
    assert known("_ZN12_GLOBAL__N_115attn_ctx_kernelILi160ELi2ELb0EEEvNS_5AttnPEi") == ("attention<160,key groups>", "keys streamed")


def test_kernel_rejects_the_short_context_and_causal_masks():
    """mlsd_attention_ctx takes 96 < Tk <= 320 without a mask; everything else is an error before any launch (null device pointers are never read)."""
    from mlimgsynth_amd import _lib, kernels
    L = _lib.lib()
    f = L.mlsd_attention_ctx
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    base = dict(q=16, k=16, v=16, out=16, ldq=64, ldk=64, ldv=64, ldo=64, bsq=64 * 64, bsk=64 * 154, bsv=64 * 154, bso=64 * 64,
                n_batch=1, n_head=1, d_head=64, Tq=64, Tk=154, causal=0)
    for bad in (dict(Tk=77), dict(Tk=96), dict(Tk=321), dict(causal=1), dict(d_head=48), dict(ldk=60)):
        a = kernels.AttnArgs(**{**base, **bad})
        assert f(ctypes.byref(a), None) < 0, bad
