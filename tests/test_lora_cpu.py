"""The device-side LoRA path, the parts that need no GPU: the exported symbols and the Python mirror, the counters of a new context, the resolve / apply
split of the host merge (resolve + a numpy restatement of apply == mlts_lora_apply, same error texts), the kernel launcher's refusals in the dry runtime,
and the adapter files of the GPU tests against the name conversion."""
import ctypes as C

import numpy as np
import pytest

import loader_cases as LC
import lora_ffi as LF
import mlis_ffi as F


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return LF.bind(_lib.LIB_PATH)


def test_symbols_are_exported_and_counters_start_at_zero(lib):
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    for name in LF.EXPORTS:
        assert hasattr(L, name), name
    m = F.Mlis(lib)
    try:
        assert LF.stats(lib, m) == (0, 0, 0)
        assert lib.mlis_amd_lora_stats(m.ctx, None, None, None) == 1
    finally:
        m.close()
    assert lib.mlis_amd_lora_stats(None, None, None, None) == -1


def test_python_mirror():
    from mlimgsynth_amd import mlimgsynth as W
    assert callable(W.MLImgSynth.lora_stats)
    with W.MLImgSynth() as s:
        assert s.lora_stats() == (0, 0, 0)


def files(tmp_path, shape, r, dtype, alpha=None, scale=None, up_edit=None):
    from safetensors.numpy import save_file
    rng = np.random.default_rng(5)
    w = (rng.standard_normal(shape) * 0.1).astype(dtype)
    down = (rng.standard_normal((r,) + tuple(shape[1:])) * 0.2).astype(dtype)
    up = (rng.standard_normal((shape[0], r) + ((1, 1) if len(shape) == 4 else ())) * 0.2).astype(dtype)
    if up_edit:
        up = up_edit(up)
    save_file({LF.KEY + ".weight": w}, str(tmp_path / "w.safetensors"))
    save_file(LF.adapter_tensors(LF.KOHYA, up, down, alpha, scale), str(tmp_path / "a.safetensors"))
    return str(tmp_path / "w.safetensors"), str(tmp_path / "a.safetensors"), w, up, down


@pytest.mark.parametrize("wtype,dtype", [(LF.MLT_F16, np.float16), (LF.MLT_F16, np.float32), (LF.MLT_F32, np.float32)], ids=["f16", "f32_as_f16", "f32"])
@pytest.mark.parametrize("shape,r", [((5, 7), 1), ((40, 72), 4), ((6, 5, 3, 3), 2)], ids=["5x7", "40x72", "conv"])
def test_resolve_then_apply_is_the_merge(lib, tmp_path, shape, r, wtype, dtype):
    """the item mlts_lora_resolve returns, applied in numpy with the merge's operation order (fp32, product and sum rounded separately, ascending rank), gives
    the bits mlts_lora_apply stores"""
    wf, af, w, up, down = files(tmp_path, shape, r, dtype, alpha=2.0)
    n0, n1, ri, s, U, D = LF.resolve(lib, wf, af, 0.75, wtype)
    assert (n0, n1, ri) == (int(np.prod(shape[1:])), shape[0], r)
    assert np.float32(s) == np.float32(2.0) / np.float32(r) * np.float32(0.75)
    rnd = (lambda x: x.astype(np.float16).astype(np.float32)) if wtype == LF.MLT_F16 else (lambda x: x.astype(np.float32))
    assert np.array_equal(U, rnd(up).reshape(n1, r)) and np.array_equal(D, rnd(down).reshape(r, n0))
    delta = np.zeros((n1, n0), np.float32)
    for k in range(r):
        delta = delta + U[:, k:k + 1] * D[k:k + 1, :]
    want = rnd(rnd(w).reshape(n1, n0) + delta * np.float32(s)).reshape(-1)
    got, err = LF.host_merge(lib, wf, [(af, 0.75)], wtype)
    assert got is not None, err
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_resolve_reports_the_merge_errors(lib, tmp_path):
    wf, af, *_ = files(tmp_path, (40, 72), 4, np.float16, up_edit=lambda u: u[:-1])
    D, L = lib.mlts_open(wf.encode(), 0), lib.mlts_open_lora(af.encode())
    try:
        it, errs = LF.LoraItem(), []
        for i in range(lib.mlts_count(L)):
            if lib.mlts_lora_resolve(D, L, i, 1.0, C.byref(it)) < 0:
                errs.append(lib.mlsd_last_error().decode())
        assert errs == ["lora up/down invalid shapes for " + LF.KEY]
        assert lib.mlts_lora_apply(D, L, 1.0, LF.MLT_F16) < 0 and lib.mlsd_last_error().decode() == errs[0]
        assert lib.mlts_lora_resolve(D, L, -1, 1.0, C.byref(it)) < 0 and lib.mlts_lora_resolve(D, L, 99, 1.0, C.byref(it)) < 0
    finally:
        lib.mlts_close(L), lib.mlts_close(D)


def test_launcher_refuses_bad_arguments_without_a_device(lib):
    """the argument checks come before anything touches the device; in the dry runtime a well-formed call is refused too (its buffers are host memory)"""
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    try:
        W, U, D = np.zeros(40 * 72, np.float32), np.zeros(40 * 4, np.float32), np.zeros(4 * 72, np.float32)
        flag = np.zeros(1, np.int32)
        ok = dict(W=W.ctypes.data, dtype=0, n0=72, n1=40, up=U.ctypes.data, down=D.ctypes.data, r=4, scale=1.0, layout=0, lp=(0, 0, 0, 0, 0), flag=flag.ctypes.data)

        def call(**kw):
            a = dict(ok, **kw)
            return lib.mlsd_lora_apply(a["W"], a["dtype"], a["n0"], a["n1"], a["up"], a["down"], a["r"], a["scale"], a["layout"], *a["lp"], a["flag"], None)
        for kw in (dict(r=0), dict(n0=0), dict(n1=-1), dict(W=None), dict(up=None), dict(down=None), dict(flag=None), dict(layout=3), dict(dtype=2),
                   dict(layout=1, lp=(3, 3, 5, 6, 8)), dict(layout=1, lp=(3, 3, 8, 40, 4)), dict(layout=2, lp=(72, 20, 0, 0, 0)), dict(n0=2**31)):
            assert call(**kw) < 0, kw
            assert b"mlsd_lora_apply" in lib.mlsd_last_error(), kw
        assert call() < 0 and b"mlsd_lora_apply" not in lib.mlsd_last_error()
        assert not W.any() and not flag.any()
    finally:
        L.mlsd_runtime_dry(0)


@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
def test_gpu_test_adapters_reach_their_targets(lib, tmp_path, model):
    """every target of the adapters the GPU tests generate with -- attention, both feed-forward linears, a 3x3 conv, a projection, the text towers -- goes through
    the name conversion and resolves against the checkpoint"""
    import test_lora_gpu as G
    ck, ad = str(tmp_path / "m.safetensors"), str(tmp_path / "a.safetensors")
    LC.write_checkpoint(ck, model, "F16")
    G.write_model_adapter(ad, model, 21)
    D, L = lib.mlts_open(ck.encode(), 1), lib.mlts_open_lora(ad.encode())
    assert D and L, lib.mlsd_last_error()
    try:
        keys, it = [], LF.LoraItem()
        for i in range(lib.mlts_count(L)):
            r = lib.mlts_lora_resolve(D, L, i, 1.0, C.byref(it))
            assert r >= 0, lib.mlsd_last_error()
            if r:
                keys.append(it.key.decode())
        want = [t + ".weight" for t, _ in G.targets_of(model)]
        assert sorted(keys) == sorted(want) and len(set(want)) == len(want)
        assert any("conv1" in k for k in keys) and any("ff.net.0.proj" in k for k in keys) and any(k.startswith("clip.") for k in keys)
    finally:
        lib.mlts_close(L), lib.mlts_close(D)
