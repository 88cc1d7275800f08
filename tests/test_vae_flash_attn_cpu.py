"""The KL-VAE's mid-block attention mode (mlctx_set_vae_attn / mlis_amd_vae_attn) without a GPU, on plans built in the dry runtime: unset == scores, record for record
(pointers as set / not set); the flash plan holds one attention op of d_head 512 over all its images, none of the four old launches, the same parameters, and at
latent 64 x 64 at least 6 T^2 bytes less device memory, less its fp16 v tensor; mlis_amd_vae_attn keeps both modes, refuses 2 and builds no engine."""
import ctypes as C

import pytest

LAT, NB, D = 64, 3, 512      # (3 images: no other block of the plan has the size of the score matrix -- the allocator hands a released block to the next allocation of exactly its size,
                             #  and at 1, 2 or 4 images the 2^26 and 2^25 bytes of S and P are also the size of later activations, which then move into them)
T = LAT * LAT
OLD = {"vae_attn_vT", "vae_attn_qk", "softmax_rows", "vae_attn_pv"}


@pytest.fixture(scope="module")
def E():
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield engine
    L.mlsd_runtime_dry(0)


def plan(E, which, mode):
    """(records, parameter list, device bytes) of the SD1.5 KL-VAE decoder / encoder plan of NB images at latent LAT x LAT; mode None: never set"""
    l, ctx, t, P = E._proto2(), E.MLCtx(), E.vp(), E.VaeParams()
    try:
        if mode is not None:
            E.set_vae_attn(ctx, mode)
        assert l.vae_params_get(b"sd1", C.byref(P)) == 1
        if which == "dec":
            assert l.sdvae_decode_init(ctx.h, C.byref(P), LAT, LAT, NB, C.byref(t)) == 1 and l.sdvae_decode_build(ctx.h, C.byref(P), t) == 1
        else:
            assert l.sdvae_encode_init(ctx.h, C.byref(P), 8 * LAT, 8 * LAT, NB, C.byref(t)) == 1 and l.sdvae_encode_build(ctx.h, C.byref(P), t) == 1
        flops = [f for _, f in ctx.op_list()]
        recs = [(kind, label, fused, once, gn, flops[i], [(n, bool(getattr(a, n)) if ty is E.vp else getattr(a, n)) for n, ty in a._fields_])
                for i, (kind, label, fused, once, gn, a) in enumerate(ctx.op_records())]
        return recs, ctx.param_list(), ctx.info().mem_compute, [a for kind, *_, a in ctx.op_records() if kind == "attn"]
    finally:
        ctx.destroy()


@pytest.mark.parametrize("which", ["dec", "enc"])
def test_plans(E, which):
    unset, scores, flash = plan(E, which, None), plan(E, which, 0), plan(E, which, 1)
    assert unset[:3] == scores[:3] and not scores[3]
    assert OLD <= {r[1] for r in scores[0]}
    assert not OLD & {r[1] for r in flash[0]}
    assert len(flash[3]) == 1                                   # one mid block per plan
    a = flash[3][0]
    assert (a.d_head, a.n_head, a.n_batch, a.Tq, a.Tk, a.causal) == (D, 1, NB, T, T, 0)
    assert (a.ldq, a.ldk, a.ldv, a.ldo, a.bsq, a.bso) == (D, D, D, D, T * D, T * D)
    assert flash[1] == scores[1]                                # the same parameters under the same names: a checkpoint loads into either
    saved = scores[2] - flash[2]
    print(f"{which}: scores plan {scores[2]} B, flash plan {flash[2]} B, {saved} B less (6 T^2 = {6 * T * T})")
    assert saved >= 6 * T * T - 2 * NB * T * D               # (the v tensor of all NB images against the one-image S, P and V^T of the scores plan)


def test_api_mode(E):
    from mlimgsynth_amd import mlimgsynth as M
    m = M.MLImgSynth()
    lib, ctx = m._lib, m._ctx
    assert m.vae_attn_info() == dict(mode="scores", plan_mode=None)
    for mode in ("flash", "scores", "flash"):
        m.vae_attn_set(mode)
        assert m.vae_attn_info()["mode"] == mode
    assert lib.mlis_amd_vae_attn(ctx, 2) == -4 and lib.mlis_amd_vae_attn(ctx, -1) == -4        # MLIS_E_OPT_VALUE
    with pytest.raises(ValueError):
        m.vae_attn_set("fast")
    assert m.vae_attn_info()["mode"] == "flash" and m.engine_builds() == 0
    assert callable(E.Generator.set_vae_attn)
