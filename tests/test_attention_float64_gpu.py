"""Every attention kernel the plans launch against a float64 reference, per output row (tests/ref64.py: attention64 and attention_bound with
C_ATTN; tests/attn64_cases.py: the cases, their input families and operand layouts).

Each case asserts the label mlsd_attention_variant gives it, then launches into an output with guard rows (and, for ldo > D, guard columns)
of 0x7C bytes, which must all be intact afterwards, and holds every output row to max |got - ref64| / (half_ulp16 + bound) <= 1.  With -s the
worst ratio of every case and, at the end, of every kernel family is printed.

The census at the end builds the bench plans (without computing them) and checks that every attention launch they record has a case here.
"""
import ctypes

import numpy as np
import pytest

import attn64_cases as AC
import ref64 as R

pytestmark = pytest.mark.gpu

WORST = {}       # kernel family -> worst row ratio


@pytest.fixture(scope="module")
def K():
    from mlimgsynth_amd import kernels, _lib
    yield kernels, _lib
    if WORST:
        print("\nfloat64 attention bound, worst row ratio per kernel family:")
        for p, w in sorted(WORST.items()):
            print(f"  {p:16s} {w:7.3f}")


@pytest.mark.parametrize("case", AC.CASES, ids=[c["id"] for c in AC.CASES])
def test_attention_float64(K, case):
    kernels, _lib = K
    L = _lib.lib()
    c = case
    nb, heads, Tq, D = c["nb"], c["heads"], c["Tq"], c["heads"] * c["d"]
    q, k, v = AC.make_operands(c)
    lay = AC.layout(c)
    dev = {n: _lib.from_numpy(a) for n, a in AC.host_buffers(c, q, k, v).items()}
    dev["o"] = _lib.DeviceBuffer(lay["bufs"]["o"] * 2)
    _lib.check(L.mlsd_memset(_lib.vp(dev["o"].ptr), AC.SENTINEL, ctypes.c_size_t(dev["o"].nbytes), None))
    a = AC.attn_args(kernels, c, {n: b.ptr for n, b in dev.items()})
    try:
        AC.apply_switches(L, c["sw"])
        label = kernels.attention_variant(a)
        assert label == c["variant"], f"{c['id']}: launch label {label}, case written for {c['variant']}"
        kernels.attention(a)
        kernels.sync()
    finally:
        AC.restore_switches(L)
    raw = dev["o"].download((nb, Tq + 2 * AC.GUARD_ROWS, lay["ldo"]), np.float16)
    guard = raw.view(np.uint16) != (AC.SENTINEL << 8 | AC.SENTINEL)
    guard[:, AC.GUARD_ROWS:AC.GUARD_ROWS + Tq, :D] = False
    assert not guard.any(), f"{c['id']} ({label}): stored outside its rows / columns at (batch, buffer row, column) {np.argwhere(guard)[:4].tolist()}"
    got = raw[:, AC.GUARD_ROWS:AC.GUARD_ROWS + Tq, :D].astype(np.float64)
    worst, at = 0.0, None
    for b in range(nb):
        o, p = R.attention64(q[b], k[b], v[b], heads, bool(c["causal"]))
        ratio = R.attention_worst(got[b], o, R.attention_bound(q[b], k[b], v[b], heads, o, p, c["q_scaled"]))
        if not ratio.max() <= worst:
            worst, at = float(ratio.max()), (b, int(np.argmax(ratio)))
    WORST[c["path"]] = max(WORST.get(c["path"], 0.0), worst)
    print(f"{c['id']:36s} {label:24s} worst row ratio {worst:7.3f}")
    assert worst <= 1.0, f"{c['id']} ({label}): ratio {worst:.3g} > 1 at (batch, row) {at}"


# ------------------------------------------------------------------ census
MLB_F_OPSHAPES = 16
COVERED_ELSEWHERE = {"attn<ctx,": "test_long_prompt_gpu.py::test_attention_ctx_against_float64_on_badly_conditioned_inputs"}


# what the plans are known to launch: a plan builder that stopped recording the attention of one model must not pass as "nothing to cover"
PLANNED = {("sd1 unet", "attn<tile,d80>"), ("sd1 unet", "attn<tile,d160>"), ("sd1 unet", "attn<tk96,d40>"), ("sd1 unet", "attn<tk96,d80>"),
           ("sd1 unet", "attn<tk96,d160>"), ("sd1 unet", "attn<64x2s,d40>"), ("sdxl unet", "attn<64x2s,d64>"),
           ("sd1 text", "attn<tile,d64,causal>"), ("sdxl text", "attn<tile,d64,causal>"), ("sdxl text 2", "attn<tile,d64,causal>")}


def planned(ctx, what, out):
    from mlimgsynth_amd import _lib, kernels
    L = _lib.lib()
    L.mlctx_op_attn_args.restype = ctypes.POINTER(kernels.AttnArgs)
    L.mlctx_op_attn_args.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.mlctx_op_attn_is_ctx.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for i in range(ctx.info().n_ops):
        p = L.mlctx_op_attn_args(ctx.h, i)
        if p:
            a = kernels.AttnArgs.from_buffer_copy(p.contents)
            label = kernels.attention_variant(a, ctx=bool(L.mlctx_op_attn_is_ctx(ctx.h, i)))
            assert label is not None, (what, i)
            out.add((what, label))


def plan_labels():
    """(plan, label) of every attention launch of the SD1.5 64x64 N = 2 and SDXL 128x128 N = 8 UNet plans, the two models' text encoders and
    their KL-VAE decoders (whose mid-block attention runs as GEMM + softmax + GEMM: no attention launch is expected there)"""
    from mlimgsynth_amd import engine, text
    out = set()
    for model, lat, n, dn in (("sd1", 64, 2, 1), ("sdxl", 128, 8, 4)):
        un = engine.Unet(model, lat, lat, n, synth=False, flags=MLB_F_OPSHAPES)
        planned(un.ctx, model + " unet", out)
        un.ctx.destroy()
        l = engine._proto2()
        ctx, t_lat, P = engine.MLCtx(flags=MLB_F_OPSHAPES), engine.vp(), engine.VaeParams()
        assert l.vae_params_get(model.encode(), ctypes.byref(P)) == 1
        assert l.sdvae_decode_init(ctx.h, ctypes.byref(P), lat, lat, dn, ctypes.byref(t_lat)) == 1
        assert l.sdvae_decode_build(ctx.h, ctypes.byref(P), t_lat) == 1
        planned(ctx, model + " vae", out)
        ctx.destroy()
    # the towers as csrc/host/textcond.c builds them: two prompts (prompt + negative prompt) per run
    for what, tower, skip, norm, feat in (("sd1 text", "vit_l", 1, True, False), ("sdxl text", "vit_l", 2, False, False), ("sdxl text 2", "vit_bigg", 1, True, True)):
        P, ctx, E = engine.ClipParams(), engine.MLCtx(), text.ClipEncoderS()
        assert text._l().clip_params_get(tower.encode(), ctypes.byref(P)) == 1
        assert text._l().clip_encoder_init(ctypes.byref(E), ctx.h, ctypes.byref(P), b"clip", 2, skip, norm, feat) == 1
        planned(ctx, what, out)
        text._l().clip_encoder_free(ctypes.byref(E))
        ctx.destroy()
    return out


def test_every_planned_attention_launch_has_a_float64_case(K):
    """every kernel instantiation the plans launch needs a case in attn64_cases.py; only the Tk > 96 family is covered elsewhere"""
    have = {c["variant"] for c in AC.CASES}
    seen = plan_labels()
    print("\nplanned attention launches:", sorted(seen))
    assert PLANNED <= seen, f"attention launches the plans are known to record, now missing: {sorted(PLANNED - seen)}"
    missing = sorted((w, lab) for w, lab in seen if lab not in have and not any(lab.startswith(p) for p in COVERED_ELSEWHERE))
    assert not missing, f"attention launches of the plans without a float64 case: {missing}"
