"""The d = 512 flash attention (mlsd_attention_wide, csrc/hip/attention_wide.hip) and the KL-VAE plans that launch it (vae_attn flash).

Kernel: every output row against float64 (tests/ref64.py, one head of 512) at the bound of every other attention kernel; the scale goes into the fp32 exp2 argument, no
scaled Q is rounded: q_scaled_f16 False.  Shapes (n_batch, T): one token; fewer keys than a 32-key tile; one tile, two images; a 128-row query block plus one row; three
images with slack between them and ldo > 512; several blocks with a tail on both axes.  Inputs: attn64_cases' sigma1 (Gaussian plus its peaked, all-equal and -225 rows)
and sigma16 (logits of tens); at T = 1, below what those builders take, plain Gaussian rows.  Guard rows (and columns, at ldo > 512) of sentinel bytes must stay.
Plans: the test-size KL-VAE "tinyw" (mid block 64 x 8 = 512 wide) through Generator(vae_attn="flash"), untiled at a 12 x 12 latent (T = 144) and with vae_tile 64 on
an 8 x 32 latent (tiles of 8 x 24), decode and encode, against the oracle under tolerances.EVAL as tests/test_vae_tile_gpu.py holds the scores path.
"""
import ctypes

import numpy as np
import pytest

import attn64_cases as AC
import ref64 as R64
import tolerances as TOL
import vae_tile_ref as VR

pytestmark = pytest.mark.gpu
D = 512
SHAPES = [(1, 1, "packed"), (1, 31, "packed"), (2, 32, "packed"), (1, 129, "packed"), (3, 200, "padded_out"), (1, 1056, "packed")]
FAMILIES = ("sigma1", "sigma16")


def case_of(nb, T, layout, family):
    return dict(id=f"wide_b{nb}_t{T}_{family}", nb=nb, heads=1, d=D, Tq=T, Tk=T, causal=0, layout=layout, family=family, late=max(T - 3, 0), sw={})


def operands(c):
    if c["Tq"] >= 6:
        return AC.make_operands(c)
    rng = np.random.default_rng(c["Tq"])
    return tuple(AC.f16r(rng.standard_normal((c["nb"], c["Tq"], D))) for _ in range(3))


def launch(c, q, k, v, args_edit=None):
    """-> (raw output buffer [nb][T + guards][ldo] as uint16, error or None)"""
    from mlimgsynth_amd import kernels, _lib
    lay = AC.layout(c)
    dev = {n: _lib.from_numpy(a) for n, a in AC.host_buffers(c, q, k, v).items()}
    dev["o"] = _lib.DeviceBuffer(lay["bufs"]["o"] * 2)
    _lib.check(_lib.lib().mlsd_memset(_lib.vp(dev["o"].ptr), AC.SENTINEL, ctypes.c_size_t(dev["o"].nbytes), None))
    a = AC.attn_args(kernels, c, {n: b.ptr for n, b in dev.items()})
    for name, val in (args_edit or {}).items():
        setattr(a, name, val)
    err = None
    try:
        kernels.attention_wide(a)
    except _lib.MlsdError as e:     # (a refusal: reported by the caller)
        err = e
    kernels.sync()
    return dev["o"].download((c["nb"], c["Tq"] + 2 * AC.GUARD_ROWS, lay["ldo"]), np.float16).view(np.uint16), err


KERNEL_CASES = [(nb, T, lay, fam) for nb, T, lay in SHAPES for fam in FAMILIES if T >= 6 or fam == FAMILIES[0]]      # (one token: Gaussian only)


@pytest.mark.parametrize("nb,T,layout,family", KERNEL_CASES, ids=[f"b{nb}_t{T}_{fam}" for nb, T, _, fam in KERNEL_CASES])
def test_kernel_against_float64(nb, T, layout, family):
    c = case_of(nb, T, layout, family)
    q, k, v = operands(c)
    raw, err = launch(c, q, k, v)
    assert err is None, err
    guard = raw != (AC.SENTINEL << 8 | AC.SENTINEL)
    guard[:, AC.GUARD_ROWS:AC.GUARD_ROWS + T, :D] = False
    assert not guard.any(), f"stored outside its rows / columns at (batch, buffer row, column) {np.argwhere(guard)[:4].tolist()}"
    got = raw.view(np.float16)[:, AC.GUARD_ROWS:AC.GUARD_ROWS + T, :D].astype(np.float64)
    worst = 0.0
    for b in range(nb):
        o, p = R64.attention64(q[b], k[b], v[b], 1)
        ratio = R64.attention_worst(got[b], o, R64.attention_bound(q[b], k[b], v[b], 1, o, p, False))
        print(f"{c['id']} image {b}: worst row ratio {ratio.max():.3f} at row {int(np.argmax(ratio))}")
        worst = max(worst, float(ratio.max())) if np.isfinite(ratio).all() else np.inf
    assert worst <= 1.0
    if (nb, T) == (3, 200):
        again, _ = launch(c, q, k, v)
        assert again.tobytes() == raw.tobytes(), "two launches on the same input differ"


@pytest.mark.parametrize("edit", [dict(d_head=256), dict(n_head=2), dict(causal=1)], ids=["d256", "heads2", "causal"])
def test_refusals(edit):
    from mlimgsynth_amd import kernels
    c = case_of(2, 32, "packed", "sigma1")
    raw, err = launch(c, *operands(c), args_edit=edit)
    assert err is not None and "mlsd_attention_wide" in str(err)
    assert (raw == (AC.SENTINEL << 8 | AC.SENTINEL)).all(), "a refused launch wrote to its output"
    assert kernels.attention_wide_variant(AC.attn_args(kernels, c, {n: 256 for n in ("q", "k", "v", "o")})) == "attn<wide,d512>"


# ------------------------------------------------------------------ the plans
def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-30)


@pytest.fixture(scope="module")
def orc():
    o = VR.Oracle("tiny")
    o.V.ch_mult[3] = 8          # vae_params_get("tinyw"): tiny's KL-VAE with the mid block 64 x 8 = 512 wide
    return o


@pytest.mark.parametrize("lw,lh,tile_px,B", [(12, 12, 0, 2), (8, 32, 64, 1)], ids=["untiled", "vae_tile64"])
def test_decode_and_encode(orc, lw, lh, tile_px, B):
    from mlimgsynth_amd import engine as E
    z = (np.random.default_rng(1000 * lw + lh).standard_normal((B, 4, lh, lw)) * 0.5).astype(np.float32)
    src = np.random.default_rng(77 * lw + lh).random((B, 3, 8 * lh, 8 * lw)).astype(np.float32)
    g = E.Generator("tinyw", 8 * lw, 8 * lh, B, n_step=2, vae_attn="flash")
    try:
        assert g.vae_attn() == "flash"
        g.set_vae_tile(tile_px)
        g.set_init_latent(z)
        g.decode()
        img = g.image()
        mean = g.encode(src, sample=False)
        # the plan that ran holds the flash launch, over all its images, and no score matrix op
        ctx = g.ctx_at(3 if tile_px else 1)
        attn = [(a.d_head, a.n_batch, a.Tq) for kind, *_, a in ctx.op_records() if kind == "attn"]
        assert attn == [(D, 1 if tile_px else B, 8 * 24 if tile_px else lw * lh)] and "softmax_rows" not in [lab for lab, _ in ctx.op_list()]
    finally:
        g.destroy()
    assert np.isfinite(img).all() and np.isfinite(mean).all()
    if tile_px:
        ref, pwins, _ = VR.decode_ref(orc, z, tile_px)
        mom, mwins, _ = VR.encode_moments_ref(orc, src, tile_px)
    else:
        ref, pwins = np.stack([orc.decode(z[b]) for b in range(B)]), [((0, 8 * lw), (0, 8 * lh))]
        mom, mwins = np.stack([orc.moments(src[b]) for b in range(B)]), [((0, lw), (0, lh))]
    for what, got, want, wins in (("decode", img - 0.5, ref - 0.5, pwins), ("encode", mean, VR.latent_sample(orc, mom), mwins)):
        for (x0, x1), (y0, y1) in wins:             # every paste window by itself, as test_vae_tile_gpu.py
            for b in range(B):
                e = rel(got[b, :, y0:y1, x0:x1], want[b, :, y0:y1, x0:x1])
                print(f"{what} image {b} window x {x0}:{x1} y {y0}:{y1}: rel-L2 {e:.3e}")
                assert e < TOL.EVAL
