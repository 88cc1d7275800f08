"""Prompts longer than 75 tokens on the GPU: the cross-attention kernel over 77 x W context rows (mlsd_attention_ctx), the
windowed text conditioning, UNet plans built for a longer context, and whole generations through the public API."""
import ctypes

import numpy as np
import pytest

import mlis_ffi as F
import oracle_lib as O
import ref64 as R
import tolerances as T

pytestmark = pytest.mark.gpu


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def run_ctx(q, k, v, heads, dh):
    """q [nb][Tq][D], k / v [nb][Tk][D] as column slices of fused buffers with the plan's strides ([q | pad] and [k | v] rows) -> out [nb][Tq][D]"""
    from mlimgsynth_amd import _lib, kernels
    nb, tq, D = q.shape
    tk = k.shape[1]
    qb = np.zeros((nb, tq, D + 8), np.float16); qb[:, :, :D] = q
    kv = np.concatenate([k, v], axis=2).astype(np.float16)
    dq, dkv = _lib.from_numpy(qb), _lib.from_numpy(np.ascontiguousarray(kv))
    do = _lib.DeviceBuffer(nb * tq * D * 2)
    a = kernels.AttnArgs(q=dq.ptr, k=dkv.ptr, v=dkv.ptr + 2 * D, out=do.ptr, ldq=D + 8, ldk=2 * D, ldv=2 * D, ldo=D, bsq=tq * (D + 8),
                         bsk=tk * 2 * D, bsv=tk * 2 * D, bso=tq * D, n_batch=nb, n_head=heads, d_head=dh, Tq=tq, Tk=tk, causal=0)
    kernels.attention_ctx(a)
    return do.download((nb, tq, D), np.float16).astype(np.float32)


def oracle(q, k, v, heads):
    return np.stack([O.from_ot(O.L().orc_attention(O.to_ot(np.ascontiguousarray(q[i])[None, None]), O.to_ot(np.ascontiguousarray(k[i])[None, None]),
                                                    O.to_ot(np.ascontiguousarray(v[i])[None, None]), heads, 0)).reshape(q.shape[1], q.shape[2])
                     for i in range(q.shape[0])])


SHAPES = [(tk, dh, tq) for tk in (97, 154, 231, 308, 320) for dh, tq in ((40, 256), (64, 1000), (80, 64), (160, 256))] + \
         [(154, 64, 4096), (308, 40, 4096), (231, 160, 1000), (154, 32, 256)]


@pytest.mark.parametrize("tk,dh,tq", SHAPES)
def test_attention_ctx_against_the_oracle(tk, dh, tq):
    """Every key count of a windowed context (97 = one key past tk96's range, 77 W, 320 = the top) at every d_head; ragged Tq; several images and heads."""
    nb, heads = 2, 3 if dh != 160 else 2
    D = heads * dh
    rng = np.random.default_rng(tk * 1000 + dh + tq)
    q, k, v = (f16r(rng.standard_normal((nb, t, D))) for t in (tq, tk, tk))
    got = run_ctx(q, k, v, heads, dh)
    assert np.isfinite(got).all()
    assert rel(got, oracle(q, k, v, heads)) < 2e-3
    again = run_ctx(q, k, v, heads, dh)
    assert np.array_equal(got, again)                                             # bit-repeatable


def bad_operands(rng, heads, d, Tq, Tk, sigma, voff):
    """Q rows N(0, sigma^2) on dims 3..; dims 0..2 carry special rows of every head: row 1 peaked on a key of the LAST group only,
    row 2 all-equal scores (q = 0), row 3 sees the whole first group (keys 0..95) at -225 below the rest (it underflows), row Tq-2
    peaked on key 5 of the first group.  V plus a common offset voff."""
    D = heads * d
    q = np.zeros((Tq, heads, d)); k = rng.standard_normal((Tk, heads, d)); v = rng.standard_normal((Tk, heads, d)) + voff
    q[:, :, 3:] = rng.standard_normal((Tq, heads, d - 3)) * sigma * np.sqrt(d / (d - 3))
    k[:, :, :3] = 0
    s = np.sqrt(d) / 8.0
    q[1], q[2], q[3], q[Tq - 2] = 0, 0, 0, 0
    q[1, :, 0] = 8.0; k[Tk - 2, :, 0] = 20.0 * s                                 # the row maximum in the last key group only
    q[3, :, 1] = 30.0; k[0:96, :, 1] = -60.0 * s                                  # the first group 225 below the rest
    q[Tq - 2, :, 2] = 8.0; k[5, :, 2] = 20.0 * s                                  # an early peak: every later group is rescaled to it
    return tuple(f16r(a.reshape(a.shape[0], D)) for a in (q, k, v))


@pytest.mark.parametrize("dh", [40, 64, 80, 160])
@pytest.mark.parametrize("tk", [154, 308])
@pytest.mark.parametrize("sigma,voff", [(1.0, 0.0), (16.0, 0.0), (1.0, 100.0)])
def test_attention_ctx_against_float64_on_badly_conditioned_inputs(dh, tk, sigma, voff):
    """Per row against the float64 attention under ref64.attention_bound (its constants unchanged); the kernel rounds no scaled Q."""
    heads, tq, nb = 2, 200, 2
    rng = np.random.default_rng(dh * 7 + tk + int(sigma))
    ops = [bad_operands(rng, heads, dh, tq, tk, sigma, voff) for _ in range(nb)]
    q, k, v = (np.stack([o[i] for o in ops]) for i in range(3))
    got = run_ctx(q, k, v, heads, dh)
    for b in range(nb):
        o, p = R.attention64(q[b], k[b], v[b], heads)
        ratio = R.attention_worst(got[b], o, R.attention_bound(q[b], k[b], v[b], heads, o, p, False))
        bad = np.nonzero(ratio > 1.0)[0]
        assert bad.size == 0, (b, bad[:8].tolist(), float(ratio.max()))


# ------------------------------------------------------------------ text conditioning

@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
@pytest.mark.parametrize("n_tok", [120, 300])
def test_windowed_conditioning_is_the_windows_concatenated(model, n_tok):
    from mlimgsynth_amd import text
    rng = np.random.default_rng(n_tok)
    toks = rng.integers(5, 300, n_tok).astype(np.int32)
    w = (1.0 + 0.1 * rng.standard_normal(n_tok)).astype(np.float32)
    tc = text.TextConditioner(model, 64, 64, seed=1234)
    cond, label = tc.encode(toks, w)
    W = (n_tok + 74) // 75
    assert cond.shape == (77 * W, tc.n_ctx)
    for i in range(W):
        seg = toks[75 * i:75 * (i + 1)]
        ref, ref_label = tc.encode(seg)
        ref = ref.copy(); ref[1:1 + seg.size] *= w[75 * i:75 * i + seg.size, None]
        assert np.array_equal(cond[77 * i:77 * (i + 1)], ref), i                  # the plan's sequences are independent: same bits
        if i == 0 and label is not None:
            assert np.array_equal(label, ref_label)                               # the label from window 0, unweighted
    # a prompt of <= 75 tokens: today's single sequence, bit for bit
    c1, _ = tc.encode(toks[:75])
    c2, _, _, _ = tc.encode_pair(toks[:75], toks[:3])
    assert c1.shape == (77, tc.n_ctx) and np.array_equal(c1, c2)
    tc.destroy()


@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
def test_shorter_negative_prompt_is_padded_with_empty_windows(model):
    from mlimgsynth_amd import text
    rng = np.random.default_rng(5)
    toks = rng.integers(5, 300, 160).astype(np.int32)
    neg = rng.integers(5, 300, 10).astype(np.int32)
    tc = text.TextConditioner(model, 64, 64, seed=1234)
    cond, _, ncond, _ = tc.encode_pair(toks, neg)
    assert cond.shape == ncond.shape == (231, tc.n_ctx)
    empty, _ = tc.encode([])
    nref, _ = tc.encode(neg)
    assert np.array_equal(ncond[:77], nref)
    assert np.array_equal(ncond[77:154], empty) and np.array_equal(ncond[154:], empty)
    # the other way round: the prompt padded to the negative prompt's W
    cond2, _, ncond2, _ = tc.encode_pair(neg, toks)
    assert np.array_equal(cond2[:77], nref) and np.array_equal(cond2[77:154], empty)
    # an empty SDXL negative prompt: zeros over all 77 W rows
    _, _, nz, _ = tc.encode_pair(toks, [])
    if tc.n_label:
        assert nz.shape == (231, tc.n_ctx) and not nz.any()
    tc.destroy()


# ------------------------------------------------------------------ UNet plans with a longer context

@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
@pytest.mark.parametrize("W", [2, 4])
def test_unet_with_repeated_context_matches_the_77_row_plan(model, W):
    """Attention over the 77 context rows repeated W times is the attention over the 77 rows (every key appears W times in
    numerator and denominator): the W-window plan (mlsd_attention_ctx in every cross attention) evaluates to the 77-row plan's output."""
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(W)
    n, lw = 2, 8
    u1 = engine.Unet(model, lw, lw, n)
    uw = engine.Unet(model, lw, lw, n, n_ctx_tok=77 * W)
    x = rng.standard_normal((n, 4, lw, lw)).astype(np.float32)
    c = rng.standard_normal((n, 77, u1.P.n_ctx)).astype(np.float32)
    lab = rng.standard_normal((n, u1.P.ch_adm_in)).astype(np.float32) if u1.P.ch_adm_in else None
    sig = np.array([3.0, 0.7], np.float32)
    d1 = u1.run(x, c, lab, sig)
    dw = uw.run(x, np.concatenate([c] * W, axis=1), lab, sig)
    assert np.isfinite(dw).all()
    assert rel(dw, d1) < T.EVAL_SMALL
    assert np.array_equal(dw, uw.run(x, np.concatenate([c] * W, axis=1), lab, sig))


def test_generator_with_a_longer_context_under_hipgraph_is_bit_identical():
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(11)
    out = []
    for hg in (False, True):
        g = engine.Generator("tiny", 64, 64, 1, n_step=3, cfg_scale=7.0, use_hipgraph=hg, n_ctx_tok=154)
        if hg is False:
            cond = rng.standard_normal((154, g.P.n_ctx)).astype(np.float32) * 0.5
            ncond = rng.standard_normal((154, g.P.n_ctx)).astype(np.float32) * 0.5
        g.set_cond(cond, None, ncond, None)
        lat, _ = g.generate([7], want_images=False)
        g.destroy()
        out.append(lat)
    assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])


# ------------------------------------------------------------------ public API

@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return F.bind(_lib.LIB_PATH)


def setup(m, toks, neg):
    m.set("model", "synth:tiny")
    m.set("image_dim", 64, 64)
    m.set("steps", 4)
    m.set("method", "euler")
    m.set("seed", 42)
    m.set("cfg_scale", 7.0)
    m.tokens(toks)
    m.tokens(neg, negative=True)


def test_generate_with_a_120_token_prompt(lib):
    from mlimgsynth_amd import engine, text
    rng = np.random.default_rng(21)
    toks = rng.integers(5, 300, 120).astype(np.int32)
    neg = rng.integers(5, 300, 10).astype(np.int32)
    m = F.Mlis(lib)
    setup(m, toks, neg)
    m.generate()
    cond = m.tensor(F.TENSOR["COND"])
    assert cond.shape[-2:] == (154, 64) or cond.reshape(-1).size == 154 * 64
    lat = m.tensor(F.TENSOR["LATENT"])
    assert np.isfinite(lat).all()
    assert m.image(0).shape == (64, 64, 3)
    # the same generation through the engine classes with the concatenated conditioning
    tc = text.TextConditioner("tiny", 64, 64, seed=1234)
    c, _, nc, _ = tc.encode_pair(toks, neg)
    tc.destroy()
    g = engine.Generator("tiny", 64, 64, 1, n_step=4, cfg_scale=7.0, s_ancestral=0.0, n_ctx_tok=154)
    g.set_cond(c, None, nc, None)
    ref, _ = g.generate([42], want_images=False)
    g.destroy()
    assert rel(lat.reshape(ref.shape), ref) < T.LATENT
    m.close()


def test_user_conditioning_of_154_rows_and_a_length_mismatch(lib):
    rng = np.random.default_rng(22)
    m = F.Mlis(lib)
    setup(m, np.array([5, 6], np.int32), np.array([7], np.int32))
    m.generate()
    n_ctx = m.tensor(F.TENSOR["COND"]).size // 77

    def user_cond(rows_c, rows_n):
        for tid, rows in (("COND", rows_c), ("NCOND", rows_n)):
            tp = lib.mlis_tensor_get(m.ctx, F.TENSOR[tid])
            lib.mlis_tensor_resize(tp, n_ctx, rows, 1, 1)
            np.ctypeslib.as_array(tp.contents.d, shape=(rows * n_ctx,))[:] = rng.standard_normal(rows * n_ctx).astype(np.float32) * 0.3
        m.set("tensor_use_flags", F.TUF["CONDITIONING"])

    user_cond(154, 154)
    m.generate()
    assert np.isfinite(m.tensor(F.TENSOR["LATENT"])).all()
    user_cond(154, 231)
    assert lib.mlis_generate(m.ctx) < 0 and "differ" in m.err()
    m.close()


# ------------------------------------------------------------------ against the oracle

def orc_clip(tower, prefix, tk, skip, norm, feat=False):
    K = O.clip_params(tower)
    P = O.Params(1234)
    full = np.full(K.n_token, K.tok_pad, np.int32)
    full[0] = K.tok_start
    full[1:1 + len(tk)] = tk
    full[1 + len(tk)] = K.tok_end
    ptr = full.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    r = O.from_ot(O.L().orc_clip_text_encode(P.h, prefix.encode(), K, ptr, skip, int(norm), int(feat), len(tk) + 1 if feat else 0))
    P.free()
    return r.reshape(K.d_embed) if feat else r.reshape(K.n_token, K.d_embed)


@pytest.mark.parametrize("model,n_tok", [("tiny", 150), ("tinyxl", 300), ("sd1", 120)])
def test_windowed_conditioning_against_orc_clip_text_encode(model, n_tok):
    """every window against the oracle's encoding of that window (BOS, its tokens, EOS, padding), weights on rows 1..n_w; the SDXL label from window 0"""
    from mlimgsynth_amd import text
    tower = "vit_l" if model == "sd1" else "tiny"
    K = O.clip_params(tower)
    rng = np.random.default_rng(n_tok)
    toks = rng.integers(0, K.n_vocab - 3, n_tok).astype(np.int32)
    w = (1.0 + 0.1 * rng.standard_normal(n_tok)).astype(np.float32)
    tc = text.TextConditioner(model, 64, 64, seed=1234)
    cond, label = tc.encode(toks, w)
    for i in range((n_tok + 74) // 75):
        seg, ws = toks[75 * i:75 * (i + 1)], w[75 * i:75 * (i + 1)]
        c = cond[77 * i:77 * (i + 1)]
        if model == "tinyxl":
            ref = np.concatenate([orc_clip(tower, "clip", seg, 2, False), orc_clip(tower, "clip2", seg, 2, False)], axis=1)
        else:
            ref = orc_clip(tower, "clip", seg, 1, True)
        ref[1:1 + seg.size] *= ws[:, None]
        assert rel(c, ref) < T.EVAL, i
    if model == "tinyxl":
        assert rel(label[:64], orc_clip(tower, "clip2", toks[:75], -1, True, True)) < T.EVAL
    tc.destroy()


def orc_unet(model, x, cond, label, sigma):
    U = O.unet_params(model)
    P = O.Params(1234)
    outs = []
    for i in range(x.shape[0]):
        lab = O.to_ot(label[i][None, None, None]) if label is not None else None
        outs.append(O.from_ot(O.L().orc_unet_denoise_run(P.h, b"unet", U, O.to_ot(x[i:i + 1]), O.to_ot(cond[i][None, None]), lab, float(sigma[i])))[0])
    P.free()
    return np.stack(outs)


@pytest.mark.parametrize("model,lat,n,W,tol", [("tiny", 8, 2, 2, "EVAL_SMALL"), ("tinyxl", 8, 2, 4, "EVAL_SMALL"), ("tiny", 8, 1, 3, "EVAL_SMALL"),
                                               ("sd1", 64, 1, 2, "EVAL_HEADLINE"), ("sdxl", 128, 1, 2, "EVAL_HEADLINE")])
def test_unet_with_a_windowed_context_against_orc_unet_denoise_run(model, lat, n, W, tol):
    """distinct rows in every window (a misplaced window changes the result); SD1.5 at 64x64 runs mlsd_attention_ctx at d 40 / 80 / 160,
    SDXL at 128x128 the tile loop at d 64 with the batched K / V projection"""
    from mlimgsynth_amd import engine
    O.L().orc_set_threads(O.host_threads())
    rng = np.random.default_rng(W * 10 + lat)
    u = engine.Unet(model, lat, lat, n, n_ctx_tok=77 * W)
    P = u.P
    x = rng.standard_normal((n, 4, lat, lat)).astype(np.float32) * 3
    c = rng.standard_normal((n, 77 * W, P.n_ctx)).astype(np.float32)
    lab = rng.standard_normal((n, P.ch_adm_in)).astype(np.float32) if P.ch_adm_in else None
    sig = np.array([2.5, 0.8][:n], np.float32)
    u.run(x, c, lab, sig)
    got = u.run(x, c, lab, sig)
    ref = orc_unet(model, x, c, lab, sig)
    assert np.isfinite(got).all()
    for i in range(n):
        assert rel(got[i], ref[i]) < getattr(T, tol), i
    u.ctx.destroy()


def test_generation_with_a_154_row_context_against_orc_sample_ex():
    from mlimgsynth_amd import engine
    U = O.unet_params("tiny")
    rng = np.random.default_rng(31)
    cond = rng.standard_normal((154, U.n_ctx)).astype(np.float32)
    uncond = rng.standard_normal((154, U.n_ctx)).astype(np.float32)
    g = engine.Generator("tiny", 64, 64, 1, n_step=6, cfg_scale=7.0, s_ancestral=1.0, n_ctx_tok=154)
    g.set_cond(cond, None, uncond, None)
    got, _ = g.generate([13], want_images=False)
    g.destroy()
    P = O.Params(1234)
    opts = O.SampleOpts(1, 1, 6, 7.0, 1.0, 0.0, 1.0, 0.0)
    out = np.empty((4, 8, 8), np.float32)
    O.L().orc_sample_ex(P.h, b"unet", U, 8, 8, O.to_ot(cond[None, None]), None, O.to_ot(uncond[None, None]), None, ctypes.byref(opts), 13, 0,
                        None, None, O.fptr(out))
    P.free()
    assert np.isfinite(got).all() and rel(got[0], out) < T.LATENT


def test_textcond_apply_sizes_the_conditioning_from_the_engine():
    """mlis_amd_textcond_apply (launchers, multi-GPU rank 0): a 120-token prompt into an engine built for 154 rows gives the engine
    exactly the windowed encoding; an engine built for 77 rows is an error, not a short copy"""
    from mlimgsynth_amd import engine, text, _lib
    rng = np.random.default_rng(41)
    toks = rng.integers(5, 300, 120).astype(np.int32)
    neg = rng.integers(5, 300, 10).astype(np.int32)
    tc = text.TextConditioner("tiny", 64, 64, seed=1234)
    l = tc._l
    I32P = ctypes.POINTER(ctypes.c_int32)
    l.mlis_amd_textcond_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p, I32P, ctypes.c_int, I32P, ctypes.c_int]
    lats = []
    for how in ("apply", "set_cond"):
        g = engine.Generator("tiny", 64, 64, 1, n_step=3, cfg_scale=7.0, n_ctx_tok=154)
        if how == "apply":
            assert l.mlis_amd_textcond_apply(tc.h, g.h, toks.ctypes.data_as(I32P), toks.size, neg.ctypes.data_as(I32P), neg.size) > 0
        else:
            c, _, nc, _ = tc.encode_pair(toks, neg)
            g.set_cond(c, None, nc, None)
        lats.append(g.generate([5], want_images=False)[0])
        g.destroy()
    assert np.array_equal(lats[0], lats[1])
    g = engine.Generator("tiny", 64, 64, 1, n_step=3, cfg_scale=7.0)
    assert l.mlis_amd_textcond_apply(tc.h, g.h, toks.ctypes.data_as(I32P), toks.size, neg.ctypes.data_as(I32P), neg.size) < 0
    assert "154" in _lib.last_error()
    g.destroy()
    tc.destroy()


def test_cli_generates_from_a_120_token_prompt(tmp_path):
    from test_cli import png_pixels, run
    out = str(tmp_path / "long.png")
    ids = ",".join(str(5 + (7 * i) % 290) for i in range(120))
    r = run("generate", "-m", "synth:tiny", "-d", "64,64", "-s", "3", "-S", "42", "--tokens", ids, "--ntokens", "9,9,8", "-o", out)
    assert "Saved" in r.stderr
    px, _ = png_pixels(open(out, "rb").read())
    assert px.shape == (64, 64, 3)
