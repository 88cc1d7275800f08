"""Token merging on the GPU (csrc/hip/tome.hip; the rule: include/mlsd_kernels.h) against tests/tome_ref.py.  match: the float64 cosine of
the chosen destination and score both lie within that element's bound (tome_ref.cosine64, from ref64) of the float64 maximum.
select: the lists exactly, score and best GIVEN.  merge: one fp16 rounding of an fp32 mean (tome_ref.merge_bound).  unmerge: numpy's fp32 sum, bit for bit."""
import ctypes

import numpy as np
import pytest

import tome_ref as TR
from mlimgsynth_amd import _lib
from mlimgsynth_amd._lib import from_numpy as dev

pytestmark = pytest.mark.gpu

MAPS = [(1, 8, 8, 64), (2, 16, 16, 320), (1, 12, 20, 640), (1, 9, 7, 64), (1, 32, 32, 1280)]
IDS = ["x".join(map(str, c)) for c in MAPS]


def peek(addr, shape, dtype):
    out = np.empty(shape, dtype)
    _lib.check(_lib.lib().mlsd_device_sync(), "sync")
    _lib.check(_lib.lib().mlsd_memcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(addr), ctypes.c_size_t(out.nbytes), 1, None), "memcpy d2h")
    _lib.check(_lib.lib().mlsd_device_sync(), "sync")
    return out


def rows16(n_img, H, W, C, seed):
    return np.random.default_rng(seed).standard_normal((n_img, H * W, C)).astype(np.float16)


def run_match(n, H, W):
    from mlimgsynth_amd import kernels as K
    n_img, T, C = n.shape
    Ns = T - (H // 2) * (W // 2)
    dn, db, ds = dev(n), dev(np.full((n_img, Ns), -7, np.int32)), dev(np.full((n_img, Ns), np.nan, np.float32))
    K.tome_match(dn.ptr, C, n_img, H, W, C, db.ptr, ds.ptr)
    K.sync()
    return db.download((n_img, Ns), np.int32), ds.download((n_img, Ns), np.float32)


def check_match(n, H, W, best, score):
    for img in range(n.shape[0]):
        s, b = TR.cosine64(n[img], H, W)
        assert ((best[img] >= 0) & (best[img] < s.shape[1])).all()
        i = np.arange(s.shape[0])
        bound, gap, err = b[i, best[img]], s.max(1) - s[i, best[img]], np.abs(score[img].astype(np.float64) - s.max(1))
        print(f"image {img}: chosen below the maximum by {gap.max():.3g}, score off by {err.max():.3g}, smallest non-zero bound {bound[bound > 0].min():.3g}")
        assert (gap <= bound).all() and (err <= bound).all()


@pytest.mark.parametrize("n_img,H,W,C", MAPS, ids=IDS)
def test_match_against_float64(n_img, H, W, C):
    n = rows16(n_img, H, W, C, H * 100 + W)
    best, score = run_match(n, H, W)
    check_match(n, H, W, best, score)
    again = run_match(n, H, W)
    assert again[0].tobytes() == best.tobytes() and again[1].tobytes() == score.tobytes()


def test_match_exact_ties_and_a_zero_row():
    H, W, C = 12, 20, 64
    (src, dst), n = TR.partition(H, W), rows16(1, H, W, C, 5)
    n[0, dst] = n[0, dst[0]]                     # all destinations equal: every score of a row is the same value
    n[0, src[3]] = 0                             # a zero norm: score 0
    best, score = run_match(n, H, W)
    assert (best == 0).all() and score[0, 3] == 0.0
    check_match(n, H, W, best, score)


def given_scores(kind, n_img, Ns, Nd, seed):
    rng = np.random.default_rng(seed)
    score = rng.uniform(-1, 1, (n_img, Ns)).astype(np.float32)
    if kind.startswith("ties"):
        score = np.round(score * 4) / 4          # nine distinct values: the r-th largest is a long run of equals
    if kind == "nan":
        score[:, Ns // 3] = np.nan
        score[:, 1] = -np.nan
    return score, rng.integers(0, Nd, (n_img, Ns)).astype(np.int32)


@pytest.mark.parametrize("kind", ["random", "ties", "nan", "ties-global"])
@pytest.mark.parametrize("n_img,H,W,C", MAPS, ids=IDS)
def test_select_merge_unmerge(n_img, H, W, C, kind):
    from mlimgsynth_amd import kernels as K
    T, Nd, Ns = H * W, (H // 2) * (W // 2), H * W - (H // 2) * (W // 2)
    score, best = given_scores(kind, n_img, Ns, Nd, T + C)
    n = rows16(n_img, H, W, C, T)
    rng = np.random.default_rng(T)
    x = rng.standard_normal((n_img, T, C)).astype(np.float32)
    dn, dsc, dbe, dx = dev(n), dev(score), dev(best), dev(x)
    was = K.tome_select_lds_limit(0 if kind == "ties-global" else -1)      # (0: the keys are formed again from global memory in every pass)
    try:
        for r in (0, 16, Ns // 16 * 16):
            per, Tm = K.tome_lists_ints(H, W, r), T - r
            dl, dm = dev(np.full((n_img, per), -9, np.int32)), dev(np.full((n_img, Tm, C), np.nan, np.float16))
            o = rng.standard_normal((n_img, Tm, C)).astype(np.float32)
            do, dy = dev(o), dev(np.full((n_img, T, C), np.nan, np.float32))
            K.tome_select(dsc.ptr, dbe.ptr, n_img, H, W, r, dl.ptr)
            K.tome_merge(dn.ptr, C, n_img, H, W, C, r, dl.ptr, dm.ptr)
            K.tome_unmerge_add(dx.ptr, C, do.ptr, C, n_img, H, W, C, r, dl.ptr, dy.ptr, C)
            K.sync()
            lists, m, y = dl.download((n_img, per), np.int32), dm.download((n_img, Tm, C), np.float16), dy.download((n_img, T, C), np.float32)
            for img in range(n_img):
                want = TR.select(score[img], best[img], H, W, r)
                got = TR.split_lists(lists[img], H, W, r)
                for k in want:
                    assert got[k].tobytes() == want[k].tobytes(), (r, img, k)
                w64, terms = TR.merge64(n[img], want, H, W)
                ratio = np.abs(m[img].astype(np.float64) - w64) / np.maximum(TR.merge_bound(w64, n[img], want, H, W, terms), 1e-300)
                assert np.isfinite(m[img]).all() and ratio.max() <= 1, (r, img, ratio.max())
                assert m[img, :Ns - r].tobytes() == n[img, want["kept"]].tobytes()                     # kept rows are copies
                assert y[img].tobytes() == TR.unmerge32(x[img], o[img], want["slot"]).tobytes()
    finally:
        K.tome_select_lds_limit(was)


# ------------------------------------------------------------------ in the plan
LW, LH, N = 24, 16, 2            # tinyxl: transformers at downscale 2, a map of 12 x 8 = 96 tokens of 128 channels; the middle block sits at the same downscale


def unet(**kw):
    from mlimgsynth_amd import engine as E
    u = E.Unet("tinyxl", LW, LH, N, flags=E.MLB_F_KEEP, **kw)
    rng = np.random.default_rng(11)
    x, cond, label = (rng.standard_normal(sh).astype(np.float32) for sh in ((N, 4, LH, LW), (N, 77, u.P.n_ctx), (N, u.P.ch_adm_in)))
    return u, (x, cond, label, np.full(N, 2.5, np.float32))


self_attention_lengths = lambda u: [(a.Tq, a.Tk) for kind, _, _, _, _, a in u.ctx.op_records() if kind == "attn" and a.Tq == a.Tk]
# every other attention of a plan: the launches of its own, and the cross attentions that end their q projection's launch
other_attention = lambda u: [(k, a.n_batch, a.Tq, a.Tk) if k != "gemm" else (k, a.M, a.xa_Tq, a.xa_Tk) for k, _, _, _, _, a in u.ctx.op_records()
                             if (k in ("attn", "attn_ctx") and a.Tq != a.Tk) or (k == "gemm" and a.xa_k)]


def test_in_the_plan():
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    H, W, C, T = LH // 2, LW // 2, 128, (LH // 2) * (LW // 2)
    Ns, r = T - (H // 2) * (W // 2), TR.r_of(H, W, 0.5)
    assert T >= 64 and r == 48
    u, inp = unet(tome=0.5)
    try:
        assert E.tome_info(u.ctx) == (0.5, 2, 10, [(0, 0, 0), (T, r, T - r), (0, 0, 0), (0, 0, 0)])
        assert self_attention_lengths(u) == [(T - r,) * 2] * 4 + [(T,) * 2] * 2 + [(T - r,) * 2] * 6      # encoder, the middle block as it was, decoder
        others, out = other_attention(u), u.run(*inp)
        assert np.isfinite(out).all() and u.run(*inp).tobytes() == out.tobytes()
        ops = [a for kind, _, _, _, _, a in u.ctx.op_records() if kind == "copy" and a.tome]
        assert [a.tome for a in ops] == [K.TOME_MATCH, K.TOME_SELECT, K.TOME_MERGE, K.TOME_UNMERGE] * 10
        per = K.tome_lists_ints(H, W, r)
        for k in range(10):                      # (kept plan: nothing is lent twice, every buffer still holds what its launch wrote)
            ma, se, me, un = ops[4 * k:4 * k + 4]
            assert all((a.n_img, a.H, a.W, a.r) == (N, H, W, r) for a in (ma, se, me, un))
            n = peek(ma.src, (N, T, C), np.float16)
            best, score = peek(ma.dst, (N, Ns), np.int32), peek(ma.dst + N * Ns * 4, (N, Ns), np.float32)
            check_match(n, H, W, best, score)
            lists = peek(se.dst, (N, per), np.int32)
            m, o = peek(me.dst, (N, T - r, C), np.float16), peek(un.src, (N, T - r, C), np.float32)
            x, y = peek(un.aux2, (N, T, C), np.float32), peek(un.dst, (N, T, C), np.float32)
            for img in range(N):
                want = TR.select(score[img], best[img], H, W, r)
                got = TR.split_lists(lists[img], H, W, r)
                assert all(got[q].tobytes() == want[q].tobytes() for q in want)
                w64, terms = TR.merge64(n[img], want, H, W)
                assert (np.abs(m[img].astype(np.float64) - w64) <= TR.merge_bound(w64, n[img], want, H, W, terms)).all()
                assert y[img].tobytes() == TR.unmerge32(x[img], o[img], want["slot"]).tobytes()
    finally:
        u.ctx.destroy()
    # tome = 0: the plain plan, op for op, and its bytes; merged: another result
    (p, inp), (z, _) = unet(), unet(tome=0.0)
    try:
        assert p.ctx.op_list() == z.ctx.op_list() and self_attention_lengths(p) == [(T, T)] * 12 and other_attention(p) == others and len(others) == 12
        plain = p.run(*inp)
        assert z.run(*inp).tobytes() == plain.tobytes() and out.tobytes() != plain.tobytes()
    finally:
        p.ctx.destroy(); z.ctx.destroy()


def test_generator_with_tome_and_a_captured_graph():
    from mlimgsynth_amd import engine as E
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, 4, LH, LW)).astype(np.float32)
    P, outs = E.unet_params("tinyxl"), []
    cond, label = rng.standard_normal((77, P.n_ctx)).astype(np.float32), rng.standard_normal(P.ch_adm_in).astype(np.float32)
    for graph in (False, True):
        g = E.Generator("tinyxl", 8 * LW, 8 * LH, 1, cfg_scale=2.0, tome=0.5, use_hipgraph=graph)
        try:
            g.set_cond(cond, label, np.zeros_like(cond), np.zeros_like(label))
            outs += [g.tome_info()[:3]] + [g.dxdt(x, 2.5).tobytes() for _ in range(3)]
        finally:
            g.destroy()
    assert len(set(outs)) == 2 and outs[0] == (0.5, 2, 10)         # eager, and three replays of the graph: the same bytes


# ------------------------------------------------------------------ through mlis_generate (tiny at 128 px: 16 x 16 = 256 tokens at downscale 1, three transformers there)
def session(lib, hypertile=0):
    import mlis_ffi as F
    m = F.Mlis(lib)
    for k, v in (("model", ("synth:tiny",)), ("image_dim", (128, 128)), ("steps", (3,)), ("cfg_scale", (7.0,)), ("method", ("euler_a",)), ("hypertile", (hypertile,))):
        m.set(k, *v)
    return m


def generate(lib, m, ratio, max_ds=0):
    """one generation with this setting -> (latent bytes, infotext, engines built so far, mlis_amd_tome_info)"""
    import mlis_ffi as F
    assert ratio is None or lib.mlis_amd_tome(m.ctx, ratio, max_ds) == 1
    m.tokens(np.array([5, 17, 300], np.int32)), m.tokens(np.array([9], np.int32), negative=True), m.set("seed", 42), m.set("no_decode", 1)
    m.generate()
    r, d, lv = ctypes.c_float(), ctypes.c_int(), (ctypes.c_int * 12)()
    assert lib.mlis_amd_tome_info(m.ctx, r, d, lv) == 1
    return m.tensor(F.TENSOR["LATENT"]).tobytes(), lib.mlis_infotext_get(m.ctx, 0).decode(), lib.mlis_amd_engine_builds(m.ctx), (r.value, d.value, list(lv))


def test_through_mlis_generate():
    import mlis_ffi as F
    lib = F.bind(_lib.LIB_PATH)
    lib.mlis_amd_tome.argtypes = [F.vp, ctypes.c_float, F.ci]
    lib.mlis_amd_tome_info.argtypes = [F.vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(F.ci), ctypes.POINTER(F.ci)]
    lib.mlis_amd_engine_builds.argtypes = [F.vp]
    fresh = {}                                   # fresh contexts: every generation starts its Philox streams at offset 0, so results compare bit for bit
    for name, ratio in (("plain", None), ("zero", 0.0), ("on", 0.5), ("again", 0.5), ("r0", 0.05)):
        m = session(lib)
        try:
            fresh[name] = generate(lib, m, ratio)
        finally:
            m.close()
    merged, text = [256, 128, 128] + [0] * 9, ", Token merging ratio: 0.5"
    assert fresh["zero"][:3] == fresh["plain"][:3] and fresh["zero"][3] == (0.0, 1, [0] * 12) and fresh["plain"][2] == 1
    assert fresh["on"][3] == (0.5, 1, merged) and fresh["on"][0] != fresh["plain"][0] and fresh["on"][:3] == fresh["again"][:3]
    assert text in fresh["on"][1] and fresh["on"][1].replace(text, "") == fresh["plain"][1]
    assert fresh["r0"][0] == fresh["plain"][0] and fresh["r0"][3][2] == [0] * 12     # floor(0.05 x 256) = 12 rounds down to r = 0: the plain engine's bytes
    m = session(lib)                             # one context: what each setting does to its two engine slots
    try:
        builds = [generate(lib, m, *a)[2] for a in ((0.0,), (0.5,), (0.5, 1), (0.0,), (0.05,), (0.5, 2))]
        assert builds == [1, 2, 2, 2, 2, 3]   # max_ds 0 is 1 for this model: one key; ratio 0 and r = 0 are the plain key; max_ds 2 is another engine
    finally:
        m.close()
    m = session(lib, hypertile=64)               # HyperTile cuts the level ToMe merges: a bad value at generate, nothing built
    try:
        assert lib.mlis_amd_tome(m.ctx, 0.5, 0) == 1
        m.tokens(np.array([5], np.int32)), m.tokens(np.array([9], np.int32), negative=True)
        assert lib.mlis_generate(m.ctx) == -4 and "HyperTile" in m.err() and lib.mlis_amd_engine_builds(m.ctx) == 0      # MLIS_E_OPT_VALUE
    finally:
        m.close()
