"""tests/attn64_cases.py without a GPU: every case's float64 reference is usable, mlsd_attention_variant gives every case the label the table
names (dry runtime, fake 16-byte-aligned addresses), and the launch entry takes the same route as the query."""
import numpy as np
import pytest

import attn64_cases as AC
import ref64 as R

IDS = [c["id"] for c in AC.CASES]


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib, kernels
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield kernels, _lib
    AC.restore_switches(L)
    L.mlsd_runtime_dry(0)


def fake_args(kernels, c):
    return AC.attn_args(kernels, c, {n: 0x10000000 * (i + 1) for i, n in enumerate(sorted(AC.layout(c)["bufs"]))})


def test_the_table_holds_what_the_suite_relies_on():
    assert len(set(IDS)) == len(IDS) >= 100
    labels = {c["variant"] for c in AC.CASES}
    want = {f"attn<tile,d{d}>" for d in (32, 40, 64, 80, 160)} | {f"attn<tk96,d{d}>" for d in (40, 64, 80, 160)}
    want |= {"attn<tile,d64,causal>", "attn<tile,d32,causal>", "attn<64x2>", "attn<64x2s,d64>", "attn<64x2s,d40>"}
    assert want <= labels, want - labels
    for lay in AC.LAYOUTS[1:]:
        assert {c["path"] for c in AC.CASES if c["layout"] == lay} == {"tile", "tile,causal", "tk96", "64x2", "64x2s"}, lay
    assert all(c["Tq"] == c["Tk"] for c in AC.CASES if c["causal"])
    assert all(c["q_scaled"] == (c["path"] in ("64x2s", "pp")) for c in AC.CASES)


@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_reference_is_usable(case):
    c = case
    q, k, v = AC.make_operands(c)
    assert all(np.isfinite(a).all() for a in (q, k, v))
    for b in range(c["nb"]):
        o, p = R.attention64(q[b], k[b], v[b], c["heads"], bool(c["causal"]))
        assert np.isfinite(p).all() and np.isfinite(o).all()
        assert (p.sum(-1) > 0.999).all() and (p.max(-1) > 0).all()              # no row of p is all zero
        bound = R.attention_bound(q[b], k[b], v[b], c["heads"], o, p, c["q_scaled"])
        assert np.isfinite(bound).all() and not ((bound == 0) & (o != 0)).any()
        if c["causal"]:
            Tq = c["Tq"]
            assert not p[:, np.triu_indices(Tq, 1)[0], np.triu_indices(Tq, 1)[1]].any()       # masked keys carry nothing
            D = c["heads"] * c["d"]
            np.testing.assert_array_equal(o[0], v[b][0].astype(np.float64).reshape(D))         # row 0 sees one key
            Rs = AC.special_dims(c)          # the traps, in the dims that carry them (the Gaussian dims add N(0, sigma^2) to every score)
            s = np.einsum("ihd,jhd->hij", q[b].reshape(Tq, c["heads"], -1)[..., :Rs], k[b].reshape(Tq, c["heads"], -1)[..., :Rs]) / np.sqrt(c["d"])
            up = np.triu(np.ones((Tq, Tq), bool), 1)
            assert (np.where(up, s, -np.inf).max(-1)[:, :Tq - 1] > 39.9).all()                 # every row but the last: a masked key at +40
            assert (np.where(up, -np.inf, s)[:, 70].max(-1) < -224).all() and (np.where(up, s, np.inf)[:, 70].min(-1) == 0).all()   # row 70
            diag = s[:, np.arange(Tq), np.arange(Tq)]
            assert (diag[:, 37::64] > 19.9).all() and (diag[:, 64::64] > 19.9).all() and (diag[:, 63:Tq - 1:64] > 39.9).all()


@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_label_and_launch_route(dry, case):
    """the query names the table's kernel, and mlsd_attention itself resolves to it: in the dry runtime the launch is refused under its route's label"""
    kernels, _lib = dry
    L = _lib.lib()
    a = fake_args(kernels, case)
    try:
        AC.apply_switches(L, case["sw"])
        assert kernels.attention_variant(a) == case["variant"]
        with pytest.raises(_lib.MlsdError, match="no GPU") as e:
            kernels.attention(a)
        assert f": {case['variant']}: no GPU" in str(e.value)
    finally:
        AC.restore_switches(L)


def test_variant_is_null_where_the_launch_refuses(dry):
    kernels, _lib = dry
    c = dict(AC.CASES[0])
    for change, ctx in ((dict(d=48), False), (dict(Tq=0), False), (dict(Tk=96), True), (dict(Tk=321), True), (dict(Tk=154, causal=1), True)):
        a = fake_args(kernels, dict(c, **change))
        assert kernels.attention_variant(a, ctx=ctx) is None, change
        with pytest.raises(_lib.MlsdError) as e:
            (kernels.attention_ctx if ctx else kernels.attention)(a)
        assert "no GPU" not in str(e.value)
    a = fake_args(kernels, c)
    a.ldk += 4
    assert kernels.attention_variant(a) is None
    a = fake_args(kernels, c)
    a.q = 0
    assert kernels.attention_variant(a) is None


@pytest.mark.parametrize("d,Tk,mode,label", [(80, 154, 0, "attn<ctx,d80,resident>"), (80, 154, 1, "attn<ctx,d80,slot>"), (64, 308, 0, "attn<ctx,d64,slot>"),
                                             (160, 154, 0, "attn<ctx,d160,slot>"), (32, 231, 0, "attn<ctx,d32,resident>"), (40, 97, 0, "attn<ctx,d40,resident>")])
def test_ctx_labels_and_launch_route(dry, d, Tk, mode, label):
    kernels, _lib = dry
    L = _lib.lib()
    a = fake_args(kernels, dict(AC.CASES[0], d=d, Tk=Tk))
    try:
        L.mlsd_attention_ctx_mode(mode)
        assert kernels.attention_variant(a, ctx=True) == label
        with pytest.raises(_lib.MlsdError) as e:
            kernels.attention_ctx(a)
        assert f": {label}: no GPU" in str(e.value)
    finally:
        L.mlsd_attention_ctx_mode(0)
