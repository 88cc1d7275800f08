"""The table of op kinds (csrc/host/mlblock_ops.c: k_op_class) as the library reports it, without a GPU.

  a. the kinds, in order, are the pinned list (the numbering mlctx_op_record promises is append only);
  b. every kind has a ctypes mirror of exactly the size the library states -- also the kinds no test plan contains;
  c. tests/plan_audit.py knows every kind: extents() returns, or refuses the kind or its arguments by name, and never falls through to "op kind ...";
  d. on the tinyxl 16 x 16 N = 2 plan (MLB_F_OPSHAPES) and the plans of a tinyxl engine with a ControlNet and FreeU: mlctx_op_bytes equals the formulas
     restated here, every label is non-empty, and no op is marked `fused` whose kind always launches.
"""
import ctypes

import pytest

import plan_audit as PA

KINDS = ["gemm", "attn", "gn", "ln", "n2h", "h2n", "temb", "act", "cemb", "smax", "copy", "xavt", "attn_ctx", "cadd", "freeu_backbone", "freeu_skip"]


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield engine
    L.mlsd_runtime_dry(0)


def test_the_kind_list_is_pinned(dry):
    assert [name for name, _ in dry.op_kinds()] == KINDS
    f = dry.L().mlctx_op_kind_info
    assert f(len(KINDS), None, None) == 0 and f(-1, None, None) == 0 and f(0, None, None) == 1


def test_every_kind_has_a_mirror_of_its_size(dry):
    types = dry._op_arg_types()
    assert sorted(types) == sorted(KINDS)
    for name, nbytes in dry.op_kinds():
        assert ctypes.sizeof(types[name]) == nbytes, (name, ctypes.sizeof(types[name]), nbytes)


def test_the_audit_knows_every_kind(dry):
    types = dry._op_arg_types()
    for name, _ in dry.op_kinds():
        try:
            PA.Op(0, name, "", 0, 0, (-1, -1), types[name]())      # (all-zero arguments: a kind the audit covers may refuse THEM, by name)
        except PA.Unknown as e:
            assert not str(e).startswith("op kind"), (name, str(e))


def want_bytes(kind, fused, a):
    """mlctx_op_bytes restated: every operand read once, every output written once"""
    if kind == "gemm":
        nout = a.N // 2 if a.act == 5 else a.N
        b = 2.0 * a.n_img * a.H * a.W * a.Cin if a.conv else 2.0 * a.M * a.K
        b += 2.0 * a.N * a.K
        b += 4.0 * a.N if a.bias else 0
        b += 4.0 * (a.M // max(a.rows_per_batch, 1)) * a.N if a.rowbias else 0
        b += 4.0 * a.M * nout if a.resid else 0
        b += 4.0 * a.M * nout if a.C32 else 0
        b += 2.0 * a.M * nout if a.C16 else 0
        b += 2.0 * a.M * nout + 4.0 * (a.M // a.xa_Tq) * a.xa_Tk * a.N if a.xa_k else 0
        return b
    if kind in ("attn", "attn_ctx"):
        return 2.0 * a.n_batch * a.n_head * a.d_head * (2.0 * a.Tq + 2.0 * a.Tk)
    if kind == "gn":
        return 0.0 if fused else float(a.n_img * a.HW * (a.C1 + a.C2)) * (6.0 + (2.0 if a.raw16 else 0.0))
    if kind == "ln":
        return 0.0 if fused else float(a.rows * a.d) * (4.0 + (2.0 if a.y16 else 0.0) + (4.0 if a.y32 else 0.0))
    if kind == "smax":
        return a.rows * a.cols * 6.0
    if kind == "act":
        return a.n * 6.0
    if kind == "copy":
        return 2.0 * a.nbytes
    if kind == "cadd":
        return 12.0 * a.n_img * a.rows * a.C
    if kind in ("freeu_backbone", "freeu_skip"):
        return 12.0 * a.n_img * a.H * a.W * a.C
    assert kind in ("n2h", "h2n", "temb", "cemb", "xavt"), kind      # counted as 0: not part of the roofline
    return 0.0


def check_plan(engine, ctx, seen):
    can_fuse = engine.L().mlctx_op_kind_can_fuse
    can_fuse.argtypes = [ctypes.c_int]
    number = {name: i for i, name in enumerate(KINDS)}
    recs, labels, nbytes = ctx.op_records(), [lab for lab, _ in ctx.op_list()], ctx.op_bytes()
    assert len(recs) == len(labels) == len(nbytes) > 0
    for i, (kind, _, fused, _, _, a) in enumerate(recs):
        assert nbytes[i] == want_bytes(kind, fused, a), (i, kind, labels[i], nbytes[i])
        assert labels[i], (i, kind)
        assert not fused or can_fuse(number[kind]), (i, kind, labels[i])
        seen.add(kind)


def test_bytes_labels_and_fused_marks(dry):
    seen = set()
    for spec in (("unet", "tinyxl", 16, 2), ("unet", "sd1", 16, 2)):      # (SD1.5: the plan at this size whose LayerNorms end their producers, so `fused` is met)
        b = PA.build(dry, spec, PA.MLB_F_OPSHAPES)
        try:
            check_plan(dry, b.ctx, seen)
            assert spec[1] != "sd1" or any(r[2] for r in b.ctx.op_records())
        finally:
            b.close()
    g = dry.Generator("tinyxl", 128, 128, 1, defer_weights=True, control=True, freeu=True)      # control = 3
    try:
        for i in (0, 5, 6):      # UNet, ControlNet, hint block
            check_plan(dry, g.ctx_at(i), seen)
    finally:
        g.destroy()
    assert seen >= {"gemm", "attn", "gn", "ln", "n2h", "temb", "act", "cadd", "freeu_backbone", "freeu_skip"}, seen
    assert [dry.L().mlctx_op_kind_can_fuse(i) for i in range(len(KINDS) + 1)] == [int(k in ("gemm", "gn", "ln")) for k in KINDS] + [0]
