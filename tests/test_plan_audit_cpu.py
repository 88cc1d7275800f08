"""The plan audit in the dry runtime (no GPU): tests/plan_audit.py on plans built with device memory served from host memory.

  a. MLB_F_KEEP (every tensor in a block of its own) does not change the op list;
  b. every byte range a launch reads was written by an earlier launch, or is a parameter, an input or a block zeroed once;
  c. the recycling arena never changes who wrote what a launch reads, on the test-size plans, the bench plans at full size and the
     windowed-context, seamless-tiling and weight-streaming variants -- and the audit notices planted lifetime faults;
  d. the launch verifier passes a memory image made by numpy emulations of every op kind and fails, at the op and output that carries it,
     on each planted fault; the bounds derived for the small ops hold float32 emulations of the kernels' steps with room.

The forms of the option plans are part of all four: the control sum (fewer control images than images; gain 0), both FreeU passes, HyperTile's permuting
copies and the four phase launches of an upsampling convolution onto one poisoned map -- in the emulated image with their planted faults, and as plans
(controlled, FreeU, ControlNet, hint block, control + PAG, the forced phase form) in a, b and c.  The bench plans of c are audited in the phase form
the device runs.
"""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import plan_audit as PA
import ref64 as R

OPSHAPES, KEEP = PA.MLB_F_OPSHAPES, PA.MLB_F_OPSHAPES | PA.MLB_F_KEEP


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield engine
    L.mlsd_runtime_dry(0)


def both(engine, spec):
    """(recycling plan, kept plan, closer)"""
    b0 = PA.build(engine, spec, OPSHAPES)
    try:
        b1 = PA.build(engine, spec, KEEP)
    except Exception:
        b0.close()
        raise
    return (PA.Plan(b0.ctx, PA.plan_id(spec), external=b0.external), PA.Plan(b1.ctx, PA.plan_id(spec) + " kept", external=b1.external),
            lambda: (b0.close(), b1.close()))


def ids(plans):
    return [PA.plan_id(s) for s in plans]


# the option plans, as tests/test_plan_audit_gpu.py audits them on the device
PHASE = dict(params=dict(n_ch=320, ch_mult=(1, 1, 0, 0, 0)), ups_phases=2)
OPTION_PLANS = [
    ("unet", "tinyxl", 16, 2, dict(control=1)), ("unet", "tinyxl", 16, 2, dict(freeu=True)), ("controlnet", "tinyxl", 16, 1), ("control_hint", "tinyxl", 16),
    ("unet", "tinyxl", 16, 3, dict(control=2, pag=1)), ("unet", "tinyxl", 16, 2, dict(control=1, freeu=True)),
    ("unet", "tinyxl", (32, 16), 2, PHASE), ("unet", "tinyxl", (32, 16), 2, dict(PHASE, tiling=3)),
]


def audit_pair(engine, spec, rec, kept):
    """a, b and c of the module docstring on one pair of plans"""
    # a. op for op: kind, label, marks, shapes, route and epilogue fields (addresses excluded)
    assert len(rec.ops) == len(kept.ops)
    diffs = [(o, p) for o, p in zip(rec.ops, kept.ops) if PA.op_signature(o) != PA.op_signature(p)]
    allowed = abs(rec.ln_alias_refused - kept.ln_alias_refused)      # a fold the alias rule refuses in one arena only: the producer and its LayerNorm differ
    for o, p in diffs:
        print(f"[plan audit] {rec.name}: {o} differs from the kept plan's {p}")
        assert {o.kind, p.kind} <= {"gemm", "ln"}, (o, p)
    assert len(diffs) <= 2 * allowed, [str(o) for o, _ in diffs[:8]]
    # b. every read has a writer, in both arenas; no output on an own operand but the LayerNorm ending's sound form
    for plan in (kept, rec):
        bad = PA.uncovered_reads(plan)
        assert not bad, [why for _, _, why in bad[:6]]
        own = PA.own_operand_overwrites(plan)
        assert not own, [f"{o}: {w} lands on its own operand {r}" for o, w, r in own[:6]]
    assert all(w.name == "ln_y16" for o in rec.ops for w in o.writes for r in o.reads if not w.scratch and PA.overlaps(w, r))
    # c. recycling never changes who wrote what a launch reads.  Where a refused fold made the op lists differ the lifetimes are audited on the pair built
    # without LayerNorm folds (their op lists are equal again), and that is said
    if not diffs:
        bad = PA.lifetime_diffs(rec, kept)
        assert not bad, bad[:6]
        return
    print(f"[plan audit] {rec.name}: {len(diffs)} ops differ by a refused LayerNorm fold; lifetimes audited on the plans built with MLSD_NO_LN_FOLD=1")
    env = os.environ.get("MLSD_NO_LN_FOLD")
    os.environ["MLSD_NO_LN_FOLD"] = "1"
    try:
        rec2, kept2, close2 = both(engine, spec)
    finally:
        if env is None:
            os.environ.pop("MLSD_NO_LN_FOLD", None)
        else:
            os.environ["MLSD_NO_LN_FOLD"] = env
    try:
        assert [PA.op_signature(o) for o in rec2.ops] == [PA.op_signature(o) for o in kept2.ops]
        assert not PA.uncovered_reads(rec2) and not PA.uncovered_reads(kept2)
        bad = PA.lifetime_diffs(rec2, kept2)
        assert not bad, bad[:6]
    finally:
        close2()


# ------------------------------------------------------------------ a, b, c on the test-size plans and the variants
@pytest.mark.parametrize("spec", PA.TEST_PLANS + PA.VARIANT_PLANS + OPTION_PLANS, ids=ids(PA.TEST_PLANS + PA.VARIANT_PLANS + OPTION_PLANS))
def test_keep_flag_coverage_and_lifetimes(dry, spec):
    rec, kept, close = both(dry, spec)
    try:
        audit_pair(dry, spec, rec, kept)
        opt = spec[4] if len(spec) > 4 else {}
        kinds = {o.kind for o in rec.ops}
        assert ("cadd" in kinds) == bool(opt.get("control")) and ({"freeu_backbone", "freeu_skip"} <= kinds) == bool(opt.get("freeu"))
        assert sorted(o.a.out_phase for o in rec.ops if o.kind == "gemm" and o.a.out_phase) == ([1, 2, 3, 4] if opt.get("ups_phases") else [])
    finally:
        close()


def _lend_out_early(rec, kept, kind, operand):
    """An op of `kind` and a tensor it needs across other launches -- its operand `operand`, or with "dst" its own output on the way to its reader: a launch in
    between gets an output moved onto that tensor.  The audit must name the reader that now sees another writer, and the rewriting."""
    for o in (o for o in rec.ops if o.kind == kind):
        if operand == "dst":
            j, w = o.i, next(w for w in o.writes if w.name == "dst")
            last = max((q.i for q in rec.ops[o.i + 1:] if any(PA.overlaps(r, w) and rec.latest_writer(q.i, r) == (o.i, "dst") for r in q.reads)), default=0)
        else:
            w = next(r for r in o.reads if r.name == operand)
            if not isinstance(rec.latest_writer(o.i, w), tuple):
                continue
            j, last = rec.latest_writer(o.i, w)[0], o.i
        thieves = [(q, x) for q in rec.ops[j + 1:last] if not q.once for x in q.writes if not x.scratch and x.name in ("C16", "dst", "y16")]
        if thieves:
            break
    else:
        raise AssertionError(f"no {kind} keeps its {operand} across a launch")
    (m, thief), saved = thieves[0], thieves[0][1].base
    thief.base = w.base + 64
    rec.reindex()
    bad = PA.lifetime_diffs(rec, kept)
    assert any(f"op {last} " in b and f"op {m.i}" in b for b in bad) and any("rewritten" in b and f"op {j} " in b and f"op {m.i} " in b for b in bad), (kind, bad[:4])
    thief.base = saved
    rec.reindex()
    assert not PA.lifetime_diffs(rec, kept)


def test_option_plans_undeclared_external_memory_and_planted_lifetime_faults(dry):
    """What a controlled FreeU plan reads from outside itself (the ControlNet plan's residuals, the gain, the FreeU factors) counts only where it was declared; a
    control sum or a FreeU pass whose operand block is lent out too early, and a phase launch's pixels rewritten before the map's reader, are named."""
    spec = ("unet", "tinyxl", 16, 2, dict(control=1, freeu=True))
    b0, b1 = PA.build(dry, spec, OPSHAPES), PA.build(dry, spec, KEEP)
    try:
        bare = PA.Plan(b0.ctx, "undeclared")
        bad = PA.uncovered_reads(bare)
        assert {nm for _, nm, _ in bad} == {"ctrl", "gain", "f"} and {o.kind for o, _, _ in bad} == {"cadd", "freeu_backbone", "freeu_skip"}
        for drop in range(len(b0.external)):      # every declared range is needed
            some = PA.uncovered_reads(PA.Plan(b0.ctx, "one undeclared", external=b0.external[:drop] + b0.external[drop + 1:]))
            assert some and all(o.kind in ("cadd", "freeu_backbone", "freeu_skip") for o, _, _ in some), b0.external[drop][0]
        rec, kept = PA.Plan(b0.ctx, "rec", external=b0.external), PA.Plan(b1.ctx, "kept", external=b1.external)
        assert not PA.lifetime_diffs(rec, kept)
        _lend_out_early(rec, kept, "freeu_backbone", "dst")
        # a read of a residual the ControlNet plan does not hold
        o = next(o for o in rec.ops if o.kind == "cadd")
        r = next(r for r in o.reads if r.name == "ctrl")
        r.base += 1 << 30
        assert [(q.i, nm) for q, nm, _ in PA.uncovered_reads(rec)] == [(o.i, "ctrl")]
        r.base -= 1 << 30
    finally:
        b0.close(), b1.close()
    for spec, kind, operand in ((("unet", "tinyxl", 16, 2, dict(control=1)), "cadd", "base"), (("unet", "tinyxl", 16, 2, dict(freeu=True)), "freeu_skip", "src")):
        rec, kept, close = both(dry, spec)      # (the skip tensors, written in the encoder)
        try:
            _lend_out_early(rec, kept, kind, operand)
        finally:
            close()
    # the phase form: a pixel row of launch 2 rewritten between the four launches and the map's reader
    spec = ("unet", "tinyxl", (32, 16), 2, PHASE)
    rec, kept, close = both(dry, spec)
    try:
        assert not PA.lifetime_diffs(rec, kept)
        ph = [o for o in rec.ops if o.kind == "gemm" and o.a.out_phase]
        # (the map's only reader follows the four launches at once, and the recycling arena rightly lends its block out after it.  So the rule is held between two
        # kept plans: their LAST launch is made a reader of one source row's pixels of launch 2, and in one of them a launch before it gets an output moved onto them)
        b2 = PA.build(dry, spec, KEEP)
        try:
            kept2 = PA.Plan(b2.ctx, "kept, with the fault")
            for p in (kept, kept2):
                p.ops[-1].reads.append(PA.Range("x1", [o for o in p.ops if o.kind == "gemm" and o.a.out_phase][1].writes[3].base, 1, 16))
            assert not PA.lifetime_diffs(kept2, kept)
            kph = [o for o in kept2.ops if o.kind == "gemm" and o.a.out_phase]
            m, thief = next((q, x) for q in kept2.ops[kph[3].i + 2:-1] for x in q.writes if not x.scratch and not q.once and x.rows == 1)
            thief.base = kph[1].writes[3].base
            kept2.reindex()
            bad = PA.lifetime_diffs(kept2, kept)
            assert any("rewritten" in b and f"op {kph[1].i} " in b and f"op {m.i} " in b for b in bad) and any(f"op {len(kept.ops) - 1} " in b and "operand x1" in b for b in bad), bad[:4]
            kept.ops[-1].reads.pop()
        finally:
            b2.close()
        # and a pixel no phase launch writes: its reader has no writer
        gone = ph[2].writes.pop(5)
        rec.reindex()
        bad = PA.uncovered_reads(rec)
        assert bad and all(any(PA.overlaps(r, gone) for r in o.reads) for o, _, _ in bad)
        ph[2].writes.insert(5, gone)
        rec.reindex()
        assert not PA.uncovered_reads(rec)
    finally:
        close()


def _largest_that_fits(engine, spec):
    """the bench plan, or the same plan at the largest smaller latent whose kept form this machine's memory holds.  Only a failed allocation moves on to a
    smaller latent: every other failure of the build or of the extents is a failure of the test."""
    from mlimgsynth_amd import _lib
    kind, model, lat, n = spec[:4]
    for l in (lat, lat * 3 // 4, lat // 2, lat // 4):
        try:
            return (kind, model, l, n), both(engine, (kind, model, l, n))
        except (_lib.MlsdError, MemoryError) as e:
            if not isinstance(e, MemoryError) and not re.search(r"allocation .*failed|allocation failed|out of host memory", str(e)):
                raise
            print(f"[plan audit] {PA.plan_id(spec)}: kept plan at latent {l} does not fit ({str(e)[:80]})")
    raise AssertionError(f"no latent of {spec} fits")


@pytest.mark.parametrize("spec", PA.BENCH_PLANS, ids=ids(PA.BENCH_PLANS))
def test_lifetimes_of_the_bench_plans(dry, spec):
    """SD1.5 64x64 N = 2, SDXL 128x128 N = 8 and their KL-VAE decoders as bench.py builds them (the dry runtime serves the kept SDXL plan's 39 GB
    with calloc: untouched pages; where that allocation fails the largest smaller latent is audited and printed)."""
    used, (rec, kept, close) = _largest_that_fits(dry, spec)
    try:
        print(f"[plan audit] {PA.plan_id(used)}: {len(rec.ops)} ops")
        audit_pair(dry, used, rec, kept)
    finally:
        close()


def test_static_audit_notices_planted_lifetime_faults(dry):
    """a block lent out too early, an output landing on a live operand, a read of memory nobody wrote: each named by op and operand"""
    spec = ("unet", "tinyxl", 16, 2)
    rec, kept, close = both(dry, spec)
    try:
        assert not PA.lifetime_diffs(rec, kept)
        # the longest-lived fp32 tensor of the plan (a skip connection): its writer j and last reader l
        span = {}
        for o in kept.ops:
            for r in o.reads:
                w = kept.latest_writer(o.i, r)
                if isinstance(w, tuple) and w[1] == "C32":
                    span[w] = max(span.get(w, 0), o.i)
        (j, name), l = max(span.items(), key=lambda t: t[1] - t[0][0])
        assert l - j > 20
        victim = next(w for w in rec.ops[j].writes if w.name == name)
        m = next(o for o in rec.ops[j + 5:l] if o.kind == "gemm" and not o.once and any(w.name == "C16" for w in o.writes))
        thief = next(w for w in m.writes if w.name == "C16")
        saved = thief.base
        thief.base = victim.base + 64                       # 1: a block lent out before its last reader has run
        rec.reindex()
        bad = PA.lifetime_diffs(rec, kept)
        assert any(f"op {m.i} " in b for b in bad) and any(f"op {l} " in b or "rewritten" in b for b in bad), bad[:4]
        thief.base = saved
        rec.reindex()
        assert not PA.lifetime_diffs(rec, kept)
        a_read = next(r for r in m.reads if r.name == "A")    # 2: the output lands on the launch's own A operand, not row for row
        thief.base = a_read.base + 2
        rec.reindex()
        assert any(o.i == m.i and w == "C16" and r == "A" for o, w, r in PA.own_operand_overwrites(rec))
        thief.base = saved
        rec.reindex()
        saved = a_read.base                                   # 3: a read of memory nobody wrote
        a_read.base = max(t[1] for t in rec.regions) + (1 << 30)
        bad = PA.uncovered_reads(rec)
        assert [(o.i, nm) for o, nm, _ in bad] == [(m.i, "A")], [why for _, _, why in bad[:4]]
        a_read.base = saved
        once = next(o for o in rec.ops if o.once and o.kind == "gemm")      # 4: a step-invariant output rewritten by a later launch (after its last reader of one evaluation)
        last = rec.ops[-1].writes[0]
        saved, last.base = last.base, once.writes[0].base
        rec.reindex()
        assert any("step-invariant" in b for b in PA.lifetime_diffs(rec, kept))
        last.base = saved
    finally:
        close()


def test_ranges():
    r = lambda *a: PA.Range("r", *a)
    q = r(0x1000, 8, 64, 192)                       # a column view: 8 rows of 64 bytes in rows of 192
    assert PA.overlaps(q, r(0x1000 + 32, 1, 8)) and not PA.overlaps(q, r(0x1000 + 64, 8, 128, 192)) and PA.overlaps(q, r(0x1000 + 63, 8, 128, 192))
    whole = r(0x1000, 8, 192)
    assert PA.covered_by(q, [whole]) and not PA.covered_by(whole, [q]) and PA.covered_by(whole, [q, r(0x1000 + 64, 8, 128, 192)])
    assert not PA.covered_by(whole, [q, r(0x1000 + 65, 8, 127, 192)]) and not PA.covered_by(r(0x1000, 9, 64, 192), [q])
    assert PA.covered_by(r(0x1000 + 192, 2, 16, 192), [q]) and not PA.covered_by(r(0x1000 + 192 + 56, 2, 16, 192), [q])
    with pytest.raises(PA.Unknown):
        PA.Range("bad", 0, 1, 4)


# ------------------------------------------------------------------ d. the verifier on an emulated memory image
def _kern():
    from mlimgsynth_amd import kernels
    return kernels


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


class OpList(list):
    """the ops of the hand-made plan; .ups as PA.Plan.ups: (derived phase weights, loaded 3x3 weight, cout, cin) of its upsampling convolutions"""
    ups = ()


class Image:
    """A small hand-made plan over a DictMemory: ops are appended with their ctypes arguments, emulate() fills their outputs."""

    def __init__(self):
        self.mem, self.ops, self.rng = PA.DictMemory(), OpList(), np.random.default_rng(7)

    def put(self, a):
        return self.mem.put(a)

    def zeros(self, n, dtype):
        return self.mem.put(np.zeros(n, dtype))

    def op(self, kind, a, fused=0, once=0):
        self.ops.append(PA.Op(len(self.ops), kind, "", fused, once, (-1, -1), a))
        return len(self.ops) - 1

    def write(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        self.mem.view(ptr, np.uint8)[:arr.nbytes] = arr.view(np.uint8).reshape(-1)

    def write_mat(self, ptr, arr, ld):
        v = self.mem.view(ptr, arr.dtype)
        for m in range(arr.shape[0]):
            v[m * ld:m * ld + arr.shape[1]] = arr[m]


def emulate(img, i, fault=None):
    """numpy float32 emulation of op i (float64 sums rounded once: inside every bound), with one optional planted fault"""
    mem, op = img.mem, img.ops[i]
    k, a = op.kind, op.a
    f32 = np.float32
    if k == "gemm":
        M, N, Kd, nout = a.M, a.N, a.K, PA._gemm_nout(a)
        if a.conv and a.out_phase:      # a phase launch: the taps and the output pixels from the library's restatement of the kernel's maps, row by row
            x = PA._mat(mem, a.A, a.n_img * a.H * a.W, a.Cin, a.lda, np.float16).astype(np.float64)
            b = type(a).from_buffer_copy(a)
            if fault == "phase_tap_offset_dropped":
                b.tap_oy = b.tap_ox = 0
            if fault == "phase_parity_swapped":
                b.out_phase = {1: 4, 2: 3, 3: 2, 4: 1}[a.out_phase]
            L = _kern().lib()
            L.mlsd_conv_tap_source.restype = L.mlsd_conv_out_pixel.restype = ctypes.c_long
            A = np.zeros((M, 2, 2, a.Cin))
            for m, ta, tb in itertools.product(range(M), range(2), range(2)):
                src = L.mlsd_conv_tap_source(ctypes.byref(b), m, ta, tb)
                if src >= 0:
                    A[m, ta, tb] = x[src]
            A = A.reshape(M, Kd)
            pix = np.array([L.mlsd_conv_out_pixel(ctypes.byref(b), m) for m in range(M)])
        elif a.conv:
            x = PA._mat(mem, a.A, a.n_img * a.H * a.W, a.Cin, a.lda, np.float16)
            A = R.im2col64(x, a.n_img, a.H, a.W, a.Cin, a.KH, a.KW, a.stride, a.pad, a.upsample, a.OH, a.OW, wrap=a.wrap)
        else:
            A = PA._mat(mem, a.A, M, Kd, a.lda, np.float16).astype(np.float64)
        W = PA._mat(mem, a.W_, N, Kd, a.ldb, np.float16).astype(np.float64)
        acc = A @ W.T
        if fault == "k_tile_dropped":
            acc[128:256, 0:128] -= A[128:256, 64:128] @ W[0:128, 64:128].T
        if fault == "stale_row_block":
            acc[128:256] = acc[0:128]
        z = acc.astype(f32)
        if a.bias:
            z = z + PA._vec(mem, a.bias, N)[None, :]
        if a.rowbias:
            rb = PA._mat(mem, a.rowbias + (4 * 128 if fault == "bias_slice_shifted" else 0), M // a.rows_per_batch, N, a.ldrb, f32)
            rows = np.arange(M) // a.rows_per_batch
            if fault == "rowbias_wrong_image":
                rows = (rows + 1) % rb.shape[0]
            z = z + rb[rows]
        if a.bias_m:
            z = z + PA._vec(mem, a.bias_m, M)[:, None]
        res = PA._mat(mem, a.resid, M, nout, a.ldr, f32) if a.resid and fault != "residual_left_out" else None
        if a.act == 5:
            vc, gc = R.geglu_cols(nout)
            y = (z[:, vc].astype(np.float64) * R.act64(z[:, gc], 2)).astype(f32)
        else:
            if res is not None and a.act_after_resid:
                z = z + res
            y = R.act64(z, a.act).astype(f32)
        if res is not None and not (a.act_after_resid and a.act != 5):
            y = y + res
        if a.out_phase:      # before the launch its pixels hold the poison; then one row of N floats per output pixel
            v = img.mem.view(a.C32, f32)
            own = np.array([L.mlsd_conv_out_pixel(ctypes.byref(a), m) for m in range(M)])
            for m in range(M):
                v[own[m] * a.ldc32:own[m] * a.ldc32 + N] = np.nan
            for m in range(M):
                if not (fault == "phase_pixel_unwritten" and m == M - 3):
                    v[pix[m] * a.ldc32:pix[m] * a.ldc32 + N] = y[m]
        elif a.C32:
            img.write_mat(a.C32, y, a.ldc32)
        if a.C16 and not a.xa_k:
            y16 = f16(y)
            if fault == "c16_rounded_twice":
                y16 = f16((y.view(np.uint32) + np.uint32(0x400) & np.uint32(0xFFFFF800)).view(f32))      # first to 13 significant bits, then to 11
            img.write_mat(a.C16, y16, a.ldc16)
        if a.colstats:
            rows = a.colstats_rows
            blk = y.astype(np.float64).reshape(M // rows, rows, N)
            d = blk - blk[:, :1] if a.colstats_shift else blk
            img.write(a.colstats, np.stack([d.sum(1), (d * d).sum(1)], axis=1).astype(f32))
        if a.ln_y16:
            be = PA._vec(mem, a.ln_beta, N) if a.ln_beta else None
            img.write_mat(a.ln_y16, f16(R.layernorm64(y, a.ln_eps, PA._vec(mem, a.ln_gamma, N), be)), a.ldln)
        if a.xa_k:
            n_img, heads = M // a.xa_Tq, N // 64
            q = f16(y).astype(np.float64)
            kk = PA._mat(mem, a.xa_k, n_img * a.xa_Tk, N, a.xa_ldk, np.float16)
            vt = PA._vec(mem, a.xa_vt, n_img * N * 96, np.float16).reshape(n_img, N, 96)
            o = np.concatenate([R.attention64(q[b * a.xa_Tq:(b + 1) * a.xa_Tq], kk[b * a.xa_Tk:(b + 1) * a.xa_Tk], vt[b, :, :a.xa_Tk].T, heads)[0]
                                for b in range(n_img)])
            img.write_mat(a.xa_out, f16(o), a.xa_ldo)
    elif k in ("attn", "attn_ctx"):
        D = a.n_head * a.d_head
        for b in range(a.n_batch):
            q = PA._mat(mem, a.q + 2 * b * a.bsq, a.Tq, D, a.ldq, np.float16)
            kk = PA._mat(mem, a.k + 2 * b * a.bsk, a.Tk, D, a.ldk, np.float16)
            v = PA._mat(mem, a.v + 2 * b * a.bsv, a.Tk, D, a.ldv, np.float16)
            if fault == "last_key_ignored":
                kk, v = kk[:-1], v[:-1]
            o, _ = R.attention64(q, kk, v, a.n_head, causal=bool(a.causal))
            img.write_mat(a.out + 2 * b * a.bso, f16(o), a.ldo)
    elif k == "gn":
        n, hw, C = a.n_img, a.HW, a.C1 + a.C2
        x = PA._mat(mem, (fault == "stale_statistics" and img.stale) or a.x1, n * hw, a.C1, a.ld1, f32)
        if a.C2:
            x = np.concatenate([x, PA._mat(mem, a.x2, n * hw, a.C2, a.ld2, f32)], axis=1)
        x = x.reshape(n, hw, C)
        if fault == "stale_statistics":      # normalised with another tensor's statistics
            mu, var, _, _ = R.group_stats(x, a.n_grp, a.eps)
            xt = PA._mat(mem, a.x1, n * hw, a.C1, a.ld1, f32).reshape(n, hw, a.n_grp, C // a.n_grp).astype(np.float64)
            y = ((xt - mu[:, None, :, None]) / np.sqrt(var + a.eps)[:, None, :, None]).reshape(n, hw, C)
            y = y * PA._vec(mem, a.gamma, C) + PA._vec(mem, a.beta, C)
            y = R.silu(y) if a.silu else y
        else:
            y = R.groupnorm64(x, None, a.n_grp, a.eps, PA._vec(mem, a.gamma, C), PA._vec(mem, a.beta, C), bool(a.silu))
        img.write(a.y16, f16(y))
        if a.raw16:
            img.write(a.raw16, f16(x))
    elif k == "ln":
        x = PA._mat(mem, a.x, a.rows, a.d, a.ldx, f32)
        y = R.layernorm64(x, a.eps, PA._vec(mem, a.g, a.d), PA._vec(mem, a.b, a.d) if a.b else None)
        if a.y16:
            img.write(a.y16, f16(y))
        if a.y32:
            img.write(a.y32, y.astype(f32))
    elif k == "n2h":
        src = PA._vec(mem, a.src, a.n_src * a.C * a.HW).reshape(a.n_src, a.C, a.HW)
        s = PA._vec(mem, a.scale, a.n_src) if a.scale else np.full(a.n_src, a.scale0, f32)
        idx = np.arange(a.n_dst) % a.n_src
        v = src[idx].transpose(0, 2, 1)
        if a.mode == 1:
            v = (np.tanh(v * f32(1.0 / 3.0)) * f32(3.0)).astype(f32)
        if a.mode == 2:
            v = (v * f32(2.0)).astype(f32) - f32(1.0)
        out = np.zeros((a.n_dst, a.HW, a.Cpad), np.float16)
        out[:, :, :a.C] = f16((v * s[idx][:, None, None]).astype(f32))
        img.write(a.dst, out)
    elif k == "h2n":
        src = PA._mat(mem, a.src, a.n * a.HW, a.C, a.ld, f32).reshape(a.n, a.HW, a.C)
        img.write(a.dst, ((src * f32(a.mul)).astype(f32) + f32(a.add)).astype(f32).transpose(0, 2, 1))
    elif k == "temb":
        img.write(a.out, f16(emu_timestep_embedding(PA._vec(mem, a.t, a.n), a.dim, a.maxp)))
    elif k == "act":
        x = PA._vec(mem, a.x, a.n)
        img.write(a.y, f16(x if a.act == 0 else emu_silu(x)))
    elif k == "cemb":
        tok = PA._vec(mem, a.tok, a.n * a.T, np.int32)
        tw = np.stack([PA._vec(mem, a.tw + 2 * int(t) * a.d, a.d, np.float16) for t in tok]).reshape(a.n, a.T, a.d)
        img.write(a.out, (tw.astype(f32) + PA._vec(mem, a.pw, a.T * a.d).reshape(1, a.T, a.d)).astype(f32))
    elif k == "smax":
        img.write_mat(a.out, f16(emu_softmax_rows(PA._mat(mem, a.in_, a.rows, a.cols, a.ld_in, f32), a.scale)), a.ld_out)
    elif k == "copy":
        src = np.array(mem.read(a.src, a.nbytes))
        if a.th > 0:      # HyperTile: row (n, ih th + u, iw tw + v) of the image order <-> row ((n nh + ih) nw + iw) th tw + u tw + v of the tile-major order
            th, tw, inv = (a.tw, a.th, a.inverse) if fault == "tile_sides_swapped" else (a.th, a.tw, a.inverse and fault != "untile_with_forward_map")
            nh, nw = a.H // th, a.W // tw
            n, ih, iw, u, v = np.unravel_index(np.arange(a.n_img * a.H * a.W), (a.n_img, nh, nw, th, tw))
            image_row = (n * a.H + ih * th + u) * a.W + iw * tw + v
            rows, out = src.reshape(-1, a.row_bytes), np.empty((a.n_img * a.H * a.W, a.row_bytes), np.uint8)
            if inv:
                out[image_row] = rows
            else:
                out = rows[image_row]
            src = out.reshape(-1)
        img.write(a.dst, src)
    elif k == "cadd":
        rows = a.n_img * a.rows
        base, gain = PA._mat(mem, a.base, rows, a.C, a.ld_base, f32), PA._vec(mem, a.gain, 1)[0]
        if gain == 0 and fault != "gain_ignored":
            img.write_mat(a.dst, base, a.ld_dst)
        else:
            ctrl = PA._mat(mem, a.ctrl, (a.n_img if fault == "ctrl_wrong_image" else a.n_ctrl) * a.rows, a.C, a.ld_ctrl, f32)
            img.write_mat(a.dst, emu_ctrl_add(base, ctrl, f32(1.0) if fault == "gain_ignored" else gain), a.ld_dst)
    elif k in ("freeu_backbone", "freeu_skip"):
        x = PA._mat(mem, a.src, a.n_img * a.H * a.W, a.C, a.ld_src, f32).reshape(a.n_img, a.H, a.W, a.C)
        f = PA._vec(mem, a.f, 1)[0]
        if f == 1:
            y = x
        elif k == "freeu_skip":
            y = emu_freeu_skip(x, f, dc_only=fault == "freeu_dc_only")
        else:
            y = emu_freeu_backbone(x, f, second_half=fault == "freeu_wrong_half")
        img.write_mat(a.dst, y.reshape(-1, a.C), a.ld_dst)
    elif k == "xavt":
        v = PA._mat(mem, a.v, a.n_img * a.Tk, a.N, a.ldv, np.float16).reshape(a.n_img, a.Tk, a.N)
        out = np.zeros((a.n_img, a.N, 96), np.float16)
        out[:, :, :a.Tk] = v.transpose(0, 2, 1)
        img.write(a.vt, out)
    else:
        raise AssertionError(k)


# float32 emulations of the kernels' steps (elementwise.hip, norm.hip, common.hpp), for the bounds derived in ref64.py
def emu_silu(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        e = np.exp2((-x * np.float32(1.4426950408889634)).astype(np.float32)).astype(np.float32)
    return (x * (np.float32(1.0) / (np.float32(1.0) + e)).astype(np.float32)).astype(np.float32)


def emu_timestep_embedding(t, dim, maxp):
    f32, half = np.float32, dim // 2
    j = np.arange(half, dtype=np.float32)
    e = ((-np.log(f32(maxp))).astype(f32) * j).astype(f32) / f32(half)
    arg = (np.asarray(t, f32)[:, None] * np.exp(e.astype(f32)).astype(f32)[None, :]).astype(f32)
    return np.concatenate([np.cos(arg).astype(f32), np.sin(arg).astype(f32)], axis=1)


def emu_softmax_rows(x, scale):
    f32 = np.float32
    x = np.asarray(x, f32)
    z = ((x - x.max(1, keepdims=True)).astype(f32) * f32(scale)).astype(f32)
    e = np.exp2((z * f32(1.4426950408889634)).astype(f32)).astype(f32)
    s = np.zeros(x.shape[0], f32)
    for c in range(0, x.shape[1], 256):            # each lane's strided sum, in order; then the tree
        s = (s + e[:, c:c + 256].sum(1, dtype=f32)).astype(f32)
    return (e * (f32(1.0) / s)[:, None].astype(f32)).astype(f32)


def emu_ctrl_add(base, ctrl, gain):
    """ctrl_add_kernel (control.hip): the product and the sum rounded once each; row r of base meets row r modulo the rows of ctrl"""
    f32 = np.float32
    k = ctrl[np.arange(base.shape[0]) % ctrl.shape[0]]
    return (base + (f32(gain) * k).astype(f32)).astype(f32)


def _fma(a, b, c):
    """one rounding: the product of two fp32 is exact in float64 (the sum's rounding to 53 bits is far below the fp32 one)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def emu_freeu_backbone(x, b, second_half=False):
    """freeu_mean_kernel + freeu_backbone_apply_kernel (freeu.hip) on x [n][H][W][C]: a wave per pixel, lane l adds the float4 vectors l, l + 64, .. component by
    component, (x + y) + (z + w), six butterfly levels, the division by C; the image's min and max; x ((b - 1) (m - min) / span + 1) on the first half"""
    f32 = np.float32
    n, H, W, C = x.shape
    v = x.reshape(n * H * W, C // 4, 4)
    acc = np.zeros((n * H * W, 64, 4), f32)
    for c4 in range(C // 4):
        acc[:, c4 % 64] = (acc[:, c4 % 64] + v[:, c4]).astype(f32)
    s = ((acc[:, :, 0] + acc[:, :, 1]).astype(f32) + (acc[:, :, 2] + acc[:, :, 3]).astype(f32)).astype(f32)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, np.arange(64) ^ o]).astype(f32)
    m = (s[:, 0] / f32(C)).astype(f32).reshape(n, H * W)
    mn, mx = m.min(axis=1, keepdims=True), m.max(axis=1, keepdims=True)
    span = (mx - mn).astype(f32)
    fac = ((f32(b) - f32(1)).astype(f32) * ((m - mn).astype(f32) / span).astype(f32)).astype(f32) + f32(1)
    fac = np.where(span > 0, fac, f32(1)).astype(f32).reshape(n, H, W, 1)
    y = x.copy()
    half = slice(C // 2, C) if second_half else slice(0, C // 2)
    y[..., half] = (x[..., half] * fac).astype(f32)
    return y


def emu_freeu_skip(x, s, dc_only=False):
    """freeu_skip_partial / _combine / _apply kernels (freeu.hip) on x [n][H][W][C]: the trig table from sincospif of an exact rational below 1/2 and a quarter
    turn, the angle sum by the addition formulas; seven plane sums in 16 parts x 16 pixel lanes, each lane adding its pixels in order (the products through a fused
    multiply-add), pixel lanes pl ^ 1, pl ^ 2, the four waves (w0 + w1) + (w2 + w3), the parts in a 4-level tree; the seven-term apply, fused multiply-adds"""
    f32 = np.float32
    n, H, W, C = x.shape
    HW = H * W

    def roots(L):
        k = np.arange(L)
        q = 4 * k // L
        ang = ((4 * k - q * L).astype(f32) / f32(2 * L)).astype(np.float64) * np.pi
        sn, cs = np.sin(ang).astype(f32), np.cos(ang).astype(f32)
        return np.choose(q, [cs, -sn, -cs, sn]), np.choose(q, [sn, cs, -sn, -cs])
    (ca, sa), (cb, sb) = roots(H), roots(W)
    p = np.arange(HW)
    ca, sa, cb, sb = ca[p // W], sa[p // W], cb[p % W], sb[p % W]
    T = [ca, sa, cb, sb, ((ca * cb).astype(f32) - (sa * sb).astype(f32)).astype(f32), ((sa * cb).astype(f32) + (ca * sb).astype(f32)).astype(f32)]
    v = x.reshape(n, HW, C)
    part_len = 16 * ((HW + 255) // 256)
    a = np.zeros((7, 16, 16, n, C), f32)
    for k, pl in itertools.product(range(16), range(16)):
        for q in range(k * part_len + pl, min(HW, (k + 1) * part_len), 16):
            a[0, k, pl] = (a[0, k, pl] + v[:, q]).astype(f32)
            for j in range(6):
                a[j + 1, k, pl] = _fma(v[:, q], T[j][q], a[j + 1, k, pl])
    lanes = np.arange(16)
    a = (a + a[:, :, lanes ^ 1]).astype(f32)
    a = (a + a[:, :, lanes ^ 2]).astype(f32)
    a = ((a[:, :, 0] + a[:, :, 4]).astype(f32) + (a[:, :, 8] + a[:, :, 12]).astype(f32)).astype(f32)      # [7][16 parts][n][C]
    for step in (1, 2, 4, 8):
        for k in range(0, 16, 2 * step):
            a[:, k] = (a[:, k] + a[:, k + step]).astype(f32)
    S = a[:, 0]
    g = ((f32(s) - f32(1)).astype(f32) / f32(HW)).astype(f32)
    e = np.broadcast_to(S[0][:, None, :], v.shape).astype(f32)
    for j in range(0 if dc_only else 6):
        e = _fma(S[j + 1][:, None, :], T[j][None, :, None], e)
    return _fma(g, e, v).reshape(x.shape)


def emu_tae_clamp(x, s):
    f32 = np.float32
    return ((np.tanh((np.asarray(x, f32) * f32(1.0 / 3.0)).astype(f32)).astype(f32) * f32(3.0)).astype(f32) * f32(s)).astype(f32)


def test_bounds_of_the_small_ops_hold_float32_emulations_with_room():
    """act_f32_to_f16 (SiLU), timestep_embedding, softmax_rows and the tanh mode of nchw_to_nhwc_f16: the fp32 bounds of ref64.py (derived from the
    kernels' rounding steps and the documented ulp errors, never from the GPU) against float32 numpy emulations of the same steps."""
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(20000) * 4, rng.standard_normal(2000) * 20, [0.0, -0.0, 1e-30, 80.0, -80.0]]).astype(np.float32)
    y, b = R.act16_bound(x, 1)
    r_act = PA._worst(R.gemm_ratio32(emu_silu(x), y, b))
    x = np.array([-90.0, -200.0, 90.0, 30000.0, -30000.0], np.float32)      # the exponential overflows fp32: the kernels return 0 for a value below 2^-120 (ACT_TINY's term)
    y, b = R.act16_bound(x, 1)
    assert PA._worst(R.gemm_ratio32(emu_silu(x), y, b)) <= 1.0
    t = np.array([0.0, 1.0, 17.25, 250.5, 999.0, 1000.0, 5e-3, 14.6], np.float32)
    y, b = R.timestep_embedding64(t, 320, 10000.0)
    r_temb = PA._worst(R.gemm_ratio32(emu_timestep_embedding(t, 320, 10000.0), y, b))
    s = (rng.standard_normal((8, 1000)) * (np.array([1, 4, 8, 16, 4, 1, 1, 8])[:, None] / 0.125)).astype(np.float32)
    s[4, 3] += 160.0
    s[5] = 2.5
    s[6, 500:] -= 1e4
    p, b = R.softmax_rows64(s, 0.125)
    r = R.gemm_ratio32(emu_softmax_rows(s, 0.125), p, b + 1e-300)
    assert PA._worst(r) <= 1.0                                # (probabilities below 2^-100 may be flushed: the bound's last term, no room asked there)
    r_smax = PA._worst(r[p >= R.ACT_TINY])
    v = np.concatenate([rng.standard_normal(20000) * 3, rng.standard_normal(2000) * 30, [0.0, 1e-20, 50.0, -50.0]]).astype(np.float32)
    y, b = R.tae_clamp64(v, 0.75)
    r_tanh = PA._worst(R.gemm_ratio32(emu_tae_clamp(v, 0.75), y, b + 1e-300))
    print(f"\n[plan audit] float32 emulations against the derived fp32 bounds, worst ratio: silu_f16 {r_act:.3f}, timestep_embedding {r_temb:.3f}, "
          f"softmax_rows {r_smax:.3f}, tanh clamp {r_tanh:.3f}")
    assert max(r_act, r_temb, r_smax, r_tanh) <= 0.8


def test_bounds_of_the_control_sum_and_freeu_hold_float32_emulations_with_room(dry):
    """mlsd_ctrl_add and the two FreeU kernels: the bounds derived in tests/test_controlnet_gpu.py and tests/test_freeu_gpu.py, as PA.verify_op applies them,
    against float32 numpy emulations of the kernels' steps in the kernels' order.

    The control sum's bound 2^-23 (|base| + |gain ctrl|) is attained where the base vanishes: the two roundings err by up to 2^-24 (|k| + |base + k|), k = gain ctrl,
    which is the whole bound at base = 0.  Where the signs agree the ratio is at most 1/2 + |k| / (2 (|base| + |k|)), less where they cancel: room of 0.8 exists
    where |k| <= 1.5 |base|, and is asked on residuals no larger than their base (|k| <= 0.975 |base|: at most 0.747); on arbitrary data the emulation must hold the
    bound itself."""
    Kn = _kern()
    rng = np.random.default_rng(5)
    img = Image()
    nan = lambda *shape: img.put(np.full(shape, np.nan, np.float32))
    base = (rng.standard_normal((3 * 63, 64)) * 3).astype(np.float32)
    small = (base * rng.uniform(-1.3, 1.3, base.shape)).astype(np.float32)                  # x 0.75: |gain ctrl| <= 0.975 |base|
    wild = (rng.standard_normal((63, 64)) * 2).astype(np.float32)
    base2 = base.copy()
    base2[0, 0], wild[0, 1], base2[5, :8] = 1e20, -1e-20, 0.0
    gain = img.put(np.array([PA.GAIN], np.float32))
    i_small = img.op("cadd", Kn.CaddArgs(dst=nan(189, 64), ld_dst=64, base=img.put(base), ld_base=64, ctrl=img.put(small), ld_ctrl=64, n_img=3, rows=63, C=64, n_ctrl=3, gain=gain))
    i_wild = img.op("cadd", Kn.CaddArgs(dst=nan(189, 64), ld_dst=64, base=img.put(base2), ld_base=64, ctrl=img.put(wild), ld_ctrl=64, n_img=3, rows=63, C=64, n_ctrl=1, gain=gain))
    fu = []
    for (H, W, Cn), f in itertools.product([(3, 5, 8), (24, 20, 72), (16, 16, 320)], (0.2, 0.9, 1.4)):      # one term per slot, several, and C beyond one wave of vectors
        y, x = np.mgrid[0:H, 0:W]
        ramp = (y / H + 0.5 * x / W)[None, :, :, None] * np.array([1.0, 1.25])[:, None, None, None]
        src = img.put((ramp + rng.standard_normal((2, H, W, Cn)) + 1.5).astype(np.float32))      # (as tests/test_freeu_gpu.py: the channel-mean map has a real spread)
        ws, fp = img.zeros(Kn.freeu_ws_bytes(2, H, W, Cn) // 4, np.float32), img.put(np.array([f], np.float32))
        for kind in ("freeu_skip", "freeu_backbone"):
            fu.append(img.op(kind, Kn.FreeuArgs(dst=nan(2 * H * W, Cn), ld_dst=Cn, src=src, ld_src=Cn, n_img=2, H=H, W=W, C=Cn, ws=ws, f=fp)))
    worst = {}
    for i in range(len(img.ops)):
        emulate(img, i)
        (kind, _), ratios = PA.verify_op(img.mem, img.ops, i)
        if i != i_wild:
            worst[kind] = max(worst.get(kind, 0.0), ratios["dst"])
        assert all(r <= 1.0 for r in ratios.values()), (img.ops[i], ratios)
    print(f"\n[plan audit] float32 emulations against the derived bounds, worst ratio: ctrl_add {worst['cadd']:.3f} (|gain ctrl| <= |base|), "
          f"freeu_skip {worst['freeu_skip']:.3f}, freeu_backbone {worst['freeu_backbone']:.3f}")
    assert 0 < min(worst.values()) and max(worst.values()) <= 0.8 and len(fu) == 18


def build_image():
    """one op of every kind the audited plans record, one GEMM of each epilogue family, wired as the plans wire them (column views, producer
    statistics, endings); returns the image and the op indices by name"""
    Kn = _kern()
    img, rng, ix = Image(), np.random.default_rng(11), {}
    nrm = lambda *s: rng.standard_normal(s)
    w16 = lambda n, k: img.put(f16(nrm(n, k) / np.sqrt(k)))
    # inputs: image through nchw_to_nhwc_f16 (modes 0, 1, 2), tokens through clip_embed, timesteps
    src = img.put(nrm(1, 4, 64).astype(np.float32))
    scale = img.put(np.array([0.7], np.float32))
    for mode in (0, 1, 2):
        dst = img.zeros(2 * 64 * 8, np.float16)
        ix[f"n2h{mode}"] = img.op("n2h", Kn.N2hArgs(src=src, n_src=1, C=4, HW=64, dst=dst, n_dst=2, Cpad=8, scale=scale if mode == 0 else None, scale0=1.5, mode=mode))
    x0 = ix["x0"] = dst                                         # [2][8 x 8][8] fp16, channels 4..7 zero
    tok = img.put(rng.integers(0, 50, (2, 16)).astype(np.int32))
    tw, pw, ce = img.put(f16(nrm(50, 64))), img.put(nrm(16, 64).astype(np.float32)), img.zeros(2 * 16 * 64, np.float32)
    ix["cemb"] = img.op("cemb", Kn.CembArgs(tok=tok, n=2, T=16, d=64, tw=tw, pw=pw, out=ce))
    t = img.put(np.array([999.0, 17.25], np.float32))
    te = img.zeros(2 * 64, np.float16)
    ix["temb"] = img.op("temb", Kn.TembArgs(t=t, n=2, dim=64, maxp=10000.0, out=te))
    # batched embedding projection [2 x 256 x 64] -> fp32, SiLU of it in fp16, and a plain fp16 conversion
    epb = img.zeros(2 * 256, np.float32)
    ix["emb_proj"] = img.op("gemm", Kn.GemmArgs(A=te, lda=64, W_=w16(256, 64), ldb=64, M=2, N=256, K=64, bias=img.put(nrm(256).astype(np.float32)), C32=epb, ldc32=256))
    s16, c16 = img.zeros(512, np.float16), img.zeros(512, np.float16)
    ix["silu"] = img.op("act", Kn.ActArgs(x=epb, y=s16, n=512, act=1))
    ix["f32_to_f16"] = img.op("act", Kn.ActArgs(x=epb, y=c16, n=512, act=0))
    # conv 3x3 on the 2x upsampled, wrapped image: row bias = columns 0..127 of the batched projection, shifted column statistics
    cv, cs = img.zeros(512 * 128, np.float32), img.zeros(8 * 2 * 128, np.float32)
    ix["conv"] = img.op("gemm", Kn.GemmArgs(A=x0, lda=8, conv=1, n_img=2, H=8, W=8, Cin=8, OH=16, OW=16, KH=3, KW=3, stride=1, pad=1, upsample=1, wrap=3,
                                            W_=w16(128, 72), ldb=72, M=512, N=128, K=72, bias=img.put(nrm(128).astype(np.float32)), rowbias=epb, rows_per_batch=256,
                                            ldrb=256, C32=cv, ldc32=128, colstats=cs, colstats_rows=64, colstats_shift=1))
    img.stale = img.put((5.0 + nrm(512, 128)).astype(np.float32))      # what an earlier tenant of a recycled block would have left
    gam, bet = img.put((1 + 0.3 * nrm(160)).astype(np.float32)), img.put(nrm(160).astype(np.float32))
    g1 = img.zeros(512 * 128, np.float16)
    ix["gn_stats"] = img.op("gn", Kn.GnArgs(x1=cv, ld1=128, C1=128, n_img=2, HW=256, n_grp=32, eps=1e-6, gamma=gam, beta=bet, silu=1, y16=g1, ws=img.zeros(512, np.float32),
                                            cs1=cs, rb_rows1=64, cs_shifted=1))
    # a strided second source (32 of 64 columns) for the concat GroupNorm with its raw fp16 copy
    x2 = img.put((3.0 + nrm(512, 64)).astype(np.float32))
    g2, raw = img.zeros(512 * 160, np.float16), img.zeros(512 * 160, np.float16)
    ix["gn_concat"] = img.op("gn", Kn.GnArgs(x1=cv, ld1=128, C1=128, x2=x2 + 4 * 16, ld2=64, C2=32, n_img=2, HW=256, n_grp=32, eps=1e-6, gamma=gam, beta=bet, silu=0, y16=g2,
                                             raw16=raw, ws=img.zeros(512, np.float32)))
    # Linear families on the GroupNorm output: SiLU + residual with C32 and C16; activation after the residual; per-row bias; GEGLU
    r32 = img.put(nrm(512, 256).astype(np.float32))
    o32, o16 = img.zeros(512 * 256, np.float32), img.zeros(512 * 256, np.float16)
    ix["lin_silu_res"] = img.op("gemm", Kn.GemmArgs(A=g1, lda=128, W_=w16(256, 128), ldb=128, M=512, N=256, K=128, bias=img.put(nrm(256).astype(np.float32)), act=1,
                                                    resid=r32, ldr=256, C32=o32, ldc32=256, C16=o16, ldc16=256))
    p16 = img.zeros(512 * 256, np.float16)
    ix["lin_relu_post"] = img.op("gemm", Kn.GemmArgs(A=g1, lda=128, W_=w16(256, 128), ldb=128, M=512, N=256, K=128, act=4, act_after_resid=1, resid=r32, ldr=256,
                                                     bias_m=img.put(nrm(512).astype(np.float32)), C16=p16, ldc16=256))
    gg = img.zeros(512 * 128, np.float16)
    ix["geglu"] = img.op("gemm", Kn.GemmArgs(A=o16, lda=256, W_=w16(256, 256), ldb=256, M=512, N=256, K=256, bias=img.put(nrm(256).astype(np.float32)), act=5, C16=gg, ldc16=128))
    # LayerNorm ending (the LayerNorm op itself is marked fused), a LayerNorm of its own with both outputs
    l32, l16 = img.zeros(512 * 128, np.float32), img.zeros(512 * 128, np.float16)
    lg, lb = img.put((1 + 0.2 * nrm(128)).astype(np.float32)), img.put(nrm(128).astype(np.float32))
    ix["lin_ln"] = img.op("gemm", Kn.GemmArgs(A=gg, lda=128, W_=w16(128, 128), ldb=128, M=512, N=128, K=128, resid=cv, ldr=128, C32=l32, ldc32=128, ln_y16=l16, ldln=128,
                                              ln_gamma=lg, ln_beta=lb, ln_eps=1e-5))
    ix["ln_fused"] = img.op("ln", Kn.LnArgs(x=l32, ldx=128, rows=512, d=128, eps=1e-5, g=lg, b=lb, y16=l16), fused=1)
    m16, m32 = img.zeros(32 * 64, np.float16), img.zeros(32 * 64, np.float32)
    ix["ln"] = img.op("ln", Kn.LnArgs(x=ce, ldx=64, rows=32, d=64, eps=1e-5, g=img.put((1 + 0.2 * nrm(64)).astype(np.float32)), b=img.put(nrm(64).astype(np.float32)), y16=m16, y32=m32))
    # fused q | k | v projection and causal attention on its column views (CLIP), then a ragged cross attention over 77 keys of a wide K | V buffer
    qkv = img.zeros(32 * 192, np.float16)
    ix["qkv"] = img.op("gemm", Kn.GemmArgs(A=m16, lda=64, W_=w16(192, 64), ldb=64, M=32, N=192, K=64, bias=img.put(nrm(192).astype(np.float32)), C16=qkv, ldc16=192))
    ao = img.zeros(32 * 64, np.float16)
    ix["attn_causal"] = img.op("attn", Kn.AttnArgs(q=qkv, k=qkv + 128, v=qkv + 256, out=ao, ldq=192, ldk=192, ldv=192, ldo=64, bsq=16 * 192, bsk=16 * 192, bsv=16 * 192,
                                                   bso=16 * 64, n_batch=2, n_head=2, d_head=32, Tq=16, Tk=16, causal=1))
    kv = img.put(f16(nrm(2 * 77, 640)))
    xo = img.zeros(512 * 128, np.float16)
    ix["attn_cross"] = img.op("attn", Kn.AttnArgs(q=l16, k=kv + 2 * 128, v=kv + 2 * 448, out=xo, ldq=128, ldk=640, ldv=640, ldo=128, bsq=256 * 128, bsk=77 * 640, bsv=77 * 640,
                                                  bso=256 * 128, n_batch=2, n_head=2, d_head=64, Tq=256, Tk=77, causal=0))
    # V^T pack and a q projection that ends with its cross attention (5 heads of 64), 77 keys
    vt = img.zeros(2 * 320 * 96, np.float16)
    ix["xavt"] = img.op("xavt", Kn.XavtArgs(v=kv + 2 * 320, ldv=640, n_img=2, Tk=77, N=320, vt=vt), once=1)
    xa = img.zeros(512 * 320, np.float16)
    ix["lin_xattn"] = img.op("gemm", Kn.GemmArgs(A=l16, lda=128, W_=w16(320, 128), ldb=128, M=512, N=320, K=128, xa_k=kv, xa_ldk=640, xa_vt=vt, xa_out=xa, xa_ldo=320,
                                                 xa_Tq=256, xa_Tk=77))
    # materialised softmax, device copy, the fp32 result back in NCHW
    sm = img.zeros(32 * 64, np.float16)
    ix["smax"] = img.op("smax", Kn.SmaxArgs(in_=m32, ld_in=64, out=sm, ld_out=64, rows=32, cols=64, scale=0.125))
    cp = img.zeros(32 * 64, np.float32)
    ix["copy"] = img.op("copy", Kn.CopyArgs(src=m32, dst=cp, nbytes=32 * 64 * 4))
    res = img.zeros(2 * 4 * 256, np.float32)
    ix["h2n"] = img.op("h2n", Kn.H2nArgs(src=cv, ld=128, n=2, C=4, HW=256, dst=res, mul=0.5, add=0.5))
    # the control sum on the convolution's output: ONE control image for two images (the buffer behind it holds a second, which nobody may read), gain 0.75; and
    # with gain 0, where the residuals are poison
    ctrl = img.put(nrm(2 * 256, 128).astype(np.float32))
    poison = lambda *shape: img.put(np.full(shape, np.nan, np.float32))
    ca = poison(512, 128)
    ix["cadd"] = img.op("cadd", Kn.CaddArgs(dst=ca, ld_dst=128, base=cv, ld_base=128, ctrl=ctrl, ld_ctrl=128, n_img=2, rows=256, C=128, n_ctrl=1,
                                            gain=img.put(np.array([PA.GAIN], np.float32))))
    ca0 = poison(512, 128)
    ix["cadd0"] = img.op("cadd", Kn.CaddArgs(dst=ca0, ld_dst=128, base=cv, ld_base=128, ctrl=poison(256, 128), ld_ctrl=128, n_img=2, rows=256, C=128, n_ctrl=1,
                                             gain=img.put(np.array([-0.0], np.float32))))
    # FreeU: the backbone pass on the control sum (a smooth ramp added first: the channel-mean map needs a spread), the Fourier filter on the strided second
    # source; destinations with padded rows, which keep their poison
    y_, x_ = np.mgrid[0:16, 0:16]
    ramp = img.put(np.repeat(((y_ / 16 + 0.5 * x_ / 16)[None] * np.array([1.0, 1.25])[:, None, None]).reshape(512, 1), 128, axis=1).astype(np.float32))
    cr = poison(512, 128)
    ix["cadd_ramp"] = img.op("cadd", Kn.CaddArgs(dst=cr, ld_dst=128, base=ca, ld_base=128, ctrl=ramp, ld_ctrl=128, n_img=2, rows=256, C=128, n_ctrl=2,
                                                 gain=img.put(np.array([1.0], np.float32))))
    ws = img.zeros(Kn.freeu_ws_bytes(2, 16, 16, 128) // 4, np.float32)
    fb, fs = poison(512, 136), poison(512, 72)
    ix["freeu_backbone"] = img.op("freeu_backbone", Kn.FreeuArgs(dst=fb, ld_dst=136, src=cr, ld_src=128, n_img=2, H=16, W=16, C=128, ws=ws,
                                                                 f=img.put(np.array([PA.FREEU_FACTORS[0]], np.float32))))
    ix["freeu_skip"] = img.op("freeu_skip", Kn.FreeuArgs(dst=fs, ld_dst=72, src=x2, ld_src=64, n_img=2, H=16, W=16, C=64, ws=ws,
                                                         f=img.put(np.array([PA.FREEU_FACTORS[3]], np.float32))))
    ix["freeu_one"] = img.op("freeu_skip", Kn.FreeuArgs(dst=poison(512, 64), ld_dst=64, src=x2, ld_src=64, n_img=2, H=16, W=16, C=64, ws=ws,
                                                        f=img.put(np.array([1.0], np.float32))))
    img.padding = {"freeu_backbone": (fb, 136, 128), "freeu_skip": (fs, 72, 64)}
    # HyperTile: the fp16 rows of the GroupNorm output into tiles of 8 x 4 (non-square: swapped sides are another map) and back
    t16, u16 = img.zeros(512 * 128, np.float16), img.zeros(512 * 128, np.float16)
    ix["tile"] = img.op("copy", Kn.CopyArgs(src=g1, dst=t16, nbytes=512 * 256, n_img=2, H=16, W=16, th=8, tw=4, row_bytes=256, inverse=0))
    ix["untile"] = img.op("copy", Kn.CopyArgs(src=t16, dst=u16, nbytes=512 * 256, n_img=2, H=16, W=16, th=8, tw=4, row_bytes=256, inverse=1))
    # an upsampling convolution in the phase form: four 2x2 convolutions (wrapped in x) of a 4 x 16 x 64 source onto one poisoned 8 x 32 x 320 map, their weights
    # derived by the library's rule (on the host in the dry runtime) from the 3x3 weight the assembled map is held against
    xs = img.put(f16(nrm(2 * 4 * 16, 64)))
    w3 = f16(nrm(320, 3, 3, 64) * 0.02)
    wd = np.empty((4, 320, 2, 2, 64), np.float16)
    assert Kn.lib().mlsd_ups_phase_weights(w3.ctypes.data_as(ctypes.c_void_p), wd.ctypes.data_as(ctypes.c_void_p), 320, 64, None) == 0
    w3p, wdp, pb, up = img.put(w3), img.put(wd), img.put(nrm(320).astype(np.float32) * 0.1), poison(2 * 8 * 32, 320)
    img.ops.ups = [(wdp, w3p, 320, 64)]
    for ph in range(4):
        ix[f"phase{ph + 1}"] = img.op("gemm", Kn.GemmArgs(A=xs, lda=64, conv=1, n_img=2, H=4, W=16, Cin=64, OH=4, OW=16, KH=2, KW=2, stride=1, pad=1, wrap=1,
                                                          W_=wdp + ph * 320 * 256 * 2, ldb=256, M=128, N=320, K=256, bias=pb, C32=up, ldc32=320,
                                                          tap_oy=ph >> 1, tap_ox=ph & 1, out_phase=1 + ph))
    for i in range(len(img.ops)):
        if not img.ops[i].fused:
            emulate(img, i)
    return img, ix


FAULTS = [      # (fault, op that carries it, output that must fail)
    ("residual_left_out", "lin_silu_res", "C32"),
    ("bias_slice_shifted", "conv", "C32"),
    ("rowbias_wrong_image", "conv", "C32"),
    ("k_tile_dropped", "lin_silu_res", "C32"),
    ("stale_statistics", "gn_stats", "y16"),
    ("c16_rounded_twice", "lin_silu_res", "C16==rne(C32)"),
    ("last_key_ignored", "attn_cross", "out"),
    ("stale_row_block", "geglu", "C16"),
    ("ctrl_wrong_image", "cadd", "dst"),
    ("gain_ignored", "cadd", "dst"),
    ("gain_ignored", "cadd0", "dst"),
    ("freeu_wrong_half", "freeu_backbone", "kept half"),
    ("freeu_dc_only", "freeu_skip", "dst"),
    ("untile_with_forward_map", "untile", "dst"),
    ("tile_sides_swapped", "tile", "dst"),
    ("phase_parity_swapped", "phase2", "C32"),
    ("phase_tap_offset_dropped", "phase4", "C32"),
    ("phase_pixel_unwritten", "phase3", "C32"),
]
# The assembled map of an upsampling convolution is held at its LAST phase launch (verify_op: "assembled"), whichever of the four spoiled it: beside its own
# launch's output a phase fault may fail there, and nowhere else
ALSO = {"phase_parity_swapped": ("phase4", "assembled"), "phase_tap_offset_dropped": ("phase4", "assembled"), "phase_pixel_unwritten": ("phase4", "assembled")}


@pytest.fixture(scope="module")
def image(dry):
    return build_image()


def verify_all(img):
    out = {}
    for i in range(len(img.ops)):
        key, ratios = PA.verify_op(img.mem, img.ops, i)
        out[i] = ratios
    return out


def test_verifier_passes_the_emulated_image(image):
    img, ix = image
    res = verify_all(img)
    names = {v: k for k, v in ix.items() if isinstance(v, int) and k != "x0"}
    print("\n[plan audit] emulated image, worst ratio per op and output:")
    for i, ratios in res.items():
        print(f"  {names.get(i, i):14s} {img.ops[i].kind:5s} " + "  ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
        assert all(r <= 1.0 for r in ratios.values()), (names.get(i), ratios)
    assert {o.kind for o in img.ops} >= {"gemm", "attn", "gn", "ln", "n2h", "h2n", "temb", "act", "cemb", "smax", "copy", "xavt", "cadd", "freeu_backbone", "freeu_skip"}
    # the new forms: every one is there and was judged by its own rule
    assert res[ix["cadd0"]] == {"dst": 0.0} and 0 < res[ix["cadd"]]["dst"] <= 1.0 and res[ix["freeu_one"]] == {"dst": 0.0}
    assert 0 < res[ix["freeu_skip"]]["dst"] <= 0.8 and 0 < res[ix["freeu_backbone"]]["dst"] <= 0.8 and res[ix["freeu_backbone"]]["kept half"] == 0.0
    assert [PA.census_key(img.ops[ix[k]])[1] for k in ("copy", "tile", "untile")] == ["", "tile", "untile"] and res[ix["tile"]] == res[ix["untile"]] == {"dst": 0.0}
    assert PA._bits_equal(img.mem.read(img.ops[ix["untile"]].a.dst, 512 * 256), img.mem.read(img.ops[ix["tile"]].a.src, 512 * 256)) == 0.0
    for ph in range(4):
        r = res[ix[f"phase{ph + 1}"]]
        assert set(r) == {"C32", "other parities"} | ({"assembled"} if ph == 3 else set()) and "phase" in PA.census_key(img.ops[ix[f"phase{ph + 1}"]])[2], r
    for ptr, ld, Cn in img.padding.values():      # the padding of a FreeU destination keeps its poison
        assert np.isnan(PA._mat(img.mem, ptr, 512, ld, ld, np.float32)[:, Cn:]).all() and np.isfinite(PA._mat(img.mem, ptr, 512, Cn, ld, np.float32)).all()
    assert res[ix["ln_fused"]] == {} and "ln_y16" in res[ix["lin_ln"]] and "xa_out" in res[ix["lin_xattn"]] and "colstats" in res[ix["conv"]]
    assert "raw16" in res[ix["gn_concat"]] and "C16==rne(C32)" in res[ix["lin_silu_res"]]


@pytest.mark.parametrize("fault,where,output", FAULTS, ids=[f[0] + ("" if [g[0] for g in FAULTS].count(f[0]) == 1 else "-" + f[1]) for f in FAULTS])
def test_verifier_fails_on_a_planted_fault(image, fault, where, output):
    img, ix = image
    i = ix[where]
    def rerun(f):      # op i with or without the fault, then everything after it on what it left (as a device would)
        for j in range(i, len(img.ops)):
            if not img.ops[j].fused:
                emulate(img, j, f if j == i else None)
    try:
        rerun(fault)
        res = verify_all(img)
        failing = [(j, n) for j, ratios in res.items() for n, r in ratios.items() if not r <= 1.0]
        assert (i, output) in failing, (fault, failing, res[i])
        # the fault stays where it is: ops that do not read the faulty output still pass (its consumers are judged on what they read)
        also = (ix[ALSO[fault][0]], ALSO[fault][1]) if fault in ALSO else None
        assert all(j == i or (j, n) == also for j, n in failing), (fault, failing)
    finally:
        rerun(None)
    assert all(r <= 1.0 for ratios in verify_all(img).values() for r in ratios.values())


def test_verifier_fails_by_name_on_what_it_does_not_know(image):
    img, ix = image
    Kn = _kern()
    t = img.ops[ix["tile"]].a
    bad = type(t).from_buffer_copy(t)
    bad.th = 5                                   # 16 rows in tiles of 5: the launcher refuses it
    with pytest.raises(PA.Unknown, match="tiles of 5 x 4"):
        PA.Op(0, "copy", "", 0, 0, (-1, -1), bad)
    bad = type(t).from_buffer_copy(t)
    bad.nbytes -= 256
    with pytest.raises(PA.Unknown, match="permuting copy of"):
        PA.verify_op(img.mem, [_with(img.ops[ix["tile"]], bad)], 0)
    p = img.ops[ix["phase4"]].a
    bad = type(p).from_buffer_copy(p)
    bad.out_phase = 5
    with pytest.raises(PA.Unknown, match="out_phase 5"):
        PA.Op(0, "gemm", "", 0, 0, (-1, -1), bad)
    bad = type(p).from_buffer_copy(p)
    bad.tap_ox = 0                               # the taps of another parity
    with pytest.raises(PA.Unknown, match="tap offsets"):
        PA.Op(0, "gemm", "", 0, 0, (-1, -1), bad)
    with pytest.raises(PA.Unknown, match="without its three sibling launches"):      # the assembled map needs all four launches
        PA.verify_op(img.mem, OpList([img.ops[ix["phase4"]]]), 0)
    with pytest.raises(PA.Unknown, match="control sum of 0 images"):
        PA.Op(0, "cadd", "", 0, 0, (-1, -1), Kn.CaddArgs())
    with pytest.raises(PA.Unknown, match="freeu_skip on 0 maps"):
        PA.Op(0, "freeu_skip", "", 0, 0, (-1, -1), Kn.FreeuArgs())
    # the backbone bound's condition on the data: an image with a (nearly) constant channel-mean map fails by op and image
    fb = img.ops[ix["freeu_backbone"]].a
    flat = type(fb).from_buffer_copy(fb)
    flat.src = img.put(np.tile(np.array([1, 2, 4, 1, -1, -2, -4, -1] * 16, np.float32), (512, 1)))
    with pytest.raises(PA.Unknown, match=r"freeu_backbone.*image 0"):
        PA.verify_op(img.mem, [PA.Op(7, "freeu_backbone", "", 0, 0, (-1, -1), flat)], 0)
    with pytest.raises(PA.Unknown, match="op kind"):
        PA.Op(0, "fft", "", 0, 0, (-1, -1), Kn.CopyArgs())
    a = img.ops[ix["n2h0"]].a
    bad = type(a).from_buffer_copy(a)
    bad.mode = 3
    with pytest.raises(PA.Unknown, match="mode 3"):
        PA.verify_op(img.mem, [PA.Op(0, "n2h", "", 0, 0, (-1, -1), bad)], 0)
    g = img.ops[ix["lin_silu_res"]].a
    bad = type(g).from_buffer_copy(g)
    bad.act = 7
    with pytest.raises(PA.Unknown, match="activation 7"):
        PA.verify_op(img.mem, [PA.Op(0, "gemm", "", 0, 0, (-1, -1), bad)], 0)


def _with(op, a):
    """op with the arguments a, its extents as they were (arguments the extents themselves refuse)"""
    q = PA.Op.__new__(PA.Op)
    for f in PA.Op.__slots__:
        setattr(q, f, getattr(op, f))
    q.a = a
    return q


def test_clobbered_operands_are_reported(image):
    """the verifier's precondition: an output landing on a range an earlier op read names both ops"""
    img, ix = image

    class P:
        pass
    plan = P()
    plan.ops, plan.rank = img.ops, {i: i for i in range(len(img.ops))}
    assert not PA.clobbered_operands(plan)
    w = img.ops[ix["copy"]].writes[0]
    saved, w.base = w.base, img.ops[ix["ln"]].reads[0].base
    try:
        bad = PA.clobbered_operands(plan)
        assert [(o.i, wn, r.i, rn) for o, wn, r, rn in bad] == [(ix["copy"], "dst", ix["ln"], "x")]
    finally:
        w.base = saved
