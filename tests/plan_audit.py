"""Audit of prepared plans (pure numpy; importable without a GPU).

A prepared plan is a list of launches on raw device pointers, rewired by mlctx_prep (folded residuals and norms, producer statistics, hoisted
step-invariant ops, column views of batched projections) over an arena that recycles blocks.  This module restates, from the RAW ARGUMENTS of
every op (MLCtx.op_records, never the C side's table of outputs, k_op_class), which byte ranges the op reads and which it writes, and derives the dataflow:

  extents(op)            -> (reads, writes): lists of Range (base, rows, row bytes, stride; column views have stride > row bytes)
  Plan.latest_writer     -> the last op before op i (in run order: `once` ops run before everything else, `fused` ops write nothing) whose
                            writes overlap a range, else "parameter" / "input" / "zeroed once" / None
  uncovered_reads(plan)  -> reads of memory nobody wrote
  lifetime_diffs(r, k)   -> where the recycling plan r disagrees with the kept plan k (MLB_F_KEEP: every tensor in a block of its own) about
                            who wrote what a launch reads, or rewrites a range between its writer and its last reader

verify_op(mem, plan, i) recomputes one op in float64 from the operands it actually read (tests/ref64.py: references and bounds) and returns
the worst ratio to the bound per output; kinds and arguments it does not know FAIL BY NAME (Unknown), they are never skipped.

Forms of the option plans: the control sum (cadd: its residuals and its gain live in ANOTHER plan's memory and a driver buffer, declared to Plan as
external ranges), the two FreeU passes, HyperTile's permuting copy (copy with th > 0) and the phase launches of an upsampling convolution (GEMM with
out_phase: the write is a strided pixel map, one Range per (image, source row)).

The census: census_key(op) is the form of an op (kind, GEMM tile and split form or attention kernel, epilogue features); unheld_forms() names the forms of a set of
plans that nothing holds.  It runs over BENCH_PLANS and over SIZE_PLANS, 35 plans at sizes other than the bench's (SD1.5 40x40 .. 96x96, SDXL 64x64 .. 168x96,
N = 1 .. 8, a long prompt, the VAEs and TAESD at other sizes), in the dry runtime and on the device.
"""
import bisect
import ctypes
import re

import numpy as np

import gemm64_cases as GC
import ref64 as R

MLB_F_OPSHAPES, MLB_F_KEEP = 16, 64


class Unknown(Exception):
    """an op kind or an argument form the audit does not know: a failure, never a skip"""


class Range:
    """rows x row_bytes bytes at base, consecutive rows `stride` bytes apart.  Stored normalised: touching rows are one row."""
    __slots__ = ("name", "base", "rows", "row_bytes", "stride", "scratch")

    def __init__(self, name, base, rows, row_bytes, stride=None, scratch=False):
        base, rows, row_bytes = int(base or 0), int(rows), int(row_bytes)
        stride = row_bytes if stride is None else int(stride)
        if not base:
            raise Unknown(f"range {name}: NULL base")
        if rows <= 0 or row_bytes <= 0 or (rows > 1 and stride < row_bytes):
            raise Unknown(f"range {name}: rows {rows} x {row_bytes} bytes, stride {stride}")
        if rows == 1 or stride == row_bytes:
            rows, row_bytes, stride = 1, rows * row_bytes, rows * row_bytes
        self.name, self.base, self.rows, self.row_bytes, self.stride, self.scratch = name, base, rows, row_bytes, stride, scratch

    @property
    def lo(self):
        return self.base

    @property
    def hi(self):
        return self.base + (self.rows - 1) * self.stride + self.row_bytes

    def __repr__(self):
        return f"{self.name}[{self.base:#x} {self.rows}x{self.row_bytes}/{self.stride}]"


def _row_hits(a, b):
    """for every row of a: (first, last) row index of b whose bytes intersect it (first > last: none)"""
    lo = a.base + np.arange(a.rows, dtype=np.int64) * a.stride
    hi = lo + a.row_bytes
    k0 = np.maximum(0, (lo - b.base - b.row_bytes) // b.stride + 1)
    k1 = np.minimum(b.rows - 1, (hi - 1 - b.base) // b.stride)
    return lo, hi, k0, k1


def overlaps(a, b):
    """exact: do the two ranges share a byte"""
    if a.lo >= b.hi or b.lo >= a.hi:
        return False
    if a.rows == 1 and b.rows == 1:
        return True
    if a.rows > b.rows:
        a, b = b, a
    _, _, k0, k1 = _row_hits(a, b)
    return bool((k0 <= k1).any())


def covered_by(r, covers):
    """exact: is every byte of r inside the union of the ranges `covers`"""
    covers = [c for c in covers if c.lo < r.hi and r.lo < c.hi]
    for c in covers:      # the common cases: inside one row of c, or a column view of c (same stride)
        if c.rows == 1 and c.lo <= r.lo and r.hi <= c.hi:
            return True
        if c.rows > 1 and r.stride == c.stride and r.rows > 1:
            k, off = divmod(r.base - c.base, c.stride)
            if k >= 0 and k + r.rows <= c.rows and off + r.row_bytes <= c.row_bytes:
                return True
        if c.rows > 1 and r.rows == 1:
            k, off = divmod(r.base - c.base, c.stride)
            if 0 <= k < c.rows and off + r.row_bytes <= c.row_bytes:
                return True
    if not covers:
        return False
    los = []      # the union of the covers' rows (those that can touch r), merged into disjoint intervals; then every row of r must lie inside one
    for c in covers:
        k0, k1 = max(0, (r.lo - c.base - c.row_bytes) // c.stride + 1), min(c.rows - 1, (r.hi - 1 - c.base) // c.stride)
        if k0 <= k1:
            lo = c.base + np.arange(k0, k1 + 1, dtype=np.int64) * c.stride
            los.append(np.stack([lo, lo + c.row_bytes]))
    if not los:
        return False
    lo, hi = np.concatenate(los, axis=1)
    o = np.argsort(lo, kind="stable")
    lo, reach = lo[o], np.maximum.accumulate(hi[o])
    first = np.ones(lo.size, bool)
    first[1:] = lo[1:] > reach[:-1]
    idx = np.nonzero(first)[0]
    starts, ends = lo[idx], reach[np.append(idx[1:] - 1, lo.size - 1)]
    rlo = r.base + np.arange(r.rows, dtype=np.int64) * r.stride
    j = np.searchsorted(starts, rlo, side="right") - 1
    return bool(((j >= 0) & (ends[np.maximum(j, 0)] >= rlo + r.row_bytes)).all())


# ------------------------------------------------------------------ what an op reads and writes
def _gemm_nout(a):
    return a.N // 2 if a.act == 5 else a.N


def _stats_rows(a):
    if a.colstats_rows > 0:
        return a.colstats_rows
    from mlimgsynth_amd import kernels
    r = kernels.gemm_route(a).stats_rows
    if r <= 0:
        raise Unknown("gemm with colstats on a launch that writes none")
    return r


def _attn_ranges(name, p, ld, bs, nb, T, width, esz=2):
    if not p:
        raise Unknown(f"attention: NULL {name}")
    if nb == 1 or bs == T * ld:
        return [Range(name, p, nb * T, width * esz, ld * esz)]
    return [Range(f"{name}[{b}]", p + b * bs * esz, T, width * esz, ld * esz) for b in range(nb)]


def _scratch_range(name, ptr, scratch, which):
    """the shared scratch block `which` of the plan (MLCtx.scratch_blocks: the sizes are the C side's) that ptr points into, from ptr to its end"""
    if scratch is None or which not in scratch:
        raise Unknown(f"{name} without the plan's {which} block")
    base, n = scratch[which]
    if not base <= ptr < base + n:
        raise Unknown(f"{name} at {ptr:#x} outside the plan's {which} block")
    return Range(name, ptr, 1, base + n - ptr, scratch=True)


def phase_of(a):
    """(py, px) of a phase launch of an upsampling convolution (mlsd_gemm_args.out_phase 1 .. 4), None for every other GEMM; fields the launcher would
    refuse (mlsd_gemm_phase_form) and forms the audit has not met raise"""
    if not a.out_phase:
        if a.tap_oy or a.tap_ox:
            raise Unknown(f"gemm with tap offsets ({a.tap_oy}, {a.tap_ox}) and no out_phase")
        return None
    if not 1 <= a.out_phase <= 4:
        raise Unknown(f"gemm with out_phase {a.out_phase}")
    py, px = (a.out_phase - 1) >> 1, (a.out_phase - 1) & 1
    if (a.tap_oy, a.tap_ox) != (py, px):
        raise Unknown(f"phase launch {a.out_phase} with tap offsets ({a.tap_oy}, {a.tap_ox})")
    if (not a.conv or (a.KH, a.KW, a.stride, a.pad, a.upsample) != (2, 2, 1, 1, 0) or (a.OH, a.OW) != (a.H, a.W) or not a.C32 or a.C16 or a.resid or a.rowbias
            or a.bias_m or a.act or a.colstats or a.ln_y16 or a.gn_y16 or a.xa_k):
        raise Unknown(f"phase launch {a.out_phase} of a form that is no plain 2x2 convolution with an fp32 output")
    return py, px


def phase_pixel_ranges(a, name="C32"):
    """what a phase launch writes: pixel (2 y + py, 2 x + px) of the [n_img][2 H][2 W] rows of ldc32 floats; per (image, y) W rows of N floats, two pixels apart"""
    py, px = phase_of(a)
    return [Range(name, a.C32 + ((n * 2 * a.H + 2 * y + py) * 2 * a.W + px) * a.ldc32 * 4, a.W, a.N * 4, 2 * a.ldc32 * 4)
            for n in range(a.n_img) for y in range(a.H)]


def tile_form(a):
    """"" for a plain device copy, "tile" / "untile" for HyperTile's row permutation (mlb_copy_args.th > 0); arguments mlsd_tile_permute would refuse raise"""
    if a.th <= 0:
        if a.th or a.tw or a.inverse:
            raise Unknown(f"copy with th {a.th}, tw {a.tw}, inverse {a.inverse}")
        return ""
    if a.tw <= 0 or a.n_img < 1 or a.H < 1 or a.W < 1 or a.row_bytes < 1 or a.H % a.th or a.W % a.tw:
        raise Unknown(f"permuting copy of {a.n_img} maps of {a.H} x {a.W} rows in tiles of {a.th} x {a.tw}")
    if a.nbytes != a.n_img * a.H * a.W * a.row_bytes:
        raise Unknown(f"permuting copy of {a.nbytes} bytes for {a.n_img} x {a.H} x {a.W} rows of {a.row_bytes} bytes")
    if a.inverse not in (0, 1):
        raise Unknown(f"permuting copy with inverse {a.inverse}")
    return "untile" if a.inverse else "tile"


def _gain_of(mem, a):
    """the gain a control sum read (None without a memory image: the static audit counts the residuals as read)"""
    return None if mem is None else float(_vec(mem, a.gain, 1)[0])


def extents(op, scratch=None, mem=None):
    """(reads, writes) of one op record, from its raw arguments; scratch: the plan's shared scratch blocks {name: (address, bytes)}; mem: the memory image
    after the evaluation, where there is one (a control sum whose gain is 0 never reads its residuals)"""
    k, a = op.kind, op.a
    rd, wr = [], []
    R_ = lambda *x, **y: rd.append(Range(*x, **y))
    W_ = lambda *x, **y: wr.append(Range(*x, **y))
    if op.fused and k in ("ln", "gn"):
        return rd, wr          # the producer's launch does it all (its ln_* / gn_* arguments)
    if k == "gemm":
        nout = _gemm_nout(a)
        phase = phase_of(a)
        if a.conv:
            if a.K != a.KH * a.KW * a.Cin or a.M != a.n_img * a.OH * a.OW:
                raise Unknown(f"conv with K {a.K} != {a.KH}x{a.KW}x{a.Cin} or M {a.M} != {a.n_img}x{a.OH}x{a.OW}")
            R_("A", a.A, a.n_img * a.H * a.W, a.Cin * 2, a.lda * 2)
        else:
            R_("A", a.A, a.M, a.K * 2, a.lda * 2)
        R_("W_", a.W_, a.N, a.K * 2, a.ldb * 2)
        if a.bias:
            R_("bias", a.bias, 1, a.N * 4)
        if a.bias_m:
            R_("bias_m", a.bias_m, 1, a.M * 4)
        if a.rowbias:
            rpb = max(a.rows_per_batch, 1)
            if a.M % rpb:
                raise Unknown(f"rowbias with M {a.M} % rows_per_batch {rpb}")
            R_("rowbias", a.rowbias, a.M // rpb, a.N * 4, a.ldrb * 4)
        if a.resid:
            R_("resid", a.resid, a.M, nout * 4, a.ldr * 4)
        xattn = bool(a.xa_k)
        if xattn:
            if a.xa_Tq <= 0 or a.M % a.xa_Tq or not a.xa_vt or not a.xa_out:
                raise Unknown("cross-attention ending with incomplete xa_* arguments")
            n_img = a.M // a.xa_Tq
            R_("xa_k", a.xa_k, n_img * a.xa_Tk, a.N * 2, a.xa_ldk * 2)
            R_("xa_vt", a.xa_vt, 1, n_img * a.N * 96 * 2)
            W_("xa_out", a.xa_out, a.M, a.N * 2, a.xa_ldo * 2)
        if phase:
            wr += phase_pixel_ranges(a)
        elif a.C32:
            W_("C32", a.C32, a.M, nout * 4, a.ldc32 * 4)
        if a.C16 and not xattn:      # (a q projection that ends with its attention does not store the projection)
            W_("C16", a.C16, a.M, nout * 2, a.ldc16 * 2)
        if not wr:
            raise Unknown("gemm without an output")
        if a.colstats:
            W_("colstats", a.colstats, 1, (a.M // _stats_rows(a)) * 2 * a.N * 4)
        if a.ln_y16:
            R_("ln_gamma", a.ln_gamma, 1, a.N * 4)
            if a.ln_beta:
                R_("ln_beta", a.ln_beta, 1, a.N * 4)
            W_("ln_y16", a.ln_y16, a.M, a.N * 2, a.ldln * 2)
            if a.ln_ws:      # (this launch's region of the plan's block: from its start to the block's end bounds it from above)
                wr.append(_scratch_range("ln_ws", a.ln_ws, scratch, "ln_ws"))
            if a.ln_cnt:
                wr.append(_scratch_range("ln_cnt", a.ln_cnt, scratch, "ln_cnt"))
        if a.gn_y16:
            R_("gn_gamma", a.gn_gamma, 1, a.N * 4)
            R_("gn_beta", a.gn_beta, 1, a.N * 4)
            W_("gn_y16", a.gn_y16, a.M, a.N * 2, a.gn_ldy * 2)
        if a.ws and a.ws_bytes:
            W_("ws", a.ws, 1, a.ws_bytes, scratch=True)
        if a.sk_flags:
            wr.append(_scratch_range("sk_flags", a.sk_flags, scratch, "sk_flags"))
    elif k in ("attn", "attn_ctx"):
        D = a.n_head * a.d_head
        rd += _attn_ranges("q", a.q, a.ldq, a.bsq, a.n_batch, a.Tq, D)
        rd += _attn_ranges("k", a.k, a.ldk, a.bsk, a.n_batch, a.Tk, D)
        rd += _attn_ranges("v", a.v, a.ldv, a.bsv, a.n_batch, a.Tk, D)
        wr += _attn_ranges("out", a.out, a.ldo, a.bso, a.n_batch, a.Tq, D)
    elif k == "gn":
        rows, C = a.n_img * a.HW, a.C1 + a.C2
        R_("x1", a.x1, rows, a.C1 * 4, a.ld1 * 4)
        if a.C2:
            R_("x2", a.x2, rows, a.C2 * 4, a.ld2 * 4)
        R_("gamma", a.gamma, 1, C * 4)
        R_("beta", a.beta, 1, C * 4)
        if a.cs1:
            if a.rb_rows1 <= 0 or a.HW % a.rb_rows1:
                raise Unknown("groupnorm statistics with a block that does not divide HW")
            R_("cs1", a.cs1, 1, (rows // a.rb_rows1) * 2 * a.C1 * 4)
        if a.cs2:
            if a.rb_rows2 <= 0 or a.HW % a.rb_rows2:
                raise Unknown("groupnorm statistics with a block that does not divide HW")
            R_("cs2", a.cs2, 1, (rows // a.rb_rows2) * 2 * a.C2 * 4)
        W_("y16", a.y16, 1, rows * C * 2)
        if a.raw16:
            W_("raw16", a.raw16, 1, rows * C * 2)
        if a.ws:
            from mlimgsynth_amd import kernels
            W_("ws", a.ws, 1, max(kernels.groupnorm_ws_bytes(a.n_img, a.HW, a.n_grp), 1), scratch=True)
    elif k == "ln":
        R_("x", a.x, a.rows, a.d * 4, a.ldx * 4)
        R_("g", a.g, 1, a.d * 4)
        if a.b:
            R_("b", a.b, 1, a.d * 4)
        if a.y16:
            W_("y16", a.y16, 1, a.rows * a.d * 2)
        if a.y32:
            W_("y32", a.y32, 1, a.rows * a.d * 4)
        if not wr:
            raise Unknown("layernorm without an output")
    elif k == "n2h":
        R_("src", a.src, 1, a.n_src * a.C * a.HW * 4)
        if a.scale:
            R_("scale", a.scale, 1, a.n_src * 4)
        W_("dst", a.dst, 1, a.n_dst * a.HW * a.Cpad * 2)
    elif k == "h2n":
        R_("src", a.src, a.n * a.HW, a.C * 4, a.ld * 4)
        W_("dst", a.dst, 1, a.n * a.C * a.HW * 4)
    elif k == "temb":
        R_("t", a.t, 1, a.n * 4)
        W_("out", a.out, 1, a.n * a.dim * 2)
    elif k == "act":
        R_("x", a.x, 1, a.n * 4)
        W_("y", a.y, 1, a.n * 2)
    elif k == "cemb":
        R_("tok", a.tok, 1, a.n * a.T * 4)
        R_("tw", a.tw, 1, a.d * 2)            # (the rows the tokens name: at least one; the table is a parameter, Plan.region_of finds its extent)
        R_("pw", a.pw, 1, a.T * a.d * 4)
        W_("out", a.out, 1, a.n * a.T * a.d * 4)
    elif k == "smax":
        R_("in", a.in_, a.rows, a.cols * 4, a.ld_in * 4)
        W_("out", a.out, a.rows, a.cols * 2, a.ld_out * 2)
    elif k == "copy":
        tile_form(a)
        R_("src", a.src, 1, a.nbytes)
        W_("dst", a.dst, 1, a.nbytes)
    elif k == "xavt":
        R_("v", a.v, a.n_img * a.Tk, a.N * 2, a.ldv * 2)
        W_("vt", a.vt, 1, a.n_img * a.N * 96 * 2)
    elif k == "cadd":
        if a.n_img < 1 or a.rows < 1 or not 1 <= a.n_ctrl <= a.n_img or a.C < 4 or a.C % 4 or min(a.ld_dst, a.ld_base, a.ld_ctrl) < a.C:
            raise Unknown(f"control sum of {a.n_img} images of {a.rows} rows x {a.C} with {a.n_ctrl} control images, strides {a.ld_dst} {a.ld_base} {a.ld_ctrl}")
        R_("base", a.base, a.n_img * a.rows, a.C * 4, a.ld_base * 4)
        R_("gain", a.gain, 1, 4)
        if _gain_of(mem, a) != 0.0:
            R_("ctrl", a.ctrl, a.n_ctrl * a.rows, a.C * 4, a.ld_ctrl * 4)
        W_("dst", a.dst, a.n_img * a.rows, a.C * 4, a.ld_dst * 4)
    elif k in ("freeu_backbone", "freeu_skip"):
        if a.n_img < 1 or a.H < 2 or a.W < 2 or a.C < 8 or a.C % 8 or min(a.ld_dst, a.ld_src) < a.C:
            raise Unknown(f"{k} on {a.n_img} maps of {a.H} x {a.W} x {a.C}, strides {a.ld_dst} {a.ld_src}")
        from mlimgsynth_amd import kernels
        R_("src", a.src, a.n_img * a.H * a.W, a.C * 4, a.ld_src * 4)
        R_("f", a.f, 1, 4)
        W_("dst", a.dst, a.n_img * a.H * a.W, a.C * 4, a.ld_dst * 4)      # (the C columns the kernels write: a destination's padding keeps its bytes)
        W_("ws", a.ws, 1, kernels.freeu_ws_bytes(a.n_img, a.H, a.W, a.C), scratch=True)
    else:
        raise Unknown(f"op kind {k!r}")
    return rd, wr


# ------------------------------------------------------------------ the plan and its dataflow
def ups_weights(ctx):
    """[(address of the derived phase weights, fp16 [4][cout][2][2][cin]; address of the loaded 3x3 weight they are derived from, fp16 [cout][3][3][cin];
    cout; cin)] of the plan's upsampling convolutions in the phase form (mlctx_ups_weights, mlctx_param_device).  A weight-streaming plan gives []: its
    addresses are virtual ones that nothing may read."""
    from mlimgsynth_amd import engine
    f = engine.L().mlctx_ups_weights
    f.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    n = f(ctx.h, -1, None, None, None, None)
    if not n or ctx.streaming_info() is not None:
        return []
    devs, out = ctx.param_devices(), []
    for i in range(n):
        pi, dev, cout, cin = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        f(ctx.h, i, ctypes.byref(pi), ctypes.byref(dev), ctypes.byref(cout), ctypes.byref(cin))
        out.append((dev.value or 0, devs[pi.value][1], cout.value, cin.value))
    return out


class Op:
    __slots__ = ("i", "kind", "label", "fused", "once", "gn_src", "a", "reads", "writes", "shape_label")

    def __init__(self, i, kind, label, fused, once, gn_src, a, shape_label="", scratch=None, mem=None):
        self.i, self.kind, self.label, self.fused, self.once, self.gn_src, self.a, self.shape_label = i, kind, label, fused, once, gn_src, a, shape_label
        self.reads, self.writes = extents(self, scratch, mem)

    def __repr__(self):
        return f"op {self.i} ({self.kind} {self.shape_label or self.label})"


class Plan:
    """Snapshot of a prepared context: ops with their extents, the read-only regions, and an index of the writes in run order.
    external: [(name, address, bytes)] of memory outside the context that its launches read (another plan's tensors, a driver's buffers): only what is
    declared counts as written.  mem: the memory image after the evaluation (extents)."""

    def __init__(self, ctx, name="", external=(), mem=None):
        self.name = name
        labels = [lab for lab, _ in ctx.op_list()]
        self.scratch = ctx.scratch_blocks()
        self.ops = [Op(i, *rec, shape_label=labels[i], scratch=self.scratch, mem=mem) for i, rec in enumerate(ctx.op_records())]
        self.ups = ups_weights(ctx)
        reg = [("parameter", key, p, n) for key, p, n in ctx.param_devices() if p and n]
        reg += [("external", nm, p, n) for nm, p, n in external if p and n]
        reg += [("parameter", f"weight slab {k}", p, n) for k, (p, n) in enumerate(ctx.weight_slabs())]
        for nm, stage, nb, src, n_src, scale in ctx.input_records():
            reg.append(("input", nm, stage, nb))
            if src:      # a bound source replaces the staging buffer: its extent is what the gather reads
                for o in self.ops:
                    if o.kind == "n2h" and o.a.src == src:
                        reg.append(("input", nm + " (bound source)", src, o.a.n_src * o.a.C * o.a.HW * 4))
                        if o.a.scale:
                            reg.append(("input", nm + " (bound scale)", o.a.scale, o.a.n_src * 4))
        reg += [("zeroed once", f"zeroed block {k}", p, n) for k, (p, n) in enumerate(ctx.zeroed_blocks())]
        reg += [("zeroed once", nm, p, n) for nm, (p, n) in self.scratch.items() if nm != "splitk_ws"]
        self.regions = sorted(((p, p + n, cls, nm) for cls, nm, p, n in reg), key=lambda t: t[0])
        self._reg_lo = [t[0] for t in self.regions]
        self.ln_alias_refused = ctx.ln_alias_refused()
        # run order: the step-invariant ops first (they run once per conditioning, before every evaluation's launches)
        self.order = sorted(range(len(self.ops)), key=lambda i: (0 if self.ops[i].once else 1, i))
        self.rank = {i: r for r, i in enumerate(self.order)}
        self.reindex()

    def reindex(self):
        """(re)build the index of the writes in run order (after a range was edited)"""
        w = [(self.rank[o.i], o.i, q) for o in self.ops for q in range(len(o.writes))]
        w.sort()
        self._w = w
        self._w_rank = np.array([t[0] for t in w], np.int64)
        self._w_lo = np.array([self.ops[t[1]].writes[t[2]].lo for t in w], np.int64)
        self._w_hi = np.array([self.ops[t[1]].writes[t[2]].hi for t in w], np.int64)

    def region_ranges(self, r, classes=("parameter", "input", "zeroed once", "external")):
        """the read-only / zeroed regions that touch range r, as ranges"""
        out = []
        j = bisect.bisect_right(self._reg_lo, r.hi)
        for lo, hi, cls, nm in self.regions[:j]:
            if hi > r.lo and cls in classes:
                out.append((cls, Range(nm, lo, 1, hi - lo)))
        return out

    def writers(self, r, rank_lo, rank_hi):
        """[(op index, write range)] of the writes of ops with rank_lo <= rank < rank_hi that overlap r, latest first"""
        m = np.nonzero((self._w_rank >= rank_lo) & (self._w_rank < rank_hi) & (self._w_lo < r.hi) & (self._w_hi > r.lo))[0]
        out = []
        for t in m[::-1]:
            _, i, q = self._w[t]
            wr = self.ops[i].writes[q]
            if overlaps(wr, r):
                out.append((i, wr))
        return out

    def latest_writer(self, i, r):
        """(op index, output name) of the last op that runs before op i and writes into r; else "parameter" / "input" / "zeroed once" / "external"; else None"""
        for j, wr in self.writers(r, 0, self.rank[i]):
            return j, wr.name
        for cls, _ in self.region_ranges(r):
            return cls
        return None


def uncovered_reads(plan):
    """[(op, operand, why)]: reads not covered by earlier writes, parameters, inputs or blocks zeroed once; and writes into read-only memory"""
    bad = []
    for o in plan.ops:
        for r in o.reads:
            cov = [c for _, c in plan.region_ranges(r)]
            if cov and covered_by(r, cov):
                continue
            cov += [wr for _, wr in plan.writers(r, 0, plan.rank[o.i])]
            if o.kind == "cemb" and r.name == "tw" and cov:
                continue
            if not covered_by(r, cov):
                bad.append((o, r.name, f"{o} reads {r}: nobody wrote it (candidates {cov[:4]})"))
        for w in o.writes:
            for cls, c in plan.region_ranges(w, classes=("parameter", "input", "external")):
                if overlaps(w, c) and not (cls == "parameter" and w.name == "colstats"):      # (statistics buffers are allocated with the parameters)
                    bad.append((o, w.name, f"{o} writes {w} into {cls} {c}"))
    return bad


def own_operand_overwrites(plan):
    """[(op, output, operand)]: launches whose output lands on one of their own operands.  One form is sound (mlblock.c ln_fold_form): the LayerNorm
    ending's fp16 rows exactly on the A operand, row for row (K == N, lda == N), the residual elsewhere; everything else is a defect."""
    bad = []
    for o in plan.ops:
        for w in o.writes:
            if w.scratch:
                continue
            for r in o.reads:
                if not overlaps(w, r):
                    continue
                a = o.a
                sound = (o.kind == "gemm" and w.name == "ln_y16" and r.name == "A" and a.ln_y16 == a.A and a.K == a.N and a.lda == a.N and a.ldln == a.N
                         and (not a.conv or (a.KH == a.KW == 1 and a.stride == 1 and a.pad == 0 and not a.upsample)))      # (a 1x1 convolution is a Linear over pixels)
                if not sound:
                    bad.append((o, w.name, r.name))
    return bad


def lifetime_diffs(rec, kept):
    """Where the recycling plan `rec` differs from the kept plan in who wrote what a launch reads.  Both plans must list the same ops."""
    bad = []
    if len(rec.ops) != len(kept.ops):
        return [f"{len(rec.ops)} ops in the recycling plan, {len(kept.ops)} in the kept plan"]
    last_reader = {}          # (writer op, output name) -> rank of its last reader, in the kept plan
    for ok, orr in zip(kept.ops, rec.ops):
        if [r.name for r in ok.reads] != [r.name for r in orr.reads] or [w.name for w in ok.writes] != [w.name for w in orr.writes]:
            bad.append(f"{ok}: operands {[r.name for r in ok.reads]} -> {[w.name for w in ok.writes]} in the kept plan, "
                       f"{[r.name for r in orr.reads]} -> {[w.name for w in orr.writes]} in the recycling plan")
            continue
        for rk, rr in zip(ok.reads, orr.reads):
            if rk.scratch:
                continue
            wk, wr = kept.latest_writer(ok.i, rk), rec.latest_writer(orr.i, rr)
            if wk != wr:
                bad.append(f"{ok} operand {rk.name}: written by {wk} in the kept plan, by {wr} in the recycling plan")
            if isinstance(wk, tuple):      # (the pixels of an upsampled map come from four phase launches: the reader keeps all of them alive)
                for w in [wk] + phase_siblings(kept, wk):
                    last_reader[w] = max(last_reader.get(w, -1), kept.rank[ok.i])
    for (j, nm), last in sorted(last_reader.items()):
        lo = rec.rank[j] + 1
        sib = {k for k, _ in phase_siblings(rec, (j, nm))}      # (the phase launches write disjoint pixels of one map: no rewriting among themselves)
        seen = set()
        for w in (x for x in rec.ops[j].writes if x.name == nm and not x.scratch):
            for k, wr in rec.writers(w, lo, last):       # strictly between the writer and its last reader
                if k not in sib and (k, wr.name) not in seen:
                    seen.add((k, wr.name))
                    bad.append(f"{rec.ops[j]} output {nm} is rewritten by {rec.ops[k]} ({wr.name}) before its last reader {rec.ops[rec.order[last]]}")
            if rec.ops[j].once:                        # never run again in later evaluations: nothing may ever write it
                for k, wr in rec.writers(w, lo, len(rec.ops)):
                    if not rec.ops[k].once:
                        bad.append(f"step-invariant {rec.ops[j]} output {nm} is rewritten by {rec.ops[k]} ({wr.name})")
    return bad


def phase_siblings(plan, w):
    """the other phase launches, [(op index, "C32")], of the upsampled map that writer w = (op index, output) is a phase launch of; else []"""
    j, nm = w
    o = plan.ops[j]
    if o.kind != "gemm" or nm != "C32" or not o.a.out_phase:
        return []
    return [(q.i, "C32") for q in plan.ops[max(0, j - 3):j + 4] if q.i != j and q.kind == "gemm" and q.a.out_phase and q.a.C32 == o.a.C32]      # (all four carry the map's base address)


# ------------------------------------------------------------------ op lists without pointers (the keep flag must not change the plan)
def op_signature(o):
    """everything of an op record but its addresses: kind, label, marks, shapes, route and epilogue fields"""
    f = {}
    for name, typ in o.a._fields_:
        v = getattr(o.a, name)
        if typ is ctypes.c_void_p:
            f[name] = bool(v)
        elif name not in ("ws_bytes", "ln_slot"):       # (scratch sizes and slots of the folds: theirs to differ only with the fold itself)
            f[name] = v
    return (o.kind, o.shape_label, o.fused, o.once, tuple(o.gn_src), tuple(sorted(f.items())))


# ------------------------------------------------------------------ the plans the audit builds (dry runtime or device)
class Built:
    """One prepared plan: .ctx (engine.MLCtx), .run(seed) -> the result tensor for seeded inputs (device only), .close()"""

    def __init__(self, ctx, run, keep, external=(), close=None, info=None):
        self.ctx, self.run, self._keep, self.external, self._close, self.info = ctx, run, keep, list(external), close, info or {}

    def close(self):
        self.ctx.destroy()
        if self._close:      # (what the plan read from outside itself lives until here: a ControlNet plan, the driver's buffers)
            self._close()


def _normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


GAIN, FREEU_FACTORS = 0.75, (1.4, 1.6, 0.9, 0.2)      # the control gain and the (b1, b2, s1, s2) of the option plans, as the feature tests use them


def _control_lib():
    import controlnet_ffi as CF
    from mlimgsynth_amd import _lib
    _lib.lib()
    return CF, CF.bind(_lib.LIB_PATH), _lib


def _upload(_lib, ptr, arr):
    arr = np.ascontiguousarray(arr)
    _lib.check(_lib.lib().mlsd_memcpy(_lib.vp(ptr), arr.ctypes.data_as(_lib.vp), ctypes.c_size_t(arr.nbytes), 0, None), "mlsd_memcpy")
    _lib.check(_lib.lib().mlsd_stream_sync(None), "sync")


def _unet_inputs(seed, P, n, lw, lh, n_ctx_tok):
    x = _normal(seed, n, P.n_ch_in, lh, lw)
    x += np.resize(np.array([0.0, 3.0, -10.0, 30.0], np.float32), P.n_ch_in)[None, :, None, None]      # channel means far from zero: badly conditioned first GroupNorm
    cond = _normal(seed + 1, n, n_ctx_tok, P.n_ctx)
    label = _normal(seed + 2, n, P.ch_adm_in) if P.ch_adm_in else None
    sigma = np.linspace(0.7, 9.0, n).astype(np.float32) * (1 + seed % 3)
    return x, cond, label, sigma


class _ControlNet:
    """A ControlNet plan at the context level (controlnet_init_nc / controlnet_build): .ctx, .K (UnetControl: where its residuals lie, for a UNet plan and for
    reading them back), .run(seed, x, cond, label, sigma) on the first n images of a UNet plan's inputs with a seeded hint embedding."""

    def __init__(self, engine, P, lw, lh, n, flags, synth, opt):
        CF, self.lib, self._lib = _control_lib()
        self.engine, self.P, self.n, self.lw, self.lh = engine, P, n, lw, lh
        self.ctx = engine.MLCtx(flags=flags)
        if opt.get("tiling"):
            engine.set_conv_wrap(self.ctx, opt["tiling"])
        if opt.get("hypertile"):
            engine.set_hypertile(self.ctx, opt["hypertile"], opt.get("hypertile_depth", 3))
        self.n_ctx_tok = int(opt.get("n_ctx_tok", 77))
        self.S = CF.ControlState()
        engine.check1(self.lib.controlnet_init_nc(ctypes.byref(self.S), self.ctx.h, ctypes.addressof(P), lw, lh, n, self.n_ctx_tok), "controlnet_init_nc")
        engine.check1(self.lib.controlnet_build(ctypes.byref(self.S)), "controlnet_build")
        if synth:
            self.ctx.params_synth(1234)
        self.gain = self._lib.from_numpy(np.array([GAIN], np.float32))
        self.K = CF.UnetControl()
        engine.check1(self.lib.controlnet_control(ctypes.byref(self.S), self.gain.ptr, ctypes.byref(self.K)), "controlnet_control")
        ld = ctypes.c_int64()
        self.hint = self.lib.mlctx_tensor_device_f32(self.ctx.h, self.S.t_hint, ctypes.byref(ld))
        if not self.hint or ld.value != P.n_ch:
            raise Unknown(f"ControlNet hint embedding at {self.hint} with rows of {ld.value} floats")
        self.hint_bytes = n * lw * lh * P.n_ch * 4

    def residuals(self):
        """[(name, address, bytes)] of the residuals, from their first to their last element"""
        K = self.K
        return [(f"control residual {i}", K.r[i], ((K.n_img * K.rows[i] - 1) * K.ld[i] + K.c[i]) * 4) for i in range(K.n)]

    def run(self, seed, x, cond, label, sigma):
        e, lib, C, S, n = self.engine, self.lib, self.ctx.h, self.S, self.n
        c_in = (1 / np.sqrt(sigma[:n].astype(np.float32) ** 2 + 1)).astype(np.float32)
        xs = np.ascontiguousarray(x[:n] * c_in[:, None, None, None], np.float32)
        ts = np.array([e.L().unet_sigma_to_t(ctypes.byref(self.P), float(s)) for s in sigma[:n]], np.float32)
        for t, a in ((S.t_x, xs), (S.t_t, ts), (S.t_c, np.ascontiguousarray(cond[:n])), (S.t_l, None if label is None else np.ascontiguousarray(label[:n]))):
            if t and a is not None:
                e.check1(lib.mlctx_input_set(C, t, a.ctypes.data_as(ctypes.c_void_p), a.nbytes), "mlctx_input_set")
        _upload(self._lib, self.hint, 0.5 * _normal(seed + 3, n, self.lh * self.lw, self.P.n_ch))
        e.check1(lib.mlctx_compute_checked(C), "mlctx_compute_checked")
        self.ctx.sync()

    def read(self):
        mem, K = DeviceMemory(self._lib), self.K
        return np.concatenate([_mat(mem, K.r[i], K.n_img * K.rows[i], K.c[i], K.ld[i], np.float32).reshape(-1) for i in range(K.n)])

    def close(self):
        self.ctx.destroy()
        self.gain.free()


def _build_option_unet(engine, model, P, lw, lh, n, flags, synth, opt, option):
    """the UNet plan with a ControlNet's residuals (control: images of the ControlNet plan; gain), FreeU (freeu) and / or the forced phase form of its upsampling
    convolutions (ups_phases), at the context level: unet_denoise_build_freeu with a UnetControl and a UnetFreeU"""
    CF, lib, _lib = _control_lib()
    L = engine.L()
    n_ctrl, gain, ups = option.get("control"), float(option.get("gain", GAIN)), option.get("ups_phases")
    net = ff = None
    ext, info = [], {}
    if ups is not None:
        L.mlsd_gemm_set_ups_phases(int(ups))
    try:
        if n_ctrl:      # the ControlNet plan first: the UNet plan is recorded on the addresses of its residuals
            net = _ControlNet(engine, P, lw, lh, n_ctrl, flags, synth, opt)
            _upload(_lib, net.gain.ptr, np.array([gain], np.float32))
            ext += net.residuals() + [("control gain", net.gain.ptr, 4)]
        un = engine.Unet.__new__(engine.Unet)
        un.P, un.ctx = P, engine.MLCtx(None, flags)
        if opt.get("hypertile"):
            engine.set_hypertile(un.ctx, opt["hypertile"], opt.get("hypertile_depth", 3))
        if opt.get("pag"):
            L.mlctx_set_pag.restype, L.mlctx_set_pag.argtypes = None, [engine.vp, ctypes.c_int]
            L.mlctx_set_pag(un.ctx.h, int(opt["pag"]))
        if opt.get("tiling"):
            engine.set_conv_wrap(un.ctx, opt["tiling"])
        if set(opt) - {"hypertile", "hypertile_depth", "pag", "tiling", "n_ctx_tok"}:
            raise Unknown(f"option plan with {sorted(opt)}")
        un.S, un.lw, un.lh, un.n, un.n_ctx_tok = engine.UnetState(), lw, lh, n, int(opt.get("n_ctx_tok", 77))
        engine.check1(L.unet_denoise_init_nc(ctypes.byref(un.S), un.ctx.h, ctypes.byref(P), lw, lh, n, un.n_ctx_tok), "unet_denoise_init_nc")
        F = None
        if option.get("freeu"):
            ff = _lib.from_numpy(np.array(FREEU_FACTORS, np.float32))
            F = CF.UnetFreeU(f=ff.ptr)
            ext.append(("FreeU factors", ff.ptr, 16))
        engine.check1(lib.unet_denoise_build_freeu(ctypes.addressof(un.S), ctypes.byref(net.K) if net else None, ctypes.byref(F) if F else None), "unet_denoise_build_freeu")
        if F:
            info["freeu_stages"] = (F.n_stage1, F.n_stage2)
        if synth:
            un.ctx.params_synth(1234)
    finally:
        if ups is not None:
            L.mlsd_gemm_set_ups_phases(-1)

    def poison_phase_outputs():      # an fp32 map the four phase launches fill: NaN before the evaluation, so an unwritten pixel is seen (kept plans: the block is the map's alone)
        for kind, _, _, _, _, a in (un.ctx.op_records() if flags & MLB_F_KEEP else ()):
            if kind == "gemm" and a.out_phase == 1:
                _upload(_lib, a.C32, np.full(4 * a.M * a.ldc32, np.nan, np.float32))

    def run(seed):
        x, cond, label, sigma = _unet_inputs(seed, P, n, lw, lh, un.n_ctx_tok)
        if ups is not None:      # (the launcher asks the mode again at every launch)
            L.mlsd_gemm_set_ups_phases(int(ups))
        try:
            if net:
                net.run(seed, x, cond, label, sigma)
                if gain == 0.0:      # the residuals are never read then: poison them
                    for _, ptr, nb in net.residuals():
                        _upload(_lib, ptr, np.full(nb // 4, np.nan, np.float32))
            poison_phase_outputs()
            return un.run(x, cond, label, sigma)
        finally:
            if ups is not None:
                L.mlsd_gemm_set_ups_phases(-1)

    def close():
        if net:
            net.close()
        if ff:
            ff.free()
    info["control"] = net
    return Built(un.ctx, run, (un, P), ext, close, info)


def build(engine, spec, flags=0, synth=False):
    """spec: ("unet", model, lat | (lw, lh), n[, dict(n_ctx_tok=, tiling=, stream_weights_mib=, params=, hypertile=, pag=, control=, gain=, freeu=, ups_phases=)])
    | ("vae_dec" | "vae_enc" | "tae_dec" | "tae_enc", model, lat, n[, dict(tiling=)]) | ("clip", model, n_prompt) | ("controlnet", model, lat, n) | ("control_hint", model, lat).
    control: the images of the ControlNet plan whose residuals the UNet plan adds (gain: 0.75), freeu: the FreeU passes with the factors (1.4, 1.6, 0.9, 0.2),
    ups_phases: mlsd_gemm_set_ups_phases around build and run.  synth: fill the parameters with the synthetic weights (seed 1234; needs a device)."""
    kind, model, opt = spec[0], spec[1], (spec[4] if len(spec) > 4 else {})
    l = engine._proto2()
    vp, FP = engine.vp, engine.FP
    if kind == "unet":
        (lw, lh), n = (spec[2] if isinstance(spec[2], tuple) else (spec[2], spec[2])), spec[3]
        opt = dict(opt)
        over = opt.pop("params", None)
        option = {k: opt.pop(k) for k in ("control", "gain", "freeu", "ups_phases") if k in opt}
        if option:
            P = engine.unet_params(model)
            for k, v in (over or {}).items():
                setattr(P, k, v)
            return _build_option_unet(engine, model, P, lw, lh, n, flags, synth, opt, option)
        if over:      # the named configuration with other hyper-parameters (another width): engine.Unet asks unet_params for them
            orig = engine.unet_params

            def patched(m):
                P = orig(m)
                for k, v in over.items():
                    setattr(P, k, v)
                return P
            engine.unet_params = patched
        try:
            un = engine.Unet(model, lw, lh, n, flags=flags, synth=synth, **opt)
        finally:
            if over:
                engine.unet_params = orig
        P = un.P

        def run(seed):
            return un.run(*_unet_inputs(seed, P, n, lw, lh, un.n_ctx_tok))
        return Built(un.ctx, run, un)
    if kind in ("controlnet", "control_hint"):
        P = engine.unet_params(model)
        if kind == "controlnet":
            lat, n = spec[2], spec[3]
            net = _ControlNet(engine, P, lat, lat, n, flags, synth, opt)

            def run(seed):
                net.run(seed, *_unet_inputs(seed, P, n, lat, lat, net.n_ctx_tok))
                return net.read()
            # (the hint embedding is written by the driver straight into the plan's memory, by no launch; the gain is not read by this plan)
            return Built(net.ctx, run, (net, P), [("hint embedding", net.hint, net.hint_bytes)], net.gain.free)
        CF, lib, _lib = _control_lib()
        lat, side = spec[2], 8 * spec[2]
        ctx, t = engine.MLCtx(flags=flags), vp()
        engine.check1(lib.control_hint_init(ctx.h, ctypes.addressof(P), side, side, ctypes.byref(t)), "control_hint_init")
        engine.check1(lib.control_hint_build(ctx.h, ctypes.addressof(P), t), "control_hint_build")
        if synth:
            ctx.params_synth(1234)

        def run(seed):
            img = np.random.default_rng(seed).random((1, 3, side, side)).astype(np.float32)
            out = np.empty((1, P.n_ch, lat, lat), np.float32)
            engine.check1(lib.mlctx_input_set(ctx.h, t, img.ctypes.data_as(vp), img.nbytes), "mlctx_input_set")
            engine.check1(lib.mlctx_compute_checked(ctx.h), "mlctx_compute_checked")
            engine.check1(lib.mlctx_output_get(ctx.h, lib.mlctx_result(ctx.h), out.ctypes.data_as(vp), out.nbytes), "mlctx_output_get")
            return out
        return Built(ctx, run, (t, P))
    ctx = engine.MLCtx(flags=flags)
    if opt.get("tiling"):
        engine.set_conv_wrap(ctx, opt["tiling"])
    t = vp()
    if kind in ("vae_dec", "vae_enc"):
        lat, n = spec[2], spec[3]
        P = engine.VaeParams()
        engine.check1(l.vae_params_get(model.encode(), ctypes.byref(P)), "vae_params_get")
        side = lat * 8
        if kind == "vae_dec":
            engine.check1(l.sdvae_decode_init(ctx.h, ctypes.byref(P), lat, lat, n, ctypes.byref(t)), "sdvae_decode_init")
            engine.check1(l.sdvae_decode_build(ctx.h, ctypes.byref(P), t), "sdvae_decode_build")

            def run(seed):
                out = np.empty((n, 3, side, side), np.float32)
                engine.check1(l.sdvae_decode_run(ctx.h, t, engine.fptr(_normal(seed, n, 4, lat, lat)), engine.fptr(out)), "sdvae_decode_run")
                return out
        else:
            l.sdvae_encode_init.argtypes = [vp, ctypes.POINTER(engine.VaeParams), ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(vp)]
            l.sdvae_encode_build.argtypes = [vp, ctypes.POINTER(engine.VaeParams), vp]
            l.sdvae_encode_run.argtypes = [vp, vp, FP, FP]
            engine.check1(l.sdvae_encode_init(ctx.h, ctypes.byref(P), side, side, n, ctypes.byref(t)), "sdvae_encode_init")
            engine.check1(l.sdvae_encode_build(ctx.h, ctypes.byref(P), t), "sdvae_encode_build")

            def run(seed):
                out = np.empty((n, 2 * P.ch_z, lat, lat), np.float32)
                img = np.random.default_rng(seed).random((n, 3, side, side)).astype(np.float32)
                img[:, 1] = 0.98 + 0.02 * img[:, 1]                  # a nearly constant bright channel
                engine.check1(l.sdvae_encode_run(ctx.h, t, engine.fptr(img), engine.fptr(out)), "sdvae_encode_run")
                return out
    elif kind in ("tae_dec", "tae_enc"):
        lat, n = spec[2], spec[3]
        side = lat * 8
        if kind == "tae_dec":
            engine.check1(l.sdtae_decode_init(ctx.h, lat, lat, n, ctypes.byref(t)), "sdtae_decode_init")
            engine.check1(l.sdtae_decode_build(ctx.h, t), "sdtae_decode_build")

            def run(seed):
                out = np.empty((n, 3, side, side), np.float32)
                engine.check1(l.sdtae_decode_run(ctx.h, t, engine.fptr(3.0 * _normal(seed, n, 4, lat, lat)), engine.fptr(out)), "sdtae_decode_run")
                return out
        else:
            l.sdtae_encode_init.argtypes = [vp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(vp)]
            l.sdtae_encode_build.argtypes = [vp, vp]
            l.sdtae_encode_run.argtypes = [vp, vp, FP, FP]
            engine.check1(l.sdtae_encode_init(ctx.h, side, side, n, ctypes.byref(t)), "sdtae_encode_init")
            engine.check1(l.sdtae_encode_build(ctx.h, t), "sdtae_encode_build")

            def run(seed):
                out = np.empty((n, 4, lat, lat), np.float32)
                img = np.random.default_rng(seed).random((n, 3, side, side)).astype(np.float32)
                engine.check1(l.sdtae_encode_run(ctx.h, t, engine.fptr(img), engine.fptr(out)), "sdtae_encode_run")
                return out
    elif kind == "clip":
        n = spec[2]
        P = engine.ClipParams()
        engine.check1(l.clip_params_get(model.encode(), ctypes.byref(P)), "clip_params_get")
        E = ctypes.create_string_buffer(512)      # ClipEncoder (include/mlimgsynth_amd.h): 112 bytes
        l.clip_encoder_init.argtypes = [vp, vp, ctypes.POINTER(engine.ClipParams), ctypes.c_char_p, ctypes.c_uint, ctypes.c_int, ctypes.c_bool, ctypes.c_bool]
        l.clip_encoder_run.argtypes = [vp, ctypes.c_uint, ctypes.POINTER(ctypes.c_int32), FP, FP]
        engine.check1(l.clip_encoder_init(E, ctx.h, ctypes.byref(P), b"clip", n, 1, True, False), "clip_encoder_init")

        def run(seed):
            n_tok = 5 + seed % 7
            toks = np.random.default_rng(seed).integers(0, P.n_vocab - 2, (n, n_tok)).astype(np.int32)
            out = np.empty((n, P.n_token, P.d_embed), np.float32)
            engine.check1(l.clip_encoder_run(E, n_tok, toks.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), engine.fptr(out), None), "clip_encoder_run")
            return out
        t = E
    else:
        raise Unknown(f"plan {spec}")
    if synth:
        ctx.params_synth(1234)
    return Built(ctx, run, t)


# the test-size plans of the static audit and of the launch-by-launch check
TEST_PLANS = [
    ("unet", "tiny", 16, 2), ("unet", "tinyxl", 16, 2), ("unet", "sd1", 16, 2), ("unet", "sdxl", 16, 2),
    ("vae_dec", "tiny", 8, 1), ("vae_enc", "tiny", 8, 1), ("tae_dec", "tiny", 8, 1), ("tae_enc", "tiny", 8, 1),
    ("vae_dec", "tiny", 8, 2), ("clip", "tiny", 2), ("clip", "vit_l", 2), ("clip", "vit_bigg", 2),
]
VARIANT_PLANS = [
    ("unet", "tinyxl", 16, 2, dict(n_ctx_tok=154)), ("unet", "sd1", 16, 2, dict(n_ctx_tok=154)),       # windowed context (long prompt)
    ("unet", "tinyxl", 16, 2, dict(tiling=3)), ("vae_dec", "tiny", 8, 1, dict(tiling=3)),              # seamless tiling
    ("unet", "tinyxl", 16, 2, dict(stream_weights_mib=1)),                                            # weight streaming
]
# as bench.py builds them: SD1.5 64x64 N = 2 and SDXL 128x128 batch 4 (N = 8), and their KL-VAE decoders
BENCH_PLANS = [("unet", "sd1", 64, 2), ("unet", "sdxl", 128, 8), ("vae_dec", "sd1", 64, 1), ("vae_dec", "sdxl", 128, 4)]

# Sizes other than the two benchmarks, for the op-form census only (built, never computed): which tile a GEMM takes is a function of its exact shape (an exact hit in
# the tune table, a neighbour's tile from 1024 rows on, else the launcher's static rule), and each (tile, split form, epilogue features) selects its own epilogue body.
# N = images x guidance groups: 1 = guidance off, 2 = batch 1, 3 = batch 1 with PAG, 4 = batch 2, ...
SIZE_PLANS = [
    # SD1.5: the square bench latent at the other row counts (N = 1 is the API's default with guidance off) ...
    ("unet", "sd1", 64, 1), ("unet", "sd1", 64, 3), ("unet", "sd1", 64, 4), ("unet", "sd1", 64, 6), ("unet", "sd1", 64, 8),
    # ... portrait, landscape and 768 x 768; latents whose deepest level has odd extents (9 x 11, 11 x 9); a small latent (deepest level 5 x 5)
    ("unet", "sd1", (64, 96), 2), ("unet", "sd1", (96, 64), 2), ("unet", "sd1", 96, 2),
    ("unet", "sd1", (72, 88), 2), ("unet", "sd1", (88, 72), 1), ("unet", "sd1", 40, 2),
    # SDXL: 1024 x 1024 at the row counts below the bench's ...
    ("unet", "sdxl", 128, 1), ("unet", "sdxl", 128, 2), ("unet", "sdxl", 128, 3), ("unet", "sdxl", 128, 4), ("unet", "sdxl", 128, 6),
    # ... the 832 x 1216 bucket both ways and at batch 4, other buckets, small squares ...
    ("unet", "sdxl", (104, 152), 2), ("unet", "sdxl", (152, 104), 2), ("unet", "sdxl", (104, 152), 8),
    ("unet", "sdxl", (112, 144), 2), ("unet", "sdxl", (168, 96), 2), ("unet", "sdxl", 96, 2), ("unet", "sdxl", 64, 2), ("unet", "sdxl", (120, 136), 4),
    # ... a deepest level of 25 x 25 = 625 rows per image (no multiple of 64), and the bench size with a long prompt (two context windows)
    ("unet", "sdxl", 100, 1), ("unet", "sdxl", 100, 2), ("unet", "sdxl", 128, 8, dict(n_ctx_tok=154)),
    # the KL-VAE decoders and encoders at other sizes and batches, and TAESD both ways
    ("vae_dec", "sd1", 96, 1), ("vae_dec", "sdxl", 128, 1), ("vae_dec", "sdxl", 96, 2), ("vae_dec", "sdxl", 100, 1),
    ("vae_enc", "sdxl", 128, 1), ("vae_enc", "sd1", 64, 1), ("tae_dec", "sd1", 64, 1), ("tae_enc", "sd1", 64, 1),
]
# latents that do not halve evenly down the UNet's levels: refused when the plan is built ("concat: shape mismatch")
REFUSED_LATENTS = [("unet", "sd1", (68, 64), 2), ("unet", "sd1", 65, 2), ("unet", "sdxl", (130, 128), 2)]


def unheld_forms(keys_by_plan, held):
    """{form: [plan ids]} of the census keys that are not in `held`.  keys_by_plan: {plan id: census keys of its ops}; held: the keys met in audited plans or bench
    plans, and those COVERED_ELSEWHERE lists with the float64 case of exactly that form."""
    out = {}
    for pid, keys in keys_by_plan.items():
        for k in keys:
            if k not in held:
                out.setdefault(k, []).append(pid)
    return {k: out[k] for k in sorted(out, key=str)}


def plan_id(spec):
    one = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else (",".join(f"{k}{one(w)}" for k, w in v.items()) if isinstance(v, dict) else str(v))
    return "-".join(one(s) for s in spec)


# ------------------------------------------------------------------ operands still intact (precondition of verify_op)
def clobbered_operands(plan):
    """[(writer op, output, reader op, operand)]: writes that land on a range an EARLIER op read (other than the writer's own operands).  In a kept plan
    there must be none: otherwise the values that reader saw are gone when the evaluation ends, and verify_op would judge it on other data."""
    reads = [(plan.rank[o.i], o.i, r) for o in plan.ops for r in o.reads if not r.scratch]
    rk = np.array([t[0] for t in reads], np.int64)
    lo = np.array([t[2].lo for t in reads], np.int64)
    hi = np.array([t[2].hi for t in reads], np.int64)
    bad = []
    for o in plan.ops:
        for w in o.writes:
            if w.scratch:
                continue
            for t in np.nonzero((rk < plan.rank[o.i]) & (lo < w.hi) & (hi > w.lo))[0]:
                _, j, r = reads[t]
                if overlaps(w, r):
                    bad.append((o, w.name, plan.ops[j], r.name))
    return bad


# ------------------------------------------------------------------ memory
class DictMemory:
    """memory image of the self-test: {address: numpy array}; a read must lie inside one array"""

    def __init__(self):
        self.blocks, self.next = {}, 0x10000

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.next
        self.blocks[p] = arr.view(np.uint8).reshape(-1).copy()
        self.next = (p + arr.nbytes + 4095) // 4096 * 4096 + 4096
        return p

    def read(self, ptr, nbytes):
        for p, b in self.blocks.items():
            if p <= ptr and ptr + nbytes <= p + b.size:
                return b[ptr - p:ptr - p + nbytes]
        raise Unknown(f"read of {nbytes} bytes at {ptr:#x} outside the memory image")

    def view(self, ptr, dtype):
        """writable typed view from ptr to the end of its block (planting faults)"""
        for p, b in self.blocks.items():
            if p <= ptr < p + b.size:
                return b[ptr - p:].view(dtype)
        raise Unknown(f"no block at {ptr:#x}")


class DeviceMemory:
    """device memory by raw pointer (mlsd_memcpy, device to host)"""

    def __init__(self, _lib):
        self._lib = _lib

    def read(self, ptr, nbytes):
        out = np.empty(nbytes, np.uint8)
        L = self._lib.lib()
        self._lib.check(L.mlsd_memcpy(out.ctypes.data_as(self._lib.vp), self._lib.vp(ptr), ctypes.c_size_t(nbytes), 1, None), "mlsd_memcpy")
        self._lib.check(L.mlsd_device_sync(), "sync")
        return out


def _mat(mem, ptr, rows, cols, ld, dtype):
    """rows x cols matrix of dtype at ptr with row stride ld (elements), as a copy"""
    esz = np.dtype(dtype).itemsize
    if not ptr:
        raise Unknown("NULL operand")
    flat = np.frombuffer(bytes(mem.read(int(ptr), ((rows - 1) * ld + cols) * esz)), dtype)
    return np.lib.stride_tricks.as_strided(flat, (rows, cols), (ld * esz, esz)).copy()


def _vec(mem, ptr, n, dtype=np.float32):
    return _mat(mem, ptr, 1, n, n, dtype)[0]


def _bits_equal(got, want):
    """0.0 if the two arrays hold the same bits, else inf"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return 0.0 if g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8)) else float("inf")


def _worst(r):
    r = np.asarray(r, np.float64)
    return float(np.nan_to_num(r, nan=np.inf, posinf=np.inf).max()) if r.size else 0.0


GENERAL_TILES = (GC.G0, GC.G1, GC.G3, GC.G4, GC.G9, GC.G16)      # gemm_kernel (32x32x16 MFMA); every other tile steps K by 32


def gemm_path(label):
    """(tile, form, k_step, nsplit incl. the stream-K hand-overs' share) of an mlsd_gemm_variant label, as tests/test_gemm_float64_gpu.py reads it"""
    m = re.match(r"gemm<([^,>]+),([a-z]+)(\+[a-z]+)?(,k/(\d+)p?)?>", label)
    if not m:
        raise Unknown(f"gemm label {label!r}")
    tile, plus = m.group(1), (m.group(3) or "")[1:]
    form = "linear+attention" if plus == "attention" else ("layernorm" if plus == "layernorm" else ("groupnorm" if plus == "groupnorm" else ""))
    if plus not in ("", "attention", "layernorm", "groupnorm"):
        raise Unknown(f"gemm label {label!r}: ending {plus!r}")
    ns = int(m.group(5)) if m.group(5) else 1
    if ns > 1 and tile != GC.SK29:
        form = (form + "+" if form else "") + "splitk"
    return tile, form, (R.K_STEP_GENERAL if tile in GENERAL_TILES else R.K_STEP_MFMA16), ns


def _phase_launches(ops, op):
    """{out_phase: op} of the phase launches in `ops` that write the upsampled map op writes"""
    return {o.a.out_phase: o for o in ops if o.kind == "gemm" and o.a.out_phase and o.a.C32 == op.a.C32}


def _verify_gemm(mem, op, ops=(), ups=()):
    from mlimgsynth_amd import kernels
    a = op.a
    phase = phase_of(a)
    label = kernels.gemm_variant(a)
    tile, form, k_step, ns = gemm_path(label)
    M, N, K, nout = a.M, a.N, a.K, _gemm_nout(a)
    if a.act not in (0, 1, 2, 3, 4, 5):
        raise Unknown(f"gemm activation {a.act}")
    if a.conv:
        x = _mat(mem, a.A, a.n_img * a.H * a.W, a.Cin, a.lda, np.float16)
        if phase:
            A = R.phase_A(x.reshape(a.n_img, a.H, a.W, a.Cin), phase[0], phase[1], a.wrap)
        else:
            A = R.im2col64(x, a.n_img, a.H, a.W, a.Cin, a.KH, a.KW, a.stride, a.pad, a.upsample, a.OH, a.OW, wrap=a.wrap)
    else:
        if a.upsample or a.wrap:
            raise Unknown("upsample / wrap on a launch that is no convolution")
        A = _mat(mem, a.A, M, K, a.lda, np.float16)
    W = _mat(mem, a.W_, N, K, a.ldb, np.float16)
    acc, S = R.gemm64(A, W)
    D = R.gemm_depth(K, k_step, ns + (K // 64 if "ppsk" in tile else 0))
    rpb = max(a.rows_per_batch, 1)
    y, b = R.gemm_epilogue64(acc, S, D, np.arange(M), np.arange(nout),
                             bias=_vec(mem, a.bias, N) if a.bias else None,
                             rowbias=_mat(mem, a.rowbias, M // rpb, N, a.ldrb, np.float32) if a.rowbias else None, rows_per_batch=rpb,
                             bias_m=_vec(mem, a.bias_m, M) if a.bias_m else None, act=a.act,
                             resid=_mat(mem, a.resid, M, nout, a.ldr, np.float32) if a.resid else None, act_after_resid=bool(a.act_after_resid))
    out, got32 = {}, None
    if phase:
        # the launch's pixels (2 y + py, 2 x + px) of the [n_img][2 H][2 W] map against its own operands; the bound of an fp32 convolution output
        full = _mat(mem, a.C32, 4 * M, N, a.ldc32, np.float32).reshape(a.n_img, 2 * a.H, 2 * a.W, N)
        out["C32"] = _worst(R.gemm_ratio32(full[:, phase[0]::2, phase[1]::2].reshape(M, N), y, b))
        # The pixels of the other three parities are not this launch's.  When the evaluation has ended each of them holds what the launch of ITS parity
        # wrote (that launch's own check says so, and a stray write that survived fails there or in the assembled map below), or, where the plan has no
        # launch for a parity, still the poison the map was filled with
        sib = _phase_launches(ops, op)
        lone = [full[:, q >> 1::2, q & 1::2] for q in range(4) if q + 1 not in sib and q + 1 != a.out_phase]
        out["other parities"] = 0.0 if all(np.isnan(v).all() for v in lone) else float("inf")
        if a.out_phase == 4:      # the assembled map against float64 of the original form, upsample + 3x3 with the loaded weight: U16 S' + b (tests/test_upsample_phases_gpu.py)
            if sorted(sib) != [1, 2, 3, 4] or any((o.a.A, o.a.bias, o.a.N, o.a.K, o.a.ldb, o.a.wrap, o.a.lda) != (a.A, a.bias, N, K, a.ldb, a.wrap, a.lda) for o in sib.values()):
                raise Unknown(f"{op}: phase launch 4 without its three sibling launches on the same operands")
            src = [u for u in ups if u[0] == sib[1].a.W_ and u[2] == N and u[3] == a.Cin]
            if len(src) != 1 or any(sib[q].a.W_ != src[0][0] + (q - 1) * N * K * 2 for q in sib):
                raise Unknown(f"{op}: phase launches whose weights are not the derived weights of one loaded 3x3 parameter")
            w3 = _mat(mem, src[0][1], N, 9 * a.Cin, 9 * a.Cin, np.float16).astype(np.float64)
            A3 = R.im2col64(x, a.n_img, a.H, a.W, a.Cin, 3, 3, 1, 1, 1, 2 * a.H, 2 * a.W, wrap=a.wrap)
            y3 = (A3 @ w3.T + (_vec(mem, a.bias, N).astype(np.float64) if a.bias else 0.0)).reshape(full.shape)
            w = 0.0
            for q, o in sib.items():
                qy, qx = phase_of(o.a)
                acc_q, S_q = (acc, S) if q == 4 else R.gemm64(R.phase_A(x.reshape(a.n_img, a.H, a.W, a.Cin), qy, qx, a.wrap), _mat(mem, o.a.W_, N, K, a.ldb, np.float16))
                _, b_q = R.gemm_epilogue64(acc_q, S_q, D, np.arange(M), np.arange(N), bias=_vec(mem, a.bias, N) if a.bias else None)
                w = max(w, _worst(R.gemm_ratio32(full[:, qy::2, qx::2].reshape(M, N), y3[:, qy::2, qx::2].reshape(M, N), R.U16 * S_q + b_q)))
            out["assembled"] = w
    elif a.C32:
        got32 = _mat(mem, a.C32, M, nout, a.ldc32, np.float32)
        out["C32"] = _worst(R.gemm_ratio32(got32, y, b))
    if a.xa_k:
        if a.xa_Tk > 96 or N % 64:
            raise Unknown("cross-attention ending beyond 96 keys or heads of 64")
        n_img, heads = M // a.xa_Tq, N // 64
        q = R.fp16_rne(y).astype(np.float64)          # the projection as the unfused launch's C16 would hold it ...
        dq = R.fp16_tie_ulp(y, b)                     # ... up to one fp16 ulp where the launch's fp32 value may fall on the other side of a tie
        kk = _mat(mem, a.xa_k, n_img * a.xa_Tk, N, a.xa_ldk, np.float16)
        vt = _vec(mem, a.xa_vt, n_img * N * 96, np.float16).reshape(n_img, N, 96)
        got = _mat(mem, a.xa_out, M, N, a.xa_ldo, np.float16)
        w = 0.0
        for i in range(n_img):
            qi, ki, vi = q[i * a.xa_Tq:(i + 1) * a.xa_Tq], kk[i * a.xa_Tk:(i + 1) * a.xa_Tk], vt[i, :, :a.xa_Tk].T
            o, p = R.attention64(qi, ki, vi, heads)
            bound = R.attention_bound(qi, ki, vi, heads, o, p, False) + R.attention_dq_term(dq[i * a.xa_Tq:(i + 1) * a.xa_Tq], ki, vi, heads, o, p)
            w = max(w, _worst(R.attention_worst(got[i * a.xa_Tq:(i + 1) * a.xa_Tq], o, bound)))
        out["xa_out"] = w
    elif a.C16:
        got16 = _mat(mem, a.C16, M, nout, a.ldc16, np.float16)
        out["C16"] = _worst(R.gemm_ratio16(got16, y, b))
        if got32 is not None:
            out["C16==rne(C32)"] = _bits_equal(got16, R.fp16_rne(got32))
    if a.colstats:
        if got32 is None:
            raise Unknown("column statistics without an fp32 output")
        rows = _stats_rows(a)
        st = _vec(mem, a.colstats, (M // rows) * 2 * N).reshape(M // rows, 2, N)
        es, eq = R.colstats_ratios(got32, st, rows, shifted=bool(a.colstats_shift))
        out["colstats"] = max(_worst(es), _worst(eq))
    if a.ln_y16:
        if got32 is None:
            raise Unknown("LayerNorm ending without an fp32 output")
        g, be = _vec(mem, a.ln_gamma, N), (_vec(mem, a.ln_beta, N) if a.ln_beta else None)
        got = _mat(mem, a.ln_y16, M, N, a.ldln, np.float16)
        want = R.layernorm64(got32, a.ln_eps, g, be)
        out["ln_y16"] = _worst(R.layernorm_worst(got, want, got32, a.ln_eps, g, be)[0])
    if a.gn_y16:
        if got32 is None or a.gn_hw <= 0 or M % a.gn_hw:
            raise Unknown("GroupNorm ending without an fp32 output or with rows that do not divide M")
        g, be = _vec(mem, a.gn_gamma, N), _vec(mem, a.gn_beta, N)
        x = got32.reshape(M // a.gn_hw, a.gn_hw, N)
        got = _mat(mem, a.gn_y16, M, N, a.gn_ldy, np.float16).reshape(x.shape)
        want = R.groupnorm64(x, None, a.gn_groups, a.gn_eps, g, be, bool(a.gn_silu))
        out["gn_y16"] = _worst(R.groupnorm_worst(got, want, x, a.gn_groups, a.gn_eps, g, be)[0])
    return (op.kind, f"{tile} {form}".strip() + (" phase" if phase else "")), out


def _verify_attn(mem, op):
    from mlimgsynth_amd import kernels
    a = op.a
    ctx = op.kind == "attn_ctx"
    label = kernels.attention_variant(a, ctx)
    if label is None:
        raise Unknown("attention launch the launcher would refuse")
    if ctx and a.causal:
        raise Unknown("causal mask on mlsd_attention_ctx")
    q_scaled = label.startswith("attn<64x2s") or label.startswith("attn<pp")
    D, w = a.n_head * a.d_head, 0.0
    for b in range(a.n_batch):
        q = _mat(mem, a.q + 2 * b * a.bsq, a.Tq, D, a.ldq, np.float16)
        k = _mat(mem, a.k + 2 * b * a.bsk, a.Tk, D, a.ldk, np.float16)
        v = _mat(mem, a.v + 2 * b * a.bsv, a.Tk, D, a.ldv, np.float16)
        got = _mat(mem, a.out + 2 * b * a.bso, a.Tq, D, a.ldo, np.float16)
        o, p = R.attention64(q, k, v, a.n_head, causal=bool(a.causal))
        w = max(w, _worst(R.attention_worst(got, o, R.attention_bound(q, k, v, a.n_head, o, p, q_scaled))))
    return (op.kind, label), {"out": w}


def _verify_gn(mem, op):
    a = op.a
    n, hw, C = a.n_img, a.HW, a.C1 + a.C2
    x = _mat(mem, a.x1, n * hw, a.C1, a.ld1, np.float32)
    if a.C2:
        x = np.concatenate([x, _mat(mem, a.x2, n * hw, a.C2, a.ld2, np.float32)], axis=1)
    x = x.reshape(n, hw, C)
    g, be = _vec(mem, a.gamma, C), _vec(mem, a.beta, C)
    got = _vec(mem, a.y16, n * hw * C, np.float16).reshape(n, hw, C)
    want = R.groupnorm64(x, None, a.n_grp, a.eps, g, be, bool(a.silu))
    out = {"y16": _worst(R.groupnorm_worst(got, want, x, a.n_grp, a.eps, g, be)[0])}
    if a.raw16:
        out["raw16"] = _bits_equal(_vec(mem, a.raw16, n * hw * C, np.float16).reshape(n, hw, C), R.fp16_rne(x))
    path = ("concat" if a.C2 else "one source") + (", producer statistics" if a.cs1 else "") + (", silu" if a.silu else "") + (", raw16" if a.raw16 else "")
    return (op.kind, path), out


def _verify_ln(mem, op):
    a = op.a
    x = _mat(mem, a.x, a.rows, a.d, a.ldx, np.float32)
    g, be = _vec(mem, a.g, a.d), (_vec(mem, a.b, a.d) if a.b else None)
    want = R.layernorm64(x, a.eps, g, be)
    out = {}
    if a.y16:
        out["y16"] = _worst(R.layernorm_worst(_vec(mem, a.y16, a.rows * a.d, np.float16).reshape(a.rows, a.d), want, x, a.eps, g, be)[0])
    if a.y32:
        out["y32"] = _worst(R.layernorm_worst(_vec(mem, a.y32, a.rows * a.d).reshape(a.rows, a.d), want, x, a.eps, g, be, half=False)[0])
    return (op.kind, "y16" + ("+y32" if a.y32 else "")), out


def _f32(x):
    return np.asarray(x, np.float32)


def _verify_small(mem, op):
    k, a = op.kind, op.a
    if k == "n2h":
        src = _vec(mem, a.src, a.n_src * a.C * a.HW).reshape(a.n_src, a.C, a.HW)
        s = _vec(mem, a.scale, a.n_src) if a.scale else np.full(a.n_src, a.scale0, np.float32)
        got = _vec(mem, a.dst, a.n_dst * a.HW * a.Cpad, np.float16).reshape(a.n_dst, a.HW, a.Cpad)
        idx = np.arange(a.n_dst) % a.n_src
        v = src[idx].transpose(0, 2, 1)                     # [n_dst][HW][C]
        sv = s[idx][:, None, None]
        out = {"pad": _bits_equal(got[:, :, a.C:], np.zeros_like(got[:, :, a.C:]))}
        if a.mode in (0, 2):
            if a.mode == 2:
                v = _f32(_f32(v * np.float32(2.0)) - np.float32(1.0))
            out["dst"] = _bits_equal(got[:, :, :a.C], R.fp16_rne(_f32(v * sv)))
        elif a.mode == 1:
            y, b = R.tae_clamp64(v, sv)
            out["dst"] = _worst(R.gemm_ratio16(got[:, :, :a.C], y, b))
        else:
            raise Unknown(f"nchw_to_nhwc_f16 mode {a.mode}")
        return (k, f"mode {a.mode}"), out
    if k == "h2n":
        src = _mat(mem, a.src, a.n * a.HW, a.C, a.ld, np.float32).reshape(a.n, a.HW, a.C)
        got = _vec(mem, a.dst, a.n * a.C * a.HW).reshape(a.n, a.C, a.HW)
        two = _f32(_f32(src * np.float32(a.mul)) + np.float32(a.add)).transpose(0, 2, 1)      # src * mul + add in two roundings ...
        one = _f32(src.astype(np.float64) * float(np.float32(a.mul)) + float(np.float32(a.add))).transpose(0, 2, 1)      # ... or contracted to one fused multiply-add (the product of two fp32 is exact in float64)
        same = (got.view(np.uint32) == two.view(np.uint32)) | (got.view(np.uint32) == one.view(np.uint32))
        return (k, ""), {"dst": 0.0 if same.all() else float("inf")}
    if k == "temb":
        y, b = R.timestep_embedding64(_vec(mem, a.t, a.n), a.dim, a.maxp)
        return (k, ""), {"out": _worst(R.gemm_ratio16(_vec(mem, a.out, a.n * a.dim, np.float16).reshape(a.n, a.dim), y, b))}
    if k == "act":
        x, got = _vec(mem, a.x, a.n), _vec(mem, a.y, a.n, np.float16)
        if a.act == 0:
            return (k, "f32_to_f16"), {"y": _bits_equal(got, R.fp16_rne(x))}
        if a.act not in (1, 2, 3, 4):
            raise Unknown(f"act_f32_to_f16 activation {a.act}")
        y, b = R.act16_bound(x, a.act)
        return (k, f"act {a.act}"), {"y": _worst(R.gemm_ratio16(got, y, b))}
    if k == "cemb":
        tok = _vec(mem, a.tok, a.n * a.T, np.int32)
        tw = np.stack([_vec(mem, a.tw + 2 * int(t) * a.d, a.d, np.float16) for t in tok]).reshape(a.n, a.T, a.d)
        pw = _vec(mem, a.pw, a.T * a.d).reshape(1, a.T, a.d)
        return (k, ""), {"out": _bits_equal(_vec(mem, a.out, a.n * a.T * a.d).reshape(a.n, a.T, a.d), _f32(tw.astype(np.float32) + pw))}
    if k == "smax":
        x = _mat(mem, a.in_, a.rows, a.cols, a.ld_in, np.float32)
        p, b = R.softmax_rows64(x, a.scale)
        return (k, ""), {"out": _worst(R.gemm_ratio16(_mat(mem, a.out, a.rows, a.cols, a.ld_out, np.float16), p, b))}
    if k == "copy":
        form = tile_form(a)
        want = np.array(mem.read(a.src, a.nbytes))
        if form:      # HyperTile's row permutation: image order -> tile-major order, or back
            import hypertile_ref as HR
            want = HR.permute_rows(want.reshape(a.n_img * a.H * a.W, a.row_bytes), a.n_img, a.H, a.W, a.th, a.tw, inverse=bool(a.inverse)).reshape(-1)
        return (k, form), {"dst": _bits_equal(np.array(mem.read(a.dst, a.nbytes)), want)}
    if k == "xavt":
        if a.Tk > 96:
            raise Unknown("xattn_pack_vt beyond 96 keys")
        v = _mat(mem, a.v, a.n_img * a.Tk, a.N, a.ldv, np.float16).reshape(a.n_img, a.Tk, a.N)
        want = np.zeros((a.n_img, a.N, 96), np.float16)
        want[:, :, :a.Tk] = v.transpose(0, 2, 1)
        return (k, ""), {"vt": _bits_equal(_vec(mem, a.vt, a.n_img * a.N * 96, np.float16).reshape(want.shape), want)}
    if k == "cadd":
        # dst = base + gain ctrl, image n with residual image n % n_ctrl (the rows of ctrl modulo its row count); |err| <= 2^-23 (|base| + |gain ctrl|), derived in
        # tests/test_controlnet_gpu.py.  Gain 0 (or -0): the bits of base, and ctrl is never read
        rows = a.n_img * a.rows
        gain = _gain_of(mem, a)
        base, got = _mat(mem, a.base, rows, a.C, a.ld_base, np.float32), _mat(mem, a.dst, rows, a.C, a.ld_dst, np.float32)
        if gain == 0.0:
            return (k, "gain 0"), {"dst": _bits_equal(got, base)}
        ctrl = _mat(mem, a.ctrl, a.n_ctrl * a.rows, a.C, a.ld_ctrl, np.float32)
        kb = ctrl[np.arange(rows) % (a.n_ctrl * a.rows)].astype(np.float64) * gain
        want = base.astype(np.float64) + kb
        return (k, ""), {"dst": _worst(R.gemm_ratio32(got, want, 2.0 ** -23 * (np.abs(base).astype(np.float64) + np.abs(kb))))}
    if k in ("freeu_backbone", "freeu_skip"):
        # the bounds `skip` and `backbone` derived in tests/test_freeu_gpu.py; a factor of exactly 1 is a bit copy
        import freeu_ref as FR
        from mlimgsynth_amd import kernels
        n, H, W, C, u = a.n_img, a.H, a.W, a.C, R.U32
        f = float(_vec(mem, a.f, 1)[0])
        src, got = _mat(mem, a.src, n * H * W, C, a.ld_src, np.float32), _mat(mem, a.dst, n * H * W, C, a.ld_dst, np.float32)
        if f == 1.0:
            return (k, "factor 1"), {"dst": _bits_equal(got, src)}
        x64 = src.astype(np.float64).reshape(n, H, W, C).transpose(0, 3, 1, 2)
        nhwc = lambda v: v.transpose(0, 2, 3, 1).reshape(n * H * W, C)
        if k == "freeu_skip":
            D = kernels.freeu_depth(H * W)
            A = np.broadcast_to(4.0 / (H * W) * np.abs(x64).sum(axis=(2, 3), keepdims=True), x64.shape)
            ref = FR.fourier_filter64(x64, f)
            return (k, ""), {"dst": _worst(R.gemm_ratio32(got, nhwc(ref), u * (2 * np.abs(nhwc(ref)) + abs(f - 1) * (D + 16) * nhwc(A))))}
        D = kernels.freeu_depth(C)
        m = x64.mean(axis=1)
        span = m.max(axis=(1, 2)) - m.min(axis=(1, 2))
        delta = u * (D + 2) * np.abs(x64).mean(axis=1).max(axis=(1, 2))
        for i in range(n):      # the bound's condition on the data (a nearly constant mean map has no normalised form): a failure by name, never a skip
            if not (span[i] > 0 and delta[i] / span[i] <= 1e-4):
                raise Unknown(f"{op}: image {i}: delta / (max - min) = {delta[i]:.3g} / {span[i]:.3g} of the channel-mean map is above 1e-4, the backbone bound does not hold")
        slack = np.broadcast_to((3 * delta / span + 4 * u)[:, None, None, None], x64.shape)
        ref = nhwc(FR.backbone64(x64, f))
        bound = 2 * u * np.abs(ref) + np.abs(src.astype(np.float64)) * abs(f - 1) * nhwc(slack)
        return (k, ""), {"dst": _worst(R.gemm_ratio32(got, ref, bound)), "kept half": _bits_equal(got[:, C // 2:], src[:, C // 2:])}
    raise Unknown(f"op kind {k!r}")


def verify_op(mem, plan, i):
    """((kind, path), {output: worst ratio to its bound}) of op i recomputed in float64 from the operands it read; exact ops give 0 or inf.
    A `fused` LayerNorm / GroupNorm gives {}: it is checked as the ending of its producer (ln_y16 / gn_y16 there).  Unknown kinds and arguments raise."""
    ops = plan.ops if isinstance(plan, Plan) else plan
    op = ops[i]
    if op.fused:
        if op.kind not in ("ln", "gn"):
            raise Unknown(f"{op}: fused mark on a {op.kind}")
        return (op.kind, "ending of its producer"), {}
    if op.kind == "gemm":      # (a phase launch of an upsampling convolution is judged with its sibling launches and the loaded 3x3 weight: the plan's `ups`)
        return _verify_gemm(mem, op, ops[max(0, i - 3):i + 4] if op.a.out_phase else (), getattr(plan, "ups", ()))
    if op.kind in ("attn", "attn_ctx"):
        return _verify_attn(mem, op)
    if op.kind == "gn":
        return _verify_gn(mem, op)
    if op.kind == "ln":
        return _verify_ln(mem, op)
    return _verify_small(mem, op)


# ------------------------------------------------------------------ census
def census_key(op):
    """(kind, path, features) of an op: what the launch-by-launch check must have met for the op's form to count as audited"""
    from mlimgsynth_amd import kernels
    a, f = op.a, set()
    path = ""
    if op.kind == "gemm":
        tile, form, _, _ = gemm_path(kernels.gemm_variant(a))
        path = (tile, form)
        for name, on in (("row bias", a.rowbias), ("residual", a.resid), ("act_after_resid", a.act_after_resid), ("GEGLU", a.act == 5),
                         ("C16 + C32", a.C16 and a.C32 and not a.xa_k), ("colstats", a.colstats), ("LN ending", a.ln_y16), ("GN ending", a.gn_y16),
                         ("xattn ending", a.xa_k), ("upsample", a.upsample), ("wrap", a.conv and a.wrap), ("phase", phase_of(a))):
            if on:
                f.add(name)
    elif op.kind in ("attn", "attn_ctx"):
        path = kernels.attention_variant(a, op.kind == "attn_ctx")
    elif op.kind == "gn":
        for name, on in (("concat source", a.C2), ("raw16", a.raw16), ("producer statistics", a.cs1)):
            if on:
                f.add(name)
    elif op.kind == "act":
        path = f"act {a.act}"
    elif op.kind == "n2h":
        path = f"mode {a.mode}"
    elif op.kind == "copy":
        path = tile_form(a)
    if op.once:
        f.add("once")
    if op.fused:
        f.add("fused")
    return op.kind, path, tuple(sorted(f))
