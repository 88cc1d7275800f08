"""Kernels of 2048x2048 decodes across 2 GiB and 4 GiB offsets (pure numpy; importable without a GPU).

An untiled KL-VAE decode or encode of a 2048x2048 image (latent 256x256) puts operand elements more than 2^31 and 2^32 bytes from their base pointer: fp32 maps of
4 GiB, fp16 copies of 2 GiB, 65536 x 65536 attention scores with rows 256 KiB apart.  A 32-bit offset wraps or is dropped there without any error.  This module

  * counts the launches that do so: far_forms() builds FAR_PLANS in the dry runtime and, from plan_audit.extents(op), names every (census key, operand, class) whose
    range ends at or beyond 2^31 bytes (`far`) or 2^32 bytes (`very far`) from its base.  FAR_CASES maps each to the GPU case that holds it; unheld_far_forms()
    names the forms without one: a failure, never a skip;
  * builds the cases.  DENSE cases keep the product's M x N and strides and cut K (the input channels) to 8, so a launch takes milliseconds; their maps are tiled
    from three host blocks of 4 MiB -- below 2^31 bytes, between 2^31 and 2^32, above 2^32 -- that differ in mean and spread, copied into place device to device by
    doubling: a read that wraps to the other side of a boundary is a wrong value.  STRIDED cases take 21 rows whose stride (306 783 376 bytes = 16 (2^27 - 1) / 7)
    puts row 7 across 2^31 bytes, rows 13 / 14 just below 2^32 and row 15 above it; only the touched rows are uploaded and downloaded;
  * carves every operand of a case from ONE allocation: the operands that are far start 2 GiB + 64 KiB into it and at least their extent rounded up to 4 GiB follows
    each, so an offset truncated to 32 bits, zero- or sign-extended, still lands inside the allocation: a wrong number, not a fault.  The outputs are filled with
    0xFF bytes before the launch and counted as fp32 words by mlsd_count_nonfinite after it (a pair of finite halves is never a non-finite fp32 word, an unwritten
    pair always is): the every-element-written check that the sampled rows cannot give;
  * samples the rows that are downloaded and recomputed in float64 (sample_rows): first and last, the rows around 2^31 and 2^32 bytes of every far operand with their
    neighbours, the first and last row of their tiles, 300 seeded others.  References and bounds are those of tests/ref64.py, unchanged;
  * restates every case as a host model with the boundary as a parameter (model_run at 2^20 takes milliseconds): the output of a correct kernel, and of kernels whose
    byte offset into one operand is truncated to "32 bits" (2 x boundary), zero- or sign-extended, on a load or a store, or whose buffer resource ends at the
    boundary (num_records 0x7fffffff: loads past it return 0, stores are discarded).

Arena per case at the real boundary: Case.arena, computed by layout(); the GPU test prints it; 6 .. 15.7 GiB.

Not held: a 32-bit ELEMENT index into an fp32 operand.  The strided fp32 rows (ldc32, ldr, ldx, softmax ld_in) reach element 1.5 x 10^9; element 2^31 is 8 GiB from
the base, and with the 8 GiB in front of it that the layout gives an operand of more than 2^31 elements (so that a sign-extended element index stays inside) and its
extent rounded up to 4 GiB behind it, such an operand needs 20 GiB.  The fp16 strided operands (lda, ldc16, softmax ld_out, attention) do pass 2^31 elements.

GroupNorm statistics of a tiled map are exact in float64 from the blocks' own moments (block_group_stats); tests/test_far_offsets_cpu.py checks the formula against
tests/ref64.py on a scaled-down map.
"""
import ctypes
import zlib

import numpy as np

import gemm64_cases as GC
import plan_audit as PA
import ref64 as R

E_REAL = 31
MAX_IMAGES = 64      # the largest batch mlis_api.c (MAX_IMAGES) and engine.c (MAX_BATCH) admit for one plan; test_far_offsets_cpu.py reads both files

FAR_PLANS = [
    ("vae_dec", "sdxl", 256, 1), ("vae_enc", "sdxl", 256, 1), ("vae_dec", "sd1", 256, 1), ("vae_enc", "sd1", 256, 1),
    ("tae_dec", "sd1", 256, 1), ("tae_enc", "sd1", 256, 1), ("unet", "sdxl", 256, 2), ("vae_dec", "sdxl", 128, MAX_IMAGES),
]
# The last plan is the SDXL decoder at latent 128 with the largest batch the API admits for one plan, 64 images: fp32 maps of 32 GiB and a score block of 64 GiB.
# No arena holds those at the product's M x N: its forms are held at the smallest M at which the operand is still far or very far, with the product's N, strides and
# tile (the launch label is asserted), and the forms that even so need more than 16 GiB are named in BEYOND_ARENA with the bytes they need.  Which tiles that plan
# takes depends on the host (the dry runtime asks a present device for its CUs) and the dry runtime refuses the plan where the host cannot reserve the 64 GiB block
# (REFUSALS): the entries of FAR_CASES_BATCH are therefore not required to occur, but every form that does occur must be held or named.
BATCH_PLAN = ("vae_dec", "sdxl", 128, MAX_IMAGES)
REFUSALS = {"vae_dec-sdxl-128-64": r"device allocation of \d+ bytes failed"}
ARENA_MAX = 16 << 30


def far_class(rng):
    ext = rng.hi - rng.base
    return "very far" if ext >= 2 ** 32 else ("far" if ext >= 2 ** 31 else None)


def far_forms(engine, plans=FAR_PLANS):
    """({census key: [(plan id, operand name, class)]}, {plan id: refusal text}) of the plans, built in the dry runtime (never computed)"""
    from mlimgsynth_amd import _lib
    forms, refused = {}, {}
    for spec in plans:
        pid = PA.plan_id(spec)
        try:
            b = PA.build(engine, spec, PA.MLB_F_OPSHAPES)
        except _lib.MlsdError as e:
            refused[pid] = str(e)
            continue
        try:
            for o in PA.Plan(b.ctx, external=b.external).ops:
                ranges = o.reads + o.writes
                if o.kind == "gemm" and o.a.out_phase:      # the audit states a phase launch's write as one range per (image, source row); the kernel addresses
                    # every pixel from the map's base pointer a.C32: its reach is the highest range end above that pointer
                    px = [r for r in o.writes if r.name == "C32"]
                    ranges = [r for r in ranges if r.name != "C32"] + [PA.Range("C32", o.a.C32, 1, max(r.hi for r in px) - o.a.C32)]
                for r in ranges:
                    cls = far_class(r)
                    if cls and (pid, r.name, cls) not in forms.setdefault(PA.census_key(o), []):
                        forms[PA.census_key(o)].append((pid, r.name, cls))
        finally:
            b.close()
    return forms, refused


def unheld_far_forms(forms, held=None):
    """{(census key, operand, class): [plan ids]} of the far forms that FAR_CASES (or `held`) maps to no case"""
    held = {**ALL_FAR_CASES, **BEYOND_ARENA} if held is None else held
    out = {}
    for key, where in forms.items():
        for pid, name, cls in where:
            if (key, name, cls) not in held:
                out.setdefault((key, name, cls), []).append(pid)
    return out


# ------------------------------------------------------------------ operands, layout, contents
class Operand:
    """rows x cols elements of dtype, consecutive rows ld elements apart.  role: "in" / "out" / "scratch".  far: carved behind 2 GiB + 64 KiB.  sparse: only its rows
    are uploaded (strided cases); else the whole extent is tiled from the blocks (dense cases).  fam: (mean, spread) per segment of the operand's bytes."""

    def __init__(self, name, dtype, rows, cols, ld=None, role="in", far=False, sparse=False, fam=None, data=None, offsets=None, tiles=None):
        self.tiles = tiles      # [(first byte, end byte, uint8 block)]: the operand is whole copies of the block over each byte range (producer statistics of a tiled map)
        self.name, self.dtype, self.rows, self.cols, self.ld = name, np.dtype(dtype), int(rows), int(cols), int(ld or cols)
        self.role, self.far, self.sparse, self.fam, self.data, self.off = role, far, sparse, fam, data, None
        self.esz = self.dtype.itemsize
        self.row_bytes, self.stride = self.cols * self.esz, self.ld * self.esz
        self.offsets = None if offsets is None else np.asarray(offsets, np.int64)      # byte offset of every row (batches a batch stride apart); else row r at r x stride
        self.extent = (self.rows - 1) * self.stride + (self.row_bytes if sparse or self.ld == self.cols else self.stride)
        if self.offsets is not None:
            self.extent = int(self.offsets.max()) + self.row_bytes

    def row_off(self, rows):
        rows = np.asarray(rows, np.int64)
        return rows * self.stride if self.offsets is None else self.offsets[rows]


FAMS = ((0.5, 1.0), (-2.0, 0.25), (3.0, 2.0))      # (mean, spread) of the blocks below 2^31 bytes, between 2^31 and 2^32, above 2^32


class Case:
    """One launch.  e: log2 of the first boundary (31 on the device, 20 in the host model: every extent scales with it, row widths do not)."""

    def __init__(self, cid, op, e, forms, tile_m, **kw):
        self.id, self.op, self.e, self.forms, self.tile_m = cid, op, e, forms, tile_m
        self.b31, self.b32 = 1 << e, 2 << e
        self.blk = max(self.b31 >> 9, 1 << 17)      # 4 MiB blocks at the real boundary (whole 64-row statistics blocks of 512-channel rows at every scale)
        self.ops, self.kw, self.exp = {}, kw, False
        self._blocks = {}

    def add(self, *a, **k):
        o = Operand(*a, **k)
        self.ops[o.name] = o
        return o

    # ---- layout: small operands from 0, far operands from boundary + boundary >> 15 (2 GiB + 64 KiB), each followed by its extent rounded up to 2 boundaries (4 GiB)
    def layout(self):
        al = lambda v: (v + 4095) // 4096 * 4096
        lo = end = 0
        for o in self.ops.values():
            if not o.far:
                o.off, lo = lo, al(lo + o.extent + 64)
        hi = max(self.b31 + (self.b31 >> 15), lo)      # (the host model's small operands do not scale with the boundary: the far operands start behind them)
        for o in self.ops.values():
            if o.far:
                if o.extent // o.esz > self.b31:      # more than 2^31 elements: a sign-extended 32-bit ELEMENT index reaches esz x 2 GiB below the base
                    hi = max(hi, o.esz * self.b31 + (self.b31 >> 15))
                o.off, hi = hi, al(hi + o.extent)
                end = max(end, o.off + -(-o.extent // self.b32) * self.b32)
        self.arena = max(end, hi, lo)
        return self

    def seg(self, name, rows):
        """segment (0, 1, 2) of the operand's bytes that rows start in"""
        off = self.ops[name].row_off(rows)
        return (off >= self.b31).astype(np.int64) + (off >= self.b32)

    def block(self, name, s):
        """block s of a dense operand: [blk / stride rows][ld] of its dtype"""
        o = self.ops[name]
        if (name, s) not in self._blocks:
            rng = np.random.default_rng(zlib.crc32(f"{self.id}/{name}/{s}".encode()))
            mean, spread = (o.fam or FAMS)[s]
            assert self.blk % o.stride == 0, (self.id, name)
            v = mean + spread * rng.standard_normal((self.blk // o.stride, o.ld))
            self._blocks[(name, s)] = v.astype(o.dtype)
        return self._blocks[(name, s)]

    def value(self, name, rows):
        """the rows of an input operand as the fill puts them, [len(rows)][cols]"""
        o, rows = self.ops[name], np.asarray(rows, np.int64)
        if o.data is not None:
            return o.data[rows]
        s = self.seg(name, rows)
        if not o.sparse:
            out = np.empty((len(rows), o.cols), o.dtype)
            for k in range(3):
                if (s == k).any():
                    b = self.block(name, k)
                    out[s == k] = b[rows[s == k] % b.shape[0], :o.cols]
            return out
        out = np.empty((len(rows), o.cols), o.dtype)
        for i, (r, k) in enumerate(zip(rows.tolist(), s.tolist())):
            mean, spread = (o.fam or FAMS)[k]
            out[i] = (mean + spread * np.random.default_rng(zlib.crc32(f"{self.id}/{name}".encode()) + r).standard_normal(o.cols)).astype(o.dtype)
        return out

    def outputs(self):
        return [o for o in self.ops.values() if o.role == "out"]

    def far_operands(self):
        return [o for o in self.ops.values() if o.far]


def fill(case, mem):
    """the inputs into place and 0xFF over the outputs.  mem: write(off, uint8 array), copy(dst, src, n), memset(off, value, n)"""
    for o in case.ops.values():
        if o.role == "out":
            mem.memset(o.off, 0xFF, o.extent)
        elif o.role == "scratch":
            mem.memset(o.off, 0, o.extent)
        elif o.tiles is not None:
            for a, b, blk in o.tiles:
                _double(mem, o.off + a, b - a, blk)
        elif o.data is not None:
            mem.write(o.off, np.ascontiguousarray(o.data).view(np.uint8).reshape(-1))
        elif o.sparse:
            for r in range(o.rows):
                mem.write(o.off + int(o.row_off(r)), case.value(o.name, [r]).view(np.uint8).reshape(-1))
        else:
            for s, (a, b) in enumerate(((0, case.b31), (case.b31, case.b32), (case.b32, o.extent))):
                b = min(b, o.extent)
                if a >= b:
                    continue
                _double(mem, o.off + a, b - a, case.block(o.name, s).view(np.uint8).reshape(-1))


def _double(mem, off, nbytes, blk):
    """nbytes at off filled with copies of the block: one upload, then device to device, doubling"""
    n = min(blk.size, nbytes)
    mem.write(off, blk[:n])
    while n < nbytes:
        m = min(n, nbytes - n)
        mem.copy(off + n, off, m)
        n += m


class HostMemory:
    """the arena of the host model"""

    def __init__(self, nbytes):
        self.buf = np.zeros(nbytes, np.uint8)

    def write(self, off, arr):
        self.buf[off:off + arr.size] = arr

    def copy(self, dst, src, n):
        self.buf[dst:dst + n] = self.buf[src:src + n]

    def memset(self, off, value, n):
        self.buf[off:off + n] = value

    def read(self, off, n):
        assert 0 <= off and off + n <= self.buf.size, (off, n)      # the arena rule: a truncated offset stays inside the allocation
        return self.buf[off:off + n]

    def count_nonfinite(self, off, nwords):
        return int((~np.isfinite(self.buf[off:off + 4 * nwords].view(np.float32))).sum())


def read_rows(case, mem, name, rows):
    o = case.ops[name]
    return np.stack([np.array(mem.read(o.off + int(o.row_off(r)), o.row_bytes)).view(o.dtype) for r in rows])


def unwritten(case, mem):
    """{output: fp32 words of it that are still not finite}: 0 everywhere for a launch that wrote every element"""
    out = {}
    for o in case.outputs():
        if o.sparse:
            out[o.name] = sum(mem.count_nonfinite(o.off + int(o.row_off(r)), o.row_bytes // 4) for r in range(o.rows))
        else:
            out[o.name] = mem.count_nonfinite(o.off, o.extent // 4)
    return out


# ------------------------------------------------------------------ the rows that are recomputed
def boundary_rows(o, B):
    """rows of operand o around byte B of it: the last row that starts below B and the first that ends beyond it, each with both neighbours"""
    if o.extent <= B:
        return []
    if o.offsets is not None:
        r0, r1 = int(np.nonzero(o.offsets < B)[0][-1]), int(np.nonzero(o.offsets + o.row_bytes > B)[0][0])
    else:
        r0, r1 = (B - 1) // o.stride, max((B - o.row_bytes) // o.stride + 1, 0)
    return sorted({r for c in (r0, r1) for r in (c - 1, c, c + 1) if 0 <= r < o.rows})


def out_rows(case):
    return next(o for o in case.outputs() if o.name != "colstats").rows


def sample_rows(case, n_random=300):
    M, T = out_rows(case), case.tile_m
    if M <= 1024:      # (the strided cases: every row)
        return np.arange(M, dtype=np.int64)
    rows = {0, M - 1}
    for o in case.far_operands():
        for B in (case.b31, case.b32):
            for r in boundary_rows(o, B):
                r = min(r * M // o.rows, M - 1) if o.rows != M else r
                rows |= {r, r // T * T, min(r // T * T + T - 1, M - 1)}
                if case.kw.get("phase"):      # the 256-row tile of the phase launch that writes output pixel r: source rows m0 .. m1 of its parity
                    W2, Ms = 2 * case.kw["W"], case.kw["M"]
                    Y, X = r // W2, r % W2
                    m = (Y >> 1) * case.kw["W"] + (X >> 1)
                    for mm in (m // 256 * 256, min(m // 256 * 256 + 255, Ms - 1)):
                        rows.add((2 * (mm // case.kw["W"]) + (Y & 1)) * W2 + 2 * (mm % case.kw["W"]) + (X & 1))
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    rows |= set(rng.integers(0, M, min(n_random, M)).tolist())
    return np.array(sorted(rows), np.int64)


def stats_blocks(case, rows):
    """the 64-row statistics blocks of a colstats case that are checked whole: those of the first and last row and of the boundary rows"""
    M = out_rows(case)
    sr = case.kw.get("srows", 64)
    want = {0, (M - 1) // sr}
    for o in case.far_operands():
        for B in (case.b31, case.b32):
            want |= {r // sr for r in boundary_rows(o, B) if o.rows == M}
    return sorted(want)


# ------------------------------------------------------------------ GroupNorm statistics of a tiled map
def block_group_stats(blocks, weights, G, eps):
    """float64 (mean, var, r, max|x^|) per group [G] of a map that is `weights[s]` whole copies of blocks[s] ([rows][C]) for every s: exact from the blocks' moments"""
    w = np.asarray([wt * b.shape[0] for wt, b in zip(weights, blocks)], np.float64)
    w = w / w.sum()
    C = blocks[0].shape[1]
    bg = [np.asarray(b, np.float64).reshape(b.shape[0], G, C // G) for b in blocks]
    mus = np.array([b.mean(axis=(0, 2)) for b in bg])                       # [s][G]
    mu = (w[:, None] * mus).sum(0)
    var = sum(wi * ((b - mu[None, :, None]) ** 2).mean(axis=(0, 2)) for wi, b in zip(w, bg) if wi > 0)
    sd = np.sqrt(var + eps)
    xh = np.max([np.abs(b - mu[None, :, None]).max(axis=(0, 2)) for wi, b in zip(w, bg) if wi > 0], axis=0) / sd
    return mu, var, np.abs(mu) / sd, xh


def gn_reference(case, x_rows):
    """(want64, tol) of the GroupNorm output rows for input rows x_rows, from the analytic statistics: R.groupnorm64 and the tolerance of R.groupnorm_worst"""
    o, G, eps = case.ops["x1"], case.kw["G"], case.kw["eps"]
    nseg = [max(0, min(b, o.extent) - a) // case.blk for a, b in ((0, case.b31), (case.b31, case.b32), (case.b32, o.extent))]
    assert sum(nseg) * case.blk == o.extent
    blocks = [case.block("x1", s)[:, :o.cols] for s in range(3)]
    mu, var, r, xh = block_group_stats(blocks, nseg, G, eps)
    g, be = case.ops["gamma"].data[0].astype(np.float64), case.ops["beta"].data[0].astype(np.float64)
    C = o.cols
    xg = np.asarray(x_rows, np.float64).reshape(len(x_rows), G, C // G)
    y = ((xg - mu[None, :, None]) / np.sqrt(var + eps)[None, :, None]).reshape(len(x_rows), C) * g + be
    y = R.silu(y) if case.kw["silu"] else y
    gm, bm = np.abs(g).reshape(G, C // G).max(1), np.abs(be).reshape(G, C // G).max(1)
    eb = R.C_NORM * R.U32 * ((1 + r + xh) * gm + bm)
    return y, R.half_ulp16(y) + np.repeat(eb, C // G)[None, :]


# ------------------------------------------------------------------ references per op: {output: (want64, bound, kind)} for output rows `rows`
def conv_A(case, rows, fetch):
    """the implicit-GEMM A rows (R.im2col64's order: kh, kw, cin) of output rows `rows`, from the pixels `fetch` returns"""
    k, H, W, p = case.kw["k"], case.kw["H"], case.kw["W"], case.kw["pad"]
    rows = np.asarray(rows, np.int64)
    oy, ox = (rows // W) % H, rows % W
    cols = []
    for kh in range(k):
        for kw in range(k):
            iy, ix = oy - p + kh, ox - p + kw
            ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
            v = np.asarray(fetch("A", np.clip(iy, 0, H - 1) * W + np.clip(ix, 0, W - 1)), np.float64)
            v[~ok] = 0.0
            cols.append(v)
    return np.concatenate(cols, axis=1)


def reference(case, rows, fetch=None):
    fetch = fetch or case.value
    kw = case.kw
    if case.op == "gemm" and kw.get("phase"):
        # output pixel (Y, X) of the [2 H][2 W] map is written by the launch of parity (py, px) = (Y & 1, X & 1) from the 2 x 2 taps (y - 1 + py + a, x - 1 + px + b)
        # of source pixel (y, x) = (Y >> 1, X >> 1), zero outside: R.phase_A's rows, R.im2col64's order (a, b, cin), against that launch's own weight
        rows = np.asarray(rows, np.int64)
        H, W, N = kw["H"], kw["W"], kw["N"]
        Y, X = rows // (2 * W), rows % (2 * W)
        y = np.empty((len(rows), N))
        b = np.empty((len(rows), N))
        D = R.gemm_depth(kw["K"], kw["k_step"], 1)
        for q in range(4):
            py, px = q >> 1, q & 1
            sel = np.nonzero(((Y & 1) == py) & ((X & 1) == px))[0]
            if not sel.size:
                continue
            cols = []
            for a_ in range(2):
                for b_ in range(2):
                    iy, ix = (Y[sel] >> 1) - 1 + py + a_, (X[sel] >> 1) - 1 + px + b_
                    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                    v = np.asarray(fetch("A", np.clip(iy, 0, H - 1) * W + np.clip(ix, 0, W - 1)), np.float64)
                    v[~ok] = 0.0
                    cols.append(v)
            acc, S = R.gemm64(np.concatenate(cols, axis=1), case.ops[f"W{q + 1}"].data)
            y[sel], b[sel] = R.gemm_epilogue64(acc, S, D, np.arange(sel.size), np.arange(N), bias=case.ops["bias"].data[0])
        return {"C32": (y, b, "32")}
    if case.op == "gemm":
        A = conv_A(case, rows, fetch) if kw.get("k") else fetch("A", rows)
        acc, S = R.gemm64(A, case.ops["W"].data)
        D = R.gemm_depth(kw["K"], kw["k_step"], 1)
        y, b = R.gemm_epilogue64(acc, S, D, np.arange(len(rows)), np.arange(kw["N"]), bias=case.ops["bias"].data[0] if "bias" in case.ops else None,
                                 resid=fetch("resid", rows) if "resid" in case.ops else None)
        return {n: (y, b, "32" if n == "C32" else "16") for n in ("C32", "C16") if n in case.ops}
    if case.op == "gn":
        y, tol = gn_reference(case, fetch("x1", rows))
        return {"y16": (y, tol, "abs")}
    if case.op == "act":
        x = fetch("x", rows)
        return {"y": (x.astype(np.float64), None, "bits16")}
    if case.op == "smax":
        p, b = R.softmax_rows64(fetch("in", rows), kw["scale"])
        return {"out": (p, b, "16")}
    if case.op == "ln":
        x = fetch("x", rows)
        g, be = case.ops["g"].data[0], case.ops["b"].data[0]
        return {"y16": (R.layernorm64(x, kw["eps"], g, be), (x, kw["eps"], g, be), "ln")}
    if case.op == "gns":      # GroupNorm of a few strided pixels: the statistics are over all of them
        allr = np.arange(kw["HW"])
        x = np.concatenate([fetch("x1", allr), fetch("x2", allr)], axis=1)[None]
        g, be = case.ops["gamma"].data[0], case.ops["beta"].data[0]
        want = R.groupnorm64(x, None, kw["G"], kw["eps"], g, be, True)
        eb, _ = R.groupnorm_bound(x, kw["G"], kw["eps"], g, be)
        return {"y16": (want[0][rows], (R.half_ulp16(want[0]) + np.repeat(eb[0], x.shape[2] // kw["G"])[None, :])[rows], "abs")}
    if case.op == "h2n":      # dst[c][pix] = src[pix][c] * mul + add: in two roundings, or contracted to one fused multiply-add (plan_audit._verify_small)
        src = fetch("src", np.arange(kw["HW"]))
        two = PA._f32(PA._f32(src * np.float32(kw["mul"])) + np.float32(kw["add"])).T.reshape(1, -1)
        one = PA._f32(src.astype(np.float64) * float(np.float32(kw["mul"])) + float(np.float32(kw["add"]))).T.reshape(1, -1)
        return {"dst": (two, one, "either32")}
    if case.op == "attn":
        Tq, Tk, nb = kw["Tq"], kw["Tk"], kw["n_batch"]
        ys, bs = [], []
        for b in range(nb):
            q, k, v = fetch("q", np.arange(b * Tq, (b + 1) * Tq)), fetch("k", np.arange(b * Tk, (b + 1) * Tk)), fetch("v", np.arange(b * Tk, (b + 1) * Tk))
            o, p = R.attention64(q, k, v, 1)
            ys.append(o)
            bs.append(R.half_ulp16(o) + R.attention_bound(q, k, v, 1, o, p, False))      # (the tolerance of R.attention_worst)
        return {"out": (np.concatenate(ys)[rows], np.concatenate(bs)[rows], "abs")}
    raise PA.Unknown(case.op)


def ratio(got, want, bound, kind):
    if kind == "ln":
        return R.layernorm_worst(got, want, *bound)[0]
    if kind == "either32":
        g = np.asarray(got).view(np.uint32)
        return np.where((g == np.asarray(want).view(np.uint32)) | (g == np.asarray(bound).view(np.uint32)), 0.0, np.inf)
    if kind == "32":
        return R.gemm_ratio32(got, want, bound)
    if kind == "16":
        return R.gemm_ratio16(got, want, bound)
    if kind == "abs":
        g = np.asarray(got, np.float64)
        r = np.abs(g - want) / bound
        r[~np.isfinite(g)] = np.inf
        return r
    same = np.asarray(got).view(np.uint16) == R.fp16_rne(want).view(np.uint16)      # "bits16": an exact conversion
    return np.where(same, 0.0, np.inf)


def correct_output(want, kind):
    return np.asarray(want).astype(np.float32 if kind in ("32", "either32") else np.float16)


def check(case, mem, rows=None):
    """{output: worst ratio to the bound over the sampled rows}, and colstats over the checked statistics blocks"""
    rows = sample_rows(case) if rows is None else rows
    out = {}
    for name, (want, bound, kind) in reference(case, rows).items():
        out[name] = PA._worst(ratio(read_rows(case, mem, name, rows), want, bound, kind))
    if "C16" in out and "C32" in out:
        out["C16==rne(C32)"] = PA._bits_equal(read_rows(case, mem, "C16", rows), R.fp16_rne(read_rows(case, mem, "C32", rows)))
    if "colstats" in case.ops:
        st, N = case.ops["colstats"], case.kw["N"]
        w = 0.0
        for k in stats_blocks(case, rows):
            sr = case.kw.get("srows", 64)
            c32 = read_rows(case, mem, "C32", np.arange(sr * k, sr * k + sr))
            got = np.array(mem.read(st.off + k * 2 * N * 4, 2 * N * 4)).view(np.float32).reshape(1, 2, N)
            es, eq = R.colstats_ratios(c32, got, sr, shifted=True)
            w = max(w, PA._worst(es), PA._worst(eq))
        out["colstats"] = w
    return out


# ------------------------------------------------------------------ the host model: a correct kernel and the seeded faults
FAULTS = [(where, mode) for where in ("load", "store") for mode in ("zext", "sext", "zext_elem", "sext_elem", "records")]


def faulty_offset(case, off, nbytes, mode, esz=1):
    """the byte offset a kernel with fault `mode` uses instead of `off` (None: the access is dropped by an exhausted num_records).  zext / sext: the byte offset kept
    in "32 bits" (2 x boundary) and zero- / sign-extended; *_elem: the same on the element index; records: a buffer resource that ends one byte below the boundary"""
    if mode == "records":
        return None if off + nbytes > case.b31 - 1 else off
    unit = esz if mode.endswith("_elem") else 1
    t = (off // unit) % case.b32
    if mode.startswith("sext") and t >= case.b31:
        t -= case.b32
    return t * unit + off % unit


def fault_changes(case, name, mode):
    """does the fault alter any access of this operand (an operand of exactly 2^31 bytes has no offset that 32 bits cannot hold)"""
    o = case.ops[name]
    return any(faulty_offset(case, int(o.row_off(r)), o.row_bytes, mode, o.esz) != int(o.row_off(r)) for r in range(o.rows))


def model_run(case, mem, fault=None):
    """the launch on the host arena: every output row from the float64 reference rounded to the output type.  fault: (operand, "load" | "store", mode)"""
    M = out_rows(case)
    rows = np.arange(M)
    fname, fwhere, fmode = fault or (None, None, None)

    def fetch(name, rr):
        o = case.ops[name]
        if o.data is not None:
            return o.data[rr]
        out = np.empty((len(rr), o.cols), o.dtype)
        for i, r in enumerate(np.asarray(rr).tolist()):
            off = int(o.row_off(r))
            if name == fname and fwhere == "load":
                off = faulty_offset(case, off, o.row_bytes, fmode, o.esz)
            out[i] = 0 if off is None else np.array(mem.read(o.off + off, o.row_bytes)).view(o.dtype)
        return out
    for name, (want, _, kind) in reference(case, rows, fetch).items():
        o = case.ops[name]
        y = correct_output(want, kind)
        if name == "C16":
            y = R.fp16_rne(correct_output(want, "32"))
        for r in range(M):
            off = int(o.row_off(r))
            if name == fname and fwhere == "store":
                off = faulty_offset(case, off, o.row_bytes, fmode, o.esz)
            if off is not None:
                mem.read(o.off + off, o.row_bytes)[:] = y[r].view(np.uint8)
    if "colstats" in case.ops:      # from the stored output, as the epilogue has them
        st, N = case.ops["colstats"], case.kw["N"]
        c = read_rows(case, mem, "C32", rows).astype(np.float64).reshape(-1, case.kw.get("srows", 64), N)
        d = c - c[:, :1]
        mem.write(st.off, np.stack([d.sum(1), (d * d).sum(1)], axis=1).astype(np.float32).view(np.uint8).reshape(-1))


# ------------------------------------------------------------------ the cases
def stride_for(e):
    """(row stride in bytes, j): row j starts 16 bytes below 2^e, row 2 j 32 bytes below 2^(e + 1); a multiple of 16 bytes.  3 j rows reach beyond 2^(e + 1)"""
    q = (1 << (e - 4)) - 1
    j = next(j for j in (3, 5, 7, 11, 13, 17, 31) if q % j == 0)
    return 16 * (q // j), j


def _small(case, name, arr):
    arr = np.ascontiguousarray(arr)
    return case.add(name, arr.dtype, 1 if arr.ndim == 1 else arr.shape[0], arr.shape[-1], data=arr.reshape(-1, arr.shape[-1]))


def _hw(M):
    H = 1 << ((M.bit_length() - 1) // 2)
    return M // H, H


def _tile_no(variant):
    from mlimgsynth_amd import kernels
    return {v: k for k, v in kernels.TILE_LABELS.items()}[variant]


def conv_case(cid, e, forms, tile, tile_m, k, lda=None, N=128, resid=False, c16=False, stats=False, cin=8, more=0, srows=64, auto=False, mrows=None):
    """a convolution of M pixels x N whose fp32 output takes 2^(e + more) bytes (2048 x 2048 x 128 at e = 31, more = 0: the product's M x N) with cin input
    channels, rows of A lda halfs apart; srows: the rows of a statistics block of the tile; auto: the launcher picks the tile (the small-N kernel is chosen by shape)"""
    c = Case(cid, "gemm", e, forms, tile_m)
    lda = lda or cin
    M = mrows >> (31 - e) if mrows else (1 << (e + more)) // (N * 4)
    H, W = _hw(M)
    K = k * k * cin
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(k=k, pad=k // 2, H=H, W=W, M=M, N=N, K=K, lda=lda, cin=cin, tile=tile, auto=auto, srows=srows, variant=GC.L(tile, "conv"), stats=stats,
                k_step=R.K_STEP_GENERAL if tile in PA.GENERAL_TILES else R.K_STEP_MFMA16)
    c.add("A", np.float16, M, cin, lda, far=M * lda * 2 >= c.b31)
    _small(c, "W", GC.f16(rng.standard_normal((N, K)) / np.sqrt(K)))
    _small(c, "bias", rng.standard_normal(N).astype(np.float32))
    if resid:
        c.add("resid", np.float32, M, N, far=True)
    if c16:
        c.add("C16", np.float16, M, N, role="out", far=M * N * 2 >= c.b31)
    if stats:
        c.add("colstats", np.float32, M // srows, 2 * N, role="out")
    c.add("C32", np.float32, M, N, role="out", far=M * N * 4 >= c.b31)
    return c.layout()


def phase_case(cid, e, forms, tile, N=256, cin=64):
    """the four phase launches of an upsampling convolution (out_phase 1 .. 4: 2 x 2 taps on the source, every launch writes the pixels of its parity of the
    [2 H][2 W] map from the map's base pointer): a source of 2^(e - 11) pixels x cin, an fp32 map of N = 256 channels and 2^(e + 1) bytes (2048 x 2048 at e = 31: the
    map of the KL-VAE's last upsampling); K = 4 cin = 256 is the smallest the phase form's rule admits"""
    c = Case(cid, "gemm", e, forms, 1)
    M = (2 << e) // (N * 4 * 4)
    H, W = _hw(M)
    K = 4 * cin
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(phase=True, H=H, W=W, M=M, N=N, K=K, lda=cin, cin=cin, tile=tile, variant=GC.L(tile, "conv"),
                k_step=R.K_STEP_GENERAL if tile in PA.GENERAL_TILES else R.K_STEP_MFMA16)
    c.add("A", np.float16, M, cin)
    for q in range(4):
        _small(c, f"W{q + 1}", GC.f16(rng.standard_normal((N, K)) / np.sqrt(K)))
    _small(c, "bias", rng.standard_normal(N).astype(np.float32))
    c.add("C32", np.float32, 4 * M, N, role="out", far=True)
    return c.layout()


def linear_case(cid, e, forms, tile, tile_m, N, far_op):
    """3 j rows (21 at e = 31) of a Linear with K = 16 whose A rows (far_op "A") or C32 rows (far_op "C32") lie stride_for(e) bytes apart"""
    c = Case(cid, "gemm", e, forms, tile_m)
    sb, j = stride_for(e)
    M, K = 3 * j, 16
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(M=M, N=N, K=K, tile=tile, k_step=R.K_STEP_GENERAL, variant=GC.L(tile), lda=sb // 2 if far_op == "A" else K, ldc32=sb // 4 if far_op == "C32" else N)
    c.add("A", np.float16, M, K, c.kw["lda"], far=far_op == "A", sparse=True)
    _small(c, "W", GC.f16(rng.standard_normal((N, K)) / np.sqrt(K)))
    c.add("C32", np.float32, M, N, c.kw["ldc32"], role="out", far=far_op == "C32", sparse=True)
    return c.layout()


def gn_case(cid, e, forms, C, nbytes_log2, stats=False):
    """GroupNorm + SiLU of one image of 2^nbytes_log2 bytes of fp32 pixels x C channels, 32 groups, eps 1e-6 (the KL-VAE's); stats: from producer statistics of 64-row blocks"""
    c = Case(cid, "gn", e, forms, 256, G=32, eps=float(np.float32(1e-6)), silu=1, stats=stats)
    HW = (1 << (e - 31 + nbytes_log2)) // (C * 4)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(HW=HW, C=C)
    x = c.add("x1", np.float32, HW, C, far=True)
    _small(c, "gamma", (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32))
    _small(c, "beta", (0.3 * rng.standard_normal(C)).astype(np.float32))
    c.add("ws", np.float32, 1, 1 << 20, role="scratch")
    if stats:      # shifted sums per block of 64 rows and column: K = the block's first row; in float64 from the blocks, rounded once
        per = []
        for s in range(3):
            b = c.block("x1", s).astype(np.float64).reshape(-1, 64, C)
            d = b - b[:, :1]
            per.append(np.stack([d.sum(1), (d * d).sum(1)], axis=1).reshape(-1, 2 * C))
        ext = HW * C * 4      # 64 rows of C floats of the map are one row of 2 C floats here: a byte of the map is 1 / 32 byte of the statistics
        tiles = [(a // 32, min(b, ext) // 32, per[s].astype(np.float32).view(np.uint8).reshape(-1)) for s, (a, b) in enumerate(((0, c.b31), (c.b31, c.b32), (c.b32, ext))) if a < ext]
        c.add("cs1", np.float32, HW // 64, 2 * C, tiles=tiles)
    c.add("y16", np.float16, HW, C, role="out", far=HW * C * 2 >= c.b31)
    return c.layout()


def act_case(cid, e, forms, more=0):
    """mlsd_act_f32_to_f16 (act 0) of 2^(e - 1) floats: 2^(e + 1) bytes in, 2^e bytes out; rows of 256 elements"""
    c = Case(cid, "act", e, forms, 256)
    n = 1 << (e - 1 + more)
    c.kw.update(n=n)
    c.add("x", np.float32, n // 256, 256, far=True)
    c.add("y", np.float16, n // 256, 256, role="out", far=True)
    return c.layout()


def smax_case(cid, e, forms):
    """mlsd_softmax_rows of 3 j rows of 65536 scores (the VAE mid block's, scale 512^-0.5), rows stride_for(e) bytes apart on both sides"""
    c = Case(cid, "smax", e, forms, 1)
    sb, j = stride_for(e)
    cols = 65536 >> max(0, (31 - e) // 2)
    c.kw.update(rows=3 * j, cols=cols, scale=float(np.float32(512 ** -0.5)), ld_in=sb // 4, ld_out=sb // 2)
    c.add("in", np.float32, 3 * j, cols, sb // 4, far=True, sparse=True, fam=((0.5, 8.0), (-2.0, 3.0), (3.0, 16.0)))
    c.add("out", np.float16, 3 * j, cols, sb // 2, role="out", far=True, sparse=True)
    return c.layout()


def linear_res_c16_case(cid, e):
    """as linear_case on the 128x128 tile, with the residual rows (ldr) and the fp16 output rows (ldc16) stride_for(e) bytes apart; C32 dense"""
    c = Case(cid, "gemm", e, [], 128)
    sb, j = stride_for(e)
    M, K, N = 3 * j, 16, 136
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(M=M, N=N, K=K, tile=G0, k_step=R.K_STEP_GENERAL, variant=GC.L(G0), lda=K, ldr=sb // 4, ldc16=sb // 2)
    c.add("A", np.float16, M, K, sparse=True)
    _small(c, "W", GC.f16(rng.standard_normal((N, K)) / np.sqrt(K)))
    c.add("resid", np.float32, M, N, sb // 4, far=True, sparse=True)
    c.add("C32", np.float32, M, N, role="out", sparse=True)
    c.add("C16", np.float16, M, N, sb // 2, role="out", far=True, sparse=True)
    return c.layout()


def ln_case(cid, e):
    """mlsd_layernorm of 3 j rows of 1280 floats stride_for(e) bytes apart (ldx)"""
    c = Case(cid, "ln", e, [], 4, eps=1e-5)
    sb, j = stride_for(e)
    d = 1280
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(rows=3 * j, d=d, ldx=sb // 4)
    c.add("x", np.float32, 3 * j, d, sb // 4, far=True, sparse=True)
    _small(c, "g", (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32))
    _small(c, "b", (0.3 * rng.standard_normal(d)).astype(np.float32))
    c.add("y16", np.float16, 3 * j, d, role="out", sparse=True)
    return c.layout()


def gn_strided_case(cid, e):
    """GroupNorm + SiLU over the virtual concat of two sources of 3 j pixels x 64 channels each, pixels stride_for(e) bytes apart in both (ld1, ld2)"""
    c = Case(cid, "gns", e, [], 1, G=32, eps=float(np.float32(1e-6)), silu=1)
    sb, j = stride_for(e)
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    c.kw.update(HW=3 * j, C1=64, C2=64, ld=sb // 4)
    c.add("x1", np.float32, 3 * j, 64, sb // 4, far=True, sparse=True)
    c.add("x2", np.float32, 3 * j, 64, sb // 4, far=True, sparse=True, fam=((1.5, 0.5), (0.0, 2.0), (-3.0, 1.0)))
    _small(c, "gamma", (1.0 + 0.2 * rng.standard_normal(128)).astype(np.float32))
    _small(c, "beta", (0.3 * rng.standard_normal(128)).astype(np.float32))
    c.add("ws", np.float32, 1, 1 << 16, role="scratch")
    c.add("y16", np.float16, 3 * j, 128, role="out", sparse=True)
    return c.layout()


def h2n_case(cid, e):
    """mlsd_nhwc_to_nchw_f32 of 3 j pixels x 8 channels, pixels stride_for(e) bytes apart (ld)"""
    c = Case(cid, "h2n", e, [], 1, mul=0.5, add=0.5)
    sb, j = stride_for(e)
    c.kw.update(HW=3 * j, C=8, ld=sb // 4)
    c.add("src", np.float32, 3 * j, 8, sb // 4, far=True, sparse=True)
    c.add("dst", np.float32, 1, 8 * 3 * j, role="out", sparse=True)      # [C][HW], dense: one row of the check
    return c.layout()


def attn_case(cid, e, far_op, how):
    """mlsd_attention, one head of 64.  how "ld": the rows of far_op stride_for(e) bytes apart (ldq / ldo: 3 j queries on 100 keys, the tile-loop kernel; ldk / ldv:
    8 queries on 3 j keys, the one-pass kernel of up to 96 keys), one batch.  how "bs": three batches of 8 queries on 100 keys, the batches of far_op 2^e - 64 bytes
    apart: batch 1 starts 64 bytes below 2^e, batch 2 128 below 2^(e + 1)"""
    c = Case(cid, "attn", e, [], 128)
    sb, j = stride_for(e)
    if how == "ld":
        nb, Tq, Tk = (1, 3 * j, 100) if far_op in ("q", "out") else (1, 8, 3 * j)
    else:
        nb, Tq, Tk = 3, 8, 100
    c.kw.update(n_batch=nb, Tq=Tq, Tk=Tk, far_op=far_op, label="attn<tk96,d64" if Tk <= 96 else "attn<tile,d64",
                ld={n: 64 for n in "qkvo"}, bs={"q": Tq * 64, "k": Tk * 64, "v": Tk * 64, "o": Tq * 64})
    for n, T, role in (("q", Tq, "in"), ("k", Tk, "in"), ("v", Tk, "in"), ("out", Tq, "out")):
        key = "o" if n == "out" else n
        if n == far_op and how == "ld":
            c.kw["ld"][key] = sb // 2
            c.add(n, np.float16, T, 64, sb // 2, role=role, far=True, sparse=True)
        elif n == far_op:
            bs = c.b31 - 64
            c.kw["bs"][key] = bs // 2
            c.add(n, np.float16, nb * T, 64, role=role, far=True, sparse=True, offsets=[b * bs + t * 128 for b in range(nb) for t in range(T)])
        else:
            c.add(n, np.float16, nb * T, 64, role=role, sparse=True)
    return c.layout()


G0, G3, G4 = GC.G0, GC.G3, GC.G4
_g = lambda tile, feats: ("gemm", (tile, ""), feats)
BUILDERS = {
    "g0_conv_c16_res": lambda e, f: conv_case("g0_conv_c16_res", e, f, G0, 128, 3, resid=True, c16=True),
    "g0_conv_stats": lambda e, f: conv_case("g0_conv_stats", e, f, G0, 128, 3, stats=True),
    "g4_conv_stats_res": lambda e, f: conv_case("g4_conv_stats_res", e, f, G4, 256, 3, resid=True, stats=True),
    "g4_conv_stats_farA": lambda e, f: conv_case("g4_conv_stats_farA", e, f, G4, 256, 3, lda=256, stats=True),
    "g4_conv1x1_farA": lambda e, f: conv_case("g4_conv1x1_farA", e, f, G4, 256, 1, lda=256),
    "p17_phase_4g": lambda e, f: phase_case("p17_phase_4g", e, f, GC.P17),
    "g0_lin_lda": lambda e, f: linear_case("g0_lin_lda", e, f, G0, 128, 512, "A"),
    "g3_lin_ldc32": lambda e, f: linear_case("g3_lin_ldc32", e, f, G3, 256, 136, "C32"),
    "gn_c256_4g": lambda e, f: gn_case("gn_c256_4g", e, f, 256, 32),
    "gn_c512_2g": lambda e, f: gn_case("gn_c512_2g", e, f, 512, 31),
    "gn_stats_c128_2g": lambda e, f: gn_case("gn_stats_c128_2g", e, f, 128, 31, stats=True),
    "act0_4g": lambda e, f: act_case("act0_4g", e, f),
    "smax_65536": lambda e, f: smax_case("smax_65536", e, f),
}
# (census key, operand, class) -> the case that holds it.  The conversion f32_to_f16 is one grid-stride loop whose only parameter is n: its launch of 2^30 elements
# (4 GiB in, 2 GiB out) crosses every boundary its launch of 2^29 does.
FAR_CASES = {
    (_g(G0, ("C16 + C32", "residual")), "C32", "far"): "g0_conv_c16_res",
    (_g(G0, ("C16 + C32", "residual")), "resid", "far"): "g0_conv_c16_res",
    (_g(G0, ("colstats",)), "C32", "far"): "g0_conv_stats",
    (_g(G4, ("colstats", "residual")), "C32", "far"): "g4_conv_stats_res",
    (_g(G4, ("colstats", "residual")), "resid", "far"): "g4_conv_stats_res",
    (_g(G4, ("colstats",)), "A", "far"): "g4_conv_stats_farA",
    (_g(G4, ("colstats",)), "C32", "far"): "g4_conv_stats_farA",
    (_g(G4, ()), "A", "far"): "g4_conv1x1_farA",
    (_g(G4, ()), "C32", "far"): "g4_conv1x1_farA",
    (_g(GC.P17, ("phase",)), "C32", "far"): "p17_phase_4g",
    (_g(GC.P17, ("phase",)), "C32", "very far"): "p17_phase_4g",
    (_g(G0, ()), "A", "very far"): "g0_lin_lda",
    (_g(G3, ()), "C32", "very far"): "g3_lin_ldc32",
    (("gn", "", ()), "x1", "very far"): "gn_c256_4g",
    (("gn", "", ()), "y16", "far"): "gn_c256_4g",
    (("gn", "", ()), "x1", "far"): "gn_c512_2g",
    (("gn", "", ("producer statistics",)), "x1", "far"): "gn_stats_c128_2g",
    (("act", "act 0", ()), "x", "very far"): "act0_4g",
    (("act", "act 0", ()), "x", "far"): "act0_4g",
    (("act", "act 0", ()), "y", "far"): "act0_4g",
    (("smax", "", ()), "in", "very far"): "smax_65536",
    (("smax", "", ()), "out", "very far"): "smax_65536",
}
P17, P21, SN31 = GC.P17, GC.P21, GC.SN31
BUILDERS.update({
    "g0_lin_ldc32": lambda e, f: linear_case("g0_lin_ldc32", e, f, G0, 128, 136, "C32"),
    "gn_c256_8g": lambda e, f: gn_case("gn_c256_8g", e, f, 256, 33),
    "gn_stats_c128_8g": lambda e, f: gn_case("gn_stats_c128_8g", e, f, 128, 33, stats=True),
    "act0_8g": lambda e, f: act_case("act0_8g", e, f, more=1),
    "g0_conv_stats_4g_farA": lambda e, f: conv_case("g0_conv_stats_4g_farA", e, f, G0, 128, 3, lda=256, stats=True, more=1),
    "g0_conv_c16_res_4g": lambda e, f: conv_case("g0_conv_c16_res_4g", e, f, G0, 128, 3, resid=True, c16=True, more=1),
    "g0_conv_stats_res": lambda e, f: conv_case("g0_conv_stats_res", e, f, G0, 128, 3, resid=True, stats=True),
    "g0_conv_stats_res_4g": lambda e, f: conv_case("g0_conv_stats_res_4g", e, f, G0, 128, 3, resid=True, stats=True, more=1),
    "p21_conv_stats": lambda e, f: conv_case("p21_conv_stats", e, f, P21, 256, 3, N=256, cin=64, stats=True, srows=128),
    "p21_conv_stats_res": lambda e, f: conv_case("p21_conv_stats_res", e, f, P21, 256, 3, N=256, cin=64, resid=True, stats=True, srows=128),
    "p21_conv_c16_res": lambda e, f: conv_case("p21_conv_c16_res", e, f, P21, 256, 3, N=256, cin=64, resid=True, c16=True),
    "n31_conv_farA": lambda e, f: conv_case("n31_conv_farA", e, f, SN31, 256, 3, N=3, cin=128, auto=True, mrows=1 << 24),
})
# the further forms of the 64-image decode (see FAR_PLANS): GroupNorm and the conversion there run over 64 images of 2^20 pixels; the cases run one image of as many bytes
FAR_CASES_BATCH = {
    (_g(G0, ()), "C32", "very far"): "g0_lin_ldc32",
    (("gn", "", ()), "y16", "very far"): "gn_c256_8g",
    (("act", "act 0", ()), "y", "very far"): "act0_8g",
    (("gn", "", ("producer statistics",)), "x1", "very far"): "gn_stats_c128_8g",
    (("gn", "", ("producer statistics",)), "y16", "far"): "gn_stats_c128_8g",
    (("gn", "", ("producer statistics",)), "y16", "very far"): "gn_stats_c128_8g",
    (_g(G0, ("colstats",)), "A", "very far"): "g0_conv_stats_4g_farA",
    (_g(G0, ("colstats",)), "C32", "very far"): "g0_conv_stats_4g_farA",
    (_g(G0, ("C16 + C32", "residual")), "resid", "very far"): "g0_conv_c16_res_4g",
    (_g(G0, ("C16 + C32", "residual")), "C32", "very far"): "g0_conv_c16_res_4g",
    (_g(G0, ("colstats", "residual")), "resid", "far"): "g0_conv_stats_res",
    (_g(G0, ("colstats", "residual")), "C32", "far"): "g0_conv_stats_res",
    (_g(G0, ("colstats", "residual")), "resid", "very far"): "g0_conv_stats_res_4g",
    (_g(G0, ("colstats", "residual")), "C32", "very far"): "g0_conv_stats_res_4g",
    (_g(P21, ("colstats",)), "C32", "far"): "p21_conv_stats",
    (_g(P21, ("colstats", "residual")), "resid", "far"): "p21_conv_stats_res",
    (_g(P21, ("colstats", "residual")), "C32", "far"): "p21_conv_stats_res",
    (_g(P21, ("C16 + C32", "residual")), "resid", "far"): "p21_conv_c16_res",
    (_g(P21, ("C16 + C32", "residual")), "C32", "far"): "p21_conv_c16_res",
    (_g(SN31, ()), "A", "very far"): "n31_conv_farA",
}
GIB = 1 << 30
# forms that no arena of 16 GiB holds: {form: (why, bytes of the operands the launch needs at the smallest M that keeps the operand in its class)}
BEYOND_ARENA = {
    (_g(G0, ("C16 + C32", "residual")), "A", "very far"): ("4 GiB of A rows of 128 halfs are 2^24 pixels: the fp32 output and the residual are 8 GiB each", (4 * GIB, 8 * GIB, 8 * GIB, 4 * GIB)),
    (_g(G0, ("C16 + C32", "residual")), "C16", "very far"): ("4 GiB of fp16 rows are 2^24 pixels: the fp32 output and the residual are 8 GiB each", (4 * GIB, 8 * GIB, 8 * GIB)),
    (_g(G0, ("colstats", "residual")), "A", "very far"): ("4 GiB of A rows of 128 halfs are 2^24 pixels: the fp32 output and the residual are 8 GiB each", (4 * GIB, 8 * GIB, 8 * GIB)),
    (_g(P17, ("phase",)), "A", "very far"): ("4 GiB of source rows of 256 halfs are 2^23 pixels: the upsampled fp32 map of 256 channels is 32 GiB", (4 * GIB, 32 * GIB)),
}
ALL_FAR_CASES = {**FAR_CASES, **FAR_CASES_BATCH}
CASE_IDS = sorted(set(ALL_FAR_CASES.values()))
# Strided operands that no plan puts far today, but whose launchers take a 64-bit leading dimension or batch stride without refusing any: the residual and fp16
# output rows of a GEMM, LayerNorm's ldx, GroupNorm's ld1 / ld2, the ld of the NHWC -> NCHW conversion, attention's ldq, ldk, ldv, ldo and bsq, bsk, bsv, bso (the tile-loop kernel, and the one-pass kernel for ldk / ldv; the
# 256-row kernels would need 2048 queries or 128 keys at these strides, more than an arena holds: tests/test_far_offsets_cpu.py holds their 2^30-element guard instead)
STRIDED_ONLY = {
    "g0_lin_ldr_ldc16": lambda e, f: linear_res_c16_case("g0_lin_ldr_ldc16", e),
    "ln_ldx": lambda e, f: ln_case("ln_ldx", e),
    "gn_ld1_ld2": lambda e, f: gn_strided_case("gn_ld1_ld2", e),
    "h2n_ld": lambda e, f: h2n_case("h2n_ld", e),
}
STRIDED_ONLY.update({f"attn_{how}{'o' if n == 'out' else n}": (lambda e, f, n=n, how=how: attn_case(f"attn_{how}{'o' if n == 'out' else n}", e, n, how))
                     for n in ("q", "k", "v", "out") for how in ("ld", "bs")})
BUILDERS.update(STRIDED_ONLY)
ALL_IDS = CASE_IDS + sorted(STRIDED_ONLY)


def build_case(cid, e=E_REAL):
    return BUILDERS[cid](e, [k for k, v in ALL_FAR_CASES.items() if v == cid])


def case_classes(case):
    """{operand: class} of the case's own operands, by the census's rule"""
    out = {}
    for o in case.ops.values():
        if o.extent >= case.b32:
            out[o.name] = "very far"
        elif o.extent >= case.b31:
            out[o.name] = "far"
    return out


# ------------------------------------------------------------------ the launch on the device
class DeviceMemory:
    """the arena of one case on the device: one DeviceBuffer, raw-pointer mlsd_memcpy / mlsd_memset / mlsd_count_nonfinite"""

    def __init__(self, _lib, nbytes):
        self._lib, self.L = _lib, _lib.lib()
        self.buf = _lib.DeviceBuffer(nbytes + 64)
        self.base = self.buf.ptr
        self.cnt = _lib.DeviceBuffer(16)

    def ptr(self, off):
        return self.base + off

    def _cp(self, dst, src, n, kind):
        self._lib.check(self.L.mlsd_memcpy(self._lib.vp(dst), self._lib.vp(src), ctypes.c_size_t(n), kind, None), "mlsd_memcpy")

    def write(self, off, arr):
        arr = np.ascontiguousarray(arr)
        self._cp(self.base + off, arr.ctypes.data, arr.size, 0)
        self._lib.check(self.L.mlsd_stream_sync(None), "sync")

    def copy(self, dst, src, n):
        self._cp(self.base + dst, self.base + src, n, 2)

    def memset(self, off, value, n):
        self._lib.check(self.L.mlsd_memset(self._lib.vp(self.base + off), value, ctypes.c_size_t(n), None), "mlsd_memset")

    def read(self, off, n):
        out = np.empty(n, np.uint8)
        self._cp(out.ctypes.data, self.base + off, n, 1)
        self._lib.check(self.L.mlsd_device_sync(), "sync")
        return out

    def count_nonfinite(self, off, nwords):
        self.cnt.upload(np.zeros(4, np.int32))
        self._lib.check(self.L.mlsd_count_nonfinite(self._lib.vp(self.base + off), ctypes.c_size_t(nwords), self._lib.vp(self.cnt.ptr), None), "mlsd_count_nonfinite")
        self._lib.check(self.L.mlsd_device_sync(), "sync")
        return int(self.cnt.download((4,), np.int32)[0])

    def free(self):
        self.buf.free()
        self.cnt.free()


def gemm_args(case, ptr):
    """mlsd_gemm_args of a gemm case on operands at ptr(offset)"""
    from mlimgsynth_amd import kernels
    kw, o = case.kw, case.ops
    a = kernels.GemmArgs(A=ptr(o["A"].off), lda=kw["lda"], W_=ptr(o["W"].off), ldb=kw["K"], M=kw["M"], N=kw["N"], K=kw["K"], ksplit=1,
                         tile_variant=0 if kw.get("auto") else kernels.tile_arg(_tile_no(kw["tile"])), C32=ptr(o["C32"].off), ldc32=kw.get("ldc32", kw["N"]))
    if kw.get("k"):
        a.conv, a.n_img, a.H, a.W, a.Cin, a.OH, a.OW, a.KH, a.KW, a.stride, a.pad = 1, 1, kw["H"], kw["W"], kw["cin"], kw["H"], kw["W"], kw["k"], kw["k"], 1, kw["pad"]
    if "bias" in o:
        a.bias = ptr(o["bias"].off)
    if "resid" in o:
        a.resid, a.ldr = ptr(o["resid"].off), kw.get("ldr", kw["N"])
    if "C16" in o:
        a.C16, a.ldc16 = ptr(o["C16"].off), kw.get("ldc16", kw["N"])
    if "colstats" in o:
        a.colstats, a.colstats_rows, a.colstats_shift = ptr(o["colstats"].off), kw.get("srows", 64), 1
    return a


def launch(case, mem):
    """the case's launch on the device arena; returns the label of the kernel that ran"""
    from mlimgsynth_amd import _lib, kernels
    kw, o, ptr = case.kw, case.ops, mem.ptr
    L = _lib.lib()
    if case.op == "gemm" and kw.get("phase"):
        for q in range(4):
            a = kernels.GemmArgs(A=ptr(o["A"].off), lda=kw["lda"], conv=1, n_img=1, H=kw["H"], W=kw["W"], Cin=kw["cin"], OH=kw["H"], OW=kw["W"], KH=2, KW=2, stride=1, pad=1,
                                 W_=ptr(o[f"W{q + 1}"].off), ldb=kw["K"], M=kw["M"], N=kw["N"], K=kw["K"], bias=ptr(o["bias"].off), C32=ptr(o["C32"].off), ldc32=kw["N"],
                                 ksplit=1, tile_variant=kernels.tile_arg(_tile_no(kw["tile"])), tap_oy=q >> 1, tap_ox=q & 1, out_phase=q + 1)
            label = kernels.gemm_variant(a)
            assert label == kw["variant"], f"{case.id}: launch label {label} of phase {q + 1}, case written for {kw['variant']}"
            kernels.gemm(a)
        label += " x 4 phases"
    elif case.op == "gemm":
        a = gemm_args(case, ptr)
        label = kernels.gemm_variant(a)
        assert label == kw["variant"], f"{case.id}: launch label {label}, case written for {kw['variant']}"
        if kw.get("stats"):
            assert kernels.gemm_route(a).stats_rows == kw.get("srows", 64), f"{case.id}: the launch writes statistics of {kernels.gemm_route(a).stats_rows} rows"
        kernels.gemm(a)
    elif case.op == "gn":
        a = kernels.GnArgs(x1=ptr(o["x1"].off), ld1=kw["C"], C1=kw["C"], n_img=1, HW=kw["HW"], n_grp=kw["G"], eps=kw["eps"], gamma=ptr(o["gamma"].off),
                           beta=ptr(o["beta"].off), silu=kw["silu"], y16=ptr(o["y16"].off), ws=ptr(o["ws"].off))
        if kw["stats"]:
            a.cs1, a.rb_rows1, a.cs_shifted = ptr(o["cs1"].off), 64, 1
        assert kernels.groupnorm_ws_bytes(1, kw["HW"], kw["G"]) <= o["ws"].extent
        kernels.groupnorm(a)
        label = "groupnorm" + (" from producer statistics" if kw["stats"] else "")
    elif case.op == "act":
        _lib.check(L.mlsd_act_f32_to_f16(_lib.vp(ptr(o["x"].off)), _lib.vp(ptr(o["y"].off)), ctypes.c_size_t(kw["n"]), 0, None), "mlsd_act_f32_to_f16")
        label = "act_f32_to_f16"
    elif case.op == "smax":
        _lib.check(L.mlsd_softmax_rows(_lib.vp(ptr(o["in"].off)), ctypes.c_int64(kw["ld_in"]), _lib.vp(ptr(o["out"].off)), ctypes.c_int64(kw["ld_out"]),
                                       kw["rows"], kw["cols"], ctypes.c_float(kw["scale"]), None), "mlsd_softmax_rows")
        label = "softmax_rows"
    elif case.op == "ln":
        kernels.layernorm(ptr(o["x"].off), kw["ldx"], kw["rows"], kw["d"], kw["eps"], ptr(o["g"].off), ptr(o["b"].off), ptr(o["y16"].off))
        label = "layernorm"
    elif case.op == "gns":
        a = kernels.GnArgs(x1=ptr(o["x1"].off), x2=ptr(o["x2"].off), ld1=kw["ld"], ld2=kw["ld"], C1=kw["C1"], C2=kw["C2"], n_img=1, HW=kw["HW"], n_grp=kw["G"], eps=kw["eps"],
                           gamma=ptr(o["gamma"].off), beta=ptr(o["beta"].off), silu=kw["silu"], y16=ptr(o["y16"].off), ws=ptr(o["ws"].off))
        assert kernels.groupnorm_ws_bytes(1, kw["HW"], kw["G"]) <= o["ws"].extent
        kernels.groupnorm(a)
        label = "groupnorm, concat source"
    elif case.op == "h2n":
        _lib.check(L.mlsd_nhwc_to_nchw_f32(_lib.vp(ptr(o["src"].off)), ctypes.c_int64(kw["ld"]), 1, kw["C"], kw["HW"], _lib.vp(ptr(o["dst"].off)),
                                           ctypes.c_float(kw["mul"]), ctypes.c_float(kw["add"]), None), "mlsd_nhwc_to_nchw_f32")
        label = "nhwc_to_nchw_f32"
    elif case.op == "attn":
        ld, bs = kw["ld"], kw["bs"]
        a = kernels.AttnArgs(q=ptr(o["q"].off), k=ptr(o["k"].off), v=ptr(o["v"].off), out=ptr(o["out"].off), ldq=ld["q"], ldk=ld["k"], ldv=ld["v"], ldo=ld["o"],
                             bsq=bs["q"], bsk=bs["k"], bsv=bs["v"], bso=bs["o"], n_batch=kw["n_batch"], n_head=1, d_head=64, Tq=kw["Tq"], Tk=kw["Tk"], causal=0)
        label = kernels.attention_variant(a)
        assert label and label.startswith(kw["label"]), f"{case.id}: launch label {label}, case written for {kw['label']}"
        kernels.attention(a)
    else:
        raise PA.Unknown(case.op)
    kernels.sync()
    return label
