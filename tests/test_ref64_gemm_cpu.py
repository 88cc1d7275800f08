"""The float64 GEMM bounds of tests/ref64.py are sharp enough to matter, shown on the CPU.

An fp32 emulation of a correct kernel -- exact fp16 products, one fp32 rounding per MFMA step of 16 products, the steps added to one fp32
accumulator in K order, split-K slices added in slice order, the epilogue in fp32 and one round-to-nearest-even to fp16 -- must stay within
the bound at the tile structure of the GPU cases (scaled down).  Each seeded fault below must exceed it somewhere.  For each fault the test
also reports whether the older global tolerances (rel-L2 <= 2e-5 for fp32 outputs, <= 1e-3 for fp16: tests/test_kernels_gpu.py) would
have caught it; run with -s to see the table.
"""
import numpy as np
import pytest

import gemm64_cases as GC
import ref64 as R

F32 = np.float32
K_STEP = R.K_STEP_GENERAL

CPU_CASES = {
    "splitk": GC.lin("cpu_splitk", "", "cpu", 96, 80, 448, bias=True, resid=True, c16=True, ksplit=3),
    "bigres": GC.lin("cpu_bigres", "", "cpu", 64, 72, 320, fam="bigres", bias=True, resid=True, c16=True),
    "geglu": GC.lin("cpu_geglu", "", "cpu", 64, 128, 136, bias=True, act=5, c16=True),
    "conv": GC.conv("cpu_conv", "", "cpu", 2, 9, 7, 16, 32, 3, 1, 1, bias=True, c16=True),
    "conv_s2_ups": GC.conv("cpu_conv_s2", "", "cpu", 1, 5, 7, 12, 24, 3, 2, 1, ups=1, fam="scales", bias=True, c16=True),
    "subnormal": GC.lin("cpu_subnormal", "", "cpu", 64, 64, 320, fam="subnormal", c16=True),
    "silu_wide": GC.lin("cpu_silu", "", "cpu", 64, 96, 72, fam="wideact", bias=True, act=1, resid=True, c16=True),
    "gelu_wide": GC.lin("cpu_gelu", "", "cpu", 64, 96, 72, fam="wideact", bias=True, act=2, c16=True),
    "qgelu_post": GC.lin("cpu_qgelu", "", "cpu", 64, 96, 72, fam="wideact", bias=True, act=3, resid=True, post=True, c16=True),
    "offset": GC.lin("cpu_offset", "", "cpu", 64, 64, 1280, fam="offset", bias=True, c16=True, ksplit=4),
    "bigout": GC.lin("cpu_bigout", "", "cpu", 64, 64, 256, fam="bigout", c16=True),
    "tinyout": GC.lin("cpu_tinyout", "", "cpu", 64, 64, 256, fam="tinyout", c16=True),
}


def im2col(c, A, clamp_top=False):
    if not c["conv"]:
        return np.asarray(A, np.float64)
    x = np.asarray(A, np.float64)
    if clamp_top:      # fault 6: the top border reads the clamped (first) source row instead of zero padding
        n, H, W, C = c["n"], c["H"], c["W"], c["cin_pad"]
        x4 = x.reshape(n, H, W, C)
        xp = np.concatenate([x4[:, :1], x4], axis=1).reshape(-1, C)
        got = R.im2col64(xp, n, H + 1, W, C, c["k"], c["k"], c["s"], c["p"] - 1 if c["p"] else 0, c["ups"], c["OH"], c["OW"])
        return got
    return R.im2col64(x, c["n"], c["H"], c["W"], c["cin_pad"], c["k"], c["k"], c["s"], c["p"], c["ups"], c["OH"], c["OW"])


def act32(z, act):
    z = z.astype(F32)
    with np.errstate(over="ignore"):
        if act == 1:
            return z / (F32(1) + np.exp(-z))
        if act in (2, 5):
            k1 = F32(-2.0 * 0.7978845608028654 * 1.4426950408889634)
            return z * (F32(1) / (F32(1) + np.exp2(z * (k1 * F32(0.044715) * z * z + k1))))
        if act == 3:
            return z / (F32(1) + np.exp(F32(-1.702) * z))
        if act == 4:
            return np.maximum(z, F32(0))
    return z


def emulate(c, ops, fault=None):
    """fp32 outputs (C32, C16) of a correct kernel, or of one with `fault`"""
    A, Wt = ops["A"], ops["W"]
    if fault == "flush_subnormal":
        tiny = lambda a: np.where(np.abs(a.astype(np.float64)) < 2.0 ** -14, np.float16(0), a)
        A, Wt = tiny(A), tiny(Wt)
    Am = im2col(c, A, clamp_top=fault == "conv_clamp")
    W64 = np.asarray(Wt, np.float64)
    M, N, K = Am.shape[0], W64.shape[0], Am.shape[1]
    nkt = -(-K // 64)
    per = -(-nkt // c["ksplit"]) if c["ksplit"] > 1 else nkt
    slices = []
    for s0 in range(0, nkt, per):
        acc = np.zeros((M, N), F32)
        for k0 in range(s0 * 64, min(K, (s0 + per) * 64), K_STEP):
            step = (Am[:, k0:k0 + K_STEP] @ W64[:, k0:k0 + K_STEP].T).astype(F32)      # exact products, one rounding per MFMA step
            if fault == "drop_ktile" and k0 // 64 == 1:
                step[:32, :32] = 0                                                      # one 64-wide K tile missing in one output tile
            acc = acc + step
        slices.append(acc)
    tot = slices[0]
    for i, s in enumerate(slices[1:], 1):
        if fault == "fp16_partial" and i == 1:
            tot = tot.astype(np.float16).astype(F32)                                    # partial sum held in fp16 at a slice boundary
        tot = tot + s
        if fault == "slice_twice" and i == 1:
            tot = tot + s
    z = tot
    rd = (lambda v: v.astype(np.float16).astype(F32)) if fault == "fp16_epilogue_operand" else (lambda v: v)
    if "bias" in ops:
        z = z + rd(ops["bias"])[None, :]
    if c["act"] == 5:
        vc, gc = R.geglu_cols(N // 2)
        a_, g_ = z[:, vc], z[:, gc]
        if fault == "geglu_f16":
            a_, g_ = a_.astype(np.float16).astype(F32), g_.astype(np.float16).astype(F32)
        y = a_ * act32(g_, 2)
        if "resid" in ops:
            y = y + rd(ops["resid"])
    else:
        r = rd(ops["resid"]) if "resid" in ops else None
        if r is not None and c["post"]:
            z = z + r
        y = act32(z, c["act"])
        if r is not None and not c["post"]:
            y = y + r
    y = y.astype(F32)
    if fault == "rtz16":
        h = y.astype(np.float16)
        over = np.abs(h.astype(np.float64)) > np.abs(y.astype(np.float64))
        h = np.where(over, np.nextafter(h, np.float16(0)), h)                           # round toward zero
        return y, h
    return y, y.astype(np.float16)


def worst(c, ops, y32, y16):
    rows, cols = np.arange(c["M"]), np.arange(c["nout"])
    A = im2col(c, ops["A"])
    acc, S = R.gemm64(A, ops["W"])
    nsl = -(-(-(-c["K"] // 64)) // (-(-(-(-c["K"] // 64)) // c["ksplit"]))) if c["ksplit"] > 1 else 1
    D = R.gemm_depth(c["K"], K_STEP, nsl)
    y, b = R.gemm_epilogue64(acc, S, D, rows, cols, bias=ops.get("bias"), act=c["act"], resid=ops.get("resid"), act_after_resid=c["post"])
    r32, r16 = R.gemm_ratio32(y32, y, b).max(), R.gemm_ratio16(y16, y, b).max()
    fin = np.isfinite(y16.astype(np.float64)) & (np.abs(y) < 65504)
    rel = lambda g, m: np.linalg.norm((g.astype(np.float64) - y)[m]) / max(np.linalg.norm(y[m]), 1e-300)
    return r32, r16, rel(y32, np.ones_like(fin)), rel(y16, fin)


@pytest.mark.parametrize("name", sorted(CPU_CASES))
def test_correct_emulation_is_within_the_bound(name):
    c = CPU_CASES[name]
    ops = GC.make_operands(c)
    r32, r16, _, _ = worst(c, ops, *emulate(c, ops))
    print(f"\ncorrect emulation {name:12s} worst ratio C32 {r32:.3f}  C16 {r16:.3f}")
    assert r32 <= 1.0 and r16 <= 1.0


FAULTS = [
    ("drop_ktile", "splitk", "one 64-wide K tile dropped in one output tile"),
    ("slice_twice", "splitk", "one split-K slice added twice"),
    ("fp16_epilogue_operand", "splitk", "bias and residual rounded to fp16 before the add"),
    ("fp16_epilogue_operand", "bigres", "bias and residual rounded to fp16 before the add (residual ~1e3)"),
    ("rtz16", "splitk", "fp16 output rounded toward zero"),
    ("geglu_f16", "geglu", "GEGLU value and gate rounded to fp16 before the product"),
    ("conv_clamp", "conv", "conv top border reads the clamped neighbour instead of zero"),
    ("flush_subnormal", "subnormal", "fp16 subnormal operands flushed to zero"),
    ("fp16_partial", "offset", "partial sum held in fp16 at a slice boundary"),
]


@pytest.mark.parametrize("fault,name,what", FAULTS, ids=[f"{f}-{n}" for f, n, _ in FAULTS])
def test_seeded_fault_exceeds_the_bound(fault, name, what):
    c = CPU_CASES[name]
    ops = GC.make_operands(c)
    r32, r16, l32, l16 = worst(c, ops, *emulate(c, ops, fault))
    old = "caught" if (l32 > 2e-5 or l16 > 1e-3) else "MISSED"
    print(f"\nfault {what:62s} worst ratio C32 {r32:10.3g}  C16 {r16:10.3g}   rel-L2 C32 {l32:.2e} C16 {l16:.2e}: old tolerance {old}")
    assert max(r32, r16) > 1.0, f"{what}: not detected"
