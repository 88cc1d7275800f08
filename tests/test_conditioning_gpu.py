"""GroupNorm, LayerNorm and attention kernels against float64 on badly conditioned inputs.

The op-level suite (test_kernels_gpu.py) feeds well-conditioned data and bounds one global rel-L2 number.  Here every statistics
path and every attention kernel meets the inputs under which normalisation and softmax go wrong -- group / row means far above the
spread (r = |mean| / std up to 3000, magnitudes to ~1e4), near-constant and exactly constant groups and rows, outlier channels,
score scales sigma = 1 .. 16, peaked rows, rows of equal scores, key tiles far below the row maximum, ragged key counts, V with a
large common offset -- and is held PER GROUP / PER ROW to the bounds of tests/ref64.py, against float64 on the exact values the
kernel reads.  Every test prints its worst ratio to the bound (<= 1 passes).
"""
import ctypes

import numpy as np
import pytest

import ref64 as R

pytestmark = pytest.mark.gpu


def _has_experiments():
    try:
        from mlimgsynth_amd import _lib
        return bool(_lib.lib().mlsd_has_experiments())
    except Exception:
        return False


HAS_EXP = _has_experiments()
needs_experiments = pytest.mark.skipif(not HAS_EXP, reason="variant not in the product build (make EXPERIMENTS=1)")

RS = (0.0, 30.0, 300.0, 3000.0)      # r = |group mean| / group std, mixed inside one tensor
EPS_GN, EPS_LN = 1e-6, 1e-5


@pytest.fixture(scope="module")
def K():
    from mlimgsynth_amd import kernels, _lib
    L = _lib.lib()
    L.mlsd_gemm_colstats_rows.argtypes = [ctypes.POINTER(kernels.GemmArgs)]
    L.mlsd_gemm_ln_fused.argtypes = [ctypes.POINTER(kernels.GemmArgs)]
    L.mlsd_gemm_xattn_fused.argtypes = [ctypes.POINTER(kernels.GemmArgs)]
    L.mlsd_xattn_pack_vt.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return kernels, _lib


def dev(_lib, a):
    return _lib.from_numpy(np.ascontiguousarray(a))


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------ GroupNorm
def group_plan(rng, G):
    """(offset, std) per group: r cycles through RS with both signs; group G-2 is near-constant (std = 1e-4 |mean|), G-1 exactly constant."""
    sd = 10.0 ** rng.uniform(-0.5, 0.5, G)
    off = np.array([RS[g % 4] for g in range(G)]) * sd * np.where(np.arange(G) % 8 < 4, 1.0, -1.0)
    off[G - 2], sd[G - 2] = 5.0, 5e-4
    off[G - 1], sd[G - 1] = 7.25, 0.0
    return off, sd


def report_gn(path, ratio, r):
    """ratio / r: [n_img][G].  Prints the worst ratio overall and per r class, asserts <= 1 per (image, group)."""
    cls = {f"r~{int(v)}": np.isclose(r, v, rtol=0.5, atol=1.0) for v in RS}
    cls["r>=1e4"] = r >= 1e4 - 1
    parts = ", ".join(f"{k} {ratio[m].max():.3f}" for k, m in cls.items() if m.any())
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"\n[conditioning] groupnorm {path}: worst ratio {ratio.max():.3f} at (image, group) {tuple(int(i) for i in worst)} r={r[worst]:.3g}  ({parts})")
    assert np.all(ratio <= 1.0), (path, float(ratio.max()), float(r[worst]))


def check_mean_rstd(path, table, x, G):
    """The [n_img][G][2] mean / rstd table the finalize writes, against float64."""
    mu, var, r, _ = R.group_stats(x, G, EPS_GN)
    sd = np.sqrt(var + EPS_GN)
    em = np.abs(table[..., 0] - mu) / (R.C_NORM * R.U32 * (np.abs(mu) + sd))
    er = np.abs(table[..., 1] * sd - 1.0) / (R.C_NORM * R.U32 * (1.0 + r))
    print(f"[conditioning] groupnorm {path}: mean / rstd table worst ratio {em.max():.3f} / {er.max():.3f}")
    assert np.all(em <= 1.0) and np.all(er <= 1.0), (path, float(em.max()), float(er.max()))


def check_shifted_colstats(name, c32, st, rows):
    """The producer's statistics themselves (colstats_shift = 1): per block and column sum (x - K) and sum (x - K)^2, K = the block's first row,
    against float64 on the stored output, each to C_NORM u32 of the sum of the magnitudes of its terms."""
    es, eq = R.colstats_ratios(c32, st, rows)
    print(f"\n[conditioning] colstats {name} rows {rows}: shifted sums worst ratio {es.max():.3f} / {eq.max():.3f}")
    assert np.all(es <= 1.0) and np.all(eq <= 1.0), (name, float(es.max()), float(eq.max()))


def run_gn(K, x1, x2, G, gamma, beta, ws, cs=None, rb=None, table=False):
    """mlsd_groupnorm on device maps x1 [/ x2] (DeviceBuffer, shape); returns fp16 output [n][HW][C] and, with table, the mean / rstd table."""
    kernels, _lib = K
    (d1, s1), (d2, s2) = x1, (x2 if x2 is not None else (None, None))
    n, hw, C1 = s1
    C2 = s2[2] if x2 is not None else 0
    C = C1 + C2
    dG, dB = dev(_lib, gamma), dev(_lib, beta)
    dY = _lib.DeviceBuffer(n * hw * C * 2)
    g = kernels.GnArgs(x1=d1.ptr, ld1=C1, C1=C1, n_img=n, HW=hw, n_grp=G, eps=EPS_GN, gamma=dG.ptr, beta=dB.ptr, silu=1, y16=dY.ptr, ws=ws.ptr)
    if x2 is not None:
        g.x2, g.ld2, g.C2 = d2.ptr, C2, C2
    if cs is not None:
        g.cs1, g.rb_rows1, g.cs_shifted = cs[0].ptr, rb[0], 1
        if x2 is not None:
            g.cs2, g.rb_rows2 = cs[1].ptr, rb[1]
    kernels.groupnorm(g)
    y = dY.download((n, hw, C), np.float16).astype(np.float64)
    t = ws.download((n * G * 2,), np.float32).astype(np.float64).reshape(n, G, 2) if table else None
    return y, t


@pytest.mark.parametrize("form,n,hw,c1,c2", [("two_kernel", 2, 1024, 320, 0), ("two_kernel_concat", 2, 1024, 164, 156),
                                             ("single_pass", 2, 256, 640, 0), ("single_pass_concat", 2, 256, 328, 312)])
def test_groupnorm_plain_paths(K, form, n, hw, c1, c2):
    """The two-kernel form (gn_stats shifted sums + gn_apply) and the one-dispatch form (gn_small_kernel, two-pass); concat forms have a group
    that straddles the two sources."""
    kernels, _lib = K
    L = _lib.lib()
    G, C = 32, c1 + c2
    rng = np.random.default_rng(hw + c1)
    off, sd = group_plan(rng, G)
    cg = C // G
    x = (off.repeat(cg) + sd.repeat(cg) * rng.standard_normal((n, hw, C))).astype(np.float32)
    gamma, beta = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    single = form.startswith("single")
    d1 = dev(_lib, x[..., :c1])
    d2 = dev(_lib, x[..., c1:]) if c2 else None
    ws = _lib.DeviceBuffer(kernels.groupnorm_ws_bytes(n, hw, G))
    try:
        L.mlsd_groupnorm_set_single(1 if single else 0)
        assert L.mlsd_groupnorm_single_pass(n, hw, C, G) == (1 if single else 0)
        y, _ = run_gn(K, (d1, (n, hw, c1)), (d2, (n, hw, c2)) if c2 else None, G, gamma, beta, ws)
    finally:
        L.mlsd_groupnorm_set_single(1)
    want = R.groupnorm64(x, None, G, EPS_GN, gamma, beta, True)
    report_gn(form, *R.groupnorm_worst(y, want, x, G, EPS_GN, gamma, beta))


# producers of column statistics: (name, tile_variant, ksplit, rows per statistics block)
PRODUCERS = [("pp17", 18, 0, 128), ("pp18", 19, 0, 64), ("pp20", 21, 0, 64), ("pp21", 22, 0, 128),
             ("general_v0", 1, 0, 64), ("general_v1", 2, 0, 32), ("splitk_reduce_stats", 2, 3, 32)]


def produce(K, rng, n, hw, N, Kd, G_off, G_sd, variant, ksplit, rows, res):
    """One GEMM that writes an fp32 map with the given per-column offsets / spreads and its column statistics.  The offsets come in the
    way the plan gets them: a per-column bias equal within a group, and with res half of it from a residual."""
    kernels, _lib = K
    L = _lib.lib()
    M = n * hw
    A = rng.standard_normal((M, Kd)).astype(np.float16)
    W = (rng.standard_normal((N, Kd)) / np.sqrt(Kd) * G_sd[:, None]).astype(np.float16)
    bias = (G_off * (0.5 if res else 1.0)).astype(np.float32)
    Rm = ((G_off * 0.5)[None, :] + 0.1 * G_sd[None, :] * rng.standard_normal((M, N))).astype(np.float32) if res else None
    keep = [dev(_lib, A), dev(_lib, W), dev(_lib, bias)]
    dC = _lib.DeviceBuffer(M * N * 4)
    dS = _lib.DeviceBuffer(M // rows * 2 * N * 4)
    a = kernels.GemmArgs(A=keep[0].ptr, lda=Kd, W_=keep[1].ptr, ldb=Kd, M=M, N=N, K=Kd, bias=keep[2].ptr, C32=dC.ptr, ldc32=N, tile_variant=variant, colstats=dS.ptr,
                         colstats_shift=1)
    if res:
        keep.append(dev(_lib, Rm))
        a.resid, a.ldr = keep[-1].ptr, N
    if ksplit:
        nws = kernels.gemm_splitk_ws_bytes(M, N, ksplit)
        keep.append(_lib.DeviceBuffer(nws))
        a.ksplit, a.ws, a.ws_bytes = ksplit, keep[-1].ptr, nws
    assert L.mlsd_gemm_colstats_rows(ctypes.byref(a)) == rows
    assert ("k/" in kernels.gemm_variant(a)) == (ksplit > 1)
    kernels.gemm(a)
    return dC, dS, keep


def producer_case(K, name, variant, ksplit, rows, n, hw, Ns, Kd, finalize2, res, seed):
    kernels, _lib = K
    L = _lib.lib()
    G = 32
    C = sum(Ns)
    rng = np.random.default_rng(seed)
    off, sd = group_plan(rng, G)
    cg = C // G
    maps, stats, keep = [], [], []
    c0 = 0
    for N in Ns:
        dC, dS, k = produce(K, rng, n, hw, N, Kd, off.repeat(cg)[c0:c0 + N], sd.repeat(cg)[c0:c0 + N], variant, ksplit, rows, res)
        maps.append((dC, (n, hw, N))); stats.append(dS); keep += k
        c0 += N
    gamma, beta = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    ws = _lib.DeviceBuffer(kernels.groupnorm_ws_bytes(n, hw, G))
    try:
        L.mlsd_groupnorm_set_finalize2(finalize2)
        y, table = run_gn(K, maps[0], maps[1] if len(Ns) > 1 else None, G, gamma, beta, ws, cs=stats, rb=[rows] * len(Ns), table=True)
    finally:
        L.mlsd_groupnorm_set_finalize2(1)
    for (dC, shp), dS, N in zip(maps, stats, Ns):
        check_shifted_colstats(name, dC.download((n * hw, N), np.float32), dS.download((n * hw // rows, 2, N), np.float32), rows)
    x = np.concatenate([m.download(s, np.float32) for m, s in maps], axis=2)
    want = R.groupnorm64(x, None, G, EPS_GN, gamma, beta, True)
    path = f"{name} rows {rows} finalize{'2' if finalize2 else '1'}{' +res' if res else ''}{' concat' if len(Ns) > 1 else ''} ({n}x{hw}x{C})"
    ratio, r = R.groupnorm_worst(y, want, x, G, EPS_GN, gamma, beta)
    try:
        check_mean_rstd(path, table, x, G)
    finally:
        report_gn(path, ratio, r)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("name,variant,ksplit,rows", PRODUCERS)
def test_groupnorm_producer_statistics(K, name, variant, ksplit, rows, res):
    """Producer statistics (the GEMM *_STATS epilogues, the general tiles' wide epilogue, splitk_reduce_stats) through the one-level finalize."""
    producer_case(K, name, variant, ksplit, rows, 2, 1024, [640], 192, 0, res, 7 + variant + ksplit + res)


P = {p[0]: p for p in PRODUCERS}


@pytest.mark.parametrize("name,Ns", [("pp17", [384, 256]), ("pp18", [320, 640]), ("general_v1", [352, 288]), ("splitk_reduce_stats", [352, 288])])
def test_groupnorm_producer_statistics_two_sources(K, name, Ns):
    """Two producers, one group straddling the virtual concat (channels 380..399 across 384, 300..329 across 320, 340..359 across 352)."""
    _, variant, ksplit, rows = P[name]
    producer_case(K, name, variant, ksplit, rows, 2, 1024, Ns, 192, 0, False, 21 + variant + ksplit)


@pytest.mark.parametrize("finalize2", [0, 1])
@pytest.mark.parametrize("name,n,hw,N,Kd", [("pp17", 1, 131072, 128, 192), ("pp18", 1, 65536, 320, 192), ("general_v0", 1, 65536, 128, 128),
                                             ("general_v1", 2, 32768, 128, 128), ("splitk_reduce_stats", 2, 32768, 128, 128)])
def test_groupnorm_producer_statistics_large_map(K, name, n, hw, N, Kd, finalize2):
    """1024 row blocks per image: the two-level finalize (gn_finalize_l1 / _l2) and the one-level one on the same kind of statistics."""
    _, variant, ksplit, rows = P[name]
    assert hw // rows == 1024
    producer_case(K, name, variant, ksplit, rows, n, hw, [N], Kd, finalize2, True, 40 + variant + ksplit)


@needs_experiments
def test_groupnorm_fused_into_split_k_reduce(K):
    """splitk_reduce_gn (mlsd_gemm_gn_fused): the GroupNorm at the end of the split-K reduce pass."""
    kernels, _lib = K
    L = _lib.lib()
    L.mlsd_gemm_gn_fused.argtypes = [ctypes.POINTER(kernels.GemmArgs)]
    n, hw, C, Kd, ksplit, G = 2, 64, 1280, 1280, 10, 32
    M = n * hw
    rng = np.random.default_rng(77)
    off, sd = group_plan(rng, G)
    cg = C // G
    A = rng.standard_normal((M, Kd)).astype(np.float16)
    W = (rng.standard_normal((C, Kd)) / np.sqrt(Kd) * sd.repeat(cg)[:, None]).astype(np.float16)
    dA, dW, dB = dev(_lib, A), dev(_lib, W), dev(_lib, off.repeat(cg).astype(np.float32))
    gamma, beta = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    dG, dBt = dev(_lib, gamma), dev(_lib, beta)
    dC, dY = _lib.DeviceBuffer(M * C * 4), _lib.DeviceBuffer(M * C * 2)
    nws = kernels.gemm_splitk_ws_bytes(M, C, ksplit)
    ws = _lib.DeviceBuffer(nws)
    a = kernels.GemmArgs(A=dA.ptr, lda=Kd, W_=dW.ptr, ldb=Kd, M=M, N=C, K=Kd, bias=dB.ptr, C32=dC.ptr, ldc32=C, tile_variant=2, ksplit=ksplit, ws=ws.ptr, ws_bytes=nws)
    a.gn_y16, a.gn_ldy, a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_groups, a.gn_hw, a.gn_silu = dY.ptr, C, dG.ptr, dBt.ptr, EPS_GN, G, hw, 1
    assert L.mlsd_gemm_gn_fused(ctypes.byref(a)) == 1
    kernels.gemm(a)
    x = dC.download((n, hw, C), np.float32)
    y = dY.download((n, hw, C), np.float16).astype(np.float64)
    want = R.groupnorm64(x, None, G, EPS_GN, gamma, beta, True)
    report_gn("splitk_reduce_gn", *R.groupnorm_worst(y, want, x, G, EPS_GN, gamma, beta))


# ------------------------------------------------------------------ LayerNorm
def row_plan(rng, rows, d, sd_noise=1.0):
    """Row offsets (r cycling through RS, both signs), rows with 3 outlier channels at 1e3 x the rest, the last row constant."""
    r = np.array([RS[i % 4] for i in range(rows)]) * np.where(np.arange(rows) % 8 < 4, 1.0, -1.0)
    x = r[:, None] * sd_noise + sd_noise * rng.standard_normal((rows, d))
    out = np.arange(rows) % 5 == 2
    x[out, :3] *= 1e3
    x[-1] = 3.5
    return x


def report_ln(path, ratio, r):
    worst = int(np.argmax(ratio))
    print(f"\n[conditioning] layernorm {path}: worst ratio {ratio.max():.3f} at row {worst} (r={r[worst]:.3g})")
    assert np.all(ratio <= 1.0), (path, float(ratio.max()), worst)


@pytest.mark.parametrize("form,rows,d", [("row_per_wave", 1000, 1280), ("row_per_wave_d320", 777, 320), ("streaming", 8200, 1280), ("streaming_d640", 9000, 640)])
def test_layernorm_kernel(K, form, rows, d):
    """mlsd_layernorm: one row per wave (ln_kernel) and the streaming form (> 4096 rows), fp32 and fp16 outputs."""
    kernels, _lib = K
    rng = np.random.default_rng(rows + d)
    x = row_plan(rng, rows, d).astype(np.float32)
    gamma, beta = (1 + 0.3 * rng.standard_normal(d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    dx, dg, db = dev(_lib, x), dev(_lib, gamma), dev(_lib, beta)
    dy16, dy32 = _lib.DeviceBuffer(rows * d * 2), _lib.DeviceBuffer(rows * d * 4)
    kernels.layernorm(dx.ptr, d, rows, d, EPS_LN, dg.ptr, db.ptr, dy16.ptr, dy32.ptr)
    want = R.layernorm64(x, EPS_LN, gamma, beta)
    report_ln(f"{form} fp32 out ({rows}x{d})", *R.layernorm_worst(dy32.download((rows, d), np.float32), want, x, EPS_LN, gamma, beta, half=False))
    report_ln(f"{form} fp16 out ({rows}x{d})", *R.layernorm_worst(dy16.download((rows, d), np.float16).astype(np.float64), want, x, EPS_LN, gamma, beta))


@pytest.mark.parametrize("form,M,N,Kd", [("pp128x320", 1024, 1280, 320), ("two_tiles_per_cu", 1024, 1280, 320), ("splitk_reduce_ln", 512, 1280, 1280)])
def test_layernorm_ending_of_the_gemm(K, form, M, N, Kd):
    """The LayerNorm endings of the GEMM: the 128x320 ping-pong tile (mlsd_gemm_ln_fused 1), the two-tiles-per-CU tile, the split-K reduce (2).
    Row offsets, outlier channels and a constant row come in through the residual."""
    kernels, _lib = K
    L = _lib.lib()
    rng = np.random.default_rng(M + N + len(form))
    A = rng.standard_normal((M, Kd)).astype(np.float16)
    A[-1] = 0                                                          # with a constant residual row: a constant output row
    W = (rng.standard_normal((N, Kd)) / np.sqrt(Kd)).astype(np.float16)
    Rm = row_plan(rng, M, N).astype(np.float32)
    gamma, beta = (1 + 0.3 * rng.standard_normal(N)).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    dA, dW, dR, dG, dBt = dev(_lib, A), dev(_lib, W), dev(_lib, Rm), dev(_lib, gamma), dev(_lib, beta)
    dC, dY = _lib.DeviceBuffer(M * N * 4), _lib.DeviceBuffer(M * N * 2)
    variant = {"pp128x320": 19, "two_tiles_per_cu": 31, "splitk_reduce_ln": 2}[form]
    a = kernels.GemmArgs(A=dA.ptr, lda=Kd, W_=dW.ptr, ldb=Kd, M=M, N=N, K=Kd, C32=dC.ptr, ldc32=N, tile_variant=variant, resid=dR.ptr, ldr=N)
    a.ln_y16, a.ldln, a.ln_gamma, a.ln_beta, a.ln_eps = dY.ptr, N, dG.ptr, dBt.ptr, EPS_LN
    keep = []
    if form == "splitk_reduce_ln":
        nws = kernels.gemm_splitk_ws_bytes(M, N, 3)
        keep.append(_lib.DeviceBuffer(nws))
        a.ksplit, a.ws, a.ws_bytes = 3, keep[-1].ptr, nws
        expect = 2
    else:
        tn = 320 if form == "pp128x320" else 160
        keep += [dev(_lib, np.zeros(max((M // 128) * (N // tn) * 128 * 4, 4), np.uint32)), dev(_lib, np.zeros(8192, np.uint32))]
        a.ln_ws, a.ln_cnt = keep[0].ptr, keep[1].ptr
        expect = 1
    assert L.mlsd_gemm_ln_fused(ctypes.byref(a)) == expect
    if form == "two_tiles_per_cu":
        assert "128x160x64tt" in kernels.gemm_variant(a)
    kernels.gemm(a)
    if len(keep) == 2:
        assert not keep[1].download((8192,), np.uint32).any()          # no give-up
    x = dC.download((M, N), np.float32)
    want = R.layernorm64(x, EPS_LN, gamma, beta)
    report_ln(f"{form} ({M}x{N}x{Kd})", *R.layernorm_worst(dY.download((M, N), np.float16).astype(np.float64), want, x, EPS_LN, gamma, beta))


# ------------------------------------------------------------------ attention
SIGMAS = (1, 4, 8, 16)
# name: (switch settings, d_head, Tq, Tk, rounds the scaled Q)
ATTN_KERNELS = {
    "tile_loop": (dict(sp=0, x2=2048, tk96=1), 64, 512, 333, False),
    "tile_loop_d40": (dict(sp=0, x2=2048, tk96=1), 40, 512, 200, False),
    "tk96_one_pass": (dict(sp=0, x2=2048, tk96=1), 64, 512, 77, False),
    "tk96_one_pass_d40": (dict(sp=0, x2=2048, tk96=1), 40, 300, 77, False),
    "x2_lds_dma_64row": (dict(sp=0, x2=256, tk96=1), 64, 512, 333, False),
    "attn64x2s": (dict(sp=2, x2=2048, tk96=1), 64, 512, 320, True),
    "attn64x2s_d40": (dict(sp=2, x2=2048, tk96=1), 40, 512, 320, True),
}
if HAS_EXP:
    ATTN_KERNELS["pingpong"] = (dict(sp=0, x2=2048, tk96=0, pp=2), 64, 512, 333, True)


def attn_operands(rng, heads, d, Tq, Tk, sigma, voff):
    """Q rows N(0, sigma^2) on dims 3.. (score std ~ sigma); dims 0..2 carry the special rows of every head:
    row 1 peaked (+20 on key 5), row 2 all-equal scores (q = 0), row 3 sees key tile 1 (keys 64..127) at -225 below the rest,
    row Tq-2 peaked on a key of the last tile.  V plus a common offset voff."""
    D = heads * d
    q = np.zeros((Tq, heads, d)); k = rng.standard_normal((Tk, heads, d)); v = rng.standard_normal((Tk, heads, d)) + voff
    q[:, :, 3:] = rng.standard_normal((Tq, heads, d - 3)) * sigma * np.sqrt(d / (d - 3))
    k[:, :, :3] = 0
    s = np.sqrt(d) / 8.0
    q[1], q[2], q[3], q[Tq - 2] = 0, 0, 0, 0
    q[1, :, 0] = 8.0; k[5, :, 0] = 20.0 * s                                   # score +20 on key 5, 0 elsewhere
    q[3, :, 1] = 30.0; k[64:min(128, Tk), :, 1] = -60.0 * s                   # -225 on key tile 1
    q[Tq - 2, :, 2] = 8.0; k[Tk - 3, :, 2] = 20.0 * s                         # a late peak: the rescale of the last tile
    return tuple(f16r(a.reshape(a.shape[0], D)) for a in (q, k, v))


def attn_check(name, sigma, voff, q, k, v, heads, got, q_scaled):
    """per-row ratios against the kernel's documented bound; for kernels that round the scaled Q also the ratio without that term (a finding, not asserted)."""
    nb = got.shape[0]
    worst, worst_noq = 0.0, 0.0
    for b in range(nb):
        o, p = R.attention64(q[b], k[b], v[b], heads)
        ratio = R.attention_worst(got[b], o, R.attention_bound(q[b], k[b], v[b], heads, o, p, q_scaled))
        assert np.isfinite(got[b]).all(), (name, sigma, voff)
        worst = max(worst, float(ratio.max()))
        if q_scaled:
            worst_noq = max(worst_noq, float(R.attention_worst(got[b], o, R.attention_bound(q[b], k[b], v[b], heads, o, p, False)).max()))
        bad = np.nonzero(ratio > 1.0)[0]
        assert bad.size == 0, (name, sigma, voff, b, bad[:8].tolist(), float(ratio.max()))
    extra = f", without the Q term {worst_noq:.3f}" if q_scaled else ""
    print(f"\n[conditioning] attention {name} sigma {sigma}{' V+%g' % voff if voff else ''}: worst row ratio {worst:.3f}{extra}")


@pytest.mark.parametrize("sigma,voff", [(s, 0.0) for s in SIGMAS] + [(4, 100.0)])
@pytest.mark.parametrize("name", list(ATTN_KERNELS))
def test_attention_kernel(K, name, sigma, voff):
    kernels, _lib = K
    L = _lib.lib()
    sw, d, Tq, Tk, q_scaled = ATTN_KERNELS[name]
    nb, heads = 2, 3
    D = heads * d
    rng = np.random.default_rng(sigma * 100 + d + Tk + int(voff))
    ops = [attn_operands(rng, heads, d, Tq, Tk, sigma, voff) for _ in range(nb)]
    q, k, v = (np.stack([o[i] for o in ops]) for i in range(3))
    dq, dk, dv = (dev(_lib, a.astype(np.float16)) for a in (q, k, v))
    do = _lib.DeviceBuffer(nb * Tq * D * 2)
    a = kernels.AttnArgs(q=dq.ptr, k=dk.ptr, v=dv.ptr, out=do.ptr, ldq=D, ldk=D, ldv=D, ldo=D, bsq=Tq * D, bsk=Tk * D, bsv=Tk * D, bso=Tq * D,
                         n_batch=nb, n_head=heads, d_head=d, Tq=Tq, Tk=Tk, causal=0)
    try:
        L.mlsd_attention_sp(sw["sp"]); L.mlsd_attention_x2_min_tq(sw["x2"]); L.mlsd_attention_tk96(sw["tk96"], 0)
        if "pp" in sw:
            L.mlsd_attention_pp(sw["pp"])
        _lib.check(L.mlsd_memset(_lib.vp(do.ptr), 0x7C, ctypes.c_size_t(do.nbytes), None))
        kernels.attention(a)
        got = do.download((nb, Tq, D), np.float16).astype(np.float64)
    finally:
        L.mlsd_attention_sp(1); L.mlsd_attention_x2_min_tq(2048); L.mlsd_attention_tk96(1, 0)
        if "pp" in sw:
            L.mlsd_attention_pp(0)
    attn_check(name, sigma, voff, q, k, v, heads, got, q_scaled)


@pytest.mark.parametrize("sigma,voff", [(s, 0.0) for s in SIGMAS] + [(4, 100.0)])
def test_attention_fused_into_the_q_projection(K, sigma, voff):
    """The cross attention at the end of its q projection (mlsd_gemm_xattn_fused): W = sigma I, so q = sigma x exactly (fp16), 77 keys."""
    kernels, _lib = K
    L, vp = _lib.lib(), _lib.vp
    nb, tq, heads, tk = 2, 256, 5, 77
    D = heads * 64
    M = nb * tq
    rng = np.random.default_rng(sigma + 31 * int(voff))
    ops = [attn_operands(rng, heads, 64, tq, tk, 1.0, voff) for _ in range(nb)]
    x = np.concatenate([o[0] for o in ops])
    kmat, vmat = np.concatenate([o[1] for o in ops]), np.concatenate([o[2] for o in ops])
    q = f16r(x * sigma)
    ldkv = 2 * D
    kv = np.concatenate([kmat, vmat], axis=1)
    dX, dW, dKV = dev(_lib, x.astype(np.float16)), dev(_lib, (np.eye(D) * sigma).astype(np.float16)), dev(_lib, kv.astype(np.float16))
    dVT = _lib.DeviceBuffer(nb * D * 96 * 2)
    _lib.check(L.mlsd_xattn_pack_vt(vp(dKV.ptr + 2 * D), ldkv, nb, tk, D, vp(dVT.ptr), None), "pack")
    dO = _lib.DeviceBuffer(M * D * 2)
    _lib.check(L.mlsd_memset(vp(dO.ptr), 0x7C, ctypes.c_size_t(dO.nbytes), None))
    try:
        L.mlsd_gemm_set_xattn(2)
        a = kernels.GemmArgs(A=dX.ptr, lda=D, conv=0, W_=dW.ptr, ldb=D, M=M, N=D, K=D, xa_k=dKV.ptr, xa_ldk=ldkv, xa_vt=dVT.ptr, xa_out=dO.ptr, xa_ldo=D, xa_Tq=tq, xa_Tk=tk)
        assert L.mlsd_gemm_xattn_fused(ctypes.byref(a)) == 1
        kernels.gemm(a)
    finally:
        L.mlsd_gemm_set_xattn(-1)
    got = dO.download((nb, tq, D), np.float16).astype(np.float64)
    attn_check("xattn_fused", sigma, voff, q.reshape(nb, tq, D), kmat.reshape(nb, tk, D), vmat.reshape(nb, tk, D), heads, got, False)


@pytest.mark.parametrize("cols", [77, 4096, 16384])
def test_softmax_rows(K, cols):
    """mlsd_softmax_rows (the VAE mid block's materialised scores): rows at score scales 1 .. 16 (in units of the scale), a peaked row, an all-equal row,
    a row whose second half is 1e4 below its maximum; per row against float64 within half an fp16 ulp plus 4 u32 of the row's largest p."""
    kernels, _lib = K
    L = _lib.lib()
    rng = np.random.default_rng(cols)
    rows, scale = 8, 0.125
    s = rng.standard_normal((rows, cols)) * (np.array([1, 4, 8, 16, 4, 1, 1, 8])[:, None] / scale)
    s[4, 3] += 20 / scale
    s[5] = 2.5
    s[6, cols // 2:] -= 1e4
    s = s.astype(np.float32)
    ds, dp = dev(_lib, s), _lib.DeviceBuffer(rows * cols * 2)
    L.mlsd_softmax_rows.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p]
    _lib.check(L.mlsd_softmax_rows(ds.ptr, cols, dp.ptr, cols, rows, cols, scale, None), "softmax")
    got = dp.download((rows, cols), np.float16).astype(np.float64)
    want = R.softmax64(s, scale)
    ratio = (np.abs(got - want) / (R.half_ulp16(want) + 4 * R.U32 * want.max(1, keepdims=True))).max(1)
    print(f"\n[conditioning] softmax_rows {cols} cols: worst row ratio {ratio.max():.3f}")
    assert np.all(ratio <= 1.0), ratio
