"""The far-offset cases without a GPU (tests/far_offsets.py).

  * the census: every (op form, operand, class) of the 2048x2048 plans whose range ends at or beyond 2^31 / 2^32 bytes has a case in FAR_CASES, every entry names a
    form that exists, an entry taken out is reported by name; the 64-image decode (the largest batch the API admits) is in the
    census: each of its forms has a case at a smaller M or is named in BEYOND_ARENA with the bytes it needs;
  * the routes keep the kernels with 32-bit offsets out of reach: attention with 2^30 elements of keys or values, in-launch split-K, the stream-K workspace;
  * every case at the real boundary has the class it is listed for, obeys the arena rule and takes at most 16 GiB;
  * the analytic GroupNorm statistics of a tiled map agree with tests/ref64.py's brute force, and conv_A with R.im2col64;
  * sample_rows covers both sides of every boundary of every far operand;
  * the host model of every case at boundary 2^20: a correct kernel passes the sampled check with nothing unwritten; a kernel whose byte or element offset into a
    far operand is kept in 32 bits (zero- or sign-extended) on a load or on a store, or whose buffer resource ends at the boundary, fails the sampled check or the
    written-everywhere count -- wherever the fault alters an access at all (an operand of exactly 2^31 bytes has no offset that 32 bits cannot hold; only the
    exhausted resource drops its last row).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import far_offsets as FO
import plan_audit as PA
import ref64 as R

E_MODEL = 20
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlimgsynth_amd", "csrc", "host")


@pytest.fixture(scope="module")
def census():
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    try:
        yield FO.far_forms(engine)
    finally:
        L.mlsd_runtime_dry(0)


def test_the_batch_limit_is_the_sources():
    api, eng = open(os.path.join(CSRC, "mlis_api.c")).read(), open(os.path.join(CSRC, "engine.c")).read()
    assert int(re.search(r"#define MAX_IMAGES (\d+)", api).group(1)) == FO.MAX_IMAGES
    assert int(re.search(r"#define MAX_BATCH (\d+)", eng).group(1)) == FO.MAX_IMAGES


def test_every_far_form_has_a_case_and_every_case_a_form(census):
    forms, refused = census
    assert forms, "no far form found: the census plans did not build"
    missing = FO.unheld_far_forms(forms)
    assert not missing, "far forms without a GPU case: " + "; ".join(f"{k} in {', '.join(p)}" for k, p in missing.items())
    found = {(key, name, cls) for key, where in forms.items() for _, name, cls in where}
    stale = sorted(set(FO.FAR_CASES) - found, key=str)      # (the 64-image plan's entries need not occur: its tiles depend on the host, see FO.FAR_PLANS)
    assert not stale, f"FAR_CASES entries that no plan has: {stale}"
    assert set(FO.ALL_FAR_CASES.values()) | set(FO.STRIDED_ONLY) == set(FO.BUILDERS) and not set(FO.ALL_FAR_CASES.values()) & set(FO.STRIDED_ONLY)
    assert not set(FO.BEYOND_ARENA) & set(FO.ALL_FAR_CASES)
    for k, (why, need) in FO.BEYOND_ARENA.items():      # a form is named as beyond an arena only with the bytes that say so
        assert why and (2 << 30) + (64 << 10) + sum(need) > FO.ARENA_MAX, k
    print(f"\n[far census] {len(found)} (form, operand, class) over {len(forms)} op forms; refused: {refused}")
    for pid, text in refused.items():
        assert pid in FO.REFUSALS and re.search(FO.REFUSALS[pid], text), (pid, text)


def test_an_entry_taken_out_is_reported_by_name(census):
    forms, _ = census
    held = {**FO.ALL_FAR_CASES, **FO.BEYOND_ARENA}
    for k in FO.FAR_CASES:
        gone = FO.unheld_far_forms(forms, {q: v for q, v in held.items() if q != k})
        assert list(gone) == [k] and gone[k], (k, gone)


RANK = {None: 0, "far": 1, "very far": 2}


@pytest.mark.parametrize("cid", FO.ALL_IDS)
def test_the_case_is_what_it_is_listed_for(cid):
    c = FO.build_case(cid)
    cls = FO.case_classes(c)
    for (key, name, want) in c.forms:
        assert RANK[cls.get(name)] >= RANK[want], (cid, name, cls.get(name), want)
        assert key[0] == c.op
        if c.op == "gemm":
            assert key[1][0] == c.kw["tile"]
            assert ("colstats" in key[2]) == ("colstats" in c.ops) and ("residual" in key[2]) == ("resid" in c.ops) and ("C16 + C32" in key[2]) == ("C16" in c.ops)
    # the arena rule
    assert c.arena <= FO.ARENA_MAX, (cid, c.arena)
    for o in c.ops.values():
        assert o.off + o.extent <= c.arena
        if cls.get(o.name):
            assert o.far and o.off >= (2 << 30) + (64 << 10) and o.off + -(-o.extent // 2 ** 32) * 2 ** 32 <= c.arena, (cid, o.name)
    spans = sorted((o.off, o.off + o.extent) for o in c.ops.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (cid, spans)
    print(f"\n[far case] {cid}: arena {c.arena / 2 ** 30:.2f} GiB, " + ", ".join(f"{n} {k}" for n, k in cls.items()))


def test_analytic_group_statistics_agree_with_brute_force():
    c = FO.build_case("gn_c256_4g", E_MODEL)
    o = c.ops["x1"]
    x = c.value("x1", np.arange(o.rows))[None]
    assert len({float(c.block("x1", s).mean()) for s in range(3)}) == 3
    g, be = c.ops["gamma"].data[0], c.ops["beta"].data[0]
    want = R.groupnorm64(x, None, 32, c.kw["eps"], g, be, True)[0]
    y, tol = FO.gn_reference(c, x[0])
    assert np.abs(y - want).max() <= 1e-12 * np.abs(want).max()
    eb, _ = R.groupnorm_bound(x, 32, c.kw["eps"], g, be)
    brute = R.half_ulp16(want) + np.repeat(eb[0], o.cols // 32)[None, :]
    assert np.allclose(tol, brute, rtol=1e-9, atol=0)
    got = want.astype(np.float16)      # and the two ratios are the same number
    assert abs(PA._worst(FO.ratio(got, y, tol, "abs")) - PA._worst(R.groupnorm_worst(got[None], want[None], x, 32, c.kw["eps"], g, be)[0])) < 1e-6


def test_conv_rows_agree_with_im2col():
    c = FO.build_case("g4_conv_stats_farA", E_MODEL)
    kw = c.kw
    x = c.value("A", np.arange(kw["M"]))
    rows = FO.sample_rows(c)
    want = R.im2col64(x, 1, kw["H"], kw["W"], 8, kw["k"], kw["k"], 1, kw["pad"], 0, kw["H"], kw["W"], rows=rows)
    assert np.array_equal(FO.conv_A(c, rows, c.value), want)


@pytest.mark.parametrize("e", [E_MODEL, FO.E_REAL])
@pytest.mark.parametrize("cid", FO.ALL_IDS)
def test_sample_rows_cover_the_boundaries(cid, e):
    c = FO.build_case(cid, e)
    rows = set(FO.sample_rows(c).tolist())
    M = FO.out_rows(c)
    assert {0, M - 1} <= rows and len(rows) >= min(M, 200)
    if M <= 1024:      # the strided cases recompute every output row (their far operand's rows need not be output rows: keys, pixels of a transposed map)
        assert len(rows) == M
        return
    for o in c.far_operands():
        for B in (c.b31, c.b32):
            if o.extent <= B:
                continue
            start = np.arange(o.rows, dtype=np.int64) * o.stride
            below, beyond = np.nonzero(start + o.row_bytes <= B)[0], np.nonzero(start + o.row_bytes > B)[0]
            assert below.size and below[-1] in rows and below[-1] - 1 in rows, (cid, o.name, B)
            assert beyond.size and beyond[0] in rows and (beyond[0] + 1 in rows or beyond[0] == M - 1), (cid, o.name, B)
            t = c.tile_m
            assert beyond[0] // t * t in rows and min(beyond[0] // t * t + t - 1, M - 1) in rows


def _run_model(cid, fault):
    c = FO.build_case(cid, E_MODEL)
    mem = FO.HostMemory(c.arena)
    FO.fill(c, mem)
    FO.model_run(c, mem, fault)
    return FO.check(c, mem), FO.unwritten(c, mem)


@pytest.mark.parametrize("cid", FO.ALL_IDS)
def test_the_model_of_a_correct_kernel_passes(cid):
    worst, holes = _run_model(cid, None)
    assert worst and all(r <= 1.0 for r in worst.values()), worst
    assert all(n == 0 for n in holes.values()), holes


@pytest.mark.parametrize("cid", FO.ALL_IDS)
def test_every_seeded_fault_is_caught(cid):
    c = FO.build_case(cid, E_MODEL)
    tried = 0
    for o in c.far_operands():
        for where, mode in FO.FAULTS:
            if (where == "store") != (o.role == "out") or not FO.fault_changes(c, o.name, mode):
                continue
            worst, holes = _run_model(cid, (o.name, where, mode))
            tried += 1
            assert any(not r <= 1.0 for r in worst.values()) or any(holes.values()), f"{cid}: {where} of {o.name} with {mode} offsets goes unnoticed: {worst} {holes}"
    # every far operand has at least the exhausted resource; every very far one also a truncation that bites
    # (an A operand whose channels were cut to 8 of 256 ends 496 bytes short of the boundary: its launch cannot touch the bytes an exhausted resource would drop)
    for o in c.far_operands():
        touched = (o.rows - 1) * o.stride + o.row_bytes
        if touched > c.b32:
            assert FO.fault_changes(c, o.name, "zext") and FO.fault_changes(c, o.name, "sext")
        if touched > c.b31:
            assert FO.fault_changes(c, o.name, "sext")
        if touched >= c.b31:
            assert FO.fault_changes(c, o.name, "records")
    assert tried >= sum(1 for o in c.far_operands() if (o.rows - 1) * o.stride + o.row_bytes >= c.b31), (cid, tried)


def test_count_nonfinite_words_see_an_unwritten_pair_of_halves():
    h = np.array([1.0, -2.0, 65504.0, 6e-8, 0.0, -0.0], np.float16)
    pairs = np.array([[a, b] for a in h for b in h], np.float16)
    assert np.isfinite(pairs.view(np.float32)).all()
    assert not np.isfinite(np.full(4, 0xFF, np.uint8).view(np.float32)).any()
    one = np.array([1.0, 0], np.float16)
    one.view(np.uint16)[1] = 0xFFFF      # one half written, its neighbour not
    assert not np.isfinite(one.view(np.float32)).any()


# ------------------------------------------------------------------ the guards that keep 32-bit offsets out of reach (the launchers' routes, no launch)
def _has_experiments():
    from mlimgsynth_amd import _lib
    return bool(_lib.lib().mlsd_has_experiments())


needs_experiments = pytest.mark.skipif(not _has_experiments(), reason="variant not in the product build (make EXPERIMENTS=1)")
P = 0x10000      # an aligned non-NULL address: the routes are resolved, nothing is launched


def _attn(Tq, Tk, ldk, ldv, heads=16):
    from mlimgsynth_amd import kernels
    return kernels.AttnArgs(q=P, k=P, v=P, out=P, ldq=64 * heads, ldk=ldk, ldv=ldv, ldo=64 * heads, bsq=0, bsk=0, bsv=0, bso=0, n_batch=1, n_head=heads, d_head=64,
                            Tq=Tq, Tk=Tk, causal=0)


@pytest.mark.parametrize("far", ["ldk", "ldv"])
def test_keys_or_values_of_2_30_elements_leave_the_software_pipelined_kernel(far):
    """attn64x2s_kernel and the ping-pong kernel address K and V with 32-bit byte offsets into one buffer resource (attention.hip: num_records is an int): the route
    must take a launch away from them as soon as Tk x ldk or Tk x ldv reaches 2^30 elements (2^31 bytes)"""
    from mlimgsynth_amd import kernels
    Tq, Tk = 2048, 1024
    near = (1 << 30) // Tk - 8
    assert kernels.attention_variant(_attn(Tq, Tk, near, near)).startswith("attn<64x2s")
    ld = dict(ldk=near, ldv=near)
    ld[far] = (1 << 30) // Tk
    lab = kernels.attention_variant(_attn(Tq, Tk, **ld))
    assert lab and not lab.startswith("attn<64x2s") and not lab.startswith("attn<pp"), lab


@needs_experiments
@pytest.mark.parametrize("far", ["ldk", "ldv"])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_keys_or_values_of_2_30_elements_leave_the_ping_pong_kernel(far, mode):
    from mlimgsynth_amd import _lib, kernels
    L = _lib.lib()
    Tq, Tk = 2048, 1024
    near = (1 << 30) // Tk - 8
    ld = dict(ldk=near, ldv=near)
    try:
        L.mlsd_attention_pp(mode)
        assert kernels.attention_variant(_attn(Tq, Tk, near, near)).startswith("attn<pp")
        ld[far] = (1 << 30) // Tk
        lab = kernels.attention_variant(_attn(Tq, Tk, **ld))
        assert lab and not lab.startswith("attn<pp") and not lab.startswith("attn<64x2s"), lab
    finally:
        L.mlsd_attention_pp(0)


def _splitk_args(M, N, K, ksplit):
    from mlimgsynth_amd import kernels
    return kernels.GemmArgs(A=P, lda=K, W_=P, ldb=K, M=M, N=N, K=K, C32=P, ldc32=N, ksplit=ksplit, tile_variant=kernels.tile_arg(0), ws=P, ws_bytes=1 << 40, sk_flags=P)


SPLITK_SHAPES = [(128, 128, 1024, 4), (300, 200, 4096, 8), (8192, 1280, 5120, 6), (65536, 8192, 1024, 2), (1 << 20, 512, 256, 2), (262016, 128, 2048, 3)]


def test_the_product_build_never_adds_split_k_slices_in_the_launch():
    """the in-launch split-K store and merge (gemm_conv.hip, PAR) keep byte offsets into the workspace in 32 bits: the product build has no such route at all"""
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    if _has_experiments():
        pytest.skip("the EXPERIMENTS build has the route: the test below bounds its workspace")
    try:
        L.mlsd_gemm_set_splitk_parallel(1)
        assert all(L.mlsd_gemm_splitk_parallel(ctypes.byref(_splitk_args(*s))) == 0 for s in SPLITK_SHAPES)
    finally:
        L.mlsd_gemm_set_splitk_parallel(0)


def test_the_stream_k_workspace_stays_below_2_gib():
    """stream-K's gather reads its contributors' slabs through one buffer resource with 32-bit slab offsets (gemm_pp.hpp): one slab per persistent block, the
    whole workspace far below 2^31 bytes"""
    from mlimgsynth_amd import _lib
    f = _lib.lib().mlsd_gemm_streamk_ws_bytes
    f.restype = ctypes.c_size_t
    assert 0 < f() < 1 << 31


def test_phase_rows_agree_with_phase_A():
    """the reference of the phase case: its rows are R.phase_A's rows of the launch's parity, times that launch's weight, plus the bias"""
    c = FO.build_case("p17_phase_4g", E_MODEL)
    kw = c.kw
    H, W, N = kw["H"], kw["W"], kw["N"]
    x = c.value("A", np.arange(kw["M"])).reshape(1, H, W, kw["cin"])
    rows = np.arange(4 * kw["M"])
    y = FO.reference(c, rows)["C32"][0].reshape(2 * H, 2 * W, N)
    for q in range(4):
        py, px = q >> 1, q & 1
        want = R.phase_A(x, py, px, 0) @ c.ops[f"W{q + 1}"].data.astype(np.float64).T + c.ops["bias"].data[0].astype(np.float64)
        assert np.allclose(y[py::2, px::2].reshape(-1, N), want, rtol=1e-12, atol=1e-12), q
    assert set(FO.sample_rows(c).tolist()) >= {0, 4 * kw["M"] - 1}
