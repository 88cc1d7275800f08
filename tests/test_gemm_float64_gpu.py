"""Every product GEMM / implicit-GEMM convolution path against a float64 reference, per output element (tests/ref64.py: bounds and their
derivation; tests/gemm64_cases.py: the cases and their input families).

Each case asserts the tile label mlsd_gemm_variant gives it, then max(|got - ref64| / bound) <= 1 for C32 and C16 element by element, and
C16 == fp16_rne(C32) bit for bit where a launch writes both.  Launches of up to 2^30 multiply-adds are compared everywhere; larger ones on
complete tiles: every tile of the first and last row block and of the last column block, and four seeded row blocks.  With -s the worst
ratio of every case and, at the end, of every path is printed (convolutions also report their border ring on its own).

The census at the end builds the bench plans (without computing them) and checks that every GEMM path they choose has a case here.
"""
import ctypes
import zlib

import numpy as np
import pytest

import gemm64_cases as GC
import plan_audit as PA
import ref64 as R

pytestmark = pytest.mark.gpu

FULL_MACS = 2 ** 30
WORST = {}       # path -> (worst C32 ratio, worst C16 ratio, worst border ratio)


def _has_experiments():
    try:
        from mlimgsynth_amd import _lib
        return bool(_lib.lib().mlsd_has_experiments())
    except Exception:
        return False


HAS_EXP = _has_experiments()


@pytest.fixture(scope="module")
def K():
    from mlimgsynth_amd import kernels, _lib
    yield kernels, _lib
    if WORST:
        print("\nfloat64 GEMM bound, worst ratio per path (C32 / C16 / conv border ring):")
        for p, (a, b, c) in sorted(WORST.items()):
            print(f"  {p:24s} C32 {a:7.3f}   C16 {b:7.3f}   border {c:7.3f}")


def _k_step(c):
    return PA.gemm_path(c["variant"])[2]      # (one parser of the launch labels for these tests and the plan audit: tests/plan_audit.py)


def _nsplit(label):
    return PA.gemm_path(label)[3]


def _rows_to_check(c):
    M, N, K = c["M"], c["N"], c["K"]
    if M * N * K <= FULL_MACS:
        return np.arange(M), None
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    blocks = {0, (M - 1) // 256} | set(rng.integers(0, -(-M // 256), 4).tolist())
    rows = np.concatenate([np.arange(b * 256, min(M, b * 256 + 256)) for b in sorted(blocks)])
    return rows, np.arange(max(0, c["nout"] - 256), c["nout"])      # (+ every row of the last column block)


def _reference(c, ops, rows, cols, D):
    """y64, bound32 on [rows][cols]"""
    if c["conv"]:
        A = R.im2col64(ops["A"], c["n"], c["H"], c["W"], c["cin_pad"], c["k"], c["k"], c["s"], c["p"], c["ups"], c["OH"], c["OW"], rows=rows)
    else:
        A = ops["A"][rows]
    Wt = ops["W"] if c["act"] == 5 or cols is None else ops["W"][cols]
    acc, S = R.gemm64(A, Wt)
    cols_ = np.arange(c["nout"]) if cols is None else cols
    return R.gemm_epilogue64(acc, S, D, rows, cols_, bias=ops.get("bias"), rowbias=ops.get("rowbias"), rows_per_batch=c["rowbias"] or 1,
                             bias_m=ops.get("bias_m"), act=c["act"], resid=ops.get("resid"), act_after_resid=c["post"])


def _args(kernels, _lib, c, dev, keep):
    M, N, K, nout = c["M"], c["N"], c["K"], c["nout"]
    d = lambda a: keep.append(_lib.from_numpy(np.ascontiguousarray(a))) or keep[-1].ptr
    a = kernels.GemmArgs(A=dev["A"], lda=c["cin_pad"] if c["conv"] else K, W_=dev["W"], ldb=K, M=M, N=N, K=K, act=c["act"],
                         act_after_resid=int(c["post"]), tile_variant=c["tv"], ksplit=c["ksplit"])
    if c["conv"]:
        a.conv, a.n_img, a.H, a.W, a.Cin, a.OH, a.OW = 1, c["n"], c["H"], c["W"], c["cin_pad"], c["OH"], c["OW"]
        a.KH = a.KW = c["k"]
        a.stride, a.pad, a.upsample = c["s"], c["p"], c["ups"]
    for f in ("bias", "bias_m"):
        if f in dev:
            setattr(a, f, dev[f])
    if "rowbias" in dev:
        a.rowbias, a.rows_per_batch, a.ldrb = dev["rowbias"], c["rowbias"], N
    if "resid" in dev:
        a.resid, a.ldr = dev["resid"], nout
    if c["ws"] or c["sk"]:
        L = _lib.lib()
        L.mlsd_gemm_streamk_ws_bytes.restype = ctypes.c_size_t
        nb = max(kernels.gemm_splitk_ws_bytes(M, N, max(c["ksplit"], 2)), L.mlsd_gemm_streamk_ws_bytes() if c["sk"] else 0)
        a.ws, a.ws_bytes = d(np.zeros(nb // 4, np.float32)), nb
    if c["sk"]:
        a.sk_flags = d(np.zeros(4096, np.uint32))
    if c["stats"]:
        a.colstats, a.colstats_shift = d(np.zeros(2 * N * (M // 32 + 2), np.float32)), 1
        keep.append(("colstats", keep[-1]))
    if c["ln"]:
        a.ln_y16, a.ldln = d(np.zeros((M, N), np.float16)), N
        keep.append(("ln_y16", keep[-1]))
        a.ln_gamma, a.ln_beta, a.ln_eps = d(np.ones(N, np.float32)), d(np.zeros(N, np.float32)), 1e-5
        a.ln_ws, a.ln_cnt, a.ln_slot = d(np.zeros(M * (N // 128 + 1) * 4, np.float32)), d(np.zeros(8192, np.uint32)), 0
    return a


@pytest.mark.parametrize("case", GC.CASES, ids=[c["id"] for c in GC.CASES])
def test_gemm_float64(K, case):
    kernels, _lib = K
    c = case
    if c["exp"] and not HAS_EXP:
        pytest.skip("variant not in the product build (make EXPERIMENTS=1)")
    ops = GC.make_operands(c)
    keep = []
    dev = {k: (keep.append(_lib.from_numpy(np.ascontiguousarray(v))) or keep[-1].ptr) for k, v in ops.items()}
    M, nout = c["M"], c["nout"]
    C32 = _lib.DeviceBuffer(M * nout * 4) if c["c32"] else None
    C16 = _lib.DeviceBuffer(M * nout * 2) if c["c16"] else None
    a = _args(kernels, _lib, c, dev, keep)
    if C32:
        a.C32, a.ldc32 = C32.ptr, nout
    if C16:
        a.C16, a.ldc16 = C16.ptr, nout
    label = kernels.gemm_variant(a)
    assert label == c["variant"], f"{c['id']}: launch label {label}, case written for {c['variant']}"
    kernels.gemm(a)
    kernels.sync()
    got32 = C32.download((M, nout), np.float32) if C32 else None
    got16 = C16.download((M, nout), np.float16) if C16 else None
    if got32 is not None and got16 is not None:
        same = R.fp16_rne(got32).view(np.uint16) == got16.view(np.uint16)
        assert same.all(), f"{c['id']}: C16 != fp16_rne(C32) at {np.argwhere(~same)[:4].tolist()}"
    side = dict(k for k in keep if isinstance(k, tuple))
    wst = wln = 0.0
    if c["stats"]:      # the column statistics the launch wrote beside C32: the launch must be one that writes them, and they must describe the stored output
        rows_st = kernels.gemm_route(a).stats_rows
        assert rows_st > 0 and M % rows_st == 0 and got32 is not None, f"{c['id']} ({label}): the launch writes no column statistics (rows {rows_st})"
        st = side["colstats"].download((M // rows_st, 2, c["N"]), np.float32)
        es, eq = R.colstats_ratios(got32, st, rows_st, shifted=True)
        wst = max(float(es.max()), float(eq.max()))
        assert wst <= 1.0, f"{c['id']} ({label}): column statistics ratio {wst:.3g} > 1 (blocks of {rows_st} rows)"
    if c["ln"]:         # the LayerNorm ending (gamma 1, beta 0, eps 1e-5 in _args) of the stored fp32 rows
        assert kernels.gemm_route(a).ln > 0 and got32 is not None, f"{c['id']} ({label}): the launch does not end with its LayerNorm"
        g, be = np.ones(c["N"]), np.zeros(c["N"])
        ratio, _ = R.layernorm_worst(side["ln_y16"].download((M, c["N"]), np.float16), R.layernorm64(got32, 1e-5, g, be), got32, 1e-5, g, be)
        wln = float(ratio.max())
        assert wln <= 1.0, f"{c['id']} ({label}): LayerNorm ending ratio {wln:.3g} > 1 at row {int(np.argmax(ratio))}"
    D = R.gemm_depth(c["K"], _k_step(c), _nsplit(label) + (c["K"] // 64 if c["sk"] else 0))
    rows, lastcols = _rows_to_check(c)
    parts = [(rows, None)] + ([] if lastcols is None else [(np.arange(M), lastcols)])
    w32 = w16 = wb = 0.0
    for rr, cc in parts:
        y, b = _reference(c, ops, rr, cc, D)
        sel = (lambda g: g[rr] if cc is None else g[rr][:, cc])
        ratios = []
        if got32 is not None:
            r32 = R.gemm_ratio32(sel(got32), y, b)
            w32 = max(w32, float(r32.max()))
            ratios.append(r32)
        if got16 is not None:
            r16 = R.gemm_ratio16(sel(got16), y, b)
            w16 = max(w16, float(r16.max()))
            ratios.append(r16)
        if c["conv"]:
            oy, ox = (rr // c["OW"]) % c["OH"], rr % c["OW"]
            ring = (oy == 0) | (oy == c["OH"] - 1) | (ox == 0) | (ox == c["OW"] - 1)
            if ring.any():
                wb = max(wb, max(float(r[ring].max()) for r in ratios))
        for r in ratios:
            if not (r <= 1.0).all():
                i = np.unravel_index(int(np.argmax(np.nan_to_num(r, nan=1e300, posinf=1e300))), r.shape)
                m_, n_ = int(rr[i[0]]), int(i[1] if cc is None else cc[i[1]])
                pytest.fail(f"{c['id']} ({label}): ratio {r[i]:.3g} > 1 at row {m_} col {n_}: ref {y[i]:.9g} bound {b[i]:.3g}")
    p = WORST.setdefault(c["path"], [0.0, 0.0, 0.0])
    p[0], p[1], p[2] = max(p[0], w32), max(p[1], w16), max(p[2], wb)
    print(f"{c['id']:22s} {label:36s} worst C32 {w32:7.3f}  C16 {w16:7.3f}  border {wb:7.3f}" + (f"  colstats {wst:7.3f}" if c["stats"] else "") +
          (f"  ln_y16 {wln:7.3f}" if c["ln"] else ""))


# ------------------------------------------------------------------ census
MLB_F_OPSHAPES = 16
COVERED_ELSEWHERE = {"linear+attention": "test_conditioning_gpu.py (the q projection's only output is the fused attention's)"}


def path_key(label):
    """(tile, form) of a plan label: form is '', 'splitk' or 'layernorm' ('linear+attention' is tested with the attention kernels)"""
    return PA.gemm_path(label)[:2]


def case_keys():
    return {path_key(c["variant"]) for c in GC.CASES if not c["exp"]}


def plan_labels():
    from mlimgsynth_amd import engine
    out = set()
    for model, lat, n, dn in (("sd1", 64, 2, 1), ("sdxl", 128, 8, 4)):
        un = engine.Unet(model, lat, lat, n, synth=False, flags=MLB_F_OPSHAPES)
        out |= {(model + " unet", lab.split(" ")[0]) for lab, _ in un.ctx.op_list() if lab.startswith("gemm<")}
        un.ctx.destroy()
        l = engine._proto2()
        ctx, t_lat, P = engine.MLCtx(flags=MLB_F_OPSHAPES), engine.vp(), engine.VaeParams()
        assert l.vae_params_get(model.encode(), ctypes.byref(P)) == 1
        assert l.sdvae_decode_init(ctx.h, ctypes.byref(P), lat, lat, dn, ctypes.byref(t_lat)) == 1
        assert l.sdvae_decode_build(ctx.h, ctypes.byref(P), t_lat) == 1
        out |= {(model + " vae", lab.split(" ")[0]) for lab, _ in ctx.op_list() if lab.startswith("gemm<")}
        ctx.destroy()
    return out


def test_every_planned_gemm_path_has_a_float64_case(K):
    """SD1.5 64x64 (N = 2) and SDXL 128x128 batch 4 (N = 8) UNet plans and their KL-VAE decoders, as bench.py runs them: every (tile, form)
    they choose needs a case in gemm64_cases.py.  Built on the device (stream-K and in-launch LayerNorm eligibility ask it for its CUs), not
    computed."""
    have = case_keys()
    seen = plan_labels()
    missing = sorted({(w, lab) for w, lab in seen if path_key(lab) not in have and path_key(lab)[1] not in COVERED_ELSEWHERE})
    print("\nplanned GEMM paths:", sorted({path_key(lab) for _, lab in seen}))
    assert not missing, f"GEMM paths the plans use without a float64 case: {missing}"
