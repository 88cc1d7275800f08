"""HyperTile without a GPU: the tile rule against its Python restatement, the options, the configuration word, dry UNet plans with and without the setting
(op records field for field), the plan audit's dataflow checks on tiled plans, what the permutation kernel refuses, and the torch reference's own properties.

The engine-key behaviour of the two options (a change builds one more engine and keeps the other resident) needs generations, and the window plans of
tiled-diffusion engines need a launch when they are built: test_what_cannot_be_built_without_a_device shows both, tests/test_hypertile_gpu.py holds them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import controlnet_ffi as CF
import hypertile_ref as HR
import mlis_ffi as F
import plan_audit as PA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPERTILE, HYPERTILE_DEPTH = 191, 192
PI = C.POINTER(C.c_int)


def bind(path):
    lib = CF.bind(path)
    lib.mlis_amd_hypertile_side.restype, lib.mlis_amd_hypertile_side.argtypes = F.ci, [F.ci, F.ci, F.ci]
    lib.mlis_amd_hypertile_info.restype, lib.mlis_amd_hypertile_info.argtypes = F.ci, [F.vp, PI, PI, PI]
    lib.mlsd_tile_permute.restype, lib.mlsd_tile_permute.argtypes = F.ci, [F.vp, F.vp, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.ci, F.vp]
    return lib


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return bind(_lib.LIB_PATH)


@pytest.fixture()
def dry(lib):
    lib.mlsd_runtime_dry(1)
    yield lib
    lib.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ the rule
def test_rule_equals_its_restatement(lib):
    for ppt in (8, 16, 32, 64):
        for tile in (32, 64, 96, 256, 512, 1000):
            for side in range(1, 261):
                got = lib.mlis_amd_hypertile_side(side, ppt, tile)
                m = min(max(tile // ppt, 4), side)
                assert got == HR.side(side, ppt, tile), (side, ppt, tile, got)
                assert side % got == 0 and got >= m and not [d for d in range(m, got) if side % d == 0]
    # the cases of the issue's table: SDXL 1024 px with tile 512 -> 64 of 128 tokens, 32 of 64; a tile of at least the picture -> one tile; the floor of 4 tokens
    assert [lib.mlis_amd_hypertile_side(s, p, 512) for s, p in ((128, 8), (64, 16), (32, 32))] == [64, 32, 16]
    assert lib.mlis_amd_hypertile_side(16, 8, 128) == 16 and lib.mlis_amd_hypertile_side(16, 32, 32) == 4 and lib.mlis_amd_hypertile_side(7, 8, 32) == 7
    assert lib.mlis_amd_hypertile_side(12, 8, 40) == 6 and lib.mlis_amd_hypertile_side(20, 8, 96) == 20     # 5 is no divisor of 12; 12 .. 19 are none of 20


def test_reference_permutation_is_the_stated_map():
    for n, H, W, th, tw in ((1, 2, 2, 1, 1), (3, 4, 6, 2, 3), (2, 6, 10, 6, 5), (1, 1, 8, 1, 4)):
        nh, nw = H // th, W // tw
        src = np.arange(n * H * W)
        fwd = HR.permute_rows(src, n, H, W, th, tw)
        for img in range(n):
            for ty in range(nh):
                for tx in range(nw):
                    for y in range(th):
                        for x in range(tw):
                            assert fwd[((img * nh + ty) * nw + tx) * th * tw + y * tw + x] == img * H * W + (ty * th + y) * W + tx * tw + x
        assert np.array_equal(HR.permute_rows(fwd, n, H, W, th, tw, inverse=True), src)


# ------------------------------------------------------------------ options, symbols, wrapper, CLI
def test_options_defaults_ranges_and_round_trip(lib):
    for oid, name in ((HYPERTILE, "hypertile"), (HYPERTILE_DEPTH, "hypertile_depth")):
        assert lib.mlis_option_str(oid).decode() == name and lib.mlis_option_fromz(name.encode()) == oid
        assert lib.mlis_option_fromz(name.replace("_", "-").encode()) == oid
    assert lib.mlis_option_str(190) == b"???" and lib.mlis_option_str(193) == b"???"
    m = F.Mlis(lib)
    try:
        i = C.c_int(-1)
        get = lambda oid: (lib.mlis_option_get(m.ctx, oid, C.byref(i)), i.value)
        assert get(HYPERTILE) == (1, 0) and get(HYPERTILE_DEPTH) == (1, 3)
        for v in (32, 64, 512, 1000, 8192, 0):
            m.set("hypertile", v)
            assert get(HYPERTILE) == (1, v)
        assert lib.mlis_option_set(m.ctx, HYPERTILE, 256) == 1 and get(HYPERTILE) == (1, 256)
        for bad in (20, 36, 8, 24, -8, 8200, 16384):            # 20: below the range; 36: not a multiple of 8
            assert lib.mlis_option_set(m.ctx, HYPERTILE, bad) == -4, bad
            assert lib.mlis_option_set_str(m.ctx, b"hypertile", str(bad).encode()) == -4, bad
        assert lib.mlis_option_set_str(m.ctx, b"hypertile", b"64x") == -4
        assert get(HYPERTILE) == (1, 256)                        # a refused value changes nothing
        for v in (0, 1, 2, 3):
            m.set("hypertile_depth", v)
            assert get(HYPERTILE_DEPTH) == (1, v)
        for bad in (-1, 4):
            assert lib.mlis_option_set(m.ctx, HYPERTILE_DEPTH, bad) == -4
        assert get(HYPERTILE_DEPTH) == (1, 3)
    finally:
        m.close()


def test_symbols_wrapper_and_cli(lib):
    for name in ("mlsd_tile_permute", "mlis_amd_hypertile_side", "mlis_amd_hypertile_info", "mlctx_set_hypertile", "mlctx_hypertile_info"):
        assert hasattr(lib, name), name
    from mlimgsynth_amd import engine as E
    from mlimgsynth_amd import kernels as K
    from mlimgsynth_amd import mlimgsynth as M
    assert (M.MLIS_OPT_AMD_HYPERTILE, M.MLIS_OPT_AMD_HYPERTILE_DEPTH) == (191, 192)
    assert callable(M.MLImgSynth.hypertile_set) and callable(M.MLImgSynth.hypertile_info) and callable(K.tile_permute) and callable(E.Generator.hypertile_info)
    assert E.hypertile_side(128, 8, 512) == 64
    assert E.control_hypertile(0) == 0 and E.control_hypertile(512, 3) == 4 | (64 << 8) | (3 << 24) and E.control_hypertile(8192, 0) == 4 | (1024 << 8)
    m = M.MLImgSynth()
    m.hypertile_set(tile=512, depth=1)
    i = C.c_int()
    m.option_get(M.MLIS_OPT_AMD_HYPERTILE, i)
    assert i.value == 512
    m.option_get(M.MLIS_OPT_AMD_HYPERTILE_DEPTH, i)
    assert i.value == 1 and m.hypertile_info() is None           # no engine yet
    with pytest.raises(RuntimeError):
        m.hypertile_set(tile=36)
    exe = os.path.join(ROOT, "mlimgsynth_amd", "bin", "mlimgsynth-amd")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--hypertile PX" in out and "--hypertile-depth N" in out
    r = subprocess.run([exe, "generate", "--hypertile", "36"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "hypertile" in r.stderr


# ------------------------------------------------------------------ the configuration word
def test_config_word(dry):
    from mlimgsynth_amd import engine as E
    assert C.sizeof(E.AmdControlConfig) == C.sizeof(E.AmdConfig)
    g = E.Generator("tiny", 128, 128, 1, defer_weights=True, hypertile=64, hypertile_depth=2)
    try:
        assert g.cfg.control == 4 | (8 << 8) | (2 << 24) and g.ctx_at(5) is None and g.freeu_info() == (0, 0)
    finally:
        g.destroy()
    for word in (4, 4 | (3 << 8), 4 | (1025 << 8), 8 << 8, 1 << 24, 4 | (8 << 8) | (1 << 26), 4 | (8 << 8) | (1 << 22)):
        cfg = E.AmdControlConfig(b"tiny", 64, 64, 1, 20, 7.0, 1.0, 1, 0, 0, 1234, 0, 0.0, 1.0, 0.0, 1, 0, 77, word)
        assert not dry.mlis_amd_create(C.byref(cfg), None), hex(word)      # the flag without a tile, a tile out of range, the fields without the flag, unknown bits


# ------------------------------------------------------------------ dry plans
def records(ctx):
    """op records with the addresses taken out: (kind, label, fused, once, gn_src, {field: value} of every field that is not a pointer)"""
    out = []
    for kind, label, fused, once, gn_src, a in ctx.op_records():
        fields = {n: getattr(a, n) for n, t in a._fields_ if t is not C.c_void_p}
        out.append((kind, label, fused, once, tuple(gn_src), fields))
    return out


def gen(model, w, h, B=1, **kw):
    from mlimgsynth_amd import engine as E
    return E.Generator(model, 8 * w, 8 * h, B, defer_weights=True, cfg_scale=2.0, **kw)


def is_tiling_copy(r):
    return r[0] == "copy" and r[5]["th"] > 0


CASES = [("tiny", 16, 16, 1, 64, 3), ("tiny", 16, 16, 1, 64, 0), ("tiny", 16, 24, 2, 64, 3), ("tinyv", 16, 16, 1, 64, 3), ("tiny", 24, 16, 1, 96, 3),
         ("tinyxl", 20, 12, 1, 32, 3), ("sdxl", 128, 128, 1, 512, 3), ("sd1", 64, 96, 1, 256, 1)]


@pytest.mark.parametrize("model,w,h,B,tile,depth", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-b{c[3]}-t{c[4]}-d{c[5]}" for c in CASES])
def test_tiled_plan_is_the_plain_plan_with_copies_and_tile_shaped_self_attention(dry, model, w, h, B, tile, depth):
    g0, g1 = gen(model, w, h, B), gen(model, w, h, B, hypertile=tile, hypertile_depth=depth)
    try:
        plain, tiled = records(g0.ctx_at(0)), records(g1.ctx_at(0))
        info = g1.hypertile_info()
        assert info == HR.plan_info(model, w, h, tile, depth) and g0.hypertile_info() == (0, info[0] + info[1], [(0, 0, 0, 0)] * 4)
        n_tiled, _, tiles = info
        assert n_tiled > 0
        copies = [r for r in tiled if is_tiling_copy(r)]
        assert len(copies) == 2 * n_tiled
        N = 2 * B
        rest, inside, n_self, at = [], None, 0, {}
        for i, r in enumerate(tiled):
            f = r[5]
            if is_tiling_copy(r):
                geo = (f["n_img"], f["H"], f["W"], f["th"], f["tw"], f["row_bytes"])
                if inside is None:                               # each pair is forward then inverse with equal geometry
                    assert f["inverse"] == 0 and r[1] == "hypertile_tile"
                    inside = geo
                    assert (f["th"], f["tw"], f["H"] // f["th"], f["W"] // f["tw"]) in tiles and f["n_img"] == N
                    assert f["nbytes"] == N * f["H"] * f["W"] * f["row_bytes"] and f["row_bytes"] % 16 == 0
                else:
                    assert f["inverse"] == 1 and geo == inside and r[1] == "hypertile_untile"
                    inside = None
                continue
            if inside is not None and r[0] == "attn" and r[5]["Tk"] != 77:     # a self-attention between a pair
                n_img, H, W, th, tw, _ = inside
                assert (f["n_batch"], f["Tq"], f["Tk"]) == (N * (H // th) * (W // tw), th * tw, th * tw), f
                assert f["bsq"] == f["Tq"] * f["ldq"] and f["bsk"] == f["Tk"] * f["ldk"] and f["bsv"] == f["Tk"] * f["ldv"] and f["bso"] == f["Tq"] * f["ldo"]
                n_self += 1
            at[i] = len(rest)
            rest.append(r)
        rest = [r[:4] + (tuple(at[j] if j >= 0 else j for j in r[4]),) + r[5:] for r in rest]      # producer indices, counted without the copies
        assert inside is None and n_self >= n_tiled
        # everything else is the plain plan: the same ops in the same order; only the self-attentions between a pair differ, and only in their batch shape
        assert len(rest) == len(plain)
        changed = 0
        for a, b in zip(rest, plain):
            if a == b:
                continue
            assert a[0] == b[0] == "attn" and a[:5] == b[:5] and b[5]["Tk"] == b[5]["Tq"] != 77, (a, b)
            same = {k for k in a[5] if a[5][k] == b[5][k]}
            assert set(a[5]) - same == {"n_batch", "Tq", "Tk", "bsq", "bsk", "bsv", "bso"}
            assert a[5]["n_batch"] * a[5]["Tq"] == b[5]["n_batch"] * b[5]["Tq"]
            changed += 1
        assert changed == n_self
        # every cross-attention has what the plain plan has: separate launches (Tk 77) compared above as equal, fused ones through the xa_* fields of their q projection
        xa = [(r[5]["xa_Tq"], r[5]["xa_Tk"], r[5]["M"]) for r in rest if r[0] == "gemm" and r[5].get("xa_Tk")]
        assert xa == [(r[5]["xa_Tq"], r[5]["xa_Tk"], r[5]["M"]) for r in plain if r[0] == "gemm" and r[5].get("xa_Tk")]
        assert [r for r in rest if r[0] == "attn" and r[5]["Tk"] == 77] == [r for r in plain if r[0] == "attn" and r[5]["Tk"] == 77]
    finally:
        g0.destroy(), g1.destroy()


@pytest.mark.parametrize("model,w,h,kw", [("tiny", 16, 16, dict(hypertile=128)), ("tinyxl", 20, 12, dict(hypertile=32, hypertile_depth=0)),
                                          ("tiny", 8, 8, dict(hypertile=64)), ("sdxl", 64, 64, dict(hypertile=512))],
                         ids=["tile-covers-the-picture", "tinyxl-depth-0", "first-pass-of-a-hires-run", "sdxl-512px-tile-512"])
def test_a_setting_that_cuts_nothing_records_the_plain_plan(dry, model, w, h, kw):
    """tinyxl attends at downscale 2 only, so depth 0 leaves nothing to tile; a tile of at least the picture leaves every level whole"""
    g0, g1 = gen(model, w, h), gen(model, w, h, **kw)
    try:
        assert records(g1.ctx_at(0)) == records(g0.ctx_at(0))
        assert g1.ctx_at(0).op_list() == g0.ctx_at(0).op_list() and g1.ctx_at(0).param_list() == g0.ctx_at(0).param_list()
        n_tiled, n_untiled, tiles = g1.hypertile_info()
        assert n_tiled == 0 and n_untiled > 0 and tiles == [(0, 0, 0, 0)] * 4
    finally:
        g0.destroy(), g1.destroy()


def test_controlnet_plan_follows_the_rule(dry):
    """(the window plans of tiled-diffusion engines cannot be built without a device: tests/test_hypertile_gpu.py holds them)"""
    g = gen("tiny", 16, 16, control=True, hypertile=64)
    try:
        ctl = records(g.ctx_at(5))
        copies = [r for r in ctl if is_tiling_copy(r)]
        assert len(copies) == 2 * 3                               # the encoder copy: one transformer per level and the middle block's
        assert {(r[5]["th"], r[5]["tw"]) for r in copies} == {(8, 8), (4, 4)}
    finally:
        g.destroy()


def test_what_cannot_be_built_without_a_device(dry):
    """why the window plans are checked in the GPU file: a tiled-diffusion engine computes its blend weights with a launch while it is created, which the dry
    runtime refuses with these words.  (The engine key is exercised by generations -- text encoders, sampler and decoder launches -- and is there for that reason.)"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import engine as E
    with pytest.raises(_lib.MlsdError, match="window_wsum"):
        E.Generator("tiny", 192, 192, 1, defer_weights=True, unet_tile=128, unet_tile_overlap=32, hypertile=64)


SETTINGS = [(model, w, h, tile, depth) for model in ("tiny", "tinyv", "tinyxl", "sd1", "sdxl") for w, h in ((8, 8), (16, 16), (20, 12), (16, 24), (64, 64), (15, 9))
            for tile, depth in ((32, 3), (64, 3), (64, 0), (96, 1), (512, 3), (512, 2))]


def test_the_key_rule_agrees_with_what_plans_report(dry):
    """unet_hypertile_cuts decides, before an engine exists, whether a pass gets the plain key: it must count exactly the transformers a built plan tiles, and
    the independent restatement of the walk (hypertile_ref.plan_info) agrees with both"""
    from mlimgsynth_amd import engine as E
    dry.unet_hypertile_cuts.restype, dry.unet_hypertile_cuts.argtypes = F.ci, [C.POINTER(E.UnetParams), F.ci, F.ci, F.ci, F.ci]
    built = 0
    for model, w, h, tile, depth in SETTINGS:
        P = E.unet_params(model)
        n = dry.unet_hypertile_cuts(C.byref(P), w, h, tile, depth)
        assert n == HR.plan_info(model, w, h, tile, depth)[0], (model, w, h, tile, depth)
        if w % 8 == 0 and h % 8 == 0 and w * h <= 16 * 24:      # build the small plans whose maps halve evenly on every level of every model
            g = gen(model, w, h, hypertile=tile, hypertile_depth=depth)
            try:
                assert g.hypertile_info()[0] == n, (model, w, h, tile, depth)
                built += 1
            finally:
                g.destroy()
    assert built == 5 * 3 * 6
    assert dry.unet_hypertile_cuts(C.byref(E.unet_params("sdxl")), 128, 128, 0, 3) == 0


AUDITED = [("unet", "tiny", 16, 2, dict(hypertile=64)), ("unet", "tinyxl", (20, 12), 2, dict(hypertile=32)), ("unet", "sd1", (16, 24), 2, dict(hypertile=64)),
           ("unet", "tinyxl", 16, 2, dict(hypertile=64, stream_weights_mib=1))]


@pytest.mark.parametrize("spec", AUDITED, ids=[PA.plan_id(s) for s in AUDITED])
def test_dataflow_of_tiled_plans(spec):
    """the plan audit's dataflow checks (its launch verifier runs on the device, tests/test_plan_audit_gpu.py): every read has a writer, no launch writes onto its own operand
    but the LayerNorm ending's sound form, and the recycling arena never changes who wrote what a launch reads"""
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    try:
        b0, b1 = PA.build(engine, spec, PA.MLB_F_OPSHAPES), PA.build(engine, spec, PA.MLB_F_OPSHAPES | PA.MLB_F_KEEP)
        try:
            rec, kept = PA.Plan(b0.ctx, PA.plan_id(spec)), PA.Plan(b1.ctx, PA.plan_id(spec) + " kept")
            assert sum(1 for o in rec.ops if o.kind == "copy" and o.a.th > 0) > 0
            for plan in (rec, kept):
                bad = PA.uncovered_reads(plan)
                assert not bad, [why for _, _, why in bad[:6]]
                own = PA.own_operand_overwrites(plan)
                assert not own, [f"{o}: {w} lands on its own operand {r}" for o, w, r in own[:6]]
            assert not PA.clobbered_operands(kept)
            if [PA.op_signature(o) for o in rec.ops] == [PA.op_signature(o) for o in kept.ops]:
                bad = PA.lifetime_diffs(rec, kept)
                assert not bad, bad[:6]
            else:      # a LayerNorm fold the alias rule refuses in one arena only (tests/test_plan_audit_cpu.py): the op lists differ there and nowhere else
                assert all({o.kind, p.kind} <= {"gemm", "ln"} for o, p in zip(rec.ops, kept.ops) if PA.op_signature(o) != PA.op_signature(p))
        finally:
            b0.close(), b1.close()
    finally:
        L.mlsd_runtime_dry(0)


# ------------------------------------------------------------------ what the kernel refuses (before any launch: the dry runtime's buffers are host memory)
def test_kernel_refuses_bad_arguments(dry):
    buf = np.zeros(4096 + 64, np.uint8)
    base = (buf.ctypes.data + 63) & ~63
    s, d = base, base + 2048
    OK = -2                                                # arguments accepted: the dry runtime then declines the launch (-2); a refused argument is -1
    call = lambda src=s, dst=d, n=1, H=4, W=6, th=2, tw=3, rb=32, inv=0: dry.mlsd_tile_permute(src, dst, n, H, W, th, tw, rb, inv, None)
    assert call() == OK and call(inv=1) == OK and call(th=4, tw=6) == OK and call(th=1, tw=1) == OK
    assert call(th=3) == -1 and call(tw=4) == -1 and call(th=8) == -1              # tiles that do not divide the map
    assert call(rb=24) == -1 and call(rb=8) == -1 and call(rb=0) == -1            # rows that are no multiple of 16 bytes
    assert call(src=s + 8) == -1 and call(dst=d + 4) == -1                        # alignment
    assert call(dst=s) == -1 and call(dst=s + 16 * 32) == -1 and call(src=d - 16) == -1      # in place, overlapping from either side
    assert call(dst=s + 24 * 32) == OK                                            # back to back is no overlap
    assert call(src=None) == -1 and call(dst=None) == -1 and call(n=0) == -1 and call(H=0) == -1 and call(th=0) == -1 and call(tw=-1) == -1
    assert not buf.any()


# ------------------------------------------------------------------ the torch reference
def test_reference_tiles_the_self_attention_only():
    torch = pytest.importorskip("torch")
    P = HR.UNET["tiny"]
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((1, 4, 16, 16)).astype(np.float32))
    ctx = torch.from_numpy(rng.standard_normal((1, 77, P["n_ctx"])).astype(np.float32))
    t = torch.full((1,), 500.0)
    net, whole, plain = HR.make_net(64), HR.make_net(128), HR.CR.make_net()
    with torch.no_grad():
        a, b, c = net.unet(P, x, t, ctx), whole.unet(P, x, t, ctx), plain.unet(P, x, t, ctx)
    assert torch.equal(b, c) and not torch.equal(a, c)            # a tile that covers the picture is the plain network, bit for bit
    assert [(ds, tl) for _, ds, tl in net.log] == [(1, (8, 8)), (2, (4, 4)), (2, (4, 4)), (2, (4, 4)), (2, (4, 4)), (1, (8, 8)), (1, (8, 8))]
    assert all(tl is None for _, _, tl in whole.log)
    n_tiled, n_untiled, _ = HR.plan_info("tiny", 16, 16, 64, 3)
    assert (n_tiled, n_untiled) == (len(net.log), 0)
