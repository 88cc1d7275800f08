"""Case table of the float64 GEMM / implicit-GEMM convolution tests (tests/test_gemm_float64_gpu.py; operands also used by
tests/test_ref64_gemm_cpu.py).  A plain module: importable without a GPU.

Every case names the label `kernels.gemm_variant(args)` must return for it, so that a case cannot drift silently to another tile; the
census (test_gemm_float64_gpu.py::test_every_planned_gemm_path_has_a_float64_case) checks that every path the bench plans pick has a case.
The two tables at the end hold one case per (tile, split form, epilogue feature set) the plans take, at the bench sizes and at the sizes of
tests/plan_audit.py SIZE_PLANS (SD1.5 from 40x40 to 96x96, SDXL from 64x64 to 168x96, N = 1 .. 8, the VAEs and TAESD at other sizes);
tests/test_plan_audit_gpu.py COVERED_ELSEWHERE names them form by form.

Input families (make_operands):
  normal     centred N(0, 1) activations, N(0, 1 / K) weights;
  offset     A = mu + sigma z with mu / sigma = 300, weight rows of zero mean: |C| << S = sum |a w|;
  silupos    post-SiLU-like activations (>= -0.28, mostly positive);
  scales     per-row A scales and per-column W scales over 2^-12 .. 2^12;
  subnormal  weights and half of the activation rows below 2^-14 (fp16 subnormals): products only fp32 represents;
  bigout     outputs of a few 10^4, some above 65504 (fp16 +-inf);
  tinyout    outputs around 2^-15: fp16 subnormal outputs;
  bigres     a residual of ~10^3 against a product of ~1;
  wideact    activation arguments spread over [-100, 100] (bias uniform in that range), with product noise of ~1.
"""
import zlib

import numpy as np

PATH_OF = {}      # filled below: case id -> path name (variant family + epilogue form) used in the printed worst ratios


def _case(cid, variant, path, **kw):
    c = dict(id=cid, variant=variant, path=path, conv=False, fam="normal", tv=0, bias=False, rowbias=0, bias_m=False, act=0, resid=False,
             post=False, c32=True, c16=False, ksplit=1, sk=False, stats=False, ln=False, exp=False, ws=False)
    c.update(kw)
    if c["conv"]:
        n, H, W, cin = c["n"], c["H"], c["W"], c["cin"]
        c["cin_pad"] = (cin + 7) // 8 * 8
        Hs, Ws = (2 * H, 2 * W) if c.get("ups") else (H, W)
        c["OH"] = (Hs + 2 * c["p"] - c["k"]) // c["s"] + 1
        c["OW"] = (Ws + 2 * c["p"] - c["k"]) // c["s"] + 1
        c["M"], c["N"], c["K"] = n * c["OH"] * c["OW"], c["cout"], c["k"] * c["k"] * c["cin_pad"]
    c["nout"] = c["N"] // 2 if c["act"] == 5 else c["N"]
    PATH_OF[cid] = path
    return c


def lin(cid, variant, path, M, N, K, **kw):
    return _case(cid, variant, path, M=M, N=N, K=K, **kw)


def conv(cid, variant, path, n, H, W, cin, cout, k, s, p, ups=0, **kw):
    return _case(cid, variant, path, conv=True, n=n, H=H, W=W, cin=cin, cout=cout, k=k, s=s, p=p, ups=ups, **kw)


def tv(v):
    """tile_variant field that selects kVariants[v]"""
    return v + 1


G0, G1, G3, G4, G9, G16 = "128x128x64s2", "64x128x64s2", "256x128x64s2", "256x128x32s3", "256x256x64s2w16", "128x320x64s2"
P17, P18, P19, P20, P21, P28 = "256x256x64pp", "128x320x64pp", "256x256x64ppsk", "128x320x64pp2", "256x256x64pp2", "128x320x64ppsk"
SK29, TT30, SN31 = "skinny128x64", "128x160x64tt", "conv3x3n16"


def L(name, kind="linear", extra=""):
    return f"gemm<{name},{kind}{extra}>"


CASES = [
    # ---- general tiles (gemm_kernel: 32x32x16 MFMA, ragged M / N / K, padded channels, upsampled sources, GEGLU)
    lin("g0_ragged_bias_c16", L(G0), "128x128x64s2", 300, 200, 136, bias=True, c16=True),
    lin("g0_k8", L(G0), "128x128x64s2", 257, 72, 8, bias=True, c16=True),
    lin("g0_offset_res", L(G0), "128x128x64s2", 385, 160, 1280, fam="offset", bias=True, resid=True, c16=True, tv=tv(0)),
    lin("g0_scales", L(G0), "128x128x64s2", 257, 130, 320, fam="scales", c16=True, tv=tv(0)),
    lin("g0_subnormal", L(G0), "128x128x64s2", 200, 136, 320, fam="subnormal", c16=True, tv=tv(0)),
    lin("g0_bigout", L(G0), "128x128x64s2", 200, 128, 256, fam="bigout", c16=True, tv=tv(0)),
    lin("g0_tinyout", L(G0), "128x128x64s2", 200, 128, 256, fam="tinyout", c16=True, tv=tv(0)),
    lin("g0_bigres", L(G0), "128x128x64s2", 129, 200, 320, fam="bigres", bias=True, resid=True, c16=True, tv=tv(0)),
    lin("g0_silu_wide", L(G0), "128x128x64s2", 129, 200, 72, fam="wideact", bias=True, act=1, c16=True, tv=tv(0)),
    lin("g0_gelu_wide_res", L(G0), "128x128x64s2", 129, 200, 72, fam="wideact", bias=True, act=2, resid=True, c16=True, tv=tv(0)),
    lin("g0_qgelu_wide", L(G0), "128x128x64s2", 129, 200, 72, fam="wideact", bias=True, act=3, c16=True, tv=tv(0)),
    lin("g0_relu_post", L(G0), "128x128x64s2", 129, 200, 136, fam="wideact", bias=True, act=4, resid=True, post=True, c16=True, tv=tv(0)),
    lin("g0_silu_post", L(G0), "128x128x64s2", 129, 200, 136, fam="wideact", bias=True, act=1, resid=True, post=True, tv=tv(0)),
    lin("g0_rowbias_biasm", L(G0), "128x128x64s2", 384, 200, 320, bias=True, rowbias=192, bias_m=True, resid=True, c16=True, tv=tv(0)),
    lin("g0_geglu_wide", L(G0), "128x128x64s2:geglu", 129, 256, 136, fam="wideact", bias=True, act=5, c16=True, tv=tv(0)),
    lin("g0_geglu_res", L(G0), "128x128x64s2:geglu", 300, 640, 320, bias=True, act=5, resid=True, tv=tv(0)),
    conv("g0_conv_cin3", L(G0, "conv"), "128x128x64s2", 2, 13, 11, 3, 64, 3, 1, 1, bias=True, c16=True, tv=tv(0)),
    conv("g0_conv_s2_odd", L(G0, "conv"), "128x128x64s2", 2, 17, 15, 40, 96, 3, 2, 1, bias=True, tv=tv(0)),
    conv("g0_conv_ups_odd", L(G0, "conv"), "128x128x64s2", 2, 7, 9, 72, 80, 3, 1, 1, ups=1, bias=True, resid=True, tv=tv(0)),
    conv("g0_conv_pad0", L(G0, "conv"), "128x128x64s2", 3, 10, 9, 24, 48, 3, 1, 0, bias=True, c16=True, tv=tv(0)),
    conv("g0_conv_straddle", L(G0, "conv"), "128x128x64s2", 3, 9, 7, 64, 64, 3, 1, 1, fam="offset", rowbias=63, bias=True, resid=True, tv=tv(0)),
    conv("g0_conv1x1", L(G0, "conv"), "128x128x64s2", 2, 9, 9, 136, 72, 1, 1, 0, fam="scales", bias=True, c16=True, tv=tv(0)),
    lin("g1_smallm", L(G1), "64x128x64s2", 64, 200, 320, bias=True, act=1, resid=True, c16=True),
    lin("g1_m1", L(G1), "64x128x64s2", 1, 8, 8, act=4, c16=True),
    conv("g1_conv_subnormal", L(G1, "conv"), "64x128x64s2", 1, 8, 7, 64, 128, 3, 1, 1, fam="subnormal", bias=True, c16=True, tv=tv(1)),
    conv("g1_conv_cin4", L(G1, "conv"), "64x128x64s2", 1, 9, 9, 4, 512, 3, 1, 1, bias=True, tv=tv(1)),
    lin("g3_offset", L(G3), "256x128x64s2", 513, 200, 640, fam="offset", bias=True, resid=True, c16=True, tv=tv(3)),
    conv("g3_conv_scales", L(G3, "conv"), "256x128x64s2", 2, 12, 11, 64, 136, 3, 1, 1, fam="scales", bias=True, tv=tv(3)),
    conv("g4_conv_vae", L(G4, "conv"), "256x128x32s3", 1, 31, 33, 128, 128, 3, 1, 1, fam="offset", bias=True, resid=True, tv=tv(4)),
    conv("g4_conv_bigout", L(G4, "conv"), "256x128x32s3", 1, 17, 19, 32, 128, 3, 1, 1, fam="bigout", bias=True, c16=True, tv=tv(4)),
    lin("g4_k72_silu", L(G4), "256x128x32s3", 300, 200, 72, fam="wideact", bias=True, act=1, c16=True, tv=tv(4)),
    lin("g9_ragged", L(G9), "256x256x64s2w16", 513, 330, 192, bias=True, c16=True, tv=tv(9)),
    conv("g9_conv_offset", L(G9, "conv"), "256x256x64s2w16", 1, 23, 21, 64, 256, 3, 1, 1, fam="offset", bias=True, resid=True, tv=tv(9)),
    lin("g16_lin", L(G16), "128x320x64s2", 257, 640, 136, bias=True, act=2, resid=True, c16=True, tv=tv(16)),
    lin("g16_scales", L(G16), "128x320x64s2", 300, 320, 320, fam="scales", c16=True, tv=tv(16)),
    # ---- split-K, two launches (slices to the workspace, splitk_reduce / splitk_reduce_stats / splitk_reduce_ln adds them in order + the epilogue)
    lin("sk0_unequal", L(G0, "linear", ",k/3"), "splitk_reduce", 300, 200, 448, ksplit=3, ws=True, bias=True, resid=True, c16=True, tv=tv(0)),
    lin("sk1_offset", L(G1, "linear", ",k/6"), "splitk_reduce", 64, 1280, 2560, fam="offset", ksplit=6, ws=True, bias=True, resid=True, tv=tv(1)),
    lin("sk1_silu_wide", L(G1, "linear", ",k/4"), "splitk_reduce", 60, 320, 1280, fam="wideact", ksplit=4, ws=True, bias=True, act=1, c16=True, tv=tv(1)),
    conv("sk1_conv_scales", L(G1, "conv", ",k/5"), "splitk_reduce", 2, 8, 8, 320, 640, 3, 1, 1, fam="scales", ksplit=5, ws=True, bias=True,
         rowbias=64, resid=True, tv=tv(1)),
    conv("sk1_conv_subnormal", L(G1, "conv", ",k/9"), "splitk_reduce", 1, 8, 8, 128, 256, 3, 1, 1, fam="subnormal", ksplit=9, ws=True, c16=True, tv=tv(1)),
    conv("sk0_stats", L(G0, "conv", ",k/3"), "splitk_reduce_stats", 2, 16, 16, 64, 128, 3, 1, 1, fam="offset", ksplit=3, ws=True, bias=True,
         stats=True, tv=tv(0)),
    lin("sk1_ln", L(G1, "linear", "+layernorm,k/3"), "splitk_reduce_ln", 128, 640, 1280, fam="offset", ksplit=3, ws=True, bias=True, resid=True,
        ln=True, tv=tv(1)),
    # ---- ping-pong tiles (gemm_pp.hpp: 16x16x32 MFMA; epilogues F16, F32, F32_RES, F32_STATS, GEGLU16, GENERIC)
    lin("p17_f16", L(P17), "256x256x64pp", 256, 512, 640, bias=True, c32=False, c16=True, tv=tv(17)),
    lin("p17_f32_offset", L(P17), "256x256x64pp", 384, 256, 1280, fam="offset", bias=True, tv=tv(17)),
    lin("p17_res_bigres", L(P17), "256x256x64pp", 256, 320, 320, fam="bigres", bias=True, resid=True, tv=tv(17)),
    lin("p17_generic_gelu", L(P17), "256x256x64pp", 256, 256, 256, fam="wideact", bias=True, act=2, resid=True, c16=True, tv=tv(17)),
    lin("p17_geglu16", L(P17), "256x256x64pp:geglu", 256, 1024, 320, fam="wideact", bias=True, act=5, c32=False, c16=True, tv=tv(17)),
    lin("p17_geglu16_normal", L(P17), "256x256x64pp:geglu", 384, 2560, 640, bias=True, act=5, c32=False, c16=True, tv=tv(17)),
    lin("p17_biasm", L(P17), "256x256x64pp", 256, 256, 512, fam="scales", bias_m=True, c16=True, tv=tv(17)),
    conv("p17_conv_stats", L(P17, "conv"), "256x256x64pp", 1, 16, 16, 64, 256, 3, 1, 1, fam="offset", bias=True, stats=True, tv=tv(17)),
    conv("p17_conv_ups", L(P17, "conv"), "256x256x64pp", 1, 8, 16, 64, 256, 3, 1, 1, ups=1, bias=True, tv=tv(17)),
    lin("p18_f32_res", L(P18), "128x320x64pp", 192, 640, 1280, fam="offset", bias=True, resid=True, tv=tv(18)),
    lin("p18_f16_bigout", L(P18), "128x320x64pp", 128, 320, 256, fam="bigout", c32=False, c16=True, tv=tv(18)),
    lin("p18_f16_tiny", L(P18), "128x320x64pp", 128, 400, 256, fam="tinyout", c32=False, c16=True, tv=tv(18)),
    lin("p18_generic_silu", L(P18), "128x320x64pp", 128, 320, 192, fam="wideact", bias=True, act=1, resid=True, c16=True, tv=tv(18)),
    lin("p18_qgelu_post", L(P18), "128x320x64pp", 128, 320, 192, fam="wideact", bias=True, act=3, resid=True, post=True, c16=True, tv=tv(18)),
    lin("p18_subnormal", L(P18), "128x320x64pp", 128, 320, 640, fam="subnormal", c16=True, tv=tv(18)),
    conv("p18_conv_rowbias", L(P18, "conv"), "128x320x64pp", 2, 8, 16, 64, 320, 3, 1, 1, fam="scales", bias=True, rowbias=128, resid=True,
         tv=tv(18)),
    conv("p18_conv_stats_res", L(P18, "conv"), "128x320x64pp", 1, 16, 8, 128, 320, 3, 1, 1, fam="offset", bias=True, resid=True, stats=True,
         tv=tv(18)),
    lin("p18_ln", L(P18, "linear", "+layernorm"), "128x320x64pp:ln", 256, 640, 640, fam="offset", bias=True, resid=True, ln=True, tv=tv(18)),
    lin("p20_res", L(P20), "128x320x64pp2", 256, 640, 640, fam="offset", bias=True, resid=True, tv=tv(20)),
    conv("p20_conv_silu", L(P20, "conv"), "128x320x64pp2", 1, 8, 16, 64, 320, 3, 1, 1, fam="wideact", bias=True, act=1, c16=True, tv=tv(20)),
    lin("p21_res", L(P21), "256x256x64pp2", 256, 512, 640, fam="scales", bias=True, resid=True, tv=tv(21)),
    conv("p21_conv", L(P21, "conv"), "256x256x64pp2", 1, 16, 16, 128, 256, 3, 1, 1, fam="offset", bias=True, resid=True, tv=tv(21)),
    # ---- stream-K (K-tile units dealt over the persistent blocks, partial tiles combined in the launch): contributors per tile = K / 64 / share
    lin("p19_sk16", L(P19), "256x256x64ppsk", 512, 512, 4096, fam="offset", sk=True, ws=True, bias=True, resid=True, tv=tv(19)),
    lin("p19_sk64", L(P19), "256x256x64ppsk", 256, 256, 16384, sk=True, ws=True, bias=True, tv=tv(19)),
    lin("p19_sk2", L(P19), "256x256x64ppsk", 4096, 2048, 512, sk=True, ws=True, bias=True, resid=True, tv=tv(19)),
    lin("p19_sk_silu", L(P19), "256x256x64ppsk", 256, 512, 4096, fam="wideact", sk=True, ws=True, bias=True, act=1, c16=True, tv=tv(19)),
    lin("p28_sk18", L(P28), "128x320x64ppsk", 256, 320, 5760, fam="scales", sk=True, ws=True, bias=True, resid=True, tv=tv(28)),
    conv("p28_conv", L(P28, "conv"), "128x320x64ppsk", 1, 16, 16, 640, 640, 3, 1, 1, fam="offset", sk=True, ws=True, bias=True, resid=True,
         tv=tv(28)),
    # ---- skinny M (weights streamed, K slices to the workspace, splitk_reduce adds them -- also for one slice)
    lin("s29_m8", L(SK29, "linear", ",k/10"), "skinny128x64", 8, 1280, 1280, ws=True, ksplit=10, bias=True, resid=True, tv=tv(29)),
    lin("s29_m2_offset", L(SK29, "linear", ",k/2"), "skinny128x64", 2, 1280, 320, fam="offset", ws=True, ksplit=2, bias=True, tv=tv(29)),
    lin("s29_m77_silu", L(SK29, "linear", ",k/4"), "skinny128x64", 77, 640, 1280, fam="wideact", ws=True, ksplit=4, bias=True, act=1, c16=True,
        tv=tv(29)),
    conv("s29_conv", L(SK29, "conv", ",k/9"), "skinny128x64", 2, 8, 8, 128, 1280, 3, 1, 1, fam="scales", ws=True, ksplit=9, bias=True,
         resid=True, tv=tv(29)),
    lin("s29_m128_one", L(SK29, "linear", ",k/1"), "skinny128x64", 128, 256, 256, fam="subnormal", ws=True, c16=True, tv=tv(29)),
    # ---- two tiles per CU (gemm_tt.hip)
    lin("t30_f32", L(TT30), "128x160x64tt", 1024, 640, 320, fam="offset", bias=True, tv=tv(30)),
    lin("t30_res", L(TT30), "128x160x64tt", 512, 1280, 640, fam="bigres", bias=True, resid=True, tv=tv(30)),
    lin("t30_f16", L(TT30), "128x160x64tt", 256, 1920, 640, fam="bigout", c32=False, c16=True, tv=tv(30)),
    conv("t30_conv1x1", L(TT30, "conv"), "128x160x64tt", 2, 16, 16, 320, 640, 1, 1, 0, fam="scales", bias=True, resid=True, tv=tv(30)),
    lin("t30_ln", L(TT30, "linear", "+layernorm"), "128x160x64tt:ln", 512, 640, 640, fam="offset", bias=True, resid=True, ln=True, tv=tv(30)),
    # ---- small-Cout 3x3 convolution (conv_smalln.hip): chosen by shape above the table
    conv("n31_vae_out", L(SN31, "conv"), "conv3x3n16", 1, 129, 128, 128, 3, 3, 1, 1, fam="offset", bias=True),
    conv("n31_tae_out", L(SN31, "conv"), "conv3x3n16", 2, 96, 91, 64, 16, 3, 1, 1, fam="scales", bias=True),
    # ---- EXPERIMENTS-only variants (skipped in the product build)
    lin("x22", L("128x320x64ppb"), "128x320x64ppb", 128, 320, 640, fam="offset", bias=True, resid=True, tv=tv(22), exp=True),
    lin("x25", L("256x128x64pp2"), "256x128x64pp2", 256, 128, 576, bias=True, tv=tv(25), exp=True),
]

# ---- the epilogue combinations the bench plans put on each tile (tests/test_plan_audit_gpu.py, COVERED_ELSEWHERE): each case carries EXACTLY the features of one
# op form -- row bias, residual, column statistics, the fp16 copy beside the fp32 output, the upsampled source -- because each combination selects its own epilogue body
def _combo(cid, tile, tvn, cout, ksplit=1, ups=0, hw=None, lin_mk=None, fam="offset", **f):
    """a 3x3 convolution of 2 images of hw = (H, W) x 64 channels (16 x 16, 8 x 8 with `ups`), or with lin_mk = (M, K) a Linear of M x cout x K, forced onto `tile`"""
    H, W = hw or ((8, 8) if ups else (16, 16))
    red = "splitk_reduce_ln" if f.get("ln") else "splitk_reduce_stats" if f.get("stats") else "splitk_reduce"
    path = (tile if tile == SK29 else red) if ksplit > 1 else tile + (":geglu" if f.get("act") == 5 else "")
    ending = ("+layernorm" if f.get("ln") else "") + (f",k/{ksplit}" if ksplit > 1 else "")
    common = dict(fam=fam, bias=True, ksplit=ksplit, ws=ksplit > 1, tv=tv(tvn), **f)
    if lin_mk:
        return lin(cid, L(tile, "linear", ending), path, lin_mk[0], cout, lin_mk[1], **common)
    return conv(cid, L(tile, "conv", ending), path, 2, H, W, 64, cout, 3, 1, 1, ups=ups, **common)


CASES += [
    _combo("sk0_c16_stats", G0, 0, 128, ksplit=3, c16=True, stats=True),
    _combo("sk0_stats_res", G0, 0, 128, ksplit=3, stats=True, resid=True),
    _combo("sk0_stats_rowbias", G0, 0, 128, ksplit=3, stats=True, rowbias=256),
    _combo("sk0_stats_ups", G0, 0, 128, ksplit=3, stats=True, ups=1),
    _combo("sk1_c16_stats_res", G1, 1, 128, ksplit=3, c16=True, stats=True, resid=True),
    _combo("g1_stats_rowbias", G1, 1, 128, stats=True, rowbias=256),
    _combo("g1_stats_ups", G1, 1, 128, stats=True, ups=1),
    _combo("g3_stats_ups", G3, 3, 128, stats=True, ups=1),
    _combo("g4_plain", G4, 4, 128),
    _combo("g4_stats", G4, 4, 128, stats=True),
    _combo("g4_stats_res", G4, 4, 128, stats=True, resid=True),
    _combo("g9_plain", G9, 9, 256),
    _combo("g9_stats", G9, 9, 256, stats=True),
    _combo("g9_stats_ups", G9, 9, 256, stats=True, ups=1),
    _combo("g9_c16_stats_ups", G9, 9, 256, c16=True, stats=True, ups=1),
    _combo("g9_c16_res", G9, 9, 256, c16=True, resid=True),
    _combo("p20_stats_res", P20, 20, 320, stats=True, resid=True),
    _combo("p20_stats_rowbias", P20, 20, 320, stats=True, rowbias=256),
    _combo("p21_stats", P21, 21, 256, stats=True),
    _combo("p21_stats_res", P21, 21, 256, stats=True, resid=True),
    _combo("p21_ups", P21, 21, 256, ups=1),
    _combo("p21_c16_res", P21, 21, 256, c16=True, resid=True),
    lin("s29_m8_c16", L(SK29, "linear", ",k/10"), "skinny128x64", 8, 1280, 1280, ws=True, ksplit=10, bias=True, resid=True, c16=True, tv=tv(29)),
    lin("p28_sk18_c16", L(P28), "128x320x64ppsk", 256, 320, 5760, fam="offset", sk=True, ws=True, bias=True, c16=True, tv=tv(28)),
    conv("p28_conv_rowbias", L(P28, "conv"), "128x320x64ppsk", 1, 16, 16, 640, 640, 3, 1, 1, fam="offset", sk=True, ws=True, bias=True, rowbias=256, tv=tv(28)),
]

# ---- the forms the plans take at sizes other than the bench's (tests/plan_audit.py SIZE_PLANS; the census of tests/test_size_census_cpu.py and
# tests/test_plan_audit_gpu.py): again EXACTLY the features of one op form, on the tile and split form the census met it on.  Where no feature forbids it the
# convolutions have one full tile plus a ragged one in M and in N: 2 x (17 x 15) = 510 rows (2 x (9 x 7) upsampled: 504) and a cout that is no multiple of the tile
# width.  Column statistics need M in whole statistics blocks: those keep 2 x (16 x 16) rows, with a ragged last column tile (as N = 320 and 640 are on 128 and 256).
ODD, ODD_UPS = (17, 15), (9, 7)
CASES += [
    # 128x128, split-K: the reduce pass ends with the LayerNorm (SD1.5 and SDXL at small N: Linear with the residual, 1x1 proj_in convolution without), ...
    _combo("sk0_ln_res", G0, 0, 640, ksplit=3, lin_mk=(128, 1280), resid=True, ln=True),
    _combo("sk0_ln", G0, 0, 640, ksplit=3, lin_mk=(128, 1280), ln=True),
    # ... a row bias alone (the time embedding on a long-K convolution of few rows), all three outputs of a 1x1 convolution, an upsampling convolution of odd extents
    _combo("sk0_rowbias", G0, 0, 200, ksplit=3, hw=ODD, rowbias=255, fam="scales"),
    _combo("sk0_c16_stats_res", G0, 0, 192, ksplit=3, c16=True, stats=True, resid=True),
    _combo("sk0_ups", G0, 0, 200, ksplit=3, ups=1, hw=ODD_UPS, fam="normal"),
    _combo("sk1_stats", G1, 1, 192, ksplit=3, stats=True),
    # skinny M with a row bias: two images of 64 rows in the one block
    _combo("s29_conv_rowbias", SK29, 29, 200, ksplit=3, hw=(8, 8), rowbias=64, fam="scales"),
    # the general 128x320 tile (wave tile 32 x 160): what every SDXL latent that is not square, and 100 x 100, puts on it
    _combo("g16_plain", G16, 16, 400, hw=ODD, fam="normal"),
    _combo("g16_ups", G16, 16, 400, ups=1, hw=ODD_UPS, fam="scales"),
    _combo("g16_res", G16, 16, 400, hw=ODD, resid=True, fam="scales"),
    _combo("g16_rowbias", G16, 16, 400, hw=ODD, rowbias=255, fam="normal"),
    _combo("g16_c16", G16, 16, 400, hw=ODD, c16=True, fam="scales"),
    _combo("g16_c16_res", G16, 16, 400, hw=ODD, c16=True, resid=True, fam="normal"),
    # the general 256x256 tile (16 waves of 64 x 64)
    _combo("g9_geglu16", G9, 9, 640, lin_mk=(300, 320), fam="wideact", act=5, c32=False, c16=True),
    _combo("g9_rowbias", G9, 9, 320, hw=ODD, rowbias=255, fam="normal"),
    _combo("g9_stats_rowbias", G9, 9, 320, stats=True, rowbias=256),
    _combo("g9_ups", G9, 9, 320, ups=1, hw=ODD_UPS, fam="scales"),
    _combo("g9_res", G9, 9, 320, hw=ODD, resid=True, fam="scales"),
    _combo("g9_stats_res", G9, 9, 320, stats=True, resid=True),
    # the ping-pong 256x256 tiles (whole 128-row wave slabs, a row bias in whole tiles of 256 rows): a ragged last column tile; 384 rows = a tile and a half
    _combo("p17_stats_rowbias", P17, 17, 320, stats=True, rowbias=256),
    _combo("p21_stats_ups", P21, 21, 320, stats=True, ups=1),
    _combo("p21_plain", P21, 21, 320, hw=(16, 12), fam="normal"),
    # 256x128 with the 2-deep and the 3-deep ring: the KL-VAE at other sizes, and TAESD (relu AFTER the residual, fp16 beside fp32, fp16 alone)
    _combo("g3_plain", G3, 3, 200, hw=ODD, fam="normal"),
    _combo("g3_stats_res", G3, 3, 192, stats=True, resid=True),
    _combo("g3_c16_relu_post", G3, 3, 200, hw=ODD, fam="wideact", act=4, resid=True, post=True, c16=True),
    _combo("g3_c16_ups", G3, 3, 200, ups=1, hw=ODD_UPS, c16=True, fam="scales"),
    _combo("g4_ups", G4, 4, 200, ups=1, hw=ODD_UPS, fam="scales"),
    _combo("g4_c16_ups", G4, 4, 200, ups=1, hw=ODD_UPS, c16=True, fam="normal"),
    _combo("g4_relu_post16", G4, 4, 200, hw=ODD, fam="wideact", act=4, resid=True, post=True, c32=False, c16=True),
    # forms only the device census meets (stream-K and the in-launch hand-offs ask the device for its CUs; the dry runtime plans their fall-backs): the statistics
    # epilogues of the four-phase ping-pong tiles with a residual and with a row bias (400 columns: a tile and one wave column of 80), ...
    _combo("p17_stats_res", P17, 17, 320, stats=True, resid=True),
    _combo("p18_stats_rowbias", P18, 18, 400, stats=True, rowbias=256),
    # ... and stream-K on the 256x256 tile with a row bias: 4 tiles x 90 K tiles in shares of 5, 18 contributors per tile
    conv("p19_conv_rowbias", L(P19, "conv"), "256x256x64ppsk", 2, 16, 16, 640, 320, 3, 1, 1, fam="scales", sk=True, ws=True, bias=True, rowbias=256, tv=tv(19)),
]
assert len({c["id"] for c in CASES}) == len(CASES)

BY_ID = {c["id"]: c for c in CASES}


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def make_operands(c, seed=None):
    """fp16 A ([M][K] for linear, the NHWC image [n H W][cin_pad] for conv), fp16 W [N][K] (conv: repacked [cout][kh][kw][cin_pad], zero
    padded channels) and the fp32 epilogue operands of case c, as numpy arrays."""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()) if seed is None else seed)
    M, N, K, fam = c["M"], c["N"], c["K"], c["fam"]
    if c["conv"]:
        rows, kin, cin = c["n"] * c["H"] * c["W"], c["cin_pad"], c["cin"]
    else:
        rows, kin, cin = M, K, K
    z = rng.standard_normal((rows, kin))
    w = rng.standard_normal((N, K)) / np.sqrt(K)
    if fam == "offset":
        a = 3.0 + 0.01 * z
        w = w.reshape(N, -1, kin) if c["conv"] else w
        w = (w - w.mean(axis=-1, keepdims=True)).reshape(N, K)
    elif fam == "silupos":
        g = 2.0 * z
        a = g / (1.0 + np.exp(-g))
    elif fam == "scales":
        a = z * 2.0 ** rng.uniform(-12, 12, (rows, 1))
        w = w * 2.0 ** rng.uniform(-12, 12, (N, 1))
    elif fam == "subnormal":
        a = z * np.where(rng.random((rows, 1)) < 0.5, 2.0 ** -16, 1.0)
        w = w * 2.0 ** -16 * np.sqrt(K)
    elif fam == "bigout":
        a, w = 64.0 * z, w * 470.0
    elif fam == "tinyout":
        a, w = z * 2.0 ** -8, w * 2.0 ** -7
    else:
        a = z
    if c["conv"]:
        a[:, cin:] = 0.0
        w = w.reshape(N, c["k"], c["k"], kin)
        w[..., cin:] = 0.0
        w = w.reshape(N, K)
    A, Wt = f16(a), f16(w)
    nout = c["nout"]
    ops = dict(A=A, W=Wt)
    big = 100.0 if fam == "wideact" else 1.0
    if c["bias"]:
        ops["bias"] = (rng.uniform(-big, big, N) if fam == "wideact" else rng.standard_normal(N)).astype(np.float32)
    if c["rowbias"]:
        nb = -(-M // c["rowbias"])
        ops["rowbias"] = rng.standard_normal((nb, N)).astype(np.float32)
    if c["bias_m"]:
        ops["bias_m"] = rng.standard_normal(M).astype(np.float32)
    if c["resid"]:
        ops["resid"] = (rng.standard_normal((M, nout)) * (1e3 if fam == "bigres" else big)).astype(np.float32)
    return ops
