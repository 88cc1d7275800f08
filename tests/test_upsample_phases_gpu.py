"""The phase form of an upsampling convolution on the device (hip/ups_phase.hip, gemm_pp.hpp PP_EPI_F32_PIX): four 2x2 convolutions over the source image,
one per output parity, instead of one 3x3 convolution over the nearest-2x upsampled image.

Kernel level (tiny shapes: n = 2 images, H = 4 or 5, W = 16, Cin = 64; Cout = 320 on the 128x320 tiles, 256 on the 256x256 tiles; bias on / off; wrap 0 / 3):
  * every phase launch, per element, against float64 of ITS OWN operands (the derived fp16 weights the device formed, the fp16 source) at the bound tests/ref64.py
    states for an fp32 convolution output (accumulation C_GEMM u32 D S + the bias add);
  * the assembled 2H x 2W output against float64 of the ORIGINAL form (upsample + 3x3, original weights).  Bound, derived and not tuned: a derived weight is the
    fp32 sum of 1, 2 or 4 fp16 weights -- exact up to a relative 2^-24 per addition, far below the next term -- rounded once to fp16: |w' - sum w| <= 2^-11 |w'|
    (half an fp16 ulp relative, 2^-11 at most), so the output moves by at most 2^-11 sum |w' x| = U16 * S' (S' from the phase operands), plus the same
    accumulation bound as above;
  * two runs give identical bits; no pixel is left unwritten (the output is poisoned first);
  * everything that is not a ping-pong convolution tile refuses the new fields.
Plan level: the SDXL UNet at a 32x32 latent (N = 2) and the tiny KL-VAE decoder at a 16x16 latent with the form forced and off: both stay under the bounds of
tests/tolerances.py against the oracle; the on / off rel-L2 is printed.  The derived weights after an on-device LoRA update equal a re-derivation from the patched weight.

Measured on MI355X (worst ratio to the bound over all cases): phase launches 0.068, assembled output 0.310 (2.0 - 2.1e-4 rel-L2 to the original form per phase);
forced / off rel-L2: UNet 5.3e-4 (1.44e-3 / 0.89e-3 against the oracle forced, 1.41e-3 / 0.87e-3 off), decoder 4.1e-4 (9.6e-4 against the oracle forced, 8.4e-4 off).
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import ref64 as R
import tolerances as T
from test_upsample_phases_cpu import derive_np

pytestmark = pytest.mark.gpu

N_IMG, W_SRC, CIN = 2, 16, 64
TILES = {18: ("128x320x64pp", 320), 20: ("128x320x64pp2", 320), 17: ("256x256x64pp", 256), 21: ("256x256x64pp2", 256)}
CASES = [(t, b, w, 4) for t in (18, 17) for b in (1, 0) for w in (0, 3)] + [(18, 1, 0, 5), (17, 1, 3, 5), (20, 1, 3, 4), (21, 0, 0, 5)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.fixture(scope="module")
def K():
    from mlimgsynth_amd import _lib, kernels
    return kernels, _lib


@pytest.fixture(scope="module")
def operands():
    """shared by every case (left unchanged): fp16 source images for H = 5 (H = 4 uses the first four rows of each), 3x3 weights of sigma 0.02, a bias"""
    rng = np.random.default_rng(2024)
    x = rng.standard_normal((N_IMG, 5, W_SRC, CIN)).astype(np.float16)
    w = (rng.standard_normal((320, 3, 3, CIN)) * 0.02).astype(np.float16)
    bias = rng.standard_normal(320).astype(np.float32) * 0.1
    return x, w, bias


phase_A = R.phase_A      # (the A operand of a phase launch: shared with the plan audit)


def phase_launch_args(kernels, x_ptr, shape, w_ptr, bias_ptr, N, tile, wrap, out_ptr, ph):
    """the arguments of phase launch ph (0 .. 3) of a case: also what the census of tests/test_plan_audit_gpu.py reads a case's form from"""
    n, H, W, C = shape
    return kernels.GemmArgs(A=x_ptr, lda=C, conv=1, n_img=n, H=H, W=W, Cin=C, OH=H, OW=W, KH=2, KW=2, stride=1, pad=1,
                            W_=w_ptr + ph * N * 4 * C * 2, ldb=4 * C, M=n * H * W, N=N, K=4 * C, bias=bias_ptr, C32=out_ptr, ldc32=N,
                            tile_variant=kernels.tile_arg(tile), wrap=wrap, tap_oy=ph >> 1, tap_ox=ph & 1, out_phase=1 + ph)


def run_phases(K, x, wdev, bias_dev, N, tile, wrap, out32):
    kernels, _lib = K
    xd = _lib.from_numpy(x)
    for ph in range(4):
        a = phase_launch_args(kernels, xd.ptr, x.shape, wdev.ptr, bias_dev, N, tile, wrap, out32.ptr, ph)
        assert kernels.gemm_variant(a) == f"gemm<{TILES[tile][0]},conv>"
        kernels.gemm(a)
    kernels.sync()


@pytest.mark.parametrize("tile,bias_on,wrap,H", CASES, ids=[f"t{t}_b{b}_w{w}_h{h}" for t, b, w, h in CASES])
def test_phase_launches_and_assembled_output_float64(K, operands, tile, bias_on, wrap, H):
    kernels, _lib = K
    x5, w_all, bias_all = operands
    N = TILES[tile][1]
    x, w, bias = np.ascontiguousarray(x5[:, :H]), np.ascontiguousarray(w_all[:N]), (bias_all[:N] if bias_on else None)
    n, M = N_IMG, N_IMG * H * W_SRC
    # the derived weights, formed on the device: the rule bit for bit
    wsrc, wdev = _lib.from_numpy(w), _lib.DeviceBuffer(16 * N * CIN * 2)
    _lib.check(_lib.lib().mlsd_ups_phase_weights(ctypes.c_void_p(wsrc.ptr), ctypes.c_void_p(wdev.ptr), N, CIN, None), "mlsd_ups_phase_weights")
    kernels.sync()
    wp = wdev.download((4, N, 4 * CIN), np.float16)
    assert np.array_equal(wp.view(np.uint16), derive_np(w).reshape(4, N, 4 * CIN).view(np.uint16))
    bias_dev = _lib.from_numpy(bias) if bias_on else None
    poison = np.full((n, 2 * H, 2 * W_SRC, N), np.nan, np.float32)
    outs = []
    for _ in range(2):
        o32 = _lib.from_numpy(poison)
        run_phases(K, x, wdev, bias_dev.ptr if bias_on else None, N, tile, wrap, o32)
        outs.append(o32.download(poison.shape, np.float32))
    got = outs[0]
    assert not np.isnan(got).any(), f"{int(np.isnan(got).any(axis=3).sum())} pixels were left unwritten"
    assert np.array_equal(got.view(np.uint32), outs[1].view(np.uint32)), "two runs differ"
    # 1. every phase launch against float64 of its own operands; 2. the assembled output against float64 of the original form
    D = R.gemm_depth(4 * CIN, R.K_STEP_MFMA16)
    A3 = R.im2col64(x.reshape(n * H * W_SRC, CIN), n, H, W_SRC, CIN, 3, 3, 1, 1, 1, 2 * H, 2 * W_SRC, wrap=wrap)
    y3 = (A3 @ w.reshape(N, 9 * CIN).astype(np.float64).T + (0 if bias is None else bias.astype(np.float64))).reshape(n, 2 * H, 2 * W_SRC, N)
    rows, cols = np.arange(M), np.arange(N)
    worst1 = worst2 = 0.0
    for ph in range(4):
        py, px = ph >> 1, ph & 1
        acc, S = R.gemm64(phase_A(x, py, px, wrap), wp[ph])
        y, b = R.gemm_epilogue64(acc, S, D, rows, cols, bias=bias)
        g = got[:, py::2, px::2, :].reshape(M, N)
        r1 = R.gemm_ratio32(g, y, b)
        r2 = R.gemm_ratio32(g, y3[:, py::2, px::2, :].reshape(M, N), R.U16 * S + b)
        worst1, worst2 = max(worst1, float(r1.max())), max(worst2, float(r2.max()))
        print(f"  phase ({py},{px}): own operands {r1.max():.3f}   original form {r2.max():.3f}   rel-L2 to the original form {rel(g, y3[:, py::2, px::2, :].reshape(M, N)):.2e}")
        assert (r1 <= 1.0).all(), f"phase {ph}: ratio {r1.max():.3g} at {np.unravel_index(int(np.argmax(r1)), r1.shape)}"
        assert (r2 <= 1.0).all(), f"phase {ph} against upsample + 3x3: ratio {r2.max():.3g} at {np.unravel_index(int(np.argmax(r2)), r2.shape)}"
    print(f"t{tile} bias {bias_on} wrap {wrap} H {H}: worst ratio own operands {worst1:.3f}, original form {worst2:.3f}")


def test_everything_else_refuses_the_new_fields(K, operands):
    kernels, _lib = K
    x5, w_all, _ = operands
    x = np.ascontiguousarray(x5[:, :4])
    xd, wd, out = _lib.from_numpy(x), _lib.from_numpy(derive_np(np.ascontiguousarray(w_all[:256]))), _lib.DeviceBuffer(N_IMG * 8 * 32 * 256 * 4)

    def args(**kw):
        a = kernels.GemmArgs(A=xd.ptr, lda=CIN, conv=1, n_img=N_IMG, H=4, W=16, Cin=CIN, OH=4, OW=16, KH=2, KW=2, stride=1, pad=1, W_=wd.ptr, ldb=4 * CIN,
                             M=N_IMG * 64, N=256, K=4 * CIN, C32=out.ptr, ldc32=256, tap_oy=1, tap_ox=0, out_phase=3)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    # whatever tile is asked for (general, stream-K, skinny, 128x160, small-Cout), a ping-pong convolution tile runs the launch: the router never offers another
    for v in (0, 1, 3, 9, 16, 19, 28, 29, 30, 31):
        assert kernels.gemm_route(args(tile_variant=kernels.tile_arg(v))).variant in TILES, v
    L = _lib.lib()
    assert L.mlsd_gemm_phase_form(ctypes.byref(args())) == 1
    # forms no ping-pong tile takes: refused, not run on another kernel
    for kw in (dict(W=8, OW=8, H=8, OH=8), dict(upsample=1), dict(stride=2), dict(act=1), dict(resid=out.ptr, ldr=256), dict(C16=out.ptr, ldc16=256), dict(out_phase=5), dict(tap_oy=2),
               dict(N=200), dict(conv=0, out_phase=0)):
        a = args(**kw)
        assert L.mlsd_gemm_phase_form(ctypes.byref(a)) == 0, kw
        with pytest.raises(_lib.MlsdError):
            kernels.gemm(a)


@pytest.fixture()
def ups_mode():
    from mlimgsynth_amd import _lib
    L = _lib.lib()
    yield L.mlsd_gemm_set_ups_phases
    L.mlsd_gemm_set_ups_phases(-1)


def n_phase_ops(ctx):
    return sum(1 for kind, _, _, _, _, a in ctx.op_records() if kind == "gemm" and a.out_phase)


def test_sdxl_unet_latent32_forced_and_off_against_the_oracle(ups_mode):
    import test_unet_gpu as TU
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(5)
    n, lat = 2, 32
    P = engine.unet_params("sdxl")
    x = rng.standard_normal((n, 4, lat, lat)).astype(np.float32) * 3
    cond = rng.standard_normal((n, 77, P.n_ctx)).astype(np.float32)
    label = rng.standard_normal((n, P.ch_adm_in)).astype(np.float32)
    sigma = np.array([7.0, 0.5], np.float32)
    got = {}
    for mode in (2, 0):
        ups_mode(mode)
        un = engine.Unet("sdxl", lat, lat, n)
        nph = n_phase_ops(un.ctx)
        assert nph == (4 if mode else 0), nph        # the 640-channel upsampling convolution (16 x 16 source); the 1280-channel one reads an 8 x 8 source: today's form
        got[mode] = un.run(x, cond, label, sigma)
        un.ctx.destroy()
    O.L().orc_set_threads(O.host_threads())
    ref, _ = TU.oracle_eval("sdxl", x, cond, label, sigma)
    e_on, e_off = [rel(got[2][i], ref[i]) for i in range(n)], [rel(got[0][i], ref[i]) for i in range(n)]
    print(f"sdxl 32x32 N=2: rel-L2 vs oracle forced {e_on}, off {e_off}; forced vs off {rel(got[2], got[0]):.3e}")
    assert np.isfinite(got[2]).all() and max(e_on) < T.EVAL_SMALL and max(e_off) < T.EVAL_SMALL


def test_tiny_vae_decoder_latent16_forced_and_off_against_the_oracle(ups_mode):
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(3)
    lat, n = 16, 1
    z = rng.standard_normal((n, 4, lat, lat)).astype(np.float32) * 0.5
    got = {}
    for mode in (2, 0):
        ups_mode(mode)
        dec = engine.Decoder("tiny", lat, lat, n)
        nph = n_phase_ops(dec.ctx)
        assert nph == (12 if mode else 0), nph       # three upsampling convolutions (16, 32, 64 wide sources); a consumer that wants fp16 gets a conversion of the finished map
        got[mode] = dec.run(z)
        dec.ctx.destroy()
    V, P = O.vae_params("tiny"), O.Params(1234)
    ref = np.stack([O.from_ot(O.L().orc_vae_decode(P.h, b"vae", V, O.to_ot(z[i:i + 1])))[0] for i in range(n)])
    e_on, e_off = rel(got[2] - 0.5, ref - 0.5), rel(got[0] - 0.5, ref - 0.5)
    print(f"tiny vae 16x16: rel-L2 vs oracle forced {e_on:.3e}, off {e_off:.3e}; forced vs off {rel(got[2], got[0]):.3e}")
    assert np.isfinite(got[2]).all() and e_on < T.EVAL and e_off < T.EVAL


def test_derived_weights_follow_a_lora_update(ups_mode):
    """mlctx_param_lora patches the loaded 3x3 weight in place; the phase weights derived from it must be those of the PATCHED weight"""
    from mlimgsynth_amd import engine, _lib
    L = engine.L()
    ups_mode(2)
    dec = engine.Decoder("tiny", 16, 16, 1)
    z = np.random.default_rng(1).standard_normal((1, 4, 16, 16)).astype(np.float32) * 0.5
    before = dec.run(z)
    L.mlctx_ups_weights.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    n_ups = L.mlctx_ups_weights(dec.ctx.h, -1, None, None, None, None)
    assert n_ups == 3
    params, devs = dec.ctx.param_list(), dec.ctx.param_devices()

    def check(i):
        pi, dev, cout, cin = ctypes.c_int(), ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        L.mlctx_ups_weights(dec.ctx.h, i, ctypes.byref(pi), ctypes.byref(dev), ctypes.byref(cout), ctypes.byref(cin))
        key, addr, nbytes = devs[pi.value]
        assert nbytes == cout.value * 9 * cin.value * 2 and key.endswith("weight")
        src, der = np.empty((cout.value, 3, 3, cin.value), np.float16), np.empty((4, cout.value, 2, 2, cin.value), np.float16)
        for arr, p in ((src, addr), (der, dev.value)):
            _lib.check(L.mlsd_memcpy(arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(p), ctypes.c_size_t(arr.nbytes), 1, None), "memcpy d2h")
        dec.ctx.sync()
        assert np.array_equal(der.view(np.uint16), derive_np(src).view(np.uint16)), key
        return key, pi.value, src
    key, pi, src0 = check(0)
    ne = params[pi][2]                                   # reference shape [3, 3, cin, cout]
    n0, n1, r = int(ne[0] * ne[1] * ne[2]), int(ne[3]), 4
    rng = np.random.default_rng(9)
    up, down = rng.standard_normal((n1, r)).astype(np.float32) * 0.05, rng.standard_normal((r, n0)).astype(np.float32) * 0.05
    f = L.mlctx_param_lora
    f.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_float]
    assert f(dec.ctx.h, key.encode(), up.ctypes.data_as(ctypes.c_void_p), down.ctypes.data_as(ctypes.c_void_p), n0, n1, r, 1.0) == 1
    _, _, src1 = check(0)
    assert not np.array_equal(src0.view(np.uint16), src1.view(np.uint16)), "the LoRA update did not change the source weight"
    for i in range(1, n_ups):
        check(i)
    after = dec.run(z)
    assert np.isfinite(after).all() and not np.array_equal(before, after)
    dec.ctx.destroy()


def test_streamed_plan_runs_the_form_and_equals_the_resident_plan(ups_mode):
    """A weight-streaming plan takes the form like the resident one (its derived weights pass through the slabs, formed on the host master): bit-identical
    evaluations, also after the upsampling convolution's weight was set again on both (the streamed master is re-derived, segments uploaded ahead are dropped)."""
    from mlimgsynth_amd import engine
    L = engine.L()
    ups_mode(2)
    n, lat = 2, 32
    res = engine.Unet("sdxl", lat, lat, n)
    st = engine.Unet("sdxl", lat, lat, n, stream_weights_mib=256)
    assert n_phase_ops(res.ctx) == 4 and n_phase_ops(st.ctx) == 4 and st.ctx.streaming_info()[0] >= 3
    L.mlctx_ups_weights.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4
    pi = ctypes.c_int()
    assert L.mlctx_ups_weights(st.ctx.h, 0, ctypes.byref(pi), None, None, None) == 1
    key, _, ne = st.ctx.param_list()[pi.value]
    P, rng = res.P, np.random.default_rng(77)
    for rep in range(3):
        x = rng.standard_normal((n, 4, lat, lat)).astype(np.float32) * 3
        cond = rng.standard_normal((n, 77, P.n_ctx)).astype(np.float32)
        label = rng.standard_normal((n, P.ch_adm_in)).astype(np.float32)
        sigma = rng.uniform(0.2, 12.0, n).astype(np.float32)
        a, b = res.run(x, cond, label, sigma), st.run(x, cond, label, sigma)
        assert np.isfinite(b).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), rep
        if rep == 0:
            w = (rng.standard_normal(tuple(reversed([int(v) for v in ne if v > 0]))) * 0.02).astype(np.float32)
            res.ctx.param_set(key, w); st.ctx.param_set(key, w)
            prev = a
        if rep == 1:
            assert not np.array_equal(a, prev)
    res.ctx.destroy(); st.ctx.destroy()
