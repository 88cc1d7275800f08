"""Real-ESRGAN compact (SRVGG) upscaler on the GPU: mlsd_conv3x3_compact against float64 per element in its three forms, the driver against the float64 net
(tests/upscale_compact_ref.py), a file against the synthetic spec, the context's calls, and the hires fix through a scale-2 model.

Per-element bound of the kernel, the one tests/test_upscale_gpu.py applies to mlsd_conv3x3_dense, from ref64: u = 2^-24, on the fp16 operand values the kernel reads,
acc = the sum over K = 9 Cin products, S = the sum of their magnitudes, D = ref64.gemm_depth(9 Cin, 32) (one v_mfma_f32_16x16x32_f16 per step, in sequence):

  z = acc + bias            ez = C_GEMM u D S + C_EPI u (|bias| + |z|)
  head, body  y = PReLU(z)  continuous with slope max(1, |slope|), the multiply rounds once:  ey = max(1, |slope|) ez + C_EPI u |y|;  C16: ref64.gemm_ratio16 (half an fp16 ulp on top)
  tail        y = z + x     ey = ez + C_EPI u (|z| + |x| + |y|);  fp32: ref64.gemm_ratio32

Shapes: a tile is 12 x 16 pixels, a wave 3 rows; 3 x 5 is below one tile; 37 x 70 is ragged on both axes and 20 tiles, which a grid of 3 persistent workgroups walks 7, 7
and 6 at a time (both patch buffers several times over); two images in one launch.  lda and ldc16 are 72 with the columns >= 64 poisoned (A) or a canary (C16).
Slopes are random in -1 .. 1 with a 0, a 1 and a -1 among them."""
import ctypes as C

import numpy as np
import pytest

import mlis_ffi as F
import ref64
import tolerances as TOL
import upscale_compact_ref as R
import upscale_ffi as U

pytestmark = pytest.mark.gpu

POISON16, CANARY16, CANARY32 = np.float16(np.inf), np.float16(-1234.0), np.float32(-7.25e11)
LD = 72
FORMS = {"head": (32, 64, 0), "body": (64, 64, 0), "tail1": (64, 3, 1), "tail2": (64, 12, 2), "tail3": (64, 27, 3), "tail4": (64, 48, 4)}


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return U.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ 1. the kernel
def operands(form, n, H, W):
    cin, cout, s = FORMS[form]
    rng = np.random.default_rng(H * 977 + W * 31 + cin + cout + n)
    M = n * H * W
    A = np.full((M, LD), POISON16, np.float16)
    A[:, :cin] = (rng.standard_normal((M, cin)) * (1 + np.arange(M) % 3)[:, None]).astype(np.float16)      # (images and pixels differ in scale too)
    Wt = np.zeros(((cout + 15) // 16 * 16, 9 * cin), np.float16)
    Wt[:cout] = (rng.standard_normal((cout, 9 * cin)) / np.sqrt(9 * cin)).astype(np.float16)
    slope = rng.uniform(-1, 1, cout).astype(np.float32)
    slope[:3] = (0.0, 1.0, -1.0)
    return dict(A=A, Wt=Wt, bias=(0.3 * rng.standard_normal(cout)).astype(np.float32), slope=None if s else slope,
                x=rng.random((n, 3, H, W)).astype(np.float32) if s else None, n=n, H=H, W=W, M=M)


def launch(form, o, grid=0, times=1):
    """the output after `times` launches: C16 image [M][LD], or the planar Y32 [n][3][sH][sW]"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    cin, cout, s = FORMS[form]
    keep = {k: _lib.from_numpy(o[k]) for k in ("A", "Wt", "bias", "slope", "x") if o[k] is not None}
    a = K.CconvArgs(A=keep["A"].ptr, lda=LD, n_img=o["n"], H=o["H"], W=o["W"], Cin=cin, Cout=cout, scale=s, W_=keep["Wt"].ptr, bias=keep["bias"].ptr, grid=grid)
    if s:
        shape, dt = (o["n"], 3, s * o["H"], s * o["W"]), np.float32
        out = _lib.from_numpy(np.full(shape, CANARY32, np.float32))
        a.X32, a.Y32 = keep["x"].ptr, out.ptr
    else:
        shape, dt = (o["M"], LD), np.float16
        out = _lib.from_numpy(np.full(shape, CANARY16, np.float16))
        a.slope, a.C16, a.ldc16 = keep["slope"].ptr, out.ptr, LD
    for _ in range(times):
        K.conv3x3_compact(a)
    K.sync()
    assert K.cconv_variant(a) == ("cconv3x3<tail,s%d>" % s if s else "cconv3x3<%s>" % form)
    return out.download(shape, dt)


def reference(form, o):
    """y and its bound e (module docstring), in the layout of the output"""
    cin, cout, s = FORMS[form]
    Wt = o["Wt"][:cout].astype(np.float64).reshape(cout, 3, 3, cin)
    y, z, S = R.layer64(o["A"][:, :cin], o["n"], o["H"], o["W"], Wt, o["bias"], o["slope"], o["x"], s)
    u, D = ref64.U32, ref64.gemm_depth(9 * cin, ref64.K_STEP_MFMA16)
    ez = ref64.C_GEMM * u * D * S + ref64.C_EPI * u * (np.abs(o["bias"].astype(np.float64))[None, :] + np.abs(z))
    if not s:
        return y, np.maximum(1.0, np.abs(o["slope"].astype(np.float64)))[None, :] * ez + ref64.C_EPI * u * np.abs(y), z
    sh = lambda v: R.shuffle64(v, o["n"], o["H"], o["W"], s)
    return y, sh(ez) + ref64.C_EPI * u * (np.abs(sh(z)) + np.abs(y - sh(z)) + np.abs(y)), z


LAYER_CASES = ([(f, 1, 3, 5, 0) for f in ("head", "body", "tail4")] + [(f, 1, 37, 70, 3) for f in FORMS] + [("body", 2, 13, 17, 0), ("tail3", 2, 13, 17, 2)])


@pytest.mark.parametrize("form,n,H,W,grid", LAYER_CASES, ids=lambda v: str(v))
def test_layer_against_float64(form, n, H, W, grid):
    o = operands(form, n, H, W)
    y, e, z = reference(form, o)
    got = launch(form, o, grid)
    if FORMS[form][2]:
        worst = ref64.gemm_ratio32(got, y, e).max()
    else:
        worst = ref64.gemm_ratio16(got[:, :64], y, e).max()
        assert (got[:, 64:].view(np.uint16) == CANARY16.view(np.uint16)).all(), "columns outside the 64 channels were written"
        assert (z < 0).mean() > 0.2 and (z > 0).mean() > 0.2                                                  # both PReLU branches
    print(f"{form} {n} x {H} x {W} grid {grid}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    if n == 2:      # neither image bleeds into the other: the second = the same image launched alone, bit for bit
        P = H * W
        alone = launch(form, dict(o, A=np.ascontiguousarray(o["A"][P:]), x=None if o["x"] is None else np.ascontiguousarray(o["x"][1:]), n=1, M=P), grid)
        second = got[1:] if FORMS[form][2] else got[P:]
        assert second.tobytes() == alone.tobytes() and not np.array_equal(got[:len(got) // 2], got[len(got) // 2:])


@pytest.mark.parametrize("form", ["body", "tail2"])
def test_two_launches_and_any_grid_give_the_same_bits(form):
    o = operands(form, 1, 37, 70)
    a = launch(form, o, grid=3)
    assert a.tobytes() == launch(form, o, grid=3, times=2).tobytes()
    assert a.tobytes() == launch(form, o, grid=0).tobytes() == launch(form, o, grid=1).tobytes()


def test_argument_errors_launch_nothing(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    M = 6 * 6
    dA, dW = _lib.from_numpy(np.zeros((M, 128), np.float16)), _lib.from_numpy(np.zeros((64, 9 * 64), np.float16))
    dB, dX = _lib.from_numpy(np.zeros(64, np.float32)), _lib.from_numpy(np.zeros((1, 3, 6, 6), np.float32))
    d16, d32 = _lib.from_numpy(np.full((M, 64), CANARY16, np.float16)), _lib.from_numpy(np.full((1, 3, 12, 12), CANARY32, np.float32))

    def args(tail=False, **kw):
        a = K.CconvArgs(A=dA.ptr, lda=128, n_img=1, H=6, W=6, Cin=64, Cout=64, W_=dW.ptr, bias=dB.ptr, slope=dB.ptr, C16=d16.ptr, ldc16=64)
        if tail:
            a.Cout, a.scale, a.slope, a.C16, a.ldc16, a.X32, a.Y32 = 12, 2, None, None, 0, dX.ptr, d32.ptr
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = dict(cin48=args(Cin=48), cin128=args(Cin=128), cout32=args(Cout=32), head_cout48=args(Cin=32, Cout=48), scale5=args(True, scale=5, Cout=75),
               tail_cout5=args(True, Cout=5), tail_cin32=args(True, Cin=32), negative_scale=args(scale=-1), empty=args(H=0), negative_grid=args(grid=-1),
               a_misaligned=args(A=dA.ptr + 2), lda_not_8=args(lda=100), lda_below_cin=args(lda=32), w_misaligned=args(W_=dW.ptr + 8), no_bias=args(bias=None),
               c16_misaligned=args(C16=d16.ptr + 8), ldc16_not_8=args(ldc16=68), ldc16_below_cout=args(ldc16=56), no_output=args(C16=None),
               c16_is_a=args(C16=dA.ptr, ldc16=128), c16_beside_the_read_columns=args(C16=dA.ptr + 128, ldc16=128), body_with_y32=args(Y32=d32.ptr),
               tail_with_c16=args(True, C16=d16.ptr, ldc16=64), tail_with_slope=args(True, slope=dB.ptr), tail_without_x=args(True, X32=None),
               y32_is_x32=args(True, Y32=dX.ptr), y32_in_a=args(True, Y32=dA.ptr))
    for name, a in bad.items():
        assert lib.mlsd_conv3x3_compact(C.byref(a), None) != 0, name
        assert "mlsd_conv3x3_compact" in _lib.last_error(), name
        assert K.cconv_variant(a) == "cconv3x3<refused>", name
    K.sync()
    assert (d16.download((M, 64), np.float16) == CANARY16).all() and (d32.download((1, 3, 12, 12), np.float32) == CANARY32).all()
    assert not dA.download((M, 128), np.float16).any() and not dX.download((1, 3, 6, 6), np.float32).any()
    for good in (args(), args(True)):
        assert lib.mlsd_conv3x3_compact(C.byref(good), None) == 0
    K.sync()


# ------------------------------------------------------------------ 2. the network
SEED, CONVS, SIZES = 7, 2, [(1, 5, 7), (2, 13, 37)]


def spec(s):
    return f"synth-compact:{SEED}:{CONVS}:{s}"


def info(up):
    nb, sc = F.ci(), F.ci()
    assert up.lib.mlis_amd_upscaler_info(up.h, C.byref(nb), C.byref(sc)) == 1
    return nb.value, sc.value


def run(up, x, s):
    """upscale_ffi.Upscaler.run for a model of scale s"""
    n, _, h, w = x.shape
    out = np.empty((n, 3, s * h, s * w), np.float32)
    fp = C.POINTER(C.c_float)
    assert up.lib.mlis_amd_upscaler_run(up.h, x.ctypes.data_as(fp), w, h, n, out.ctypes.data_as(fp)) == 1, up.lib.mlsd_last_error()
    return out


@pytest.fixture(scope="module")
def net_out(lib):
    """the synthetic models' outputs, computed once, shared, read-only"""
    out = {}
    for s in (2, 3, 4):
        up = U.Upscaler(lib, spec(s))
        try:
            assert info(up) == (CONVS, s)
            for n, h, w in SIZES:
                out[(s, n, h, w)] = run(up, R.E.test_input(n, h, w), s)
                out[(s, n, h, w)].setflags(write=False)
        finally:
            up.close()
    return out


@pytest.mark.parametrize("shape", SIZES, ids=lambda c: "%dx%dx%d" % c)
@pytest.mark.parametrize("s", [2, 3, 4])
def test_network_against_float64(net_out, s, shape):
    """held as the RRDB net is: rel-L2 per image <= tolerances.EVAL (fp16-operand convolutional nets with fp32 summation).  The float64 net with fp16-rounded
    activations is the error no engine that stores fp16 activations can avoid: the GPU is allowed twice that figure as well, the sharper of the two here
    (profiles/upscale_compact.md records both)."""
    n, h, w = shape
    x, wts = R.E.test_input(n, h, w), R.synth_weights(SEED, CONVS, s)
    got, want = net_out[(s,) + shape], R.forward64(wts, x)
    err, floor = R.E.rel_l2(got, want), R.E.rel_l2(R.forward64(wts, x, round16=True), want)
    print(f"compact net {CONVS} convs x{s}, {n} x {h} x {w}: rel-L2 vs float64 {err}, of the float64 net with fp16 activations {floor}, output rms {np.sqrt((want ** 2).mean()):.3f}")
    assert got.shape == (n, 3, s * h, s * w) and np.isfinite(got).all()
    assert (err <= TOL.EVAL).all() and (err <= 2 * floor).all(), (err, floor)
    assert R.E.rel_l2(want, np.repeat(np.repeat(x, s, 2), s, 3)).min() > 0.1           # the body moves the output: not the nearest upsample alone


# ------------------------------------------------------------------ 3. files and the public calls
def test_a_file_and_the_context_give_the_driver_s_bits(lib, net_out, tmp_path):
    s, shape = 3, SIZES[1]
    x, want = R.E.test_input(*shape), net_out[(3,) + SIZES[1]]
    p = str(tmp_path / "compact.safetensors")
    R.save_safetensors(p, R.synth_weights(SEED, CONVS, s), prefix="params_ema.")
    up = U.Upscaler(lib, p)
    try:
        assert info(up) == (CONVS, s) and run(up, x, s).tobytes() == want.tobytes()
    finally:
        up.close()
    up = U.Upscaler(lib, "synth-compact")                       # the defaults of the spec
    try:
        assert info(up) == (32, 4)
    finally:
        up.close()
    m = F.Mlis(lib)
    res = C.c_int(-1)
    try:
        m.set("upscale_model", spec(s))
        out = F.Tensor()
        for _ in range(2):
            assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(U.as_tensor(x)), C.byref(out)) == 1, m.err()
            assert tuple(out.n) == (s * shape[2], s * shape[1], 3, shape[0]) and F.tensor_np(out).tobytes() == want.tobytes()
        assert lib.mlis_amd_upscaler_builds(m.ctx, C.byref(res)) == 1 and res.value == 1          # built once, resident
        lib.mlis_tensor_free(C.byref(out))
    finally:
        m.close()
    from mlimgsynth_amd import mlimgsynth as W
    with W.MLImgSynth() as ms:
        ms.option_set("upscale_model", spec(s))
        y = ms.upscale(W.tensor_from_numpy(x))
        assert y.n == (s * shape[2], s * shape[1], 3, shape[0]) and y.numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------ 4. the hires fix through a scale-2 model
def prompt(m):
    m.tokens(np.array([5, 17, 300, 42, 7], np.int32))
    m.tokens(np.array([9, 250], np.int32), negative=True)


def generate(lib, hires):
    """64 x 64 with the hires fix at scale 2 through the model, or its composition by hand in one context (seeds and Philox offsets run on as inside mlis_generate)"""
    m = F.Mlis(lib)
    try:
        for k, v in (("model", "synth:tiny"), ("steps", 4), ("seed", 42), ("cfg_scale", 7.0), ("method", "euler_a"), ("upscale_model", spec(2))):
            m.set(k, v)
        m.set("image_dim", 64, 64)
        if hires:
            m.set("hires_scale", 2), m.set("hires_denoise", 0.6), m.set("hires_steps", 3), m.set("hires_use_model", 1)
        prompt(m)
        m.generate()
        if not hires:
            t = lib.mlis_tensor_get(m.ctx, F.TENSOR["IMAGE"])
            assert lib.mlis_amd_tensor_upscale(m.ctx, t, t) == 1, m.err()
            assert tuple(t.contents.n) == (128, 128, 3, 1)
            assert lib.mlis_amd_tensor_resample(m.ctx, t, t, 128, 128, 1) == 1, m.err()
            prompt(m)
            m.set("tensor_use_flags", F.TUF["IMAGE"]), m.set("f_t_ini", 0.6), m.set("steps", 3)
            m.generate()
        return m.tensor(F.TENSOR["LATENT"]), m.tensor(F.TENSOR["IMAGE"])
    finally:
        m.close()


def test_hires_with_a_scale_2_model_equals_its_manual_composition(lib):
    (hl, hi), (ml, mi) = generate(lib, True), generate(lib, False)
    assert hl.shape == (1, 4, 16, 16) and hi.shape == (1, 3, 128, 128)
    assert hl.tobytes() == ml.tobytes() and hi.tobytes() == mi.tobytes(), np.abs(hi - mi).max()
