"""ESRGAN upscaler on the GPU: mlsd_conv3x3_dense against float64 per element, the RRDBNet driver against the float64 restatement (tests/esrgan_ref.py), the context's
resident upscaler, and the hires fix with hires_use_model against its own manual composition through the public API.

Per-element bound of the kernel, u = 2^-24 (ref64.U32), on the fp16 operand values the kernel reads.  acc = sum over K = 9 Cin products, S = sum of their magnitudes:

  accumulation  |acc_gpu - acc| <= C_GEMM u D S,  D = ref64.gemm_depth(9 Cin, 32): the kernel adds one v_mfma_f32_16x16x32_f16 (32 products) per step, 9 Cin / 32
                steps in sequence (cin chunk, kh, kw), as the project's other MFMA-16 kernels are held (ref64 module docstring).
  z = acc + bias          ez = C_GEMM u D S + C_EPI u (|bias| + |z|)
  a = lrelu(z)            LeakyReLU is continuous with slope <= 1, so an argument known to +-ez gives a to +-ez even where the sign of z is misjudged; the multiply by
                          0.2f (the float, which the reference uses as well) rounds once:  ea = ez + C_EPI u |a|
  y = a scale + resid     ey = |scale| ea + C_EPI u (|a scale| + |resid| + |y|)         one multiply, one add
  y = y scale2 + resid2   ey2 = |scale2| ey + C_EPI u (|y scale2| + |resid2| + |y2|)
  C32: |got - y| <= e.   C16: ref64.gemm_ratio16, half an fp16 ulp of |y| + e on top of e.

Cases: tile geometry -- a workgroup owns 8 rows x 32 columns, a wave 2 rows, an MFMA 16 pixels -- crossed by one pixel ((9, 33), (17, 65)), below one MFMA ((1, 1), (3, 5)),
ragged in both ((17, 19)) and several tiles each way ((33, 129)); every Cin with N = 32 and the two ends with N = 64; lda = 192 with the columns >= Cin holding
fp16 infinity (7e30 rounded to fp16), which would poison every sum if read; destinations as slices of 192-wide (fp16) and 80-wide (fp32) buffers filled with a canary, the
slice of the SOURCE buffer itself included (what the driver does); two different images in one launch; the folded 2x upsample; every epilogue form.

The network is held to tolerances.EVAL per image (fp16-operand convolutional nets with fp32 summation); tests/test_upscale_cpu.py asserts in float64 that every constant
of the net moves these very outputs by more than 10 x that."""
import ctypes as C
import re

import numpy as np
import pytest

import esrgan_ref as E
import mlis_ffi as F
import ref64
import tolerances as TOL
import upscale_ffi as U

pytestmark = pytest.mark.gpu

POISON16 = np.float16(np.inf)          # 7e30 in fp16
CANARY16, CANARY32 = np.float16(-1234.0), np.float32(-7.25e11)
LD16, LD32, OFF32 = 192, 80, 8


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return U.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ 1. the kernel
def case(H, W, Cin=64, N=32, n_img=1, ups=0, lrelu=1, scale=1.0, resid=False, resid2=False, scale2=1.0, c32=True, c16=True, lda=192, inplace=False, bias=True):
    return dict(H=H, W=W, Cin=Cin, N=N, n_img=n_img, ups=ups, lrelu=lrelu, scale=scale, resid=resid, resid2=resid2, scale2=scale2, c32=c32, c16=c16, lda=lda,
                inplace=inplace, bias=bias)


def case_id(c):
    d = case(1, 1)
    return f"{c['H']}x{c['W']}-" + ",".join(f"{k}{v}" for k, v in c.items() if k not in ("H", "W") and v != d[k])


def operands(c):
    """host side of a launch: A [Min][lda] fp16 (columns >= Cin poisoned), W [N][9 Cin] fp16, bias, residuals, and the output images before the launch"""
    rng = np.random.default_rng(c["H"] * 977 + c["W"] * 31 + c["Cin"] + c["N"] + c["n_img"])
    Min = c["n_img"] * c["H"] * c["W"]
    M = Min * (4 if c["ups"] else 1)
    A = np.full((Min, c["lda"]), POISON16, np.float16)
    A[:, :c["Cin"]] = (rng.standard_normal((Min, c["Cin"])) * (1 + np.arange(Min) % 3)[:, None]).astype(np.float16)      # (images and pixels differ in scale too)
    Wt = (rng.standard_normal((c["N"], 9 * c["Cin"])) / np.sqrt(9 * c["Cin"])).astype(np.float16)
    o = dict(A=A, W=Wt, M=M, Min=Min)
    o["bias"] = (0.3 * rng.standard_normal(c["N"])).astype(np.float32) if c["bias"] else None
    o["resid"] = rng.standard_normal((M, c["N"] + 4)).astype(np.float32) if c["resid"] else None
    o["resid2"] = rng.standard_normal((M, c["N"])).astype(np.float32) if c["resid2"] else None
    return o


def launch(c, o, times=1):
    """-> (C16 image [M][LD16] or None, C32 image [M][LD32] or None, slice start of C16) after `times` launches"""
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    dA, dW = _lib.from_numpy(o["A"]), _lib.from_numpy(o["W"])
    keep = [dA, dW]
    a = K.DconvArgs(A=dA.ptr, lda=c["lda"], n_img=c["n_img"], H=c["H"], W=c["W"], Cin=c["Cin"], upsample=c["ups"], W_=dW.ptr, N=c["N"], lrelu=c["lrelu"],
                    scale=c["scale"], scale2=c["scale2"])
    for name, ld in (("bias", None), ("resid", "ldr"), ("resid2", "ldr2")):
        if o[name] is not None:
            keep.append(_lib.from_numpy(o[name]))
            setattr(a, name, keep[-1].ptr)
            if ld:
                setattr(a, ld, o[name].shape[1])
    d16 = d32 = None
    off16 = c["Cin"] if c["inplace"] else 64
    if c["c16"]:
        d16 = dA if c["inplace"] else _lib.from_numpy(np.full((o["M"], LD16), CANARY16, np.float16))
        a.C16, a.ldc16 = d16.ptr + 2 * off16, LD16
    if c["c32"]:
        d32 = _lib.from_numpy(np.full((o["M"], LD32), CANARY32, np.float32))
        a.C32, a.ldc32 = d32.ptr + 4 * OFF32, LD32
    for _ in range(times):
        K.conv3x3_dense(a)
    K.sync()
    label = K.dconv_variant(a)
    assert label == f"dconv3x3<n{c['N']},c{c['Cin']}{',up' if c['ups'] else ''}>", label
    return (d16.download((o["M"], LD16), np.float16) if d16 else None, d32.download((o["M"], LD32), np.float32) if d32 else None, off16)


def reference(c, o):
    """y and its bound e [M][N] in float64 (module docstring)"""
    f = 2 if c["ups"] else 1
    A64 = ref64.im2col64(o["A"][:, :c["Cin"]], c["n_img"], c["H"], c["W"], c["Cin"], 3, 3, 1, 1, c["ups"], f * c["H"], f * c["W"])
    acc, S = ref64.gemm64(A64, o["W"])
    u, D = ref64.U32, ref64.gemm_depth(9 * c["Cin"], ref64.K_STEP_MFMA16)
    b = np.zeros(c["N"]) if o["bias"] is None else o["bias"].astype(np.float64)
    z = acc + b[None, :]
    e = ref64.C_GEMM * u * D * S + ref64.C_EPI * u * (np.abs(b)[None, :] + np.abs(z))
    a = z
    if c["lrelu"]:
        a = np.where(z >= 0, z, float(np.float32(0.2)) * z)
        e = e + ref64.C_EPI * u * np.abs(a)
    s = float(np.float32(c["scale"]))
    r = np.zeros_like(a) if o["resid"] is None else o["resid"][:, :c["N"]].astype(np.float64)
    y = a * s + r
    e = abs(s) * e + ref64.C_EPI * u * (np.abs(a * s) + np.abs(r) + np.abs(y))
    if o["resid2"] is not None:
        s2, r2 = float(np.float32(c["scale2"])), o["resid2"].astype(np.float64)
        y2 = y * s2 + r2
        e = abs(s2) * e + ref64.C_EPI * u * (np.abs(y * s2) + np.abs(r2) + np.abs(y2))
        y = y2
    return y, e, z


def check(c, times=1):
    o = operands(c)
    y, e, z = reference(c, o)
    g16, g32, off16 = launch(c, o, times)
    N = c["N"]
    worst = {}
    if g32 is not None:
        r = ref64.gemm_ratio32(g32[:, OFF32:OFF32 + N], y, e)
        worst["C32"] = r.max()
        rest = np.delete(g32, np.s_[OFF32:OFF32 + N], axis=1)
        assert (rest.view(np.uint32) == CANARY32.view(np.uint32)).all(), "fp32 columns outside the slice were written"
    if g16 is not None:
        r = ref64.gemm_ratio16(g16[:, off16:off16 + N], y, e)
        worst["C16"] = r.max()
        before = o["A"] if c["inplace"] else np.full((o["M"], LD16), CANARY16, np.float16)
        rest, rest0 = np.delete(g16, np.s_[off16:off16 + N], axis=1), np.delete(before, np.s_[off16:off16 + N], axis=1)
        assert rest.view(np.uint16).tobytes() == rest0.view(np.uint16).tobytes(), "fp16 columns outside the slice were written"
    print(f"{case_id(c)}: worst error / bound {worst}, negative pre-activations {(z < 0).mean():.2f}")
    assert all(v <= 1.0 for v in worst.values()), worst
    return o, y, z, g16, g32


SHAPES = [(1, 1), (3, 5), (17, 19), (9, 33), (17, 65), (33, 129)]
KERNEL_CASES = (
    [case(H, W) for H, W in SHAPES]
    + [case(17, 19, Cin=ci, inplace=ci < 192) for ci in (32, 64, 96, 128, 160, 192)]
    + [case(17, 19, Cin=ci, N=64, scale=0.2, resid=True, lrelu=0) for ci in (64, 192)]
    + [case(5, 7, n_img=2, Cin=96), case(9, 33, n_img=2, N=64)]
    + [case(3, 5, ups=1, N=64, lda=64), case(17, 19, ups=1, N=64, lda=64), case(9, 17, ups=1, Cin=96)]
    + [case(9, 33, Cin=96, lrelu=0, bias=False), case(9, 33, Cin=96, lrelu=0), case(9, 33, Cin=96, lrelu=1), case(9, 33, Cin=96, lrelu=0, scale=0.2, resid=True),
       case(9, 33, Cin=96, lrelu=0, scale=0.2, resid=True, scale2=0.2, resid2=True), case(9, 33, Cin=96, lrelu=1, scale=0.5, resid=True, scale2=-1.5, resid2=True),
       case(9, 33, Cin=96, c16=False), case(9, 33, Cin=96, c32=False), case(9, 33, Cin=96, scale=0.2)])


@pytest.mark.parametrize("c", KERNEL_CASES, ids=case_id)
def test_dense_conv_against_float64(c):
    o, y, z, g16, g32 = check(c)
    assert (z < 0).any() and (z > 0).any()                     # the LeakyReLU slope is exercised (where it is on) and so is the identity branch
    if c["lrelu"]:
        assert np.abs(np.where(z >= 0, z, 0.2 * z) - z).max() > 0.05


def test_two_images_do_not_bleed():
    """the second image of a launch = the same image launched alone, bit for bit (its first row's taps must read zeros, not the first image's last row)"""
    c2 = case(5, 7, n_img=2, Cin=96)
    o2 = operands(c2)
    _, g2, _ = launch(c2, o2)
    c1 = dict(c2, n_img=1)
    o1 = dict(o2, A=np.ascontiguousarray(o2["A"][35:]), M=35, Min=35)
    _, g1, _ = launch(c1, o1)
    assert g2[35:].tobytes() == g1.tobytes()
    assert not np.array_equal(g2[:35], g2[35:])


def test_two_launches_give_the_same_bits():
    c = case(17, 65, Cin=160, N=32, scale=0.2, resid=True)
    o = operands(c)
    a16, a32, _ = launch(c, o)
    b16, b32, _ = launch(c, o, times=2)
    assert a16.tobytes() == b16.tobytes() and a32.tobytes() == b32.tobytes()


def test_argument_errors_launch_nothing(lib):
    from mlimgsynth_amd import _lib
    from mlimgsynth_amd import kernels as K
    M = 6 * 6
    dA = _lib.from_numpy(np.zeros((M, 192), np.float16))
    dW = _lib.from_numpy(np.zeros((64, 9 * 192), np.float16))
    d32 = _lib.from_numpy(np.full((M, 64), CANARY32, np.float32))
    d16 = _lib.from_numpy(np.full((M, 192), CANARY16, np.float16))

    def args(**kw):
        a = K.DconvArgs(A=dA.ptr, lda=192, n_img=1, H=6, W=6, Cin=64, upsample=0, W_=dW.ptr, N=32, lrelu=1, scale=1.0, C32=d32.ptr, ldc32=64, C16=d16.ptr, ldc16=192)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.mlsd_conv3x3_dense(C.byref(args()), None) == 0          # the base arguments are good
    K.sync()
    d32.upload(np.full((M, 64), CANARY32, np.float32)), d16.upload(np.full((M, 192), CANARY16, np.float16))
    bad = dict(cin48=args(Cin=48), cin224=args(Cin=224), cin0=args(Cin=0), n16=args(N=16), n48=args(N=48), n128=args(N=128),
               a_misaligned=args(A=dA.ptr + 2), lda_not_8=args(lda=100), lda_below_cin=args(lda=32), w_misaligned=args(W_=dW.ptr + 8),
               c32_misaligned=args(C32=d32.ptr + 4), ldc32_not_4=args(ldc32=66), c16_misaligned=args(C16=d16.ptr + 2), ldc16_not_4=args(ldc16=190),
               resid_misaligned=args(resid=d32.ptr + 8, ldr=64), no_output=args(C32=None, C16=None), upsample2=args(upsample=2), empty=args(H=0),
               c16_is_a=args(C16=dA.ptr), c16_in_read_columns=args(C16=dA.ptr + 2 * 32), c16_slice_other_stride=args(C16=dA.ptr + 2 * 64, ldc16=96),
               c16_slice_upsampled=args(C16=dA.ptr + 2 * 64, upsample=1), c16_slice_past_the_row=args(C16=dA.ptr + 2 * 176),
               c32_in_a=args(C32=dA.ptr, ldc32=96), resid_overlaps_c32=args(resid=d32.ptr + 16, ldr=64))
    for name, a in bad.items():
        assert lib.mlsd_conv3x3_dense(C.byref(a), None) != 0, name
        assert "mlsd_conv3x3_dense" in _lib.last_error(), name
        assert K.dconv_variant(a) == "dconv3x3<refused>", name
    K.sync()
    assert (d32.download((M, 64), np.float32) == CANARY32).all() and (d16.download((M, 192), np.float16) == CANARY16).all()
    assert not dA.download((M, 192), np.float16).any()
    # the slice of the source buffer beyond the columns read is NOT an alias; nor is a residual that is the fp32 output itself
    assert lib.mlsd_conv3x3_dense(C.byref(args(C16=dA.ptr + 2 * 64, resid=d32.ptr, ldr=64)), None) == 0
    K.sync()


# ------------------------------------------------------------------ 2. the network
NET_CASES = [(2, 12, 20), (1, 1, 1), (1, 7, 70)]       # as tests/test_upscale_cpu.py CASES
SPEC, SEED, BLOCKS = "synth:1234:2", 1234, 2


@pytest.fixture(scope="module")
def weights():
    return E.synth_weights(SEED, BLOCKS)


@pytest.fixture(scope="module")
def net_out(lib):
    """the synth model's outputs on the three inputs: computed once, shared, read-only"""
    up = U.Upscaler(lib, SPEC)
    try:
        assert up.n_block() == BLOCKS
        out = {}
        for n, h, w in NET_CASES:
            out[(n, h, w)] = up.run(E.test_input(n, h, w))
            out[(n, h, w)].setflags(write=False)
        return out
    finally:
        up.close()


@pytest.mark.parametrize("shape", NET_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_network_against_float64(net_out, weights, shape):
    n, h, w = shape
    got = net_out[shape]
    want = E.forward_torch(weights, E.test_input(n, h, w))
    err = E.rel_l2(got, want)
    print(f"RRDBNet {BLOCKS} blocks, {n} x {h} x {w}: per-image rel-L2 vs float64 = {err}, output rms {np.sqrt((want ** 2).mean()):.3f}")
    assert got.shape == (n, 3, 4 * h, 4 * w) and np.isfinite(got).all()
    assert (err <= TOL.EVAL).all(), err
    if n == 2:
        assert not np.array_equal(got[0], got[1])


def test_a_file_of_the_same_weights_gives_the_same_bits(lib, net_out, weights, tmp_path):
    p = str(tmp_path / "synth_rrdb.safetensors")
    E.save_safetensors(p, weights, prefix="params_ema.")
    up = U.Upscaler(lib, p)
    try:
        assert up.n_block() == BLOCKS
        for n, h, w in NET_CASES[:2]:
            assert up.run(E.test_input(n, h, w)).tobytes() == net_out[(n, h, w)].tobytes()
    finally:
        up.close()
    E.save_safetensors(p, weights, old_names=True)          # the older naming maps onto the same tensors
    up = U.Upscaler(lib, p)
    try:
        assert up.run(E.test_input(*NET_CASES[1])).tobytes() == net_out[NET_CASES[1]].tobytes()
    finally:
        up.close()


# ------------------------------------------------------------------ 3. the context's upscaler
def builds(lib, m):
    res = C.c_int(-1)
    return lib.mlis_amd_upscaler_builds(m.ctx, C.byref(res)), res.value


def test_tensor_upscale_is_the_driver_and_stays_resident(lib, net_out):
    n, h, w = NET_CASES[0]
    x = E.test_input(n, h, w)
    m = F.Mlis(lib)
    try:
        m.set("upscale_model", SPEC)
        m.set("tiling", "xy")                                   # the upscaler pads with zeros whatever the tiling
        assert builds(lib, m) == (0, 0)
        out = F.Tensor()
        assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(U.as_tensor(x)), C.byref(out)) == 1, m.err()
        assert F.tensor_np(out).tobytes() == net_out[NET_CASES[0]].tobytes()
        assert builds(lib, m) == (1, 1)
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["TMP"])         # src == dst
        lib.mlis_tensor_resize(t, w, h, 3, n)
        C.memmove(t.contents.d, x.ctypes.data, x.nbytes)
        assert lib.mlis_amd_tensor_upscale(m.ctx, t, t) == 1, m.err()
        assert F.tensor_np(t.contents).tobytes() == net_out[NET_CASES[0]].tobytes()
        m.set("upscale_model", SPEC)                            # the same value again
        assert builds(lib, m) == (1, 1)                         # a second call built nothing
        m.set("upscale_model", "synth:7:1")
        assert builds(lib, m) == (1, 0)                         # a changed model frees the resident one ...
        assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(U.as_tensor(x)), C.byref(out)) == 1, m.err()
        assert builds(lib, m) == (2, 1)                         # ... and the next use builds the new one
        assert F.tensor_np(out).tobytes() != net_out[NET_CASES[0]].tobytes()
        m.set("upscale_model", "")
        assert builds(lib, m) == (2, 0)
        assert lib.mlis_amd_tensor_upscale(m.ctx, C.byref(U.as_tensor(x)), C.byref(out)) == -4 and "upscale_model" in m.err()
        lib.mlis_tensor_free(C.byref(out))
    finally:
        m.close()
    from mlimgsynth_amd import mlimgsynth as W
    with W.MLImgSynth() as s:
        s.option_set("upscale_model", SPEC)
        y = s.upscale(W.tensor_from_numpy(x))
        assert y.n == (4 * w, 4 * h, 3, n) and y.numpy().tobytes() == net_out[NET_CASES[0]].tobytes()


# ------------------------------------------------------------------ 4. the hires fix through the model
TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NTOKS = np.array([9, 250], np.int32)
STEPS, DENOISE, HIRES_STEPS = 4, 0.6, 3


def context(lib, batch):
    m = F.Mlis(lib)
    m.set("model", "synth:tiny")
    m.set("image_dim", 64, 64)
    m.set("steps", STEPS)
    m.set("seed", 42)
    m.set("cfg_scale", 7.0)
    m.set("method", "euler_a")                 # ancestral: every step draws noise, so the Philox offsets of the two passes matter
    m.set("upscale_model", SPEC)
    if batch > 1:
        m.set("batch_size", batch)
    return m


def prompt(m):
    m.tokens(TOKS)
    m.tokens(NTOKS, negative=True)


def results(lib, m):
    return dict(latent=m.tensor(F.TENSOR["LATENT"]), image=m.tensor(F.TENSOR["IMAGE"]), info=lib.mlis_infotext_get(m.ctx, 0).decode(),
                builds=lib.mlis_amd_engine_builds(m.ctx), up_builds=builds(lib, m))


def hires(lib, batch, use_model, upscaler="bilinear"):
    m = context(lib, batch)
    try:
        m.set("hires_scale", 2), m.set("hires_denoise", DENOISE), m.set("hires_steps", HIRES_STEPS), m.set("hires_upscaler", upscaler)
        m.set("hires_use_model", use_model)
        prompt(m)
        m.generate()
        return results(lib, m)
    finally:
        m.close()


def by_hand(lib, batch, upscaler="bilinear"):
    """generate, mlis_amd_tensor_upscale, mlis_amd_tensor_resample, generate from the image: one context, so seeds and Philox offset run on as inside mlis_generate"""
    m = context(lib, batch)
    try:
        prompt(m)
        m.generate()
        t = lib.mlis_tensor_get(m.ctx, F.TENSOR["IMAGE"])
        assert tuple(t.contents.n) == (64, 64, 3, batch)
        assert lib.mlis_amd_tensor_upscale(m.ctx, t, t) == 1, m.err()
        assert tuple(t.contents.n) == (256, 256, 3, batch)
        assert lib.mlis_amd_tensor_resample(m.ctx, t, t, 128, 128, ["nearest", "bilinear", "bicubic"].index(upscaler)) == 1, m.err()
        prompt(m)
        m.set("tensor_use_flags", F.TUF["IMAGE"])
        m.set("f_t_ini", DENOISE)
        m.set("steps", HIRES_STEPS)
        m.generate()
        return results(lib, m)
    finally:
        m.close()


@pytest.mark.parametrize("batch,upscaler", [(1, "bilinear"), (2, "bicubic")])
def test_hires_with_the_model_equals_its_manual_composition(lib, batch, upscaler):
    h, man = hires(lib, batch, 1, upscaler), by_hand(lib, batch, upscaler)
    assert h["latent"].shape == (batch, 4, 16, 16) and h["image"].shape == (batch, 3, 128, 128)
    assert h["latent"].tobytes() == man["latent"].tobytes(), np.abs(h["latent"] - man["latent"]).max()
    assert h["image"].tobytes() == man["image"].tobytes(), np.abs(h["image"] - man["image"]).max()
    assert h["builds"] == 2 and man["builds"] == 2 and h["up_builds"] == (1, 1)
    assert re.search(r"Hires upscale: 2, Hires steps: 3, Hires upscaler: synth:1234:2, Denoising strength: 0.6", h["info"]), h["info"]
    plain = hires(lib, batch, 0, upscaler)
    assert plain["image"].shape == h["image"].shape and not np.array_equal(plain["image"], h["image"])
    assert f"Hires upscaler: {upscaler}" in plain["info"] and plain["up_builds"] == (0, 0)
    if batch == 2:
        assert not np.array_equal(h["image"][0], h["image"][1])
