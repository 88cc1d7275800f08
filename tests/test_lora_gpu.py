"""LoRA applied on the GPU to resident engines.  The kernel (mlsd_lora_apply) against the host merge it has to equal bit for bit (mlts_lora_apply on one-weight
files: existing code, not the code under test) in every device layout, and against float64; then, through the C-ABI, a context that changes its LoRA set
while its engines are resident ("warm") against fresh contexts that merge the same set on the host before anything is built ("cold"): same latents, same
images, no engine rebuilt."""
import ctypes as C

import numpy as np
import pytest

import loader_cases as LC
import lora_ffi as LF
import mlis_ffi as F

pytestmark = pytest.mark.gpu

TOKS = np.array([5, 17, 300, 42, 7], np.int32)
NEG = np.array([9, 9, 8], np.int32)


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    return LF.bind(_lib.LIB_PATH)


# ------------------------------------------------------------------ kernel
# (layout, torch shape of the weight, rank): the smallest shapes that can go wrong -- one partial tile, more than one block in both directions, a rank that is
# no multiple of the staging chunk and one of several chunks, a padded conv, a pointwise conv, GEGLU with one and with one and a half 64-row groups per half
SHAPES = [(0, (5, 7), 1), (0, (40, 72), 4), (0, (130, 257), 3), (0, (130, 257), 128),
          (1, (6, 5, 3, 3), 2), (1, (24, 16, 1, 1), 4), (2, (128, 40), 4), (2, (192, 40), 4)]
IDS = ["5x7r1", "40x72r4", "130x257r3", "130x257r128", "conv3x3cin5", "conv1x1", "geglu64", "geglu96"]


def write_weight(tmp_path, shape, dtype, rng, name="w.safetensors"):
    from safetensors.numpy import save_file
    w = (rng.standard_normal(shape) * 0.1).astype(dtype)
    save_file({LF.KEY + ".weight": w}, str(tmp_path / name))
    return str(tmp_path / name), w


def write_adapter(tmp_path, name, shape, r, rng, dtype=np.float16, alpha=None, scale=None, edit=None):
    from safetensors.numpy import save_file
    conv = len(shape) == 4
    down = (rng.standard_normal((r,) + tuple(shape[1:])) * 0.2).astype(dtype)
    up = (rng.standard_normal((shape[0], r) + ((1, 1) if conv else ())) * 0.2).astype(dtype)
    if edit:
        edit(up, down)
    save_file(LF.adapter_tensors(LF.KOHYA, up, down, alpha, scale), str(tmp_path / name))
    return str(tmp_path / name)


def device_merge(lib, wfile, w, layout, adapters, wtype):
    """the weight in its device layout and type, every adapter applied by the kernel -> (values in reference order, padding elements, flags)"""
    import torch
    f16 = wtype == LF.MLT_F16
    lp, n_dev = LF.layout_params(layout, w.shape)
    dev = LF.to_device_layout(w.reshape(-1).astype(np.float16 if f16 else np.float32), layout, lp, n_dev)
    W = torch.from_numpy(dev).cuda()
    flags = []
    for path, mult in adapters:
        n0, n1, r, scale, up, down = LF.resolve(lib, wfile, path, mult, wtype)
        U, D, flag = torch.from_numpy(up).cuda(), torch.from_numpy(down).cuda(), torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.mlsd_lora_apply(W.data_ptr(), 1 if f16 else 0, n0, n1, U.data_ptr(), D.data_ptr(), r, scale, layout, *lp, flag.data_ptr(), None)
        assert rc == 0, lib.mlsd_last_error()
        torch.cuda.synchronize()
        flags.append(int(flag.item()))
    got, pad = LF.from_device_layout(W.cpu().numpy(), layout, lp, w.size)
    return got.astype(np.float32), pad, flags


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("wtype", [LF.MLT_F16, LF.MLT_F32], ids=["f16", "f32"])
@pytest.mark.parametrize("layout,shape,r", SHAPES, ids=IDS)
def test_kernel_equals_the_host_merge(lib, tmp_path, layout, shape, r, wtype):
    rng = np.random.default_rng(hash((layout, shape, r)) % 2**32)
    dt = np.float16 if wtype == LF.MLT_F16 else np.float32
    wfile, w = write_weight(tmp_path, shape, dt, rng)
    ad = [(write_adapter(tmp_path, "a.safetensors", shape, r, rng, dt, alpha=2.0), 0.75)]
    ref, err = LF.host_merge(lib, wfile, ad, wtype)
    assert ref is not None, err
    got, pad, flags = device_merge(lib, wfile, w, layout, ad, wtype)
    assert flags == [0]
    assert same_bits(got, ref), np.abs(got - ref).max()
    assert not same_bits(got, w.reshape(-1).astype(np.float32))           # (the adapter did something)
    assert pad.size == LF.layout_params(layout, shape)[1] - w.size and not pad.any()      # padding elements are never written


def test_kernel_outlier_scale_alpha_and_stacking(lib, tmp_path):
    """a 1e4 outlier in up; the adapter's own `scale` tensor (it wins over alpha); two adapters stacked on one weight (F16 rounds between them)"""
    rng = np.random.default_rng(7)
    shape, r = (130, 257), 3
    wfile, w = write_weight(tmp_path, shape, np.float16, rng)

    def outlier(up, down):
        up[77, 1] = 1e4
        down *= 0.05
    a = write_adapter(tmp_path, "a.safetensors", shape, r, rng, alpha=1.5, edit=outlier)
    b = write_adapter(tmp_path, "b.safetensors", shape, r + 2, rng, alpha=9.0, scale=0.3)
    c = write_adapter(tmp_path, "c.safetensors", shape, r, rng)                     # neither: scale 1
    for ads in ([(a, 1.0)], [(b, 0.6)], [(c, 0.5)], [(a, 0.4), (b, 0.8)], [(b, 0.8), (a, 0.4)]):
        ref, err = LF.host_merge(lib, wfile, ads, LF.MLT_F16)
        assert ref is not None, err
        got, pad, flags = device_merge(lib, wfile, w, 0, ads, LF.MLT_F16)
        assert same_bits(got, ref) and not any(flags), ads
    assert LF.resolve(lib, wfile, b, 0.6, LF.MLT_F16)[3] == np.float32(0.3) * np.float32(0.6)
    assert LF.resolve(lib, wfile, a, 1.0, LF.MLT_F16)[3] == np.float32(1.5) / np.float32(r)


@pytest.mark.parametrize("wtype", [LF.MLT_F16, LF.MLT_F32], ids=["f16", "f32"])
@pytest.mark.parametrize("layout,shape,r", [SHAPES[3], SHAPES[4], SHAPES[7]], ids=[IDS[3], IDS[4], IDS[7]])
def test_kernel_against_float64(lib, tmp_path, layout, shape, r, wtype):
    """Guards against the host merge and the kernel sharing a mistake.  v = w + s sum_k u_k d_k in float64 from the operands the merge reads.  In fp32, with
    u = 2^-24: every product is rounded once and the r-term sum takes r - 1 additions, the scaling one more rounding -- |error of s delta| <= gamma(r + 1) |s|
    sum_k |u_k d_k|, gamma(n) = n u / (1 - n u); the final addition rounds once more, u times the value it computed.  An F16 weight adds one rounding to 11
    bits, 2^-11 times the fp32 value, or half a subnormal step, 2^-25.  Nothing here is fitted to what the kernel returns."""
    rng = np.random.default_rng(11)
    dt = np.float16 if wtype == LF.MLT_F16 else np.float32
    wfile, w = write_weight(tmp_path, shape, dt, rng)
    ad = write_adapter(tmp_path, "a.safetensors", shape, r, rng, dt, alpha=3.0)
    n0, n1, r_, s, up, down = LF.resolve(lib, wfile, ad, 0.75, wtype)
    got, _, flags = device_merge(lib, wfile, w, layout, [(ad, 0.75)], wtype)
    w64 = w.reshape(n1, n0).astype(np.float64)
    v = w64 + float(s) * (up.astype(np.float64) @ down.astype(np.float64))
    u = 2.0 ** -24
    gamma = (r + 1) * u / (1 - (r + 1) * u)
    tol = gamma * abs(float(s)) * (np.abs(up).astype(np.float64) @ np.abs(down).astype(np.float64))
    tol = tol + u * (np.abs(v) + tol)                           # the final addition rounds the value it computed, |v| + what it is off by at most
    if wtype == LF.MLT_F16:
        tol = tol + 2.0 ** -11 * (np.abs(v) + tol) + 2.0 ** -25
    err = np.abs(got.reshape(n1, n0).astype(np.float64) - v)
    print("float64: max err / tol", (err / tol).max())
    assert flags == [0] and (err <= tol).all()


def test_kernel_flags_a_non_finite_result_and_refuses_bad_arguments(lib, tmp_path):
    import torch
    rng = np.random.default_rng(3)
    shape, r = (40, 72), 4
    wfile, w = write_weight(tmp_path, shape, np.float32, rng)

    def poison(up, down):
        up[13, 2] = np.inf
    bad = write_adapter(tmp_path, "bad.safetensors", shape, r, rng, np.float32, edit=poison)
    ref, err = LF.host_merge(lib, wfile, [(bad, 1.0)], LF.MLT_F32)
    assert ref is None and err == "NaN in LoRA result"
    _, _, flags = device_merge(lib, wfile, w, 0, [(bad, 1.0)], LF.MLT_F32)
    assert flags == [1]
    W, U, D = torch.zeros(40 * 72, device="cuda"), torch.zeros(40 * 4, device="cuda"), torch.zeros(4 * 72, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = dict(W=W.data_ptr(), dtype=0, n0=72, n1=40, up=U.data_ptr(), down=D.data_ptr(), r=4, scale=1.0, layout=0, lp=(0, 0, 0, 0, 0), flag=flag.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mlsd_lora_apply(a["W"], a["dtype"], a["n0"], a["n1"], a["up"], a["down"], a["r"], a["scale"], a["layout"], *a["lp"], a["flag"], None)
    assert call() == 0
    for kw in (dict(r=0), dict(r=-3), dict(n0=0), dict(n1=0), dict(n1=-1), dict(W=None), dict(up=None), dict(down=None), dict(flag=None), dict(layout=3),
               dict(layout=7), dict(dtype=2), dict(dtype=-1), dict(layout=1, lp=(3, 3, 5, 6, 8)), dict(layout=1, lp=(1, 1, 72, 40, 64)),
               dict(layout=2, lp=(72, 20, 0, 0, 0)), dict(layout=2, lp=(72, 32, 0, 0, 0))):
        assert call(**kw) < 0, kw
    torch.cuda.synchronize()
    assert not W.any().item() and flag.item() == 0


# ------------------------------------------------------------------ warm equals cold, through the C-ABI
RANK = 4


def targets_of(model):
    """adapter targets by role: self and cross attention, both feed-forward linears (GEGLU and plain), a 3x3 conv and a projection the name conversion
    reaches, text-tower linears (both towers of the XL model)"""
    params = {k: shape for k, f16, shape in LC.model_params(model) if f16 and k.endswith(".weight")}
    first = lambda suffix, prefix="unet.": next(k for k in params if k.startswith(prefix) and k.endswith(suffix))
    t = [first("attn1.q_proj.weight"), first("attn2.k_proj.weight"), first("ff.net.0.proj.weight"), first("ff.net.2.weight"), first("attn2.out_proj.weight"),
         first("in.1.0.conv1.weight"), first("proj_in.weight"), first("layers.1.attn.v_proj.weight", "clip."), first("layers.0.mlp.fc1.weight", "clip.")]
    if model == "tinyxl":
        t += [first("layers.0.attn.q_proj.weight", "clip2."), first("layers.1.mlp.fc2.weight", "clip2.")]
    return [(k[:-len(".weight")], params[k]) for k in t]


def kohya_of(internal, model):
    fam = "sd1" if model == "tiny" else "sdxl"
    for pre, te in (("clip.text.", "te" if fam == "sd1" else "te1"), ("clip2.text.", "te2")):
        if internal.startswith(pre):
            return "lora_%s_text_model_" % te + internal[len(pre):].replace(".attn.", ".self_attn.").replace(".", "_")
    return LF.kohya_name(internal, fam)


def write_model_adapter(path, model, seed, which=None, edit=None):
    from safetensors.numpy import save_file
    rng = np.random.default_rng(seed)
    tensors = {}
    for i, (t, shape) in enumerate(targets_of(model)):
        if which is not None and i not in which:
            continue
        shp = LC.squeeze_shape(shape) if not (shape[-1] <= 3 and shape[-2] <= 3 and shape[0] > 1) else shape
        conv = len(shp) == 4
        down = (rng.standard_normal((RANK,) + tuple(shp[1:])) * 0.25).astype(np.float16)
        up = (rng.standard_normal((shp[0], RANK) + ((1, 1) if conv else ())) * 0.25).astype(np.float16)
        if edit:
            up, down = edit(t, up, down)
        tensors.update(LF.adapter_tensors(kohya_of(t, model), up, down, alpha=2.0 + i % 3))
    save_file(tensors, path)


def write_tae(path):
    """a TAESD file (bare names, as distributed) holding the synthetic rule's values"""
    import ctypes
    from mlimgsynth_amd import _lib, engine
    from safetensors.numpy import save_file
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    try:
        l = engine._proto2()
        out = {}
        for init, build, a in ((l.sdtae_decode_init, l.sdtae_decode_build, 8),):
            ctx, t = engine.MLCtx(), engine.vp()
            engine.check1(init(ctx.h, a, a, 1, ctypes.byref(t)), "init")
            engine.check1(build(ctx.h, t), "build")
            for k, ty, ne in ctx.param_list():
                shape = tuple(int(d) for d in ne[::-1])
                v = LC.synth_values(k, shape, ty == 1)
                out[k[len("tae."):]] = v.reshape(shape if len(shape) == 4 and shape[0] > 1 else LC.squeeze_shape(shape))
            ctx.destroy()
        save_file(out, path)
    finally:
        L.mlsd_runtime_dry(0)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("lora")
    (d / "loras").mkdir()
    f = dict(dir=str(d), loras=str(d / "loras"))
    for model in ("tiny", "tinyxl"):
        f[model] = str(d / (model + ".safetensors"))
        LC.write_checkpoint(f[model], model, "F16")
        sub = d / "loras" / model
        sub.mkdir()
        write_model_adapter(str(sub / "style.safetensors"), model, 21)
        write_model_adapter(str(sub / "second.safetensors"), model, 22, which=(0, 2, 3, 5, 7))
    sub = d / "loras" / "tiny"

    def poison(t, up, down):
        if t.endswith("ff.net.2"):
            up = up.copy(); up[3, 1] = np.inf
        return up, down

    def misshape(t, up, down):
        return (up[:-1] if t.endswith("attn2.k_proj") else up), down
    write_model_adapter(str(sub / "poison.safetensors"), "tiny", 23, which=(0, 3, 7), edit=poison)
    write_model_adapter(str(sub / "misshape.safetensors"), "tiny", 24, which=(0, 1, 7), edit=misshape)
    f["tae"] = str(d / "tae.safetensors")
    write_tae(f["tae"])
    return f


def configure(m, files, model, opts):
    m.set("model_type", model)
    m.set("lora_dir", files["loras"] + "/" + model)
    m.set("model", files[model])
    m.set("image_dim", 64, 64)
    m.set("steps", 3)
    m.set("method", "euler_a")
    m.set("cfg_scale", 7.0)
    for k, v in opts:
        m.set(k, *v) if isinstance(v, tuple) else m.set(k, v)


def generate(lib, m, loras=(), prompt_loras=()):
    """one generation from seed 42 with the option list `loras` and the prompt's `prompt_loras`: (latent, image of every batch element)"""
    m.set("lora_clear", "")
    for name, mult in loras:
        m.set("lora", name, mult)
    m.set("seed", 42)
    if prompt_loras:
        m.set("prompt", "".join("<lora:%s:%s>" % nm for nm in prompt_loras))       # no text is left: no vocabulary needed
    m.tokens(TOKS)
    m.tokens(NEG, negative=True)
    m.generate()
    lat = m.tensor(F.TENSOR["LATENT"])
    return lat, [m.image(i) for i in range(lat.shape[0])]


_cold = {}


def cold(lib, files, model, opts, loras, n_prior=0):
    """The same configuration in a fresh context, which merges on the host before it builds anything (computed once per configuration).  A context's Philox
    streams run on from one generation to the next whatever the seed option says, so the generation that is compared is the fresh context's (n_prior + 1)-th,
    all of them with the same LoRA list: the same point of the streams as the warm context's, reached without ever changing a resident weight."""
    key = (model, opts, tuple(loras), n_prior)
    if key not in _cold:
        m = F.Mlis(lib)
        try:
            configure(m, files, model, opts)
            for _ in range(n_prior):
                generate(lib, m, loras)
            _cold[key] = generate(lib, m, loras)
            assert LF.stats(lib, m) == (0, 0, len(loras))
        finally:
            m.close()
    return _cold[key]


class Warm:
    """one long-lived context and the number of generations it has completed"""

    def __init__(self, lib, files, model, opts):
        self.lib, self.files, self.model, self.opts, self.n = lib, files, model, opts, 0
        self.m = F.Mlis(lib)
        configure(self.m, files, model, opts)

    def gen(self, loras=(), prompt_loras=()):
        out = generate(self.lib, self.m, loras, prompt_loras)
        self.n += 1
        return out

    def equals_cold(self, loras=(), prompt_loras=(), opts=None):
        want = cold(self.lib, self.files, self.model, self.opts if opts is None else opts, tuple(loras) + tuple(prompt_loras), self.n)
        return same(self.gen(loras, prompt_loras), want)

    def builds(self):
        return self.lib.mlis_amd_engine_builds(self.m.ctx)

    def stats(self):
        return LF.stats(self.lib, self.m)


def same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


SEQ = [(), (("style", 0.75),), (("style", 0.4),), ()]
CONFIGS = {
    "tiny": ("tiny", ()),
    "tinyxl": ("tinyxl", ()),
    "two_adapters": ("tiny", ()),
    "hires": ("tiny", (("hires_scale", 1.5), ("hires_steps", 2), ("hires_denoise", 0.6))),
    "unet_split": ("tiny", (("unet_split", "1"),)),
    "tae": ("tiny", (("tae", "TAE"),)),
    "batch2": ("tiny", (("batch_size", 2),)),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_warm_sequence_equals_cold_contexts(lib, files, name):
    model, opts = CONFIGS[name]
    opts = tuple((k, files["tae"] if v == "TAE" else v) for k, v in opts)
    seq = [(), (("style", 0.75), ("second", 0.5)), (("second", 0.5), ("style", 0.75)), (("style", 0.3),), ()] if name == "two_adapters" else SEQ
    builds = 2 if name == "hires" else 1
    w = Warm(lib, files, model, opts)
    try:
        prev = (0, 0, 0)
        for i, loras in enumerate(seq):
            assert w.equals_cold(loras), (name, i, loras)
            assert w.builds() == builds, (name, i)
            st = w.stats()
            assert st[2] == 0                                               # nothing was merged on the host after the first load
            if i:
                assert st[1] > prev[1] if loras else st[1] == prev[1]       # adapters were patched in
                assert st[0] > prev[0] if seq[i - 1] else st[0] == prev[0]  # what the previous set patched was restored
            prev = st
        assert not same(cold(lib, files, model, opts, seq[1], 1), cold(lib, files, model, opts, (), 1))          # (the adapters change the image)
        assert not same(cold(lib, files, model, opts, seq[1], 1), cold(lib, files, model, opts, seq[2], 1))     # (and so do their multipliers / order)
    finally:
        w.m.close()


def test_prompt_lora_twice_costs_nothing_the_second_time(lib, files):
    w = Warm(lib, files, "tiny", ())
    try:
        assert w.equals_cold()
        for mult in (0.75, 0.4):
            assert w.equals_cold(prompt_loras=(("style", mult),))
            st = w.stats()
            assert w.equals_cold(prompt_loras=(("style", mult),))
            assert w.stats() == st                                           # the same set two generations running: nothing restored, nothing patched
        assert w.equals_cold()
        assert w.builds() == 1 and w.stats()[2] == 0
    finally:
        w.m.close()


def test_cold_start_with_an_adapter_then_warm_changes(lib, files):
    """the first load merges on the host; later changes patch the resident plans, and a size built afterwards gets the same weights"""
    w = Warm(lib, files, "tiny", ())
    try:
        assert w.equals_cold((("style", 0.75),))
        assert w.stats() == (0, 0, 1)
        assert w.equals_cold((("style", 0.4),))
        st = w.stats()
        assert st[0] > 0 and st[1] > 0 and st[2] == 1 and w.builds() == 1
        w.m.set("batch_size", 2)                                             # a third engine while the adapter is active: loaded, then patched
        assert w.equals_cold((("style", 0.4),), opts=(("batch_size", 2),))
        assert w.builds() == 2 and w.stats()[2] == 1
    finally:
        w.m.close()


@pytest.mark.parametrize("bad,text", [("misshape", "lora up/down invalid shapes"), ("poison", "NaN in LoRA result"), ("missing", "not found")])
def test_failure_leaves_a_correct_context(lib, files, bad, text):
    w = Warm(lib, files, "tiny", ())
    try:
        assert w.equals_cold((("style", 0.75),))
        if bad == "missing":
            assert lib.mlis_option_set_str(w.m.ctx, b"lora", b"does_not_exist,1") == -6 and text in w.m.err()
        else:
            with pytest.raises(RuntimeError, match=text):
                generate(lib, w.m, (("style", 0.4), (bad, 1.0)))            # fails in mlis_setup: nothing is sampled, the Philox streams stay put
        assert w.equals_cold()
        assert w.equals_cold((("style", 0.4),))
        assert w.builds() == 1
    finally:
        w.m.close()
