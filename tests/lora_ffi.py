"""What the LoRA tests share: the prototypes of the device-side LoRA path on top of mlis_ffi's table (mlis_amd_lora_stats, the resolve / apply halves of
the host merge, the kernel launcher), a numpy restatement of the engine's parameter layouts, adapter files with kohya names, and the host merge
(mlts_lora_apply: existing code, the reference of the kernel tests) driven on one-weight files."""
import ctypes as C

import numpy as np

import mlis_ffi as F

i64, pf, pi = C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_int)
MLT_F32, MLT_F16 = 0, 1


class Entry(C.Structure):        # MLTSEntry
    _fields_ = [("name", C.c_char_p), ("dtype", C.c_int), ("n_dim", C.c_int), ("shape", i64 * 4), ("size", C.c_size_t), ("data", C.c_void_p)]


class LoraItem(C.Structure):     # MLTSLoraItem
    _fields_ = [("key", C.c_char * 600), ("down", C.POINTER(Entry)), ("up", C.POINTER(Entry)), ("n0", i64), ("n1", i64), ("n_inner", i64), ("scale", C.c_float)]


PROTOTYPES = [
    ("mlis_amd_lora_stats", F.ci, [F.vp, pi, pi, pi]),
    ("mlis_amd_engine_builds", F.ci, [F.vp]),
    ("mlts_open", F.vp, [F.cs, F.ci]),
    ("mlts_open_lora", F.vp, [F.cs]),
    ("mlts_close", None, [F.vp]),
    ("mlts_count", F.ci, [F.vp]),
    ("mlts_find", C.POINTER(Entry), [F.vp, F.cs]),
    ("mlts_entry_to_f32", F.ci, [C.POINTER(Entry), pf, i64]),
    ("mlts_lora_apply", F.ci, [F.vp, F.vp, F.cf, F.ci]),
    ("mlts_lora_resolve", F.ci, [F.vp, F.vp, F.ci, F.cf, C.POINTER(LoraItem)]),
    ("mlts_lora_operands", F.ci, [C.POINTER(LoraItem), F.ci, pf, pf]),
    ("mlsd_lora_apply", F.ci, [F.vp, F.ci, i64, i64, F.vp, F.vp, F.ci, F.cf, F.ci, i64, i64, i64, i64, i64, F.vp, F.vp]),
    ("mlsd_last_error", F.cs, []),
]
EXPORTS = [p[0] for p in PROTOTYPES] + ["mlctx_param_lora", "mlctx_param_find", "mlctx_tstore_load_key", "mlis_amd_ctx_at"]

# a name both files of a one-weight case can carry: internal in the weight file (opened without name conversion), kohya in the adapter
KEY = "unet.in.1.1.transf.0.attn1.q_proj"
KOHYA = "lora_unet_input_blocks_1_1_transformer_blocks_0_attn1_to_q"


def bind(path):
    lib = F.bind(path)
    for name, res, args in PROTOTYPES:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def stats(lib, m):
    a, b, c = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.mlis_amd_lora_stats(m.ctx, C.byref(a), C.byref(b), C.byref(c)) == 1
    return a.value, b.value, c.value


def fptr(a):
    return a.ctypes.data_as(pf)


# ------------------------------------------------------------------ the engine's parameter layouts (param_dst_index of mlblock.c)
def layout_params(layout, shape):
    """(lp0..lp4, device element count) of a weight of torch shape `shape`: 0 row-major [n1, n0]; 1 conv [cout, cin, k1, k0] with cin padded to 8;
    2 GEGLU linear [2 d, n_in]"""
    if layout == 1:
        co, ci, k1, k0 = shape
        cpad = (ci + 7) // 8 * 8
        return (k0, k1, ci, co, cpad), k0 * k1 * cpad * co
    if layout == 2:
        return (shape[1], shape[0] // 2, 0, 0, 0), shape[0] * shape[1]
    return (0, 0, 0, 0, 0), int(np.prod(shape))


def dst_index(layout, lp, n):
    i = np.arange(n, dtype=np.int64)
    if layout == 1:
        k0 = i % lp[0]; t = i // lp[0]
        k1 = t % lp[1]; t //= lp[1]
        ci, co = t % lp[2], t // lp[2]
        return ((co * lp[1] + k1) * lp[0] + k0) * lp[4] + ci
    if layout == 2:
        k, row, d = i % lp[0], i // lp[0], lp[1]
        j = np.where(row < d, row, row - d)
        return ((j >> 5) * 64 + np.where(row < d, 0, 32) + (j & 31)) * lp[0] + k
    return i


def to_device_layout(w_flat, layout, lp, n_dev):
    out = np.zeros(n_dev, w_flat.dtype)
    out[dst_index(layout, lp, w_flat.size)] = w_flat
    return out


def from_device_layout(dev, layout, lp, n):
    """(reference-order values, the padding elements)"""
    at = dst_index(layout, lp, n)
    pad = np.ones(dev.size, bool)
    pad[at] = False
    return dev[at], dev[pad]


# ------------------------------------------------------------------ files
def adapter_tensors(kohya, up, down, alpha=None, scale=None):
    t = {kohya + ".lora_down.weight": down, kohya + ".lora_up.weight": up}
    if alpha is not None:
        t[kohya + ".alpha"] = np.array(alpha, np.float32)
    if scale is not None:
        t[kohya + ".scale"] = np.array(scale, np.float32)
    return t


def kohya_name(internal, model_family="sd1"):
    """kohya key of an internal "<...>.weight"-less name, as LoRA files spell it"""
    import ckpt_names as CN
    ext = CN.external_name(internal + ".weight", model_family)[:-len(".weight")]
    for prefix, k in (("model.diffusion_model.", "lora_unet_"), ("cond_stage_model.transformer.", "lora_te_"),
                      ("conditioner.embedders.0.transformer.", "lora_te1_")):
        if ext.startswith(prefix):
            return k + ext[len(prefix):].replace(".", "_")
    return None


def host_merge(lib, wfile, adapters, wtype, key=KEY + ".weight"):
    """mlts_lora_apply of every (adapter file, mult) in turn on the one-weight file -> (fp32 values of the entry in reference order, or None and the
    error text)"""
    D = lib.mlts_open(wfile.encode(), 0)
    assert D
    try:
        for path, mult in adapters:
            L = lib.mlts_open_lora(path.encode())
            assert L, lib.mlsd_last_error()
            r = lib.mlts_lora_apply(D, L, mult, wtype)
            lib.mlts_close(L)
            if r < 0:
                return None, lib.mlsd_last_error().decode()
            assert r == 1
        e = lib.mlts_find(D, key.encode())
        n = int(np.prod([e.contents.shape[i] for i in range(4)]))
        out = np.empty(n, np.float32)
        assert lib.mlts_entry_to_f32(e, fptr(out), n) == 1
        return out, ""
    finally:
        lib.mlts_close(D)


def resolve(lib, wfile, path, mult, wtype, key=KEY + ".weight"):
    """the resolve half on the same files: (n0, n1, r, scale, up [n1, r], down [r, n0]) of the one item the adapter holds, operands as the merge reads them"""
    D, L = lib.mlts_open(wfile.encode(), 0), lib.mlts_open_lora(path.encode())
    assert D and L
    try:
        items = []
        for i in range(lib.mlts_count(L)):
            it = LoraItem()
            r = lib.mlts_lora_resolve(D, L, i, mult, C.byref(it))
            assert r >= 0, lib.mlsd_last_error()
            if r:
                up, down = np.empty((it.n1, it.n_inner), np.float32), np.empty((it.n_inner, it.n0), np.float32)
                assert lib.mlts_lora_operands(C.byref(it), wtype, fptr(up), fptr(down)) == 1
                items.append((it.key.decode(), int(it.n0), int(it.n1), int(it.n_inner), float(it.scale), up, down))
        assert len(items) == 1 and items[0][0] == key
        return items[0][1:]
    finally:
        lib.mlts_close(L)
        lib.mlts_close(D)
