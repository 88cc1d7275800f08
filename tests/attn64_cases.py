"""The cases of tests/test_attention_float64_gpu.py: every attention kernel mlsd_attention can launch, with the inputs under which a
flash-style softmax goes wrong, the operand layouts the plans use and the label `kernels.attention_variant(args)` must return, so that a
case cannot drift silently to another kernel.  Plain data and numpy: importable without a GPU (tests/test_attn64_cases_cpu.py checks every
case's label in the dry runtime and that its float64 reference is usable).

A case is a dict:
  id        test id
  variant   the label mlsd_attention_variant must return (include/mlsd_kernels.h)
  sw        switch settings the route needs, over DEFAULT_SW (mlsd_attention_sp / _x2_min_tq / _tk96 / _pp)
  nb, heads, d, Tq, Tk, causal
  layout    packed     ld = D, Q / K / V in buffers of their own
            fused_qkv  one buffer of [nb][max(Tq, Tk)][3 D] rows: Q, K, V at columns 0, D, 2 D (mlb_attn_mhead_ex's self attention)
            wide_kv    Q packed; K and V column blocks (at 32 and 32 + D) of one [nb * Tk][2 D + 64] buffer (the batched context projection)
            padded_out Q / K / V with slack between the batches, the output with ldo = D + 8
            Every layout's output has eight guard rows before and after each batch's rows (bso = (Tq + 16) ldo).
  family    sigma1 | sigma4 | sigma16 (+v100: V plus a common offset of 100): attn_operands of test_conditioning_gpu.py -- Q rows N(0, sigma^2),
            row 1 peaked (+20 on key 5), row 2 all-equal scores, row 3 with key tile 1 at -225, row Tq-2 peaked on key `late` (Tk-3; the Tk
            sweep of the one-pass kernel puts it on the last key);
            causal_traps1 | causal_traps8: the same at sigma 1 / 8 under the causal mask, plus
              row 0 sees one key;
              rows 64t+37: +20 on the diagonal key, one row in every 64-key tile;
              every row i has a masked key j >= i inside its own key tile (the tile's last key) with a score of +40 -- for i = 64m-1 that key
              is the diagonal, so those rows get a second +40 key at 64m, the first key of a tile they must not enter at all;
              row 70: the visible keys all sit 225 below the masked ones;
              rows 64m-1 / 64m: peaked on their diagonal, either side of a key-tile edge; for even m either side of a 128-row query block.
  q_scaled  the kernel rounds Q * log2(e) / sqrt(d) to fp16 before QK^T (ref64.attention_bound's q_scaled_f16 term): attn64x2s_kernel
            (attention.hip, "qf[sb][ks][j] = (_Float16)((float)qf[sb][ks][j] * p.sc)" under SP_QSCALE) and the EXPERIMENTS ping-pong kernel
            ("sc8[j] = (_Float16)((float)raw[j] * p.sc)").  attn_kernel, attn_tk96_kernel and attn64x2_kernel apply the scale to the fp32
            scores inside exp2_pair.
  path      kernel family for the worst-ratio summary

Causal cases have Tq == Tk only: the plans record no other causal launch (CLIP's self attention, csrc/host/clip.c).
"""
import zlib

import numpy as np

DEFAULT_SW = dict(sp=-1, x2=2048, tk96=1, qb=0, pp=0)
LAYOUTS = ("packed", "fused_qkv", "wide_kv", "padded_out")
GUARD_ROWS = 8
SENTINEL = 0x7C


def has_experiments():
    """the library was built with EXPERIMENTS=1; False only where it is not built at all (this module stays importable), any other failure surfaces"""
    from mlimgsynth_amd import _lib
    try:
        L = _lib.lib()
    except ImportError:           # (_lib.lib(): the shared library is missing)
        return False
    return bool(L.mlsd_has_experiments())


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------ the table
CASES = []


def case(id, variant, d, Tq, Tk, family, sw=None, causal=0, layout="packed", nb=2, heads=3, late=None, q_scaled=False):
    assert layout in LAYOUTS and all(c["id"] != id for c in CASES), id
    path = variant.split("<")[1].split(",")[0].rstrip(">") + (",causal" if causal else "")
    CASES.append(dict(id=id, variant=variant, sw=dict(sw or {}), nb=nb, heads=heads, d=d, Tq=Tq, Tk=Tk, causal=causal, layout=layout,
                      family=family, late=max(Tk - 3, 0) if late is None else late, q_scaled=q_scaled, path=path))


THREE = ("sigma1", "sigma16", "sigma4+v100")
ALL_FAMILIES = ("sigma1", "sigma4", "sigma16", "sigma1+v100", "sigma4+v100", "sigma16+v100")
SW_X2 = dict(sp=0, x2=256)        # attn64x2_kernel from Tq = 256 on
SW_X2S = dict(sp=2)               # attn64x2s_kernel from Tq = 256 on

# the tile loop: ragged query count, two block rows; 200 keys = 3 full tiles + 8, 333 = 5 full + 13; 65 = one key in the second tile
for d in (32, 80, 160):
    for Tk in (200, 333):
        for fam in THREE:
            case(f"tile_d{d}_tk{Tk}_{fam}", f"attn<tile,d{d}>", d, 200, Tk, fam)
for d in (64, 40, 32):              # (up to 96 keys the one-pass kernel takes d_head 64 and 40: the tile loop meets them with it switched off, d_head 32 always)
    for fam in THREE:
        case(f"tile_d{d}_tk65_{fam}", f"attn<tile,d{d}>", d, 200, 65, fam, sw=dict(tk96=0) if d != 32 else None)

# the causal mask: 77 = CLIP's launch, 300 crosses four 64-key and two 128-query edges
for d in (64, 32):
    for T in (77, 300):
        for s in (1, 8):
            case(f"causal_d{d}_t{T}_sigma{s}", f"attn<tile,d{d},causal>", d, T, T, f"causal_traps{s}", causal=1)

# the one-pass kernel: SD1.5's cross attention; every key-count skip condition (32-key sub-tiles, 16-key steps) from both sides; QB grouping
for d in (80, 160):
    for fam in ALL_FAMILIES:
        case(f"tk96_d{d}_{fam}", f"attn<tk96,d{d}>", d, 130, 77, fam)
for d in (40, 64, 80, 160):
    for Tk in (1, 17, 33, 65, 96):
        case(f"tk96_d{d}_tk{Tk}", f"attn<tk96,d{d}>", d, 130, Tk, "sigma4", late=Tk - 1)
for qb in (1, 2, 8):
    case(f"tk96_d80_tq1000_qb{qb}", "attn<tk96,d80>", 80, 1000, 77, "sigma4+v100", sw=dict(qb=qb))

# 64 query rows per wave: the shortest loops
for fam in THREE:
    case(f"x2_tk128_{fam}", "attn<64x2>", 64, 256, 128, fam, sw=SW_X2)
    case(f"x2s_tk128_{fam}", "attn<64x2s,d64>", 64, 256, 128, fam, sw=SW_X2S, q_scaled=True)
    case(f"x2s_d40_tk192_{fam}", "attn<64x2s,d40>", 40, 256, 192, fam, sw=SW_X2S, q_scaled=True)
for Tk in (64, 1):
    # a single key tile never reaches the 64-row kernels while the one-pass kernel is on: the label says so ...
    case(f"x2s_switches_tk{Tk}", "attn<tk96,d64>", 64, 256, Tk, "sigma16", sw=SW_X2S, late=Tk - 1)
    # ... and with it off attn64x2_kernel runs its loop once, on a full tile and on a tile of one key and 63 clamped duplicates
    case(f"x2_tk{Tk}_one_tile", "attn<64x2>", 64, 256, Tk, "sigma16", sw=dict(SW_X2, tk96=0), late=Tk - 1)

# the operand layouts of the plans, one case per kernel family and layout
for lay in ("fused_qkv", "wide_kv", "padded_out"):
    case(f"{lay}_tile_d80", "attn<tile,d80>", 80, 200, 200, "sigma4+v100", layout=lay)
    case(f"{lay}_causal_d64", "attn<tile,d64,causal>", 64, 300, 300, "causal_traps8", causal=1, layout=lay)
    case(f"{lay}_tk96_d160", "attn<tk96,d160>", 160, 130, 77, "sigma4+v100", layout=lay)
    case(f"{lay}_x2", "attn<64x2>", 64, 256, 128, "sigma4+v100", sw=SW_X2, layout=lay)
    case(f"{lay}_x2s_d40", "attn<64x2s,d40>", 40, 256, 192, "sigma4+v100", sw=SW_X2S, layout=lay, q_scaled=True)

# the rows of ATTN_KERNELS in test_conditioning_gpu.py, with their labels
SW_OLD = dict(sp=0, x2=2048)
case("cond_tile_loop", "attn<tile,d64>", 64, 512, 333, "sigma16", sw=SW_OLD)
case("cond_tile_loop_d40", "attn<tile,d40>", 40, 512, 200, "sigma16", sw=SW_OLD)
case("cond_tk96_one_pass", "attn<tk96,d64>", 64, 512, 77, "sigma16", sw=SW_OLD)
case("cond_tk96_one_pass_d40", "attn<tk96,d40>", 40, 300, 77, "sigma16", sw=SW_OLD)
case("cond_x2_lds_dma_64row", "attn<64x2>", 64, 512, 333, "sigma16", sw=SW_X2)
case("cond_attn64x2s", "attn<64x2s,d64>", 64, 512, 320, "sigma16", sw=SW_X2S, q_scaled=True)
case("cond_attn64x2s_d40", "attn<64x2s,d40>", 40, 512, 320, "sigma16", sw=SW_X2S, q_scaled=True)
if has_experiments():
    case("cond_pingpong", "attn<pp,32rows,w4>", 64, 512, 333, "sigma16", sw=dict(sp=0, x2=2048, tk96=0, pp=2), q_scaled=True)


# ------------------------------------------------------------------ switches
def apply_switches(L, sw):
    s = dict(DEFAULT_SW, **sw)
    L.mlsd_attention_sp(s["sp"]); L.mlsd_attention_x2_min_tq(s["x2"]); L.mlsd_attention_tk96(s["tk96"], s["qb"]); L.mlsd_attention_pp(s["pp"])


def restore_switches(L):
    apply_switches(L, {})


# ------------------------------------------------------------------ operands
def parse_family(fam):
    """-> (sigma, voff, causal traps)"""
    name, _, off = fam.partition("+")
    traps = name.startswith("causal_traps")
    sigma = float(name[len("causal_traps"):] if traps else name[len("sigma"):])
    assert off in ("", "v100"), fam
    return sigma, 100.0 if off else 0.0, traps


def _one_batch(rng, c):
    heads, d, Tq, Tk, late = c["heads"], c["d"], c["Tq"], c["Tk"], c["late"]
    sigma, voff, traps = parse_family(c["family"])
    assert traps == bool(c["causal"]) and Tq >= 6 and (not traps or (Tq == Tk and Tk > 70))
    nt = -(-Tk // 64)
    R = special_dims(c)                   # leading dims kept for the special rows: zero in K and in the ordinary rows of Q
    q = np.zeros((Tq, heads, d)); k = rng.standard_normal((Tk, heads, d)); v = rng.standard_normal((Tk, heads, d)) + voff
    q[:, :, R:] = rng.standard_normal((Tq, heads, d - R)) * sigma * np.sqrt(d / (d - R))
    k[:, :, :R] = 0
    s = np.sqrt(d) / 8.0                  # q = 8, k = x s: a score of x
    q[1], q[2], q[3], q[Tq - 2] = 0, 0, 0, 0
    q[1, :, 0] = 8.0; k[min(5, Tk - 1), :, 0] = 20.0 * s                     # score +20 on key 5, 0 elsewhere
    q[3, :, 1] = 30.0                                                         # -225 ...
    q[Tq - 2, :, 2] = 8.0; k[late, :, 2] = 20.0 * s                           # a late peak: the rescale of the last tile
    if not traps:
        k[64:min(128, Tk), :, 1] = -60.0 * s                                  # ... on key tile 1
        return q, k, v
    i0 = 70
    q[3] = 0; q[i0] = 0; q[i0, :, 1] = 30.0; k[:i0 + 1, :, 1] = -60.0 * s     # ... on every key row 70 sees, the masked ones at 0 (row 3: equal scores)
    for t in range(nt):
        r = 64 * t + 37
        if r < Tk:
            q[r] = 0; q[r, :, 0] = 8.0; k[r, :, 0] = 20.0 * s                 # +20 on the diagonal, one row per key tile
    for e in range(64, Tk, 64):
        q[e - 1] = 0; q[e - 1, :, 4] = 8.0; k[e, :, 4] = 40.0 * s             # row 64m-1: +40 on key 64m (masked) and on the earlier tile starts
        q[e] = 0; q[e, :, 5] = 8.0; k[e, :, 5] = 20.0 * s                     # row 64m: +20 on its diagonal, the one key of tile m it sees
    for t in range(nt):
        q[64 * t:64 * t + 64, :, 6 + t] = 8.0                                 # every row: +40 on the last key of its own key tile
        k[min(64 * t + 63, Tk - 1), :, 6 + t] = 40.0 * s
    return q, k, v


def special_dims(c):
    """the leading dims of every head that carry the special rows (the rest is Gaussian)"""
    return 6 + -(-c["Tk"] // 64) if c["causal"] else 3


def make_operands(c):
    """q [nb][Tq][D], k / v [nb][Tk][D]: float32 arrays of fp16 values"""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    D = c["heads"] * c["d"]
    ops = [_one_batch(rng, c) for _ in range(c["nb"])]
    return tuple(np.stack([f16r(o[i].reshape(o[i].shape[0], D)) for o in ops]) for i in range(3))


# ------------------------------------------------------------------ layouts
def layout(c):
    """-> dict(bufs={name: elements}, q/k/v/o=(buffer, element offset), ldq.., bsq..).  o points at the first output row of batch 0,
    GUARD_ROWS rows into its buffer."""
    nb, Tq, Tk, D, lay = c["nb"], c["Tq"], c["Tk"], c["heads"] * c["d"], c["layout"]
    ldo = D + 8 if lay == "padded_out" else D
    bso = (Tq + 2 * GUARD_ROWS) * ldo
    L = dict(ldo=ldo, bso=bso, o=("o", GUARD_ROWS * ldo), bufs={"o": nb * bso})
    if lay == "fused_qkv":
        T = max(Tq, Tk)
        L["bufs"]["qkv"] = nb * T * 3 * D
        L.update(q=("qkv", 0), k=("qkv", D), v=("qkv", 2 * D), ldq=3 * D, ldk=3 * D, ldv=3 * D, bsq=T * 3 * D, bsk=T * 3 * D, bsv=T * 3 * D)
        return L
    slack = 64 if lay == "padded_out" else 0
    L["bufs"]["q"] = nb * (Tq * D + slack)
    L.update(q=("q", 0), ldq=D, bsq=Tq * D + slack)
    if lay == "wide_kv":
        W = 2 * D + 64
        L["bufs"]["kv"] = nb * Tk * W
        L.update(k=("kv", 32), v=("kv", 32 + D), ldk=W, ldv=W, bsk=Tk * W, bsv=Tk * W)
    else:
        L["bufs"]["k"] = L["bufs"]["v"] = nb * (Tk * D + slack)
        L.update(k=("k", 0), v=("v", 0), ldk=D, ldv=D, bsk=Tk * D + slack, bsv=Tk * D + slack)
    return L


def rows_view(flat, off, ld, bs, nb, T, D):
    """the [nb][T][D] view of an operand inside its flat buffer"""
    return np.lib.stride_tricks.as_strided(flat[off:], (nb, T, D), (bs * flat.itemsize, ld * flat.itemsize, flat.itemsize))


def host_buffers(c, q, k, v):
    """{name: flat fp16 array} of the input buffers of layout(c), the operands in place, NaN everywhere else (nothing may read it)"""
    L = layout(c)
    D = c["heads"] * c["d"]
    out = {n: np.full(sz, np.nan, np.float16) for n, sz in L["bufs"].items() if n != "o"}
    for name, a, T in (("q", q, c["Tq"]), ("k", k, c["Tk"]), ("v", v, c["Tk"])):
        buf, off = L[name]
        rows_view(out[buf], off, L["ld" + name], L["bs" + name], c["nb"], T, D)[...] = a.astype(np.float16)
    return out


def attn_args(kernels, c, ptr):
    """mlsd_attn_args of the case; ptr = {buffer name: address}"""
    L = layout(c)
    at = lambda name: ptr[L[name][0]] + 2 * L[name][1]
    return kernels.AttnArgs(q=at("q"), k=at("k"), v=at("v"), out=at("o"), ldq=L["ldq"], ldk=L["ldk"], ldv=L["ldv"], ldo=L["ldo"],
                            bsq=L["bsq"], bsk=L["bsk"], bsv=L["bsv"], bso=L["bso"], n_batch=c["nb"], n_head=c["heads"], d_head=c["d"],
                            Tq=c["Tq"], Tk=c["Tk"], causal=c["causal"])

