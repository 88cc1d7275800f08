"""Token merging (include/mlsd_kernels.h, rules 1 to 6) restated in numpy / float64, and the bounds its tests use."""
import numpy as np

import ref64 as R64


def partition(H, W):
    """(source tokens, destination tokens), both ascending"""
    y, x = np.divmod(np.arange(H * W), W)
    d = (y % 2 == 0) & (x % 2 == 0) & (y + 1 < H // 2 * 2) & (x + 1 < W // 2 * 2)
    return np.flatnonzero(~d), np.flatnonzero(d)


def r_of(H, W, ratio):
    T, Ns = H * W, H * W - (H // 2) * (W // 2)
    return min(int(np.floor(float(np.float32(ratio)) * T)), Ns) // 16 * 16 if ratio > 0 else 0


def cosine64(n, H, W):
    """n [T][C] fp16 -> (s [Ns][Nd] float64, b [Ns][Nd] its bound: ref64's bound of a length-C fp16 dot product in MFMA steps of 32, C_GEMM u32 D S, over the norms)"""
    a = np.asarray(n, np.float64)
    src, dst = partition(H, W)
    A, B = a[src], a[dst]
    na, nb = np.sqrt((A * A).sum(1)), np.sqrt((B * B).sum(1))
    den = na[:, None] * nb[None, :]
    ok = den > 0
    s = np.where(ok, (A @ B.T) / np.where(ok, den, 1), 0.0)
    C = a.shape[1]
    b = R64.C_GEMM * R64.U32 * R64.gemm_depth(C, R64.K_STEP_MFMA16) * np.where(ok, (np.abs(A) @ np.abs(B).T) / np.where(ok, den, 1), 0.0)
    return s, b


def key(score):
    """unsigned order = the order of the floats; a NaN by its bits"""
    u = np.asarray(score, np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def select(score, best, H, W, r):
    """score, best [Ns] -> dict of int32 arrays: slot [T], kept [Ns - r], off [Nd + 1], members [r], cnt [Nd]"""
    src, dst = partition(H, W)
    Ns, Nd = len(src), len(dst)
    order = np.lexsort((np.arange(Ns), ~key(score)))      # largest key first, lower index on equal keys
    merged = np.zeros(Ns, bool)
    merged[order[:r]] = True
    kept = src[~merged]
    slot = np.empty(H * W, np.int64)
    slot[kept] = np.arange(Ns - r)
    slot[dst] = Ns - r + np.arange(Nd)
    b = np.asarray(best, np.int64)[merged]
    slot[src[merged]] = Ns - r + b
    o = np.argsort(b, kind="stable")                       # per destination, ascending source index
    cnt = np.bincount(b, minlength=Nd)
    off = np.concatenate([[0], np.cumsum(cnt)])
    return {k: np.asarray(v, np.int32) for k, v in dict(slot=slot, kept=kept, off=off, members=src[merged][o], cnt=cnt).items()}


def split_lists(flat, H, W, r):
    """one image's device lists -> the dict of select()"""
    T, Nd = H * W, (H // 2) * (W // 2)
    cuts = np.cumsum([T, T - Nd - r, Nd + 1, r, Nd])
    assert cuts[-1] == len(flat)
    return dict(zip(("slot", "kept", "off", "members", "cnt"), np.split(np.asarray(flat, np.int32), cuts[:-1])))


def merge64(n, L, H, W):
    """(merged rows [T'][C] in float64, terms of each row's mean [T']): kept rows are copies"""
    a = np.asarray(n, np.float64)
    _, dst = partition(H, W)
    rows, terms = [a[t] for t in L["kept"]], [1] * len(L["kept"])
    for j, t in enumerate(dst):
        m = L["members"][L["off"][j]:L["off"][j + 1]]
        rows.append((a[t] + a[m].sum(0)) / (1 + len(m)))
        terms.append(1 + len(m))
    return np.array(rows), np.array(terms)


def merge_bound(want, n, L, H, W, terms):
    """a mean of k fp32 terms (sum and division: at most k u32 of max|input|), then half an fp16 ulp; a copied row is exact"""
    a = np.abs(np.asarray(n, np.float64)).max()
    b32 = (terms[:, None] > 1) * terms[:, None] * R64.U32 * a
    return b32 + (terms[:, None] > 1) * R64.half_ulp16(np.abs(want) + b32)


def unmerge32(x, o, slot):
    return np.asarray(x, np.float32) + np.asarray(o, np.float32)[slot]
