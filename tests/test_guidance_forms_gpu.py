"""The guidance mix (csrc/hip/guidance.hip) on every kernel form: the two general entries mlsd_dxdt_guided / mlsd_euler_guided_update bit for bit against a numpy
fp32 restatement, the six narrow entries against the general ones, and all of them against SHA-256 digests of what the commit before the unification computed.

Bounds: none.  Every operation of the mix is an explicit _rn intrinsic, rounded once, and numpy's float32 arithmetic rounds the same way, so the bytes are equal.

Forms (guide_launch's rule): C == 4, ld % 4 == 0 and a 16-byte aligned eps take the pixel-owning kernel -- four pixels per thread (PX = 4) where HW % 4 == 0 and
x, out and noise are 16-byte aligned, else one (PX = 1) -- and everything else the element-per-thread kernel.  SHAPES holds, per form, the smallest shapes at which
it can go wrong; BIG the two shapes whose launches exceed the 4096 x 256 work items a grid is capped at, so that the grid-stride loop takes a second trip.  The
PX = 4 form would need 200 MB of eps for that and is left out: its loop statement is the same source line as the PX = 1 form's.

tests/golden/guidance_digests.json: one digest per (narrow entry, shape) over the outputs of all its cases in case order, written by record() with the library of
the commit before the unification, and one digest of all the input bytes: where that one differs the inputs changed (another numpy), not the kernels."""
import ctypes as C
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
POISON = F32(7e30)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guidance_digests.json")
SEED, PHI = 20240607, 0.7
C_OUT, C_SKIP, DT, S_UP = F32(0.31), F32(0.29), F32(-0.9), F32(0.4)
ALIGNED = (0, 0, 0, 0)
# name: C, ld, HW, offsets in floats from a 16-byte boundary of (eps, x, out, noise)
SHAPES = {
    "px4-ld4-hw4": (4, 4, 4, ALIGNED), "px4-ld8-hw4": (4, 8, 4, ALIGNED), "px4-ld4-hw1028": (4, 4, 1028, ALIGNED), "px4-ld8-hw1028": (4, 8, 1028, ALIGNED),
    "px1-hw1": (4, 4, 1, ALIGNED), "px1-hw63": (4, 8, 63, ALIGNED),
    "px1-planes-off": (4, 4, 64, (0, 1, 1, 1)), "px1-x-off": (4, 4, 64, (0, 1, 0, 0)), "px1-out-off": (4, 4, 64, (0, 0, 1, 0)), "px1-noise-off": (4, 4, 64, (0, 0, 0, 1)),
    "elem-c3": (3, 3, 101, ALIGNED), "elem-ld5": (4, 5, 101, ALIGNED), "elem-eps-off": (4, 8, 101, (1, 0, 0, 0)),
}
BIG = {"elem-big": (4, 4, 262400, (1, 0, 0, 0)), "px1-big": (4, 4, 1048832, (0, 1, 0, 0))}
MODES = ("dxdt-v0", "dxdt-v1", "euler", "euler-noise")
NARROW = ("mlsd_dxdt_cfg", "mlsd_dxdt_pag", "mlsd_dxdt_rescaled", "mlsd_euler_cfg_update", "mlsd_euler_pag_update", "mlsd_euler_rescaled_update")


def cases(name):
    """(B, cfg, pag, rescaled, mode) of a shape, in the order the digests run over"""
    if name in BIG:
        return [(1, 7.0, 1.5, True, "dxdt-v1"), (1, 7.0, 1.5, True, "euler-noise")]
    return list(itertools.product((1, 3), (0.5, 7.0), (0.0, 1.5), (False, True), MODES))


# ------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def lib():
    return bind()


def bind():
    from mlimgsynth_amd import _lib
    _lib.lib()
    l = C.CDLL(_lib.LIB_PATH)                                    # (a handle of its own: the argtypes below are this module's)
    i64, cf, vp, ci = C.c_int64, C.c_float, C.c_void_p, C.c_int
    sig = {"mlsd_dxdt_cfg": [vp, i64, vp, vp, ci, ci, ci, cf, ci, cf, cf, vp],
           "mlsd_dxdt_pag": [vp, i64, vp, vp, ci, ci, ci, cf, cf, ci, cf, cf, vp],
           "mlsd_dxdt_rescaled": [vp, i64, vp, vp, ci, ci, ci, cf, cf, vp, ci, cf, cf, vp],
           "mlsd_dxdt_guided": [vp, i64, vp, vp, ci, ci, ci, cf, cf, vp, ci, cf, cf, vp],
           "mlsd_euler_cfg_update": [vp, vp, i64, ci, ci, ci, cf, cf, vp, cf, vp],
           "mlsd_euler_pag_update": [vp, vp, i64, ci, ci, ci, cf, cf, cf, vp, cf, vp],
           "mlsd_euler_rescaled_update": [vp, vp, i64, ci, ci, ci, cf, cf, vp, cf, vp, cf, vp],
           "mlsd_euler_guided_update": [vp, vp, i64, ci, ci, ci, cf, cf, vp, cf, vp, cf, vp],
           "mlsd_guidance_stats": [vp, i64, ci, ci, ci, cf, cf, cf, vp, C.c_size_t, vp, vp]}
    for k, v in sig.items():
        if hasattr(l, k):                                        # (record() runs on a library without the general entries)
            getattr(l, k).argtypes = v
    l.mlsd_guidance_scratch_bytes.restype, l.mlsd_guidance_scratch_bytes.argtypes = C.c_size_t, [ci, ci]
    l.mlsd_last_error.restype = C.c_char_p
    return l


def dxdt(l, entry, eps, ld, x, out, B, Cn, HW, cfg, pag, fac, vparam, c_out=C_OUT, c_skip=C_SKIP):
    """one of the four dxdt entries with the arguments it takes"""
    f = getattr(l, entry)
    if entry == "mlsd_dxdt_cfg":
        return f(eps, ld, x, out, B, Cn, HW, cfg, vparam, c_out, c_skip, None)
    if entry == "mlsd_dxdt_pag":
        return f(eps, ld, x, out, B, Cn, HW, cfg, pag, vparam, c_out, c_skip, None)
    return f(eps, ld, x, out, B, Cn, HW, cfg, pag, fac, vparam, c_out, c_skip, None)


def euler(l, entry, x, eps, ld, B, Cn, HW, cfg, pag, fac, noise, dt=DT, s_up=S_UP):
    f = getattr(l, entry)
    if entry == "mlsd_euler_cfg_update":
        return f(x, eps, ld, B, Cn, HW, cfg, dt, noise, s_up, None)
    if entry == "mlsd_euler_pag_update":
        return f(x, eps, ld, B, Cn, HW, cfg, pag, dt, noise, s_up, None)
    return f(x, eps, ld, B, Cn, HW, cfg, pag, fac, dt, noise, s_up, None)


def narrow_of(pag, rescaled, mode):
    """the narrow entries that take a case: the arguments each fixes are the case's"""
    stem = ("mlsd_dxdt_%s", "mlsd_euler_%s_update")[mode.startswith("euler")]
    if rescaled:
        return [stem % "rescaled"]
    return [stem % "pag"] + ([stem % "cfg"] if pag == 0 else [])


# ------------------------------------------------------------------ inputs
class Dev:
    """a host array in device memory at `off` floats past a 16-byte boundary, one POISON float on either side"""

    def __init__(self, arr, off=0):
        from mlimgsynth_amd import _lib
        self.shape, self.off = arr.shape, off + 4                # (the front guard keeps the offset: four floats more)
        host = np.concatenate([np.full(self.off, POISON, F32), np.ascontiguousarray(arr, F32).ravel(), np.full(1, POISON, F32)])
        self.n = host.size
        self.buf = _lib.from_numpy(host)
        self.ptr = self.buf.ptr + 4 * self.off

    def get(self):
        host = self.buf.download((self.n,), F32)
        assert (host[:self.off] == POISON).all() and host[-1] == POISON, "a write outside the output"
        return host[self.off:-1].reshape(self.shape)


def poison(shape, off=0):
    return Dev(np.full(shape, POISON, F32), off)


_INPUTS = {}


def inputs(name, B):
    """the three row groups NHWC [B][HW][C] (raw UNet outputs), x and noise NCHW [B][C][HW], B factors; once per (shape, B), read-only"""
    if (name, B) not in _INPUTS:
        Cn, ld, HW, _ = {**SHAPES, **BIG}[name]
        rng = np.random.default_rng([SEED, list({**SHAPES, **BIG}).index(name), B])
        d = dict(c=(rng.standard_normal((B, HW, Cn), F32) * 2), u=(rng.standard_normal((B, HW, Cn), F32) * 2), p=(rng.standard_normal((B, HW, Cn), F32) * 2),
                 x=(rng.standard_normal((B, Cn, HW), F32) * 3), noise=rng.standard_normal((B, Cn, HW), F32), fac=rng.uniform(0.5, 1.5, B).astype(F32))
        for v in d.values():
            v.setflags(write=False)
        _INPUTS[(name, B)] = d
    return _INPUTS[(name, B)]


def eps_of(name, B, cfg, nan=()):
    """the row groups as the plan lays them out: [cond | uncond (only at cfg > 1) | perturbed], [N][HW][ld] with POISON in the padding; `nan`: groups filled with NaN"""
    Cn, ld, HW, _ = {**SHAPES, **BIG}[name]
    d = inputs(name, B)
    groups = "cup" if cfg > 1 else "cp"
    eps = np.full((len(groups) * B, HW, ld), POISON, F32)
    for i, k in enumerate(groups):
        eps[i * B:(i + 1) * B, :, :Cn] = np.nan if k in nan else d[k]
    return eps


def inputs_digest():
    h = hashlib.sha256()
    for name in list(SHAPES) + list(BIG):
        for B in sorted({c[0] for c in cases(name)}):
            d = inputs(name, B)
            for k in ("c", "u", "p", "x", "noise", "fac"):
                h.update(d[k].tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ the numpy restatement: float32 arrays and scalars, so every operation is rounded once
def guided(c, u, p, cfg, pag):
    cfg, pag = F32(cfg), F32(pag)
    g = c
    if cfg > 1:
        g = c * cfg + u * (F32(1) - cfg)
    if pag != 0:
        g = g + pag * (c - p)
    return g


def expect(name, B, cfg, pag, rescaled, mode):
    d = inputs(name, B)
    c, u, p = (np.ascontiguousarray(d[k].transpose(0, 2, 1)) for k in "cup")
    x = d["x"]
    vmap = lambda e: e * C_OUT + x * C_SKIP
    if rescaled:                                                 # the raw mix, the factor, then the v map once
        g = guided(c, u, p, cfg, pag) * d["fac"][:, None, None]
        g = vmap(g) if mode == "dxdt-v1" else g
    else:                                                        # the v map on each group, then the mix
        g = guided(vmap(c), vmap(u), vmap(p), cfg, pag) if mode == "dxdt-v1" else guided(c, u, p, cfg, pag)
    if mode.startswith("euler"):
        g = x + g * DT
        if mode == "euler-noise":
            g = g + d["noise"] * S_UP
    assert g.dtype == F32
    return g


# ------------------------------------------------------------------ running a case
class Shape:
    """the device side of one (shape, B, cfg): eps, x, noise and the factors, uploaded once"""

    def __init__(self, name, B, cfg, nan=()):
        from mlimgsynth_amd import _lib
        self.name, self.B, self.cfg = name, B, cfg
        self.Cn, self.ld, self.HW, (eo, self.xo, self.oo, no) = {**SHAPES, **BIG}[name]
        d = inputs(name, B)
        self.eps, self.x, self.noise = Dev(eps_of(name, B, cfg, nan), eo), Dev(d["x"], self.xo), Dev(d["noise"], no)
        self.fac = _lib.from_numpy(d["fac"])

    def run(self, l, entry, pag, rescaled, mode):
        from mlimgsynth_amd import _lib
        from mlimgsynth_amd import kernels as K
        B, Cn, HW = self.B, self.Cn, self.HW
        fac = self.fac.ptr if rescaled else None
        if mode.startswith("dxdt"):
            out = poison((B, Cn, HW), self.oo)
            _lib.check(dxdt(l, entry, self.eps.ptr, self.ld, self.x.ptr, out.ptr, B, Cn, HW, self.cfg, pag, fac, int(mode == "dxdt-v1")), entry)
        else:                                                    # in place: the latent is the output, at either's offset
            out = Dev(inputs(self.name, B)["x"], self.xo or self.oo)
            _lib.check(euler(l, entry, out.ptr, self.eps.ptr, self.ld, B, Cn, HW, self.cfg, pag, fac, self.noise.ptr if mode == "euler-noise" else None), entry)
        K.sync()
        return out.get()

    def factors(self, l, pag):
        from mlimgsynth_amd import _lib
        from mlimgsynth_amd import kernels as K
        nb = l.mlsd_guidance_scratch_bytes(self.B, self.HW)
        scratch, fac = _lib.DeviceBuffer(max(nb, 16)), _lib.from_numpy(np.full(self.B, POISON, F32))
        _lib.check(l.mlsd_guidance_stats(self.eps.ptr, self.ld, self.B, self.Cn, self.HW, self.cfg, pag, PHI, scratch.ptr, nb, fac.ptr, None), "mlsd_guidance_stats")
        K.sync()
        return fac.download((self.B,), F32)


def narrow_digests(l, name, check=None):
    """{entry: SHA-256 over the entry's outputs of the shape's cases, in case order}; check(shape, case, entry, bytes) sees each output"""
    hs = {e: hashlib.sha256() for e in NARROW + ("mlsd_guidance_stats",)}
    shapes = {}
    for case in cases(name):
        B, cfg, pag, rescaled, mode = case
        if (B, cfg) not in shapes:
            shapes[(B, cfg)] = s = Shape(name, B, cfg)
            for pg in sorted({c[2] for c in cases(name)}):
                hs["mlsd_guidance_stats"].update(s.factors(l, pg).tobytes())
        for entry in narrow_of(pag, rescaled, mode):
            got = shapes[(B, cfg)].run(l, entry, pag, rescaled, mode).tobytes()
            hs[entry].update(got)
            if check:
                check(shapes[(B, cfg)], case, entry, got)
    empty = hashlib.sha256().hexdigest()                         # (an entry that takes none of the shape's cases)
    return {e: h.hexdigest() for e, h in hs.items() if h.hexdigest() != empty}


def record(path=GOLDEN):
    """the golden file, from whatever library is loaded (run once, on the commit before the unification)"""
    l = bind()
    dig = {f"{e}|{name}": v for name in list(SHAPES) + list(BIG) for e, v in narrow_digests(l, name).items()}
    with open(path, "w") as f:
        json.dump(dict(numpy=np.__version__, seed=SEED, phi=PHI, inputs_sha256=inputs_digest(), digests=dig), f, indent=0, sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert inputs_digest() == g["inputs_sha256"], (f"the INPUTS changed, not the kernels: numpy {np.__version__} draws other bytes from seed {SEED} than numpy "
                                                   f"{g['numpy']}, which recorded the digests")
    return g["digests"]


# ------------------------------------------------------------------ 1. every form: general == numpy, narrow == general, narrow == the recorded parent
@pytest.mark.parametrize("name", list(SHAPES) + list(BIG))
def test_entries_bit_for_bit(lib, golden, name):
    """the general entries against numpy; each narrow entry against the general one with the arguments it fixes; the narrow entries' digests against the recorded
    ones.  BIG shapes: the second trip of the grid-stride loop (element form: 1 049 600 items; PX = 1: 1 048 832; the cap is 1 048 576)"""
    general = {}

    def check(s, case, entry, got):
        B, cfg, pag, rescaled, mode = case
        if case not in general:
            g = s.run(lib, "mlsd_dxdt_guided" if mode.startswith("dxdt") else "mlsd_euler_guided_update", pag, rescaled, mode)
            assert g.tobytes() == expect(name, B, cfg, pag, rescaled, mode).tobytes(), ("general entry against numpy", name, case)
            general[case] = g.tobytes()
        assert got == general[case], (entry, "against the general entry", name, case)

    dig = narrow_digests(lib, name, check)
    assert len(general) == len(cases(name))                      # every case has a narrow entry, so every case was checked
    want = {k.split("|")[0]: v for k, v in golden.items() if k.split("|")[1] == name}
    assert dig == want, (name, "differs from what the commit before the unification computed")


# ------------------------------------------------------------------ 2. rows a launch does not need are not read
@pytest.mark.parametrize("name", ["px4-ld8-hw1028", "px1-hw63", "px1-planes-off", "elem-ld5"])
def test_unneeded_rows_are_not_read(lib, name):
    """NaN in the B rows after the cond group at cfg = 0.5, pag = 0 (a plan's uncond or perturbed rows, whichever it put there), and in the perturbed group at
    cfg = 7, pag = 0"""
    B = 3
    for cfg, pag, nan in ((0.5, 0.0, "p"), (7.0, 0.0, "p")):
        s = Shape(name, B, cfg, nan)
        for rescaled, mode in itertools.product((False, True), MODES):
            for entry in ["mlsd_dxdt_guided" if mode.startswith("dxdt") else "mlsd_euler_guided_update"] + narrow_of(pag, rescaled, mode):
                got = s.run(lib, entry, pag, rescaled, mode)
                assert np.isfinite(got).all() and got.tobytes() == expect(name, B, cfg, pag, rescaled, mode).tobytes(), (entry, cfg, pag, rescaled, mode)
        assert np.isfinite(s.factors(lib, pag)).all()


# ------------------------------------------------------------------ 3. refusals, before any launch
def refusals(entry):
    """(what, argument overrides) the entry must refuse; pag only where the entry takes one"""
    nan = float("nan")
    r = [("NULL eps", dict(eps=None)), ("NULL out", dict(out=None)), ("B 0", dict(B=0)), ("C 0", dict(Cn=0)), ("HW 0", dict(HW=0)), ("ld < C", dict(ld=3)),
         ("cfg NaN", dict(cfg=nan)), ("2^31 elements", dict(HW=1 << 29))]
    if "dxdt" in entry:
        r.append(("NULL x with vparam", dict(x=None, vparam=1)))
    if "cfg" not in entry:
        r += [("pag < 0", dict(pag=-1.0)), ("pag NaN", dict(pag=nan))]
    if "rescaled" in entry:
        r.append(("NULL factor", dict(fac=None)))
    return r


@pytest.mark.parametrize("entry", ["mlsd_dxdt_guided", "mlsd_euler_guided_update", "mlsd_dxdt_cfg", "mlsd_euler_cfg_update", "mlsd_dxdt_pag", "mlsd_euler_pag_update",
                                   "mlsd_dxdt_rescaled", "mlsd_euler_rescaled_update"])
def test_bad_arguments_are_refused_before_any_launch(lib, entry):
    from mlimgsynth_amd import kernels as K
    name, B, cfg = "px4-ld4-hw4", 3, 7.0
    s = Shape(name, B, cfg)
    out = poison((B, 4, 4))
    for what, kw in refusals(entry):
        a = dict(eps=s.eps.ptr, ld=s.ld, x=s.x.ptr, out=out.ptr, B=B, Cn=4, HW=4, cfg=cfg, pag=1.5, fac=s.fac.ptr, vparam=0)
        a.update(kw)
        if "dxdt" in entry:
            rc = dxdt(lib, entry, a["eps"], a["ld"], a["x"], a["out"], a["B"], a["Cn"], a["HW"], a["cfg"], a["pag"], a["fac"], a["vparam"])
        else:
            rc = euler(lib, entry, a["out"], a["eps"], a["ld"], a["B"], a["Cn"], a["HW"], a["cfg"], a["pag"], a["fac"], s.noise.ptr)
        assert rc < 0 and entry in lib.mlsd_last_error().decode(), (entry, what)       # the text names the entry that was called
    K.sync()
    assert (out.get() == POISON).all()
    for d in (s.eps, s.x, s.noise):
        d.get()                                                  # (the guards of the inputs)
