"""Guidance limiters without a GPU: what the kernels and the public call refuse (on the dry runtime a good call gets as far as the launch), the exports, the CLI
flags, and the quantile restatement of the GPU tests against torch.quantile."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import freeu_ffi as FF
import mlis_ffi as F
from guidance_limit_ref import F32, plane_inputs, quantile_np

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mlimgsynth_amd", "bin", "mlimgsynth-amd")
cf, vp, ci, NAN, INF = C.c_float, C.c_void_p, C.c_int, float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from mlimgsynth_amd import _lib
    _lib.lib()
    l = FF.bind(_lib.LIB_PATH)
    l.mlis_amd_guidance_limit.argtypes = [vp, ci, cf, cf]
    l.mlis_amd_guidance_limit_info.argtypes = [vp, C.POINTER(ci), C.POINTER(cf), C.POINTER(cf), C.POINTER(ci), vp, ci]
    return l


BASE = dict(eps=1, ld=8, x=1, dx=1, B=2, Cn=4, HW=20, mode=1, cfg=12.0, pag=1.0, mimic=5.0, p=0.995, eta=0.5, norm=2.0, scratch=1, nb=2 * 8 * 8, out=1, vparam=0)
SHARED = [dict(eps=None), dict(B=0), dict(Cn=0), dict(HW=0), dict(ld=3), dict(cfg=NAN), dict(B=1 << 20, HW=1 << 10)]      # what mlsd_dxdt_guided refuses
STATS = SHARED + [dict(cfg=1.0), dict(out=None), dict(scratch=None)]      # (plane_select's `scratch` is its means argument)
ENTRIES = {"guidance_plane_means": ("eps ld B Cn HW cfg mimic scratch nb out", STATS + [dict(mimic=0.5), dict(mimic=NAN), dict(mimic=INF), dict(nb=8)]),
           "guidance_plane_select": ("eps ld B Cn HW cfg mimic p scratch out", STATS + [dict(mimic=0.5), dict(p=0.49), dict(p=1.01), dict(p=NAN)]),
           "guidance_apg_coef": ("eps ld B Cn HW cfg eta norm scratch nb out", STATS + [dict(eta=-0.1), dict(eta=1.1), dict(eta=NAN), dict(norm=-1.0), dict(norm=INF), dict(nb=8)]),
           "dxdt_limited": ("eps ld x dx B Cn HW mode cfg pag out vparam", SHARED + [dict(dx=None), dict(x=None, vparam=1), dict(pag=-1.0), dict(mode=0), dict(mode=3), dict(out=None)])}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_kernel_entries_refuse_before_any_launch(lib, entry):
    from mlimgsynth_amd import kernels as K
    host = np.zeros(1 << 12, np.float64)                                   # stands for every buffer: nothing reads it on the dry runtime
    lib.mlsd_runtime_dry(1)
    try:
        for kw in [{}] + ENTRIES[entry][1]:
            a = dict(BASE, **kw)
            a.update({k: host.ctypes.data if a[k] else None for k in ("eps", "x", "dx", "scratch", "out")})
            with pytest.raises(RuntimeError) as e:
                getattr(K, entry)(*[a[k] for k in ENTRIES[entry][0].split()])
            assert ("no GPU" in str(e.value)) == (not kw), (entry, kw, str(e.value))      # only the good call reaches the launch
    finally:
        lib.mlsd_runtime_dry(0)
    assert [K.guidance_limit_scratch_bytes(*s) for s in ((3, 4, 1030), (1, 1, 64), (0, 4, 64))] == [3 * 2 * 8 * 8, 3 * 8, 0]
    assert [K.guidance_select_lds_limit(n) for n in (-1, 1 << 20, 4096, 1 << 17)] == [1 << 17, 1 << 17, 1 << 17, 4096]      # (returns the previous limit)


def test_the_public_call_refuses_bad_values_and_pairs(lib):
    m = F.Mlis(lib)
    try:
        mode, a, b, n = ci(-1), cf(-1), cf(-1), ci(-1)
        info = lambda: (lib.mlis_amd_guidance_limit_info(m.ctx, C.byref(mode), C.byref(a), C.byref(b), C.byref(n), None, 0), mode.value, a.value, b.value, n.value)
        for bad in ((1, 0.5, 1.0), (1, NAN, 1.0), (1, 5.0, 0.4), (1, 5.0, 1.5), (1, 5.0, NAN), (2, -0.1, 0.0), (2, 1.5, 0.0), (2, 0.5, -1.0), (2, 0.5, INF),
                    (3, 5.0, 1.0), (-1, 0.0, 0.0)):                       # (3: both limiters at once)
            assert lib.mlis_amd_guidance_limit(m.ctx, *bad) == -4, bad
        assert info() == (0, 0, 0.0, 0.0, 0)                              # off, no engine: a refused call changes nothing
        assert lib.mlis_amd_guidance_limit(m.ctx, 2, 0.25, 3.0) == 1 and info() == (0, 2, 0.25, 3.0, 0)
        assert lib.mlis_amd_guidance_limit(m.ctx, 0, 9.0, 9.0) == 1 and info() == (0, 0, 0.0, 0.0, 0)
        m.set("cfg_rescale", 0.7)
        assert lib.mlis_amd_guidance_limit(m.ctx, 1, 5.0, 1.0) == -4 and "cfg_rescale" in m.err()
        m.set("cfg_rescale", 0)                                           # the other order is refused when the generation starts, before anything is loaded
        assert lib.mlis_amd_guidance_limit(m.ctx, 1, 5.0, 1.0) == 1
        m.set("cfg_rescale", 0.7)
        assert lib.mlis_generate(m.ctx) == -4 and "cfg_rescale" in m.err()
    finally:
        m.close()


def test_exports_and_cli(lib):
    for name in ("mlsd_guidance_plane_means", "mlsd_guidance_plane_select", "mlsd_guidance_apg_coef", "mlsd_dxdt_limited", "mlsd_guidance_limit_scratch_bytes",
                 "mlsd_guidance_select_lds_limit", "mlis_amd_set_guidance_limit", "mlis_amd_guidance_limit_state", "mlis_amd_guidance_limit", "mlis_amd_guidance_limit_info"):
        assert hasattr(lib, name), name
    run = lambda *args: subprocess.run([EXE, *args], capture_output=True, text=True, timeout=60)
    assert "--dyn-thresh MIMIC[:PERCENTILE]" in run("--help").stdout and "--apg ETA[:NORM]" in run("--help").stdout
    for args, word in ((["--dyn-thresh", "7:0.2"], "percentile"), (["--dyn-thresh", "7:"], "MIMIC[:PERCENTILE]"), (["--apg", "0", "--dyn-thresh", "7"], "exclude"),
                       (["--dyn-thresh", "7:0.995", "--apg", "x"], "ETA[:NORM]")):      # (the last: the first flag parses, the complaint is about the second)
        r = run("generate", *args)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("p", [0.5, 0.75, 0.995, 1.0])
@pytest.mark.parametrize("HW", [1, 2, 63, 4096])
def test_quantile_restatement_against_torch(HW, p):
    """torch works in float32: its position p (n - 1) is known to one float32 ulp of itself, which moves the weight by as much and the result by that times the
    gap between the two neighbours; its lerp then rounds twice, at most one ulp of the larger neighbour each.  The restatement's own error is one rounding."""
    import torch
    a = np.abs(plane_inputs(3, HW)[:3] * F32(12))
    want = torch.quantile(torch.from_numpy(a.copy()), float(F32(p)), dim=-1, interpolation="linear").numpy()
    pos, s = float(F32(p)) * (HW - 1), np.sort(a, -1).astype(np.float64)
    lo, hi = s[..., int(pos)], s[..., min(int(pos) + 1, HW - 1)]
    assert (np.abs(quantile_np(a, p).astype(np.float64) - want) <= np.spacing(F32(pos)) * (hi - lo) + 3 * np.spacing(hi.astype(F32))).all()
