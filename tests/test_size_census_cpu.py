"""The op-form census beyond the bench sizes, in the dry runtime (no GPU).

tests/plan_audit.py SIZE_PLANS lists plans at ordinary sizes nobody tuned: the SD1.5 UNet at 64x64 with N = 1, 3, 4, 6, 8, at 64x96, 96x64, 96x96, 72x88, 88x72
and 40x40; the SDXL UNet at 128x128 with N = 1, 2, 3, 4, 6, at 104x152 (N = 2 and 8), 152x104, 112x144, 168x96, 96x96, 64x64, 120x136, 100x100 and at the bench size
with a 154-token context; the KL-VAE decoders at 96 (sd1), 128, 96 (two images) and 100 (sdxl), the encoders at 128 (sdxl) and 64 (sd1), and TAESD both ways at 64.
Each is built (never computed) and the census key of every op -- kind, GEMM tile and split form or attention kernel, epilogue features -- must be HELD: met in an
audited plan of tests/test_plan_audit_gpu.py, in a bench plan (whose forms that file's own census holds), or listed in its COVERED_ELSEWHERE with the float64 case of
exactly that form.  The same rule runs on the device in test_plan_audit_gpu.py; there the device answers for its CUs, here the dry runtime's defaults do.

Latents that do not halve evenly down the UNet's levels are refused when the plan is built, and leave no plan behind.
"""
import pytest

import plan_audit as PA
import test_plan_audit_gpu as TG

OPSHAPES = PA.MLB_F_OPSHAPES


@pytest.fixture(scope="module")
def dry():
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    L.mlsd_runtime_dry(1)
    yield engine
    L.mlsd_runtime_dry(0)


def _keys(engine, spec, xattn=None):
    from mlimgsynth_amd import _lib
    with TG._built((engine, _lib), spec, xattn, OPSHAPES, False) as b:
        return {PA.census_key(o) for o in PA.Plan(b.ctx, external=b.external).ops}


@pytest.fixture(scope="module")
def met(dry):
    """the census keys of every audited plan (built under its xattn mode) and of the bench plans"""
    keys = set()
    for spec, xattn, _ in TG.AUDITED:
        keys |= _keys(dry, spec, xattn)
    for spec in PA.BENCH_PLANS:
        keys |= _keys(dry, spec)
    return keys


SIZE_KEYS = {}      # plan id -> census keys, each plan built once per module


def _size_keys(dry, spec):
    pid = PA.plan_id(spec)
    if pid not in SIZE_KEYS:
        SIZE_KEYS[pid] = _keys(dry, spec)
    return pid, SIZE_KEYS[pid]


@pytest.mark.parametrize("spec", PA.SIZE_PLANS, ids=[PA.plan_id(s) for s in PA.SIZE_PLANS])
def test_every_op_form_at_this_size_is_held(dry, met, spec):
    pid, keys = _size_keys(dry, spec)
    assert keys
    missing = PA.unheld_forms({pid: keys}, met | set(TG.COVERED_ELSEWHERE))
    assert not missing, "op forms that no audited plan, no bench plan and no COVERED_ELSEWHERE entry holds: " + "; ".join(f"{k} in {', '.join(p)}" for k, p in missing.items())


def test_the_census_reports_a_form_taken_out_of_the_held_set(dry, met):
    """every COVERED_ELSEWHERE key that only the size plans need: without it the census names exactly that form, with the plans that need it"""
    by_plan = dict(_size_keys(dry, s) for s in PA.SIZE_PLANS)
    held = met | set(TG.COVERED_ELSEWHERE)
    assert not PA.unheld_forms(by_plan, held)
    only_listed = [k for k in TG.COVERED_ELSEWHERE if k not in met and any(k in v for v in by_plan.values())]
    print(f"\n[size census] {len(only_listed)} op forms of the size plans are held by their COVERED_ELSEWHERE entry alone")
    assert len(only_listed) >= 30, only_listed
    for k in only_listed:
        gone = PA.unheld_forms(by_plan, held - {k})
        assert gone == {k: [p for p, v in by_plan.items() if k in v]} and gone[k], (k, gone)


@pytest.mark.parametrize("spec", PA.REFUSED_LATENTS, ids=[PA.plan_id(s) for s in PA.REFUSED_LATENTS])
def test_a_latent_that_does_not_halve_evenly_is_refused_at_build_time(dry, spec, monkeypatch):
    from mlimgsynth_amd import _lib
    made, init = [], dry.MLCtx.__init__

    def tracked(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(dry.MLCtx, "__init__", tracked)
    with pytest.raises(_lib.MlsdError, match="concat: shape mismatch"):
        PA.build(dry, spec, OPSHAPES).close()
    assert made and all(c.h is None for c in made), "the refused plan's context is still alive"
    ok = ("unet", spec[1], 16, 2)      # and the next plan of that model builds
    assert _keys(dry, ok)


def test_covered_elsewhere_entries_name_cases_of_exactly_their_form(dry):
    """the check of tests/test_plan_audit_gpu.py on its table needs no device: a wrong entry is seen here first"""
    TG.test_covered_elsewhere_names_cases_of_exactly_that_form()
