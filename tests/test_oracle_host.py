"""Pin the oracle's host-side restatement against the reference's own golden vectors
(SURVEY.md §8c): Philox KAT, reference RNG build (oracle/_ref, or its stored outputs), sigma tables, schedule."""
import ctypes

import numpy as np

import oracle_lib as O
import reference_answers as RA

# src/test_rng.c:11-24 (seed 0, offset 0, n 12), printed by the reference with %12.8f
KAT_SEED0 = [-0.92466259, -0.42534414, -2.64384580, 0.14518388, -0.12086648, -0.57972562,
             -0.62285119, -0.32838708, -1.07454228, -0.36314407, -1.67105067, 2.26550508]
# reference `test_rng 42 0 8`
KAT_SEED42 = [0.19401896, 2.16137385, -0.17205083, 0.84906018, -1.92439914, 0.65298533, -0.64944100, -0.81752473]
# reference dnsamp_init, 20 steps, uniform schedule, SD sigma table
SIGMAS20 = [14.61464, 10.7468, 8.081519, 6.204935, 4.855652, 3.865378, 3.123761, 2.557166, 2.115658, 1.764822,
            1.480581, 1.245813, 1.048142, 0.878428, 0.7297186, 0.5964336, 0.4735847, 0.3555453, 0.2321642,
            0.02916716, 0]


def test_rng_kat_reference_comment():
    out = O.randn(0, 0, 12)
    assert [f"{v:.8f}" for v in out] == [f"{v:.8f}" for v in KAT_SEED0]
    out = O.randn(42, 0, 8)
    assert [f"{v:.8f}" for v in out] == [f"{v:.8f}" for v in KAT_SEED42]


def test_rng_bitexact_vs_reference_build():
    for seed, off, n in RA.RNG_CASES:
        ref, ref_off = RA.randn(seed, off, n)
        mine = O.randn(seed, off, n)
        assert np.array_equal(ref.view(np.uint32), mine.view(np.uint32)), (seed, off)
        assert ref_off == (off + 1) % 2**32
    assert O.randn(1, 0, 0).size == 0  # empty request


def test_sigma_table_endpoints_and_schedule():
    L = O.L()
    ls = np.empty(1000, np.float32)
    L.orc_log_sigmas(O.fptr(ls))
    # src/unet.c:34-35 sigma_min / sigma_max constants of the reference
    assert abs(np.exp(ls[0]) - 0.029167158) < 1e-8
    assert abs(np.exp(ls[999]) - 14.614641) < 2e-6
    # SURVEY App. B item 6 (reference run): sigma(t=0), sigma(t=999), t(sigma=1)
    assert f"{L.orc_t_to_sigma(0.0):.10f}" == "0.0291671604"
    assert f"{L.orc_t_to_sigma(999.0):.7f}" == "14.6146402"
    assert f"{L.orc_sigma_to_t(1.0):.5f}" == "353.89035"
    sig = np.empty(64, np.float32)
    n = L.orc_schedule(20, 1, 1.0, 0.0, O.fptr(sig))
    assert n == 20
    for got, exp in zip(sig[:21], SIGMAS20):
        assert f"{got:.7g}" == f"{exp:.7g}", (got, exp)
    # ancestral split on the last step: sigma_to = 0 -> no noise, s_down = 0
    sd, su = ctypes.c_float(), ctypes.c_float()
    L.orc_ancestral(sig[19], sig[20], 1.0, ctypes.byref(sd), ctypes.byref(su))
    assert sd.value == 0 and su.value == 0
    L.orc_ancestral(sig[0], sig[1], 1.0, ctypes.byref(sd), ctypes.byref(su))
    s1, s2 = np.float64(sig[0]), np.float64(sig[1])
    up = np.sqrt(s2 * s2 * (s1 * s1 - s2 * s2) / (s1 * s1))
    assert abs(su.value - up) < 1e-5 and abs(sd.value - np.sqrt(s2 * s2 - up * up)) < 1e-5


def test_sigma_t_roundtrip():
    L = O.L()
    for t in [10.0, 353.89, 500.25, 998.0]:
        s = L.orc_t_to_sigma(t)
        # linear_est extrapolates from the NEXT interval (reference quirk, src/unet.c:315-322):
        # close but not exact, and clearly off where the table is strongly curved (t < 1)
        assert abs(L.orc_sigma_to_t(s) - t) < 0.02
    assert abs(L.orc_sigma_to_t(L.orc_t_to_sigma(0.5)) - 0.5) < 0.5
