"""The case table of the sampler-loop test (tests/sampler_loop_cases.py) and the oracle's loop with the model as a callback (orc_sample_loop), on the CPU.

1. The table meets the conditions its GPU test relies on: every solver meets every option of the loop, every engine form runs a one-evaluation and a
   two-evaluation solver, and every option of every row is alive: taking it away changes the bytes of the result (orc_sample_loop on a cheap analytic model).
2. The callback plumbing: orc_sample_loop driven from Python on the oracle's own orc_unet_denoise_run equals orc_sample_ex bit for bit, for all five solvers,
   and two images in one loop equal the two single-image loops.

Bounds: none.  The same C loop runs on both sides of every comparison, and the callback's CFG mix rounds each operation once, as the C statement
dx*f + du*(1-f) does under -ffp-contract=off."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import sampler_loop_cases as T

F32 = np.float32


def opts_of(r, **change):
    d = dict(method=T.METHOD_ID[r.method], sched=r.sched, steps=r.steps, s_ancestral=r.s_ancestral, s_noise=r.s_noise, f_t_ini=r.f_t_ini, f_t_end=r.f_t_end)
    d.update(change)
    return O.SampleOpts(d["method"], d["sched"], d["steps"], T.FORMS[r.form].cfg, d["s_ancestral"], d["s_noise"], d["f_t_ini"], d["f_t_end"])


def n_steps(r):
    return O.sample_steps(opts_of(r))[0]


def analytic_run(r, init, mask, dxdt=T.analytic_dxdt, **change):
    shp = (len(r.seeds), 4, 8, 8)           # (the liveness of an option does not depend on the canvas: every update is elementwise)
    return O.sample_loop(opts_of(r, **change), shp, 64, r.seeds, [0] * shp[0], dxdt, init=init, lmask=mask, want_steps=True)


# ------------------------------------------------------------------ 1. the table
ALL_ROWS = T.ROWS + [r for r, _ in T.ABORT_ROWS]


def test_rows_are_well_formed():
    assert 40 <= len(T.ROWS) <= 60 and len(set(T.ROWS)) == len(T.ROWS)
    for r in ALL_ROWS:
        f = T.FORMS[r.form]
        assert r.method in T.METHOD_ID and len(r.seeds) == f.B and len(set(r.seeds)) == f.B
        assert r.s_noise == 0 or r.s_noise > 0.7072          # at or below: s_hat < s_curr and a NaN scale
        assert r.f_t_ini in (1.0, 0.6) and r.f_t_end in (0.0, 0.2) and (r.f_t_ini == 0.6) == r.init
        if r.form == "draws":
            assert (r.steps, r.method, r.s_ancestral) == (3, "euler", 1.0) and 4 * (f.px // 8) ** 2 * f.B >= 32768
        else:
            assert 5 <= r.steps <= 8
        calls = n_steps(r) * (2 if r.method in T.TWO_EVAL else 1)
        assert calls <= 16
        if r.method == "taylor3":
            assert n_steps(r) >= 4                           # the third-order term is live from the third step on
        if r.method == "dpmpp2m":
            assert n_steps(r) >= 3
        if f.control:
            assert r.method == "heun"                        # both evaluations of a step share the window decision


@pytest.mark.parametrize("method", sorted(T.METHOD_ID))
def test_every_solver_meets_every_option(method):
    rows = [r for r in T.ROWS if r.method == method]
    has = lambda p: any(p(r) for r in rows)
    assert has(lambda r: r.s_noise == 0.8) and has(lambda r: r.s_noise == 1.0)
    assert has(lambda r: r.s_ancestral == 1.0) and has(lambda r: r.s_ancestral == 0.6) and has(lambda r: r.s_ancestral == 0.0)
    assert has(lambda r: r.sched == T.KARRAS) and has(lambda r: r.sched == T.UNIFORM)
    assert has(lambda r: r.mask) and has(lambda r: r.init and r.f_t_ini == 0.6)
    assert has(lambda r: r.f_t_end == 0.2) and has(lambda r: r.f_t_end == 0.0)
    assert has(lambda r: T.FORMS[r.form].B == 2 and r.seeds[0] != r.seeds[1])
    assert has(lambda r: r.s_noise > 0 and r.s_ancestral > 0 and r.mask)       # two draws a step plus the first, a blend after each


def test_every_engine_form_runs_both_kinds_of_solver():
    assert {r.form for r in T.ROWS} == set(T.FORMS)
    for name, f in T.FORMS.items():
        methods = {r.method for r in T.ROWS if r.form == name}
        if name in ("control", "draws"):
            continue
        assert methods - set(T.TWO_EVAL) and methods & set(T.TWO_EVAL), name
    assert sum(r.form == "tiled-rescale" for r in T.ROWS) >= 1
    kinds = [(r.s_noise > 0 and r.s_ancestral > 0, r.method in T.TWO_EVAL, r.form.startswith("tiled")) for r, _ in T.ABORT_ROWS]
    assert any(k[0] for k in kinds) and any(k[1] for k in kinds) and any(k[2] for k in kinds)
    for r, k in T.ABORT_ROWS:
        assert 1 < k < n_steps(r)


def test_mask_has_interior_values():
    for side in (8, 12, 64):
        assert set(np.unique(T.latent_mask(side, side))) == {F32(0), F32(0.25), F32(1)}


@pytest.mark.parametrize("r", ALL_ROWS, ids=[T.row_id(r) for r in ALL_ROWS])
def test_every_option_of_a_row_is_alive(r):
    """A row whose option does nothing tests nothing: without any one of its ingredients the loop gives other bytes."""
    init = T.init_latent((len(r.seeds), 4, 8, 8)) if r.init else None
    mask = T.latent_mask(8, 8) if r.mask else None
    calls = []

    def recording(i_step, t, x):
        d = T.analytic_dxdt(i_step, t, x)
        calls.append((i_step, F32(t), x, d))
        return d
    full, off, n_call, steps = analytic_run(r, init, mask, recording)
    n = n_steps(r)
    assert np.isfinite(full).all() and n_call == len(calls) and steps.shape[0] == n
    assert n_call == sum(2 if (r.method in T.TWO_EVAL and s_down > 0) else 1 for s_down in t_ends(r))
    again = analytic_run(r, init, mask)
    assert again[0].tobytes() == full.tobytes() and again[1] == off and steps[-1].tobytes() == full.tobytes()
    draws = 1 + (n - 1 if r.s_noise > 0 else 0) + (sum(1 for s in range(n - 1) if s_ups(r)[s] > 0) if r.s_ancestral > 0 else 0)
    assert off == [draws] * len(r.seeds)
    if len(r.seeds) == 2:
        assert not np.array_equal(full[0], full[1])
    differs = lambda other: other[0].tobytes() != full.tobytes()
    if r.s_noise > 0:
        assert differs(analytic_run(r, init, mask, s_noise=0.0))
    if r.s_ancestral > 0:
        assert differs(analytic_run(r, init, mask, s_ancestral=0.0))
    if r.mask:
        assert differs(analytic_run(r, init, None))
    if r.init:
        assert differs(analytic_run(r, None, mask))
    if r.f_t_end > 0:
        assert differs(analytic_run(r, init, mask, f_t_end=0.0))
        # what f_t_end moves is the last sigma above 0 (dnsamp_init ends every table with sigma 0, src/sampling.c:60): the last step, the one that takes the
        # !(t1 > 0) branches, is a longer jump
        assert schedule_scalars(r)[0][-2] > 2 * O.sample_steps(opts_of(r, f_t_end=0.0))[1][-2]
    assert t_ends(r)[-1] == 0 and all(t > 0 for t in t_ends(r)[:-1])
    if r.method == "taylor3":
        assert third_order_steps(r, calls) >= 2


def schedule_scalars(r):
    """(sigmas, s_down, s_up per step) of a row, from the oracle's own functions"""
    n, sig = O.sample_steps(opts_of(r))
    down, up = [], []
    for s in range(n):
        d, u = ctypes.c_float(sig[s + 1]), ctypes.c_float(0)
        if r.s_ancestral > 0:
            O.L().orc_ancestral(sig[s], sig[s + 1], r.s_ancestral, ctypes.byref(d), ctypes.byref(u))
        down.append(F32(d.value))
        up.append(F32(u.value))
    return sig, down, up


def t_ends(r):
    return schedule_scalars(r)[1]


def s_ups(r):
    return schedule_scalars(r)[2]


def third_order_steps(r, calls):
    """steps of a taylor3 run at which dropping the third-order term would change the bytes of the update (solvers.c:150-165 on the recorded evaluations)"""
    down = t_ends(r)
    live, dt_prev, dp1, dp2 = 0, None, None, None
    for (s, t0, x, dx) in calls:
        dt = F32(down[s] - t0)
        x1 = x + dx * dt
        if s >= 1:
            idtp = F32(1) / dt_prev
            d2 = (dx - dp1) * idtp
            f2 = dt * dt / F32(2)
            if s >= 2:
                d3 = (d2 - dp2) * idtp
                f3 = dt * dt * dt / F32(6)
                live += int(not np.array_equal(x1 + (d2 * f2 + d3 * f3), x1 + d2 * f2))
        else:
            d2 = np.zeros_like(dx)
        dt_prev, dp1, dp2 = dt, dx, d2
    return live


# ------------------------------------------------------------------ 2. the callback plumbing
def oracle_model(model, cfg):
    """dxdt(i_step, t, x [n_img][4][8][8]) on the oracle's own UNet, image by image, with the CFG mix in numpy float32"""
    U = O.unet_params(model)
    P = O.Params(1234)
    cond, uncond = T.conditioning(U.n_ctx)
    f = F32(cfg)

    def dxdt(i_step, t, x):
        out = np.empty_like(x)
        for b in range(x.shape[0]):
            run = lambda c: O.from_ot(O.L().orc_unet_denoise_run(P.h, b"unet", U, O.to_ot(x[b][None]), O.to_ot(c[None, None]), None, t))[0]
            dx, du = run(cond), run(uncond)
            out[b] = (dx * f).astype(F32) + (du * (F32(1) - f)).astype(F32)
        return out
    return U, P, cond, uncond, dxdt


def sample_ex(U, P, cond, uncond, opts, seed, init, mask, offset=0):
    out = np.empty((4, 8, 8), F32)
    nfe = O.L().orc_sample_ex(P.h, b"unet", U, 8, 8, O.to_ot(cond[None, None]), None, O.to_ot(uncond[None, None]), None, ctypes.byref(opts), seed, offset,
                              O.fptr(init) if init is not None else None, O.fptr(mask) if mask is not None else None, O.fptr(out))
    return out, nfe


PLUMBING = [T._r("cfg7", "euler", anc=1.0, steps=5), T._r("cfg7", "heun", noise=0.8, steps=8, end=0.2), T._r("cfg7", "taylor3", anc=0.6, steps=5, sched=T.KARRAS),
            T._r("cfg7", "dpmpp2m", anc=1.0, noise=0.8, steps=6, ini=0.6, init=True, mask=True), T._r("cfg7", "dpmpp2s", steps=5)]


@pytest.mark.parametrize("r", PLUMBING, ids=[T.row_id(r) for r in PLUMBING])
def test_loop_with_a_python_callback_equals_orc_sample_ex(r):
    U, P, cond, uncond, dxdt = oracle_model("tiny", 7.0)
    init = T.init_latent((1, 4, 8, 8)) if r.init else None
    mask = T.latent_mask(8, 8) if r.mask else None
    seed, opts = r.seeds[0], opts_of(r)
    want, nfe = sample_ex(U, P, cond, uncond, opts, seed, init, mask, offset=3)
    got, off, calls, steps = O.sample_loop(opts, (1, 4, 8, 8), 64, [seed], [3], dxdt, init=init, lmask=mask, want_steps=True)
    assert np.isfinite(want).all() and got[0].tobytes() == want.tobytes()
    assert nfe == 2 * calls and off[0] > 3 and steps[-1].tobytes() == got.tobytes()
    # stop_after: the latent after k completed steps, and the draws consumed until then
    k = 2
    part, off_k, calls_k, _ = O.sample_loop(opts, (1, 4, 8, 8), 64, [seed], [3], dxdt, init=init, lmask=mask, stop_after=k)
    assert part.tobytes() == steps[k - 1].tobytes() and 3 < off_k[0] <= off[0] and calls_k < calls
    P.free()


def test_two_images_in_one_loop_equal_two_single_image_loops():
    U, P, cond, uncond, dxdt = oracle_model("tiny", 7.0)
    r = PLUMBING[3]
    opts, seeds, offs = opts_of(r), [5, 6], [0, 2]
    init, mask = T.init_latent((2, 4, 8, 8)), T.latent_mask(8, 8)
    both, off, calls, _ = O.sample_loop(opts, (2, 4, 8, 8), 64, seeds, offs, dxdt, init=init, lmask=mask)
    for b in range(2):
        one, off1, calls1, _ = O.sample_loop(opts, (1, 4, 8, 8), 64, [seeds[b]], [offs[b]], dxdt, init=init[b:b + 1], lmask=mask)
        assert one[0].tobytes() == both[b].tobytes() and off1[0] == off[b] and calls1 == calls
    assert not np.array_equal(both[0], both[1])
    P.free()


def test_a_callback_that_aborts_or_raises_ends_the_loop():
    r = T.ROWS[0]
    seen = []

    def stop_at_third(i_step, t, x):
        seen.append(i_step)
        return None if len(seen) == 3 else T.analytic_dxdt(i_step, t, x)
    out, off, ret, _ = O.sample_loop(opts_of(r), (2, 4, 8, 8), 64, r.seeds, [0, 0], stop_at_third)
    assert out is None and ret < 0 and len(seen) == 3

    def broken(i_step, t, x):
        raise KeyError("model")
    with pytest.raises(KeyError):
        O.sample_loop(opts_of(r), (2, 4, 8, 8), 64, r.seeds, [0, 0], broken)
