"""The engine's denoising loop (csrc/host/engine.c: denoise_body, unet_eval, dxdt_finish, the draw prefetch, the abort rewind) against the oracle's loop
(orc_sample_loop: dnsamp_step and the solvers of the reference restated) driven by the engine's own evaluations, bit for bit, for every solver on every
engine form of tests/sampler_loop_cases.py.

Bounds: none.  An evaluation is a pure function of (x, sigma, conditioning), and mlis_amd_dxdt runs it through the same unet_eval and dxdt_finish the loop
uses, for plain and tiled engines; the solver kernels, the guidance mix and the fused Euler update are each bit-exact against fp32 restatements of the
reference's statements (tests/test_sampler_gpu.py, tests/test_guidance_forms_gpu.py), and the oracle is compiled without contraction.  What is left between the
two loops is the host side: the scalars handed to the kernels (idtp, f2, f3, c, h_last, solver_t after a draw, the shared window decision of a two-evaluation
step), the order of draws, mask blends and copies, and the Philox states.  Equal bytes hold all of them.

Per row: the generation and the loop agree in the final latent, the evaluation count, the step count and image 0's Philox offset; a second generation without
seeds agrees with the loop continued from the offsets the first loop returned, which holds every image's Philox state and that the one-step-ahead prefetch
consumed exactly what the schedule needed.  On a mismatch the message names the first step and element that differ (the engine's per-step latents come from
a progress callback).  Three rows are aborted at step k by the callback and continued."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import sampler_loop_cases as T

pytestmark = pytest.mark.gpu

F32 = np.float32
PROGRESS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int)


def api():
    from mlimgsynth_amd import engine as E
    l = E._proto2()
    l.mlis_amd_rng_offset.argtypes, l.mlis_amd_rng_offset.restype = [ctypes.c_void_p], ctypes.c_uint32
    l.mlis_amd_handoff_retries.argtypes = [ctypes.c_void_p]
    return l


@pytest.fixture(scope="module")
def engines():
    """name of FORMS[...].engine -> the resident Generator, created on first use"""
    from mlimgsynth_amd import engine as E
    made = {}

    def get(form):
        f = T.FORMS[form]
        if f.engine not in made:
            g = E.Generator(f.model, f.px, f.px, f.B, n_step=8, cfg_scale=f.cfg, **f.kw)
            made[f.engine] = g
            cond, uncond = T.conditioning(O.unet_params(f.model).n_ctx)
            g.set_cond(cond, None, uncond if f.cfg > 1 else None, None)
            if f.pag:
                g.set_pag(f.pag)
            if f.control:
                g.set_control_image(T.control_image(f.px))
        g = made[f.engine]
        g.set_cfg_rescale(f.rescale)
        if f.control:
            g.set_control(T.CONTROL_STRENGTH, *T.CONTROL_WINDOW)
        return g
    yield get
    for g in made.values():
        g.destroy()


def download_latent(g, shape):
    from mlimgsynth_amd import _lib
    out = np.empty(shape, F32)
    _lib.lib().mlsd_memcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(g.latent_ptr()), ctypes.c_size_t(out.nbytes), 1, None)
    _lib.lib().mlsd_device_sync()
    return out


def opts_of(r):
    return O.SampleOpts(T.METHOD_ID[r.method], r.sched, r.steps, T.FORMS[r.form].cfg, r.s_ancestral, r.s_noise, r.f_t_ini, r.f_t_end)


class Run:
    """one row on its engine: generations (with the per-step latents) and the oracle's loop on the engine's evaluations"""

    def __init__(self, g, r):
        self.g, self.r, self.f, self.l = g, r, T.FORMS[r.form], api()
        self.shape = T.latent_shape(r)
        self.hw = self.shape[2] * self.shape[3]
        self.init, self.mask = T.row_inputs(r)
        self.opts = opts_of(r)
        self.n_step = O.sample_steps(self.opts)[0]
        g.set_sampler(r.steps, r.method, r.sched, self.f.cfg, r.s_ancestral, r.s_noise, r.f_t_ini, r.f_t_end)
        g.set_lmask(self.mask)

    def generate(self, seeds, abort_at=0):
        """-> dict(latent, steps, nfe, n_step, offset, ctl_evals); with abort_at = k the callback ends the generation after step k"""
        from mlimgsynth_amd import _lib
        g = self.g
        g.set_init_latent(self.init)         # (a generation clears it)
        steps = []

        def progress(user, step, n_step, nfe):
            steps.append(download_latent(g, self.shape))
            return -1 if step == abort_at else 1
        cb = PROGRESS_FN(progress)
        self.l.mlis_amd_set_callback(g.h, ctypes.cast(cb, ctypes.c_void_p), None)
        try:
            if abort_at:
                with pytest.raises(_lib.MlsdError):
                    g.generate(seeds, want_images=False)
                latent = download_latent(g, self.shape)
            else:
                latent, _ = g.generate(seeds, want_images=False)
        finally:
            self.l.mlis_amd_set_callback(g.h, None, None)
        assert self.l.mlis_amd_handoff_retries(g.h) == 0
        return dict(latent=latent, steps=steps, nfe=g.last_nfe(), n_step=g.last_n_step(), offset=self.l.mlis_amd_rng_offset(g.h),
                    ctl_evals=g.control_info()[1] if self.f.control else 0)

    def loop(self, offsets, stop_after=0):
        """orc_sample_loop on g.dxdt -> dict(latent, offsets, calls, steps, active): active counts the evaluations inside the control window"""
        from mlimgsynth_amd import engine as E
        g, f = self.g, self.f
        active = [0]

        def dxdt(i_step, t, x):
            if f.control:     # strength 0 is the loop's own off path: the gain is 0 and the ControlNet plan does not run
                on = E.control_active(i_step, self.n_step, *T.CONTROL_WINDOW)
                g.set_control(T.CONTROL_STRENGTH if on else 0.0, *T.CONTROL_WINDOW)
                active[0] += int(on)
            return g.dxdt(x, t)
        try:
            latent, off, calls, steps = O.sample_loop(self.opts, self.shape, self.hw, self.r.seeds, offsets, dxdt, init=self.init, lmask=self.mask,
                                                      stop_after=stop_after, want_steps=True)
        finally:
            if f.control:
                g.set_control(T.CONTROL_STRENGTH, *T.CONTROL_WINDOW)
        return dict(latent=latent, offsets=off, calls=calls, steps=steps, active=active[0])


def first_difference(got, want):
    """'' when the engine's per-step latents and final latent equal the loop's, else where they first differ"""
    for s, x in enumerate(got["steps"]):
        y = want["steps"][s]
        if x.tobytes() != y.tobytes():
            i = int(np.flatnonzero(x.reshape(-1).view(np.uint32) != y.reshape(-1).view(np.uint32))[0])
            idx = tuple(int(v) for v in np.unravel_index(i, x.shape))
            n_bad = int((x.view(np.uint32) != y.view(np.uint32)).sum())
            return (f"first difference after step {s + 1} of {len(want['steps'])}, element {idx}: engine {x[idx]!r}, loop {y[idx]!r}; {n_bad} of {x.size} elements of that "
                    f"step differ, rel-L2 {np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(y.astype(np.float64)):.3e}")
    if got["latent"].tobytes() != want["latent"].tobytes():
        return "the per-step latents agree, the returned latent does not"
    return ""


def check(got, want, groups, n_step):
    assert len(got["steps"]) == n_step, (len(got["steps"]), n_step)
    assert np.isfinite(got["latent"]).all()
    diff = first_difference(got, want)
    assert not diff, diff
    assert got["nfe"] == want["calls"] * groups and got["n_step"] == n_step


@pytest.mark.parametrize("r", T.ROWS, ids=[T.row_id(r) for r in T.ROWS])
def test_generation_equals_the_loop_on_the_engines_evaluations(engines, r):
    run = Run(engines(r.form), r)
    f, B = run.f, len(r.seeds)
    got = run.generate(r.seeds)
    want = run.loop([0] * B)
    check(got, want, f.groups, run.n_step)
    assert got["offset"] == want["offsets"][0] and len(set(want["offsets"])) == 1
    if f.control:
        assert 0 < want["active"] < want["calls"] and got["ctl_evals"] == want["active"]      # 2 evaluations per active step
        assert want["active"] == 2 * sum(1 for s in range(run.n_step - 1) if control_on(s, run.n_step))
    if B == 2:
        assert not np.array_equal(got["latent"][0], got["latent"][1])
    # without seeds: every image's Philox stream goes on where the first generation's schedule left it
    again = run.generate(None)
    want2 = run.loop(want["offsets"])
    check(again, want2, f.groups, run.n_step)
    assert again["offset"] == want2["offsets"][0] and again["latent"].tobytes() != got["latent"].tobytes()


def control_on(s, n_step):
    from mlimgsynth_amd import engine as E
    return E.control_active(s, n_step, *T.CONTROL_WINDOW)


@pytest.mark.parametrize("r,k", T.ABORT_ROWS, ids=[T.row_id(r) for r, _ in T.ABORT_ROWS])
def test_abort_at_step_k_and_continue(engines, r, k):
    """the callback aborts after step k: the latent and the Philox states are those of the loop stopped there (the draws the prefetch made ahead are given
    back), and a generation without seeds goes on from them"""
    run = Run(engines(r.form), r)
    B = len(r.seeds)
    assert 1 < k < run.n_step
    got = run.generate(r.seeds, abort_at=k)
    want = run.loop([0] * B, stop_after=k)
    want["steps"] = want["steps"][:k]
    assert len(got["steps"]) == k and got["steps"][-1].tobytes() == got["latent"].tobytes()
    diff = first_difference(got, want)
    assert not diff, diff
    assert got["offset"] == want["offsets"][0] and got["nfe"] == want["calls"] * run.f.groups
    again = run.generate(None)
    want2 = run.loop(want["offsets"])
    check(again, want2, run.f.groups, run.n_step)
    assert again["offset"] == want2["offsets"][0]
