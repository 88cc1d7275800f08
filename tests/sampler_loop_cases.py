"""The case table of tests/test_sampler_loop_gpu.py (the engine's denoising loop against the oracle's loop on the engine's own evaluations) and the numpy-only
helpers both that test and tests/test_sampler_loop_cpu.py use.  Importable without a GPU: test_sampler_loop_cpu.py asserts the conditions the table has to meet
(every solver meets every option, every option of every row changes the bytes of the result).

A row is one generation: the sampler options, whether an initial latent and a latent mask are set, the seeds of the batch, and the engine form that runs it.
Shapes are the smallest at which every branch of the loop is alive: the `tiny` family at 64 x 64 px (an 8 x 8 latent), 5 to 8 requested steps.

f_t_end: dnsamp_init ends every sigma table with 0 (src/sampling.c:60), so the last step of every row takes the !(t1 > 0) branches -- one evaluation for Heun
and DPM++ 2S, c = 0 for DPM++ 2M -- and every step before it the other ones.  What f_t_end = 0.2 changes is the step count and the last sigma above 0: the
last step becomes a jump from sigma(0.2) to 0 instead of a short one."""
import collections

import numpy as np

F32 = np.float32
METHOD_ID = {"euler": 1, "heun": 2, "taylor3": 3, "dpmpp2m": 4, "dpmpp2s": 5}
TWO_EVAL = ("heun", "dpmpp2s")
UNIFORM, KARRAS = 1, 2
CONTROL_WINDOW = (0.3, 0.7)
CONTROL_STRENGTH = 0.8
PAG_SCALE = 3.0
RESCALE_PHI = 0.7

# Engine forms: one resident Generator each (`engine`), options set on it per form (`pag`, `rescale`, `control`).  groups: row groups of one evaluation.
Form = collections.namedtuple("Form", "engine model px B cfg kw groups pag rescale control")
_tiled = dict(unet_tile=64, unet_tile_overlap=32, unet_tile_batch=2)
FORMS = {
    "cfg7": Form("cfg7", "tiny", 64, 2, 7.0, {}, 2, 0.0, 0.0, False),                      # the fused Euler step of an eps model
    "cfg7-rescale": Form("cfg7", "tiny", 64, 2, 7.0, {}, 2, 0.0, RESCALE_PHI, False),
    "cfg1": Form("cfg1", "tiny", 64, 1, 1.0, {}, 1, 0.0, 0.0, False),                      # guidance off: one row group
    "tinyv": Form("tinyv", "tinyv", 64, 2, 5.0, {}, 2, 0.0, 0.0, False),                   # v-prediction: Euler through dxdt_finish + axpy
    "pag": Form("pag", "tiny", 64, 2, 7.0, dict(pag=True), 3, PAG_SCALE, 0.0, False),
    "hipgraph": Form("hipgraph", "tiny", 64, 2, 7.0, dict(use_hipgraph=True), 2, 0.0, 0.0, False),
    "tiled": Form("tiled", "tiny", 96, 2, 7.0, _tiled, 2, 0.0, 0.0, False),
    "tiled-rescale": Form("tiled", "tiny", 96, 2, 7.0, _tiled, 2, 0.0, RESCALE_PHI, False),   # the statistics are taken over the blended canvas
    "control": Form("control", "tiny", 64, 2, 7.0, dict(control=True), 2, 0.0, 0.0, True),
    "draws": Form("draws", "tiny", 512, 2, 7.0, {}, 2, 0.0, 0.0, False),                   # 4 * hw * B = 32768 values a draw: split into ranges across threads
}

Row = collections.namedtuple("Row", "form method s_ancestral s_noise sched steps f_t_ini f_t_end init mask seeds")


def _r(form, method, anc=0.0, noise=0.0, sched=UNIFORM, steps=8, ini=1.0, end=0.0, init=False, mask=False, seeds=None):
    B = FORMS[form].B
    return Row(form, method, anc, noise, sched, steps, ini, end, init, mask, tuple(seeds or (31, 47))[:B])


def _core(method, steps):
    """the rows every solver gets on the plain engine: between them every option of the loop"""
    return [
        _r("cfg7", method, steps=steps, seeds=(11, 12)),
        _r("cfg7", method, noise=0.8, steps=steps, seeds=(13, 14)),
        _r("cfg7", method, anc=1.0, sched=KARRAS, steps=steps, end=0.2, seeds=(15, 16)),
        _r("cfg7", method, anc=0.6, noise=1.0, steps=steps, ini=0.6, init=True, mask=True, seeds=(17, 18)),     # the most draws and blends a step can have
    ]


ROWS = (
    _core("euler", 6) + _core("heun", 8) + _core("taylor3", 8) + _core("dpmpp2m", 6) + _core("dpmpp2s", 8) + [
        _r("cfg7-rescale", "euler", anc=1.0, steps=6),
        _r("cfg7-rescale", "dpmpp2s", noise=0.8, steps=8, end=0.2),
        _r("cfg7-rescale", "taylor3", anc=0.6, steps=6, mask=True),
        _r("cfg1", "euler", anc=0.6, steps=8, ini=0.6, init=True, mask=True),
        _r("cfg1", "heun", sched=KARRAS, steps=8, end=0.2),
        _r("cfg1", "dpmpp2m", noise=0.8, steps=5),
        _r("tinyv", "euler", anc=1.0, noise=0.8, steps=6, mask=True),
        _r("tinyv", "heun", anc=0.6, steps=8, sched=KARRAS),
        _r("tinyv", "taylor3", steps=7, end=0.2),
        _r("tinyv", "dpmpp2m", anc=1.0, steps=6, end=0.2),
        _r("tinyv", "dpmpp2s", noise=1.0, steps=8, ini=0.6, init=True),
        _r("pag", "euler", anc=1.0, steps=5),
        _r("pag", "dpmpp2s", anc=0.6, steps=8, sched=KARRAS),
        _r("pag", "taylor3", noise=0.8, steps=5),
        _r("hipgraph", "euler", anc=1.0, steps=6, sched=KARRAS),
        _r("hipgraph", "heun", noise=0.8, steps=8, mask=True),
        _r("hipgraph", "dpmpp2m", anc=0.6, steps=5, ini=0.6, init=True),
        _r("tiled", "euler", anc=1.0, steps=5, ini=0.6, init=True, mask=True),
        _r("tiled", "heun", anc=0.6, steps=8, end=0.2),
        _r("tiled", "dpmpp2m", noise=0.8, steps=5, sched=KARRAS),
        _r("tiled-rescale", "euler", anc=0.6, steps=5),
        _r("tiled-rescale", "dpmpp2s", steps=6, end=0.2),
        _r("control", "heun", steps=8),
        _r("control", "heun", anc=1.0, noise=0.8, steps=8, end=0.2),
        _r("draws", "euler", anc=1.0, steps=3),
    ])

# abort at completed step k (1 < k < n_step) and continue: s_noise with ancestral noise, a two-evaluation solver, a tiled engine
ABORT_ROWS = [
    (_r("cfg7", "euler", anc=0.6, noise=0.8, steps=6, mask=True, seeds=(21, 22)), 3),
    (_r("cfg7", "dpmpp2s", anc=1.0, steps=8, seeds=(23, 24)), 2),
    (_r("tiled", "taylor3", anc=1.0, steps=5, seeds=(25, 26)), 3),
]


def row_id(r):
    s = f"{r.form}-{r.method}-a{r.s_ancestral:g}-n{r.s_noise:g}-{'karras' if r.sched == KARRAS else 'uniform'}-{r.steps}-{r.f_t_ini:g}-{r.f_t_end:g}"
    return s + ("-init" if r.init else "") + ("-mask" if r.mask else "")


def latent_shape(r):
    f = FORMS[r.form]
    return (f.B, 4, f.px // 8, f.px // 8)


def init_latent(shape, seed=9):
    return (np.random.default_rng(seed).standard_normal(shape) * 0.8).astype(F32)


def latent_mask(lh, lw, seed=10):
    """0 / 1 values with interior values of 0.25 among them, as test_sampler_gpu.py::test_img2img_and_inpaint_vs_oracle builds it"""
    m = (np.random.default_rng(seed).random((lh, lw)) > 0.5).astype(F32)
    m[0, 0] = m[lh // 2, lw // 2] = m[lh - 1, 1] = 0.25
    return m


def row_inputs(r):
    """(initial latent or None, latent mask or None) of a row"""
    shp = latent_shape(r)
    return (init_latent(shp) if r.init else None), (latent_mask(shp[2], shp[3]) if r.mask else None)


def conditioning(n_ctx, seed=8):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((77, n_ctx)).astype(F32), rng.standard_normal((77, n_ctx)).astype(F32)


def control_image(px, seed=4):
    return np.random.default_rng(seed).random((3, px, px)).astype(F32)


def analytic_dxdt(i_step, t, x):
    """a cheap nonlinear model for the CPU checks of the table: the denoised image is tanh(x)"""
    return ((x - np.tanh(x)) / F32(t)).astype(F32)
