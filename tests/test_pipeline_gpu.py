"""Decoder / text-encoder / full-generation parity of the HIP engine against the oracle."""
import ctypes

import numpy as np
import tolerances as T
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("model,lat,n", [("tiny", 8, 2), ("tiny", 16, 1)])
def test_vae_decode_parity(model, lat, n):
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(3)
    z = rng.standard_normal((n, 4, lat, lat)).astype(np.float32) * 0.5
    dec = engine.Decoder(model, lat, lat, n)
    got = dec.run(z)
    V, P = O.vae_params(model), O.Params(1234)
    ref = np.stack([O.from_ot(O.L().orc_vae_decode(P.h, b"vae", V, O.to_ot(z[i:i + 1])))[0] for i in range(n)])
    assert got.shape == ref.shape == (n, 3, lat * 8, lat * 8)
    err = rel(got - 0.5, ref - 0.5)
    print("vae", model, lat, "rel-L2", err)
    assert err < T.EVAL                       # tolerance as for the UNet (fp16 attention operands, fp32 order)
    mine = {k for k, _, _ in dec.ctx.param_list()}
    assert mine == {k for k, _, _ in P.names()}


def test_vae_decode_sd_real_config():
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(4)
    lat = 8
    z = rng.standard_normal((1, 4, lat, lat)).astype(np.float32) * 0.5
    dec = engine.Decoder("sd1", lat, lat, 1)
    npar = sum(int(np.prod(ne)) for _, _, ne in dec.ctx.param_list())
    assert abs(npar - 49.5e6) < 0.2e6       # VAE decoder 49.5 M parameters
    got = dec.run(z)
    V, P = O.vae_params("sd1"), O.Params(1234)
    ref = O.from_ot(O.L().orc_vae_decode(P.h, b"vae", V, O.to_ot(z)))
    err = rel(got - 0.5, ref - 0.5)
    print("vae sd1 rel-L2", err)
    assert err < T.EVAL


def test_vae_decode_512_parity():
    """The real SD1.5 KL decoder (configs[1]'s decode) against the oracle at a 32x32 latent -> 256x256 image (the CPU side is the cost of this test: 0.63 TFLOP in fp32;
    the full 512x512 and SDXL 1024x1024 decodes are held against the independent torch vectors by tests/test_golden_gpu.py::*full_resolution*, and against the oracle
    by tools/full_size_latent_parity.py)."""
    import os
    from mlimgsynth_amd import engine
    O.L().orc_set_threads(O.host_threads())
    rng = np.random.default_rng(5)
    lat = 32
    z = rng.standard_normal((1, 4, lat, lat)).astype(np.float32) * 0.5
    dec = engine.Decoder("sd1", lat, lat, 1)
    dec.run(z)
    got = dec.run(z)
    V, P = O.vae_params("sd1"), O.Params(1234)
    ref = O.from_ot(O.L().orc_vae_decode(P.h, b"vae", V, O.to_ot(z)))
    err = rel(got - 0.5, ref - 0.5)
    print("vae sd1 256x256 rel-L2", err)
    assert np.isfinite(got).all() and err < T.EVAL


def test_tae_decode_parity():
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(5)
    lat, n = 8, 2
    z = rng.standard_normal((n, 4, lat, lat)).astype(np.float32) * 2
    dec = engine.Decoder("sd1", lat, lat, n, tae=True)
    got = dec.run(z)
    P = O.Params(1234)
    ref = np.stack([O.from_ot(O.L().orc_tae_decode(P.h, b"tae", O.to_ot(z[i:i + 1])))[0] for i in range(n)])
    err = rel(got, ref)
    print("tae rel-L2", err)
    assert err < 2e-3
    assert {k for k, _, _ in dec.ctx.param_list()} == {k for k, _, _ in P.names()}


@pytest.mark.parametrize("model,prefix,skip,norm,feat", [("tiny", "clip", 1, True, False), ("tiny", "clip2", 2, False, True),
                                                          ("vit_l", "clip", 1, True, False)])
def test_clip_text_encode_parity(model, prefix, skip, norm, feat):
    from mlimgsynth_amd import engine
    K = O.clip_params(model)
    rng = np.random.default_rng(6)
    n_tok = 9
    toks = rng.integers(0, K.n_vocab - 3, (2, n_tok)).astype(np.int32)
    emb, ft = engine.clip_text_encode(model, prefix, toks, want_embed=True, want_feat=feat, clip_skip=skip, norm=norm)
    P = O.Params(1234)
    for p in range(2):
        full = np.full(K.n_token, K.tok_pad, np.int32)
        full[0] = K.tok_start
        full[1:1 + n_tok] = toks[p]
        full[1 + n_tok] = K.tok_end
        ptr = full.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        if feat:
            # feat forces all layers + final norm; embed then is that same tensor (src/clip.c:446)
            e_ref = O.from_ot(O.L().orc_clip_text_encode(P.h, prefix.encode(), K, ptr, -1, 1, 0, 0)).reshape(K.n_token, K.d_embed)
            f_ref = O.from_ot(O.L().orc_clip_text_encode(P.h, prefix.encode(), K, ptr, -1, 1, 1, n_tok + 1)).reshape(K.d_embed)
            assert rel(ft[p], f_ref) < T.EVAL
        else:
            e_ref = O.from_ot(O.L().orc_clip_text_encode(P.h, prefix.encode(), K, ptr, skip, int(norm), 0, 0)).reshape(K.n_token, K.d_embed)
        err = rel(emb[p], e_ref)
        print("clip", model, "prompt", p, "rel-L2", err)
        assert err < T.EVAL


@pytest.mark.parametrize("model", ["tiny", "tinyxl"])
def test_text_cond_assembly_vs_oracle(model):
    """mlis_text_cond_encode assembly (src/mlimgsynth.c:1501-1563) of the C object MLIS_AmdTextCond: SD1 = one tower;
    SDXL = [CLIP-L skip 2 no norm || bigG skip 2 no norm], label = pooled feature || size block; empty negative
    prompt zeroes the SDXL uncond but not its label."""
    from mlimgsynth_amd import text
    K = O.clip_params("tiny")
    toks = np.random.default_rng(8).integers(0, K.n_vocab - 3, 7).astype(np.int32)
    tc = text.TextConditioner(model, 64, 64, seed=1234)
    cond, label, ncond, nlabel = tc.encode_pair(toks, ())
    P = O.Params(1234)

    def oracle(prefix, tk, skip, norm, feat):
        full = np.full(K.n_token, K.tok_pad, np.int32)
        full[0] = K.tok_start
        full[1:1 + len(tk)] = tk
        full[1 + len(tk)] = K.tok_end
        ptr = full.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        r = O.from_ot(O.L().orc_clip_text_encode(P.h, prefix.encode(), K, ptr, skip, int(norm), int(feat), len(tk) + 1 if feat else 0))
        return r.reshape(K.d_embed) if feat else r.reshape(K.n_token, K.d_embed)
    if model == "tiny":
        assert cond.shape == (77, 64) and label is None and nlabel is None
        assert rel(cond, oracle("clip", toks, 1, True, False)) < T.EVAL
        assert rel(ncond, oracle("clip", toks[:0], 1, True, False)) < T.EVAL     # SD1: the empty prompt is encoded, not zeroed
    else:
        assert cond.shape == (77, 128) and label.shape == (96,)
        assert rel(cond[:, :64], oracle("clip", toks, 2, False, False)) < T.EVAL
        assert rel(cond[:, 64:], oracle("clip2", toks, 2, False, False)) < T.EVAL
        assert rel(label[:64], oracle("clip2", toks, -1, True, True)) < T.EVAL
        assert not label[64:].any()
        assert not ncond.any()                                                 # uncond_empty_zero
        assert rel(nlabel[:64], oracle("clip2", toks[:0], -1, True, True)) < T.EVAL
        c2, l2, nc2, nl2 = tc.encode_pair(toks, toks[:3])                      # a non-empty negative prompt is encoded
        assert nc2.any() and rel(nc2[:, :64], oracle("clip", toks[:3], 2, False, False)) < T.EVAL
        assert np.array_equal(c2, cond)
    tc.destroy()


def test_clip_prompt_too_long_is_an_error():
    from mlimgsynth_amd import engine, _lib
    with pytest.raises(_lib.MlsdError):
        engine.clip_text_encode("tiny", "clip", np.zeros((1, 76), np.int32))     # max n_token-2 = 75 (src/clip.c:449-450)


@pytest.mark.parametrize("model,steps", [("tiny", 20), ("tinyxl", 6)])
def test_generate_latent_parity_vs_oracle(model, steps):
    """Whole denoising loop (schedule, Philox noise, CFG, Euler-a) on the tiny configs: HIP engine vs the
    oracle's restatement of mlis_generate.  The ancestral loop is chaotic, so the stated tolerance on the FINAL
    latent is looser (rel-L2 <= 1e-2, tests/tolerances.py) while every single evaluation is held to 2e-3 by test_unet_gpu."""
    from mlimgsynth_amd import engine
    lat, B = 8, 2
    U = O.unet_params(model)
    rng = np.random.default_rng(8)
    cond = rng.standard_normal((77, U.n_ctx)).astype(np.float32)
    uncond = np.zeros_like(cond) if U.uncond_empty_zero else rng.standard_normal((77, U.n_ctx)).astype(np.float32)
    label = rng.standard_normal(U.ch_adm_in).astype(np.float32) if U.ch_adm_in else None
    unlabel = rng.standard_normal(U.ch_adm_in).astype(np.float32) if U.ch_adm_in else None
    g = engine.Generator(model, lat * 8, lat * 8, B, n_step=steps, cfg_scale=7.0, s_ancestral=1.0)
    g.set_cond(cond, label, uncond, unlabel)
    seeds = [42, 43]
    lat_got, img = g.generate(seeds)
    assert np.isfinite(lat_got).all() and np.isfinite(img).all()
    assert g.last_nfe() == 2 * steps
    P = O.Params(1234)
    for b in range(B):
        out = np.empty((4, lat, lat), np.float32)
        tu = ctypes.c_double()
        nfe = O.L().orc_generate_latent(P.h, b"unet", U, lat, lat, O.to_ot(cond[None, None]),
                                        O.to_ot(label[None, None, None]) if label is not None else None,
                                        O.to_ot(uncond[None, None]), O.to_ot(unlabel[None, None, None]) if unlabel is not None else None,
                                        7.0, steps, 1.0, seeds[b], 0, O.fptr(out), ctypes.byref(tu))
        assert nfe == 2 * steps
        err = rel(lat_got[b], out)
        print(model, "image", b, "final latent rel-L2", err)
        assert err < T.LATENT
    # the two images used different seeds: different latents
    assert rel(lat_got[0], lat_got[1]) > 0.1
    # determinism: a second run with the same seeds is bit-identical
    lat2, _ = g.generate(seeds, want_images=False)
    assert np.array_equal(lat2, lat_got)


def test_generate_with_hipgraph_matches_plain():
    from mlimgsynth_amd import engine
    rng = np.random.default_rng(9)
    U = O.unet_params("tiny")
    cond = rng.standard_normal((77, U.n_ctx)).astype(np.float32)
    unc = rng.standard_normal((77, U.n_ctx)).astype(np.float32)
    outs = []
    for hg in (False, True):
        g = engine.Generator("tiny", 64, 64, 1, n_step=5, use_hipgraph=hg)
        g.set_cond(cond, None, unc, None)
        outs.append(g.generate([7])[0])
        g.destroy()
    assert np.array_equal(outs[0], outs[1])


def test_host_rng_and_schedule_match_oracle():
    from mlimgsynth_amd import engine
    for seed, off, n in [(0, 0, 12), (42, 3, 5000), (2**63 + 5, 2**32 - 1, 100)]:
        got, o2 = engine.randn(seed, off, n)
        assert np.array_equal(got.view(np.uint32), O.randn(seed, off, n).view(np.uint32))
        assert o2 == (off + 1) % 2**32
    sig = engine.schedule("sd1", 20)
    ref = np.empty(64, np.float32)
    O.L().orc_schedule(20, 1, 1.0, 0.0, O.fptr(ref))
    assert np.array_equal(sig, ref[:21])


def test_rccl_entry_points_single_rank():
    """The library's RCCL path (mlsd_rccl_*, mlis_amd_bcast_cond, mlis_amd_gather_results) on a 1-rank communicator: the same
    calls the multi-GPU launcher makes, runnable on the 1-GPU box (the N > 1 behaviour is covered by tests/test_dist_cpu.py
    for the sharding logic and by the driver's 8-GPU run for the collectives themselves)."""
    from mlimgsynth_amd import _lib, engine
    L = _lib.lib()
    Lh = engine._proto2()
    Lh.mlis_amd_bcast_cond.argtypes = [_lib.vp, _lib.vp, ctypes.c_int]
    Lh.mlis_amd_gather_results.argtypes = [_lib.vp, _lib.vp, ctypes.c_int, _lib.vp]
    uid = ctypes.create_string_buffer(128)
    assert L.mlsd_rccl_unique_id(uid) == 0, _lib.last_error()
    comm = ctypes.c_void_p()
    assert L.mlsd_rccl_init(ctypes.byref(comm), 1, 0, uid.raw) == 0, _lib.last_error()
    U = O.unet_params("tiny")
    rng = np.random.default_rng(2)
    cond, unc = rng.standard_normal((77, U.n_ctx)).astype(np.float32), rng.standard_normal((77, U.n_ctx)).astype(np.float32)
    g = engine.Generator("tiny", 64, 64, 2, n_step=3)
    g.set_cond(cond, None, unc, None)
    ref, _ = g.generate([5, 6], want_images=False)
    engine.check1(Lh.mlis_amd_bcast_cond(g.h, comm, 0), "bcast")          # root == self: conditioning unchanged
    got, _ = g.generate([5, 6], want_images=False)
    assert np.array_equal(got, ref)
    recv = _lib.DeviceBuffer(ref.nbytes)
    engine.check1(Lh.mlis_amd_gather_results(g.h, comm, 0, _lib.vp(recv.ptr)), "gather")
    engine.check1(Lh.mlis_amd_sync(g.h), "sync")
    assert np.array_equal(recv.download(ref.shape, np.float32), ref)
    assert L.mlsd_rccl_destroy(comm) == 0
    g.destroy()


def test_bench_two_gpu_smoke_when_available():
    """the world > 1 branch of bench.py on real GPUs (skipped on the 1-GPU boxes of this pool)"""
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                          "--workload", "tiny", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["value"] > 0


@pytest.mark.timeout(900)
def test_bench_world2_branch_on_one_gpu_over_the_host_transport():
    """bench.py's `world > 1` branch -- communicator + gather sizing, the fence, max-over-ranks, the rank != 0 exit -- executed on the 1-GPU box: two
    ranks launched exactly as the driver launches them (torch.distributed.run, one process per rank), both on cuda:0, the library's communicator over the host transport
    (RCCL refuses two ranks on one device).  The 8-GPU run of the driver then exercises only the RCCL calls themselves."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--transport", "host", "--workload", "tiny",
                          "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline"], capture_output=True, text=True, timeout=800, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])          # torch.distributed.run returns non-zero when ANY rank does
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]                                      # rank 0 alone prints
    d = json.loads(lines[0])
    B = d["config"]["batch_per_gpu"]
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 2 * B and d["value"] > 0 and d["scaling"] == "weak"
    assert abs(d["value"] - 2 * B * 1e3 / d["ms_per_step"]) / d["value"] < 0.02     # value = the units ALL ranks processed / the max-over-ranks time
    assert d["transport"] == "host" and d["host_transport_ranks"] == 2 and "rccl_ranks" not in d
    assert "HOST transport" in d["config"]["parallelism"] and d["roofline"]["frac"] > 0
    # a rank that fails must end the job non-zero (no re-exec, no hang): --gpus disagrees with the launched world
    bad = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port + 1 if port < 65000 else port - 1), os.path.join(root, "bench.py"), "--gpus", "3", "--transport", "host",
                          "--workload", "tiny", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"], capture_output=True, text=True, timeout=300, env=env)
    assert bad.returncode != 0


def test_bench_json_contract_on_tiny_workload():
    """bench.py --full prints ONE JSON line with the driver's contract keys plus the `roofline` and `cpu_baseline` objects (run on the
    tiny workload so that the CPU leg takes a second); values are sane and the metric / config follow BASELINE.json's wording"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "tiny",
                          "--full"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", float),
                 ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert "vs_baseline" in d and d["vs_baseline"] is None                     # BASELINE.md publishes no number for this metric
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "images/s" and d["value"] > 0 and d["dtype"] == "f16" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - d["config"]["global_batch"] * 1e3 / d["ms_per_step"]) / d["value"] < 0.02
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and r["peak"] in (8000.0, 2500.0)
    assert r["achieved"] > 0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and "traffic" in r and "kernel" in r
    if r["bound"] == "mfma":       # the matrix rate this box sustains with no memory traffic (mlsd_probe_mfma_rate), reported beside the contract's peak
        assert 1000.0 < r["sustained_mfma_tflops_measured"] < 2600.0 and abs(r["frac_of_sustained_measured"] - r["achieved"] / r["sustained_mfma_tflops_measured"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] and c["value"] > 0 and c["unit"] == "images/s" and "oracle" in c["sample"]
    assert d["value"] > 2 * c["value"]       # sanity only: the tiny model is launch-bound on the GPU (79 images/s) and the round-5 oracle does 2.4 images/s on 16 CPUs; the ratio is no measure of anything
    m = d["unet_eval_mfma"]                                                       # time-weighted matrix-pipe fraction of one whole evaluation
    assert 0 < m["frac_of_mfma_peak"] < 1 and abs(m["frac_of_mfma_peak"] - m["tflops"] / 2500.0) < 1e-3 and m["by_family"]
    assert abs(sum(v["share"] for v in m["by_family"].values()) - 1) < 0.35       # (top six families)


def test_bench_plain_run_measures_the_headline_only():
    """Without --full bench.py runs set-up, warm-up and the timed steps and prints the contract keys; the PCIe-inclusive step, the roofline
    pass, the secondary workloads and the CPU baseline are --full's."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "tiny"],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["unit"] == "images/s" and d["dtype"] == "f16" and d["higher_is_better"] is True
    assert abs(d["value"] - d["config"]["global_batch"] * 1e3 / d["ms_per_step"]) / d["value"] < 0.02
    for k in ("roofline", "unet_eval_mfma", "cpu_baseline", "images_per_s_with_d2h_of_fp32_images", "sd15", "sdxl_tae"):
        assert k not in d, k


def test_bench_dump_outputs_repeat_bit_identically(tmp_path):
    """bench.py --dump-outputs: the final latents and decoded images of the last timed step, float32, the same bits from two processes
    with the same arguments (the inputs depend on the arguments only); with one more timed step the dump is that step's (other seeds)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for name, steps in (("a", 2), ("b", 2), ("c", 3)):
        d = tmp_path / name
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--workload", "tiny",
                              "--no-cpu-baseline", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["dump_outputs"]["dir"] == str(d)
        runs.append({k: np.load(d / f"{k}.npy") for k in ("latents", "images")})
    a, b, c = runs
    assert a["latents"].shape == (2, 4, 8, 8) and a["images"].shape == (2, 3, 64, 64)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and a[k].std() > 0
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert not np.array_equal(a["latents"], c["latents"])           # the last timed step of run c draws other seeds (image indices 4, 5)


def test_bench_line_carries_the_whole_baseline_metric():
    """beside the unchanged headline value the one JSON line of --full holds SD1.5 512x512 b1 (BASELINE configs[1]) and
    SDXL + TAESD as extra keys, each with its own roofline, and the CPU sample of BASELINE.md section 3 (one SD1.5 evaluation).
    Run with the tiny model as the headline (--extras) so that the test is about the keys, not about minutes of SDXL."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--workload", "tiny",
                          "--full", "--extras", "--extra-steps", "1"], capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    for key, cfg in (("sd15", "sd15-512x512"), ("sdxl_tae", "sdxl-1024x1024")):
        e = d[key]
        assert e["config"].startswith(cfg) and e["value"] > 0 and e["unit"] == "images/s" and e["ms_per_step"] > 0
        assert abs(e["value"] - (4 if key == "sdxl_tae" else 1) * 1e3 / e["ms_per_step"]) / e["value"] < 0.02
        assert e["roofline"]["frac"] > 0 and 0 < e["unet_eval_mfma"]["frac_of_mfma_peak"] < 1
        # the dominant label of the SDXL b4 / SD1.5 b1 plans is a key of the NEWEST committed PMC summaries (profiles/r<N>_*_pmc_{traffic,mfma}.json):
        # `traffic` can only be null again if somebody breaks tools/kernel_labels.py AND tests/test_profile_labels_cpu.py
        r_ = e["roofline"]
        assert r_["traffic"] and r_["traffic"] > 0 and r_["traffic_source"].startswith("profiles/r") and r_["mfma_busy_frac_pmc"], (key, r_["kernel"], r_["traffic_source"])
        assert r_["traffic"] >= 0.5 * r_["algorithmic_bytes_per_launch"], (key, r_)
    assert d["sdxl_tae"]["config"].endswith("-tae") and d["sd15"]["config"].endswith("-vae")
    # round 4: one rank's share of configs[3] (batch 8 per GPU) and configs[4] with the weights streamed (--unet-split)
    b8, sp = d["sdxl_b8"], d["sdxl_tae_split"]
    assert b8["config"] == "sdxl-1024x1024-euler_a-20-cfg7-b8-vae" and b8["value"] > 0 and b8["roofline"]["frac"] > 0 and b8["tile_table_misses"] == 0
    assert abs(b8["value"] - 8e3 / b8["ms_per_step"]) / b8["value"] < 0.02
    ws = sp["weight_streaming"]
    assert sp["config"].endswith("-tae") and sp["value"] > 0 and ws["segments"] >= 2 and ws["streamed_mib_per_eval"] > 3000 and ws["h2d_gb_per_s_sustained"] > 1
    assert ws["unet_params_on_device_mib"] < 2500 and sp["value"] < d["sdxl_tae"]["value"]          # PCIe-bound at batch 4: never faster than the resident plan
    assert d["sd15"]["tile_table_misses"] == 0 and d["cpu_baseline"]["host_cpus"] >= d["cpu_baseline"]["cores"]
    c15 = d["cpu_baseline"]["sd15"]
    assert c15["kind"] == "port" and c15["value"] > 0 and c15["s_per_unet_eval"] > 0 and "SD1.5" in c15["sample"] and c15["linear_weights"] == "f32" and d["sd15"]["value"] > 50 * c15["value"]       # (the GPU / CPU ratio asserted on a workload that is not launch-bound -- measured ~300 x;) configs[0] is the fp32 checkpoint: fp32 linear weights in the CPU sample (src/mlimgsynth.c:1235-1236)
