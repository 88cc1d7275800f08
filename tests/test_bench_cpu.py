"""bench.py parts that need no GPU: the --dump-outputs writer (size limit, fixed sample), the --steps check and the options that only --full takes."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_whole_arrays_when_they_fit(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"latents": rng.standard_normal((4, 4, 128, 128)).astype(np.float32),
              "images": rng.random((4, 3, 1024, 1024), np.float32)}           # the SDXL batch-4 headline: 51.4 MB of outputs
    info = bench.dump_outputs(str(tmp_path), arrays)
    for name, x in arrays.items():
        y = np.load(tmp_path / f"{name}.npy")
        assert y.dtype == np.float32 and np.array_equal(y, x)
        assert info[name] == {"shape": list(x.shape), "sampled_elements": None}


def test_dump_outputs_samples_the_same_elements_under_the_limit(tmp_path):
    rng = np.random.default_rng(1)
    lat = rng.standard_normal((8, 4, 128, 128)).astype(np.float32)
    img = rng.random((8, 3, 1024, 1024), np.float32)                           # batch 8: 100.7 MB of images
    info = bench.dump_outputs(str(tmp_path / "a"), {"latents": lat, "images": img})
    assert info["latents"]["sampled_elements"] is None and info["images"]["shape"] == [8, 3, 1024, 1024]
    a = np.load(tmp_path / "a" / "images.npy")
    assert a.ndim == 1 and a.size == info["images"]["sampled_elements"] > 0.99 * (bench.DUMP_BYTES - lat.nbytes) / 4
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_BYTES
    assert np.isin(a, img).all()
    # another output of the same shape: the same element positions are kept
    img2 = img + 1.0
    bench.dump_outputs(str(tmp_path / "b"), {"latents": lat, "images": img2})
    assert np.array_equal(np.load(tmp_path / "b" / "images.npy"), a + 1.0)


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_parts_of_full_are_refused_alone():
    for opt in (["--kernel-table", "t.txt"], ["--extras"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + opt, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, opt
