#!/usr/bin/env python3
"""Regenerates tests/golden/reference_answers.json.gz and tests/golden/clip_merges.npz (tests/reference_answers.py) from the
REFERENCE's own code: its Philox RNG, tensor-name conversion and prompt parser as oracle/Makefile builds them into oracle/_ref,
and its CLIP merge table src/clip_merges.c.h.  Only runs where the reference sources are present (after build()).

usage:  python tools/make_reference_answers.py <reference checkout>"""
import ctypes
import gzip
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import reference_answers as RA  # noqa: E402
import test_prompt_cpu  # noqa: E402

ref = sys.argv[1]
nums = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*\}", open(os.path.join(ref, "src", "clip_merges.c.h")).read())
pairs = np.array(nums, np.int64)
assert pairs.shape == (48894, 2) and pairs.max() < 65536
np.savez_compressed(RA.MERGES, pairs=pairs.astype(np.uint16))

tn, pp = ctypes.CDLL(RA.TNCONV_SO), ctypes.CDLL(RA.PROMPT_SO)
ans = {"_source": "outputs of the reference's own rng_philox_randn, tnconv_sd and prompt parser (oracle/_ref), tools/make_reference_answers.py",
       "rng": {f"{s},{o},{n}": RA.live_randn(s, o, n) for s, o, n in RA.RNG_CASES},
       "tnconv": {e: RA.live_tnconv(tn, e) for e, _ in RA.tiny_checkpoint_names()},
       "prompt": {t: RA.live_prompt(pp, t) for t in [k[0] for k in test_prompt_cpu.KATS] + RA.PROMPT_CASES}}
with gzip.GzipFile(RA.ANSWERS, "wb", compresslevel=9, mtime=0) as f:
    f.write(json.dumps(ans, ensure_ascii=False, sort_keys=True).encode("utf-8"))
print("wrote", RA.MERGES, "and", RA.ANSWERS)
