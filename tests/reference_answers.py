"""Answers of the reference's own code for the tests that compare against it: the Philox RNG, the tensor-name conversion and
the prompt parser (oracle/_ref, compiled by oracle/Makefile where the reference sources are present) and the CLIP merge table.
The answers are stored in tests/golden/ (tools/make_reference_answers.py) so that the tests run on every checkout; where
oracle/_ref is built, every stored answer a test uses is also checked against the live build."""
import ctypes
import gzip
import json
import os

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ANSWERS = os.path.join(GOLD, "reference_answers.json.gz")
MERGES = os.path.join(GOLD, "clip_merges.npz")
TNCONV_SO = os.path.join(ROOT, "oracle", "_ref", "libtnconv_ref.so")
PROMPT_SO = os.path.join(ROOT, "oracle", "_ref", "libprompt_ref.so")

# (seed, offset, n) of the RNG comparison
RNG_CASES = [(0, 0, 12), (42, 0, 4096), (42, 7, 1000), (2**40 + 17, 123456, 777), (2**64 - 1, 2**32 - 1, 50)]
# prompts of the parser comparison beside the known-answer cases of tests/test_prompt_cpu.py, error cases included
PROMPT_CASES = [
    "", "()", "(a)(b)[c]", "a ((b) c) d", "x (y:0.25)z", "[[deep]] (mix [of] both)", "line\\nbreak", "a BREAK b BREAKING", "BREAK",
    "<lora:one><lora:two:1.5> tail", "(a:1.2", "a) b", "a] b", "(a [b:2])", "[a:2]", "<lora:bad:1.x>", "<lorax:foo>", "<unclosed", "(w:)",
    "((a:2))", "trailing\\", "(:1.5)", "a (b:1.5e-1) c", "éè (中文:1.3)"]


def tiny_checkpoint_names():
    """(external checkpoint name, internal parameter key) of every parameter of the tiny / tinyxl models."""
    import ckpt_names as CN
    import loader_cases as LC
    out = []
    for model in ("tiny", "tinyxl"):
        for k, _, _ in LC.model_params(model):
            e = CN.external_name(k, "sd1" if model == "tiny" else "sdxl")
            out.append((e[1] if isinstance(e, tuple) else e, k))
    return out

_stored = None


def stored():
    global _stored
    if _stored is None:
        with gzip.open(ANSWERS, "rt", encoding="utf-8") as f:
            _stored = json.load(f)
    return _stored


def _lib(path):
    return ctypes.CDLL(path) if os.path.exists(path) else None


def live_randn(seed, off, n):
    ref, ref_off = O.ref_randn(seed, off, n)
    return [[int(v) for v in ref.view(np.uint32)], int(ref_off)]


def live_tnconv(ref, name):
    buf = ctypes.create_string_buffer(1024)
    r = ref.ref_tnconv_sd(name.encode(), buf, 1024)
    return [r, buf.value.decode()]


def live_prompt(ref, text):
    ref.ref_prompt_parse.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    buf = ctypes.create_string_buffer(8192)
    rr = ref.ref_prompt_parse(text.encode(), 0, buf, 8192)
    return [rr, buf.value.hex()]


def randn(seed, off, n):
    """rng_philox_randn(seed, off, n) of the reference: (float32 values, offset after the call)."""
    bits, ref_off = stored()["rng"][f"{seed},{off},{n}"]
    if os.path.exists(O.REF_RNG_SO):
        assert live_randn(seed, off, n) == [bits, ref_off], (seed, off, n)
    return np.array(bits, np.uint32).view(np.float32), ref_off


def tnconv():
    """name -> [return code, converted name] of the reference's tnconv_sd."""
    ref, table = _lib(TNCONV_SO), stored()["tnconv"]

    def f(name):
        want = table[name]
        if ref:
            assert live_tnconv(ref, name) == want, name
        return want
    return f


def prompt_parse():
    """text -> (return code, output buffer) of the reference's prompt parser (behind oracle/ref_harness/prompt_harness.c)."""
    ref, table = _lib(PROMPT_SO), stored()["prompt"]

    def f(text):
        want = table[text]
        if ref:
            assert live_prompt(ref, text) == want, text
        return want[0], bytes.fromhex(want[1])
    return f


def clip_merges():
    """The CLIP BPE merge table as token id pairs [48894][2] (OpenAI's bpe_simple_vocab_16e6, as the reference compiles it in)."""
    return np.load(MERGES)["pairs"].astype(np.int32)
