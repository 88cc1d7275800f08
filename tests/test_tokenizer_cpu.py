"""CLIP tokenizer (csrc/host/clip_tokenizer.c) against the reference's 14 known-answer tests
(src/test_text_tokenize_clip.c:41-66, committed as data in tests/golden/reference_kats.json).

The BPE merge table is user-supplied data in this engine (the reference compiles src/clip_merges.c.h in).  The tests
read its id pairs from tests/golden/clip_merges.npz (tests/reference_answers.py), and also spell them out in OpenAI's
public vocabulary format to exercise the text loader."""
import json
import os

import numpy as np
import pytest

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))["clip_tokenize_kats"]["cases"]


@pytest.fixture(scope="module")
def T():
    from mlimgsynth_amd import text
    return text


@pytest.fixture(scope="module")
def pairs():
    import reference_answers as RA
    p = RA.clip_merges()
    assert p.shape == (48894, 2)
    return p


def test_byte_token_maps_are_clip_bytes_to_unicode(T):
    """ids 0..255 = bytes in the order of OpenAI's bytes_to_unicode(): '!'..'~', '¡'..'¬', '®'..'ÿ', then the rest."""
    from mlimgsynth_amd._lib import lib
    order = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    order += [b for b in range(256) if b not in order]
    for tok, b in enumerate(order):
        assert lib().clip_tokr_byte_to_token(b) == tok
        assert lib().clip_tokr_token_to_byte(tok) == b


def test_word_split_without_merges(T):
    """With an empty merge table the output is the byte tokens of each word, last one +256: isolates the word rules."""
    tk = T.ClipTokenizer.from_pairs(np.zeros((0, 2), np.int32))
    assert tk.n_vocab == 514
    b = lambda ch: ord(ch) - 33                        # printable ASCII byte -> token
    assert tk.encode("") == [] and tk.encode(" \t\n 　 ") == []
    assert tk.encode("Ab") == [b("a"), b("b") + 256]                               # lower-cased
    assert tk.encode("ab12") == [b("a"), b("b") + 256, b("1"), b("2") + 256]       # letters | digit RUN (reference rule)
    assert tk.encode("a,.b") == [b("a") + 256, b(","), b(".") + 256, b("b") + 256]
    assert tk.encode("it's") == [b("i"), b("t") + 256, b("'"), b("s") + 256]       # contraction splits
    assert tk.encode("IT'S") == [b("i"), b("t") + 256, b("'"), b("s") + 256]
    assert tk.encode("a'd") == [b("a") + 256, b("'") + 256, b("d") + 256]          # 'd is NOT in the reference's list
    assert tk.encode("É") == [0xC3 - 68, 0xA9 - 67 + 256]                     # É -> é = C3 A9


def test_bad_merge_tables_are_rejected(T):
    from mlimgsynth_amd._lib import MlsdError
    with pytest.raises(MlsdError):
        T.ClipTokenizer.from_pairs(np.array([[5, 600]], np.int32))      # refers to a merge not yet defined
    with pytest.raises(MlsdError):
        T.ClipTokenizer.from_pairs(np.array([[5, 6], [5, 6]], np.int32))  # duplicate
    with pytest.raises(MlsdError):
        T.ClipTokenizer.from_file("/nonexistent/merges.txt")


def test_reference_kats(T, pairs):
    tk = T.ClipTokenizer.from_pairs(pairs)
    assert tk.n_vocab == 49408                          # clip.c:264 assert; ClipParams.n_vocab
    for text, want in GOLD:
        assert tk.encode(text) == want, text


def test_openai_vocab_text_loader(T, pairs, tmp_path):
    """Spell the id pairs in the public bpe_simple_vocab format and load them back: same table, same KATs."""
    tk = T.ClipTokenizer.from_pairs(pairs)

    def spell(tok):
        raw, eow = tk.token_bytes(tok)
        s = "".join(chr(c) if (33 <= c <= 126 or 161 <= c <= 172 or 174 <= c <= 255) else
                    chr(256 + [b for b in range(256) if not (33 <= b <= 126 or 161 <= b <= 172 or 174 <= b <= 255)].index(c))
                    for c in raw)
        return s + ("</w>" if eow else "")
    f = tmp_path / "bpe_simple_vocab_16e6.txt"
    with open(f, "w", encoding="utf-8") as fh:
        fh.write('"#version: 0.2\n'.lstrip('"'))
        for l, r in pairs:
            fh.write(f"{spell(int(l))} {spell(int(r))}\n")
        fh.write("zz zz\n")                              # the real file has more lines than CLIP uses: must be ignored
    tk2 = T.ClipTokenizer.from_file(f)
    assert tk2.n_merges == 48894
    for text, want in GOLD:
        assert tk2.encode(text) == want, text
    # decode round trip on the long KAT
    text, want = GOLD[-1]
    assert tk2.decode(want) == "stable diffusion is a deep learning , text - to - image model released in 2022 based on diffusion techniques ."
