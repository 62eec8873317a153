"""The ARPA loader and the n-gram tables of speechbrain_amd/decoders/ngram.py: known answers through the tables the device
reads (and through the kenlm stand-in that tools/make_ctc_lm_golden.py serves to the reference), and the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the four-word bigram model of the KenlmScorer docstring: score(start, "Hello") is -0.803
HELLO = ("\\data\\\nngram 1=4\nngram 2=1\n\n\\1-grams:\n-1.0\t<s>\t-1.0\n-1.0\t</s>\t-1.0\n-1.0\tHello\t-0.23\n"
         "-0.7\tworld\t-0.25\n\n\\2-grams:\n-0.3\tHello world\n\n\\end\\")
# a trigram model for back-off by hand
TRIGRAM = """\\data\\
ngram 1=6
ngram 2=3
ngram 3=1

\\1-grams:
-2.0\t<unk>\t-0.1
-99\t<s>\t-0.5
-1.5\t</s>
-1.0\ta\t-0.4
-1.2\tb\t-0.3
-1.4\tc\t-0.2

\\2-grams:
-0.6\t<s> a\t-0.25
-0.7\ta b\t-0.15
-0.9\tb c

\\3-grams:
-0.2\t<s> a b

\\end\\
"""


def _write(tmp_path, text, name="lm.arpa"):
    p = tmp_path / name
    p.write_text(text, encoding="utf-8")
    return str(p)


def _standin():
    sys.path.insert(0, os.path.join(ROOT, "tools", "ref_standins"))
    try:
        import importlib

        return importlib.import_module("kenlm")
    finally:
        sys.path.pop(0)


def test_hello_world_known_answer(tmp_path):
    from speechbrain_amd.decoders.ngram import NgramLM

    # (the docstring's model has no <unk>; kenlm substitutes one, our loader wants it spelled out)
    text = HELLO.replace("ngram 1=4", "ngram 1=5").replace("\\1-grams:\n", "\\1-grams:\n-100\t<unk>\n")
    lm = NgramLM(_write(tmp_path, text), unigrams=["Hello", "world"])
    assert lm.order == 2
    score, ctx = lm.score(lm.start_context(), "Hello")
    # no "<s> Hello" bigram: p(Hello) + backoff(<s>) = -2.0; 0.5 * -2.0 * ln 10 + 1.5
    assert round(score, 3) == -0.803
    score, _ = lm.score(ctx, "world")
    assert abs(score - (0.5 * -0.3 / np.log10(np.e) + 1.5)) < 1e-6
    m = _standin().Model(_write(tmp_path, text))
    st, out = _standin().State(), _standin().State()
    m.BeginSentenceWrite(st)
    assert abs(m.BaseScore(st, "Hello", out) - -2.0) < 1e-6 and abs(m.BaseScore(out, "world", st) - -0.3) < 1e-6
    assert "Hello" in m and "<unk>" not in m and "nope" not in m and m.order == 2


@pytest.mark.parametrize("score_boundary", [True, False])
def test_trigram_backoff_by_hand(tmp_path, score_boundary):
    from speechbrain_amd.decoders.ngram import NgramLM

    lm = NgramLM(_write(tmp_path, TRIGRAM), alpha=1.0, beta=0.0, unk_score_offset=-10.0, score_boundary=score_boundary)
    ln10 = 1.0 / np.log10(np.e)
    wid = lm.model.word_id
    f = np.float32
    if score_boundary:
        # <s> a: the bigram; <s> a b: the trigram; a b c: no trigram, no "a b" context miss -> backoff(a b) + p(c | b)
        want = [("a", f(-0.6)), ("b", f(-0.2)), ("c", f(f(-0.9) + f(-0.15))),
                # b c a: nothing longer than the unigram: p(a) + backoff(c) + backoff(b c) (absent: 0)
                ("a", f(f(-1.0) + f(-0.2))),
                # an unknown word: <unk>'s unigram + backoff(a) + backoff(c a) (absent), and the OOV offset
                ("zzz", f(f(-2.0) + f(-0.4)))]
    else:
        want = [("a", f(-1.0)), ("b", f(-0.7)), ("c", f(f(-0.9) + f(-0.15)))]
    ctx = lm.start_context()
    assert ctx == ((wid["<s>"],) if score_boundary else ())
    m = _standin().Model(_write(tmp_path, TRIGRAM, "again.arpa"))
    st = _standin().State()
    (m.BeginSentenceWrite if score_boundary else m.NullContextWrite)(st)
    for word, logp in want:
        score, ctx = lm.score(ctx, word)
        off = -10.0 if word == "zzz" else 0.0
        assert abs(score - (float(logp) + off) * ln10) < 1e-9, (word, score)
        out = _standin().State()
        assert abs(m.BaseScore(st, word, out) - float(logp)) < 1e-7, word
        st = out
    assert len(ctx) == 2
    # the unigram set is read as load_unigram_set_from_arpa reads it: three-field lines only ("</s>" has two), and
    # <unk> is not "in" the model
    assert lm.unigram_set == {"<s>", "a", "b", "c"}
    assert lm.score_partial_token("a") == 0.0 and lm.score_partial_token("ab") == -10.0
    assert abs(lm.score_partial_token("abcdefgh") - -10.0 * 8 / 6) < 1e-12


def test_tables_and_standin_agree_at_order_five(tmp_path):
    """Two implementations written apart (dictionaries of word tuples; hashed tables of ids) on a random 5-gram model:
    contexts shorter than, equal to and longer than the model's, in-vocabulary and unknown words."""
    from speechbrain_amd.decoders.ngram import NgramLM
    from tools.arpa_synth import arpa_text

    words = ["w%d" % i for i in range(12)]
    path = _write(tmp_path, arpa_text(words, 5, seed=9, per_order=150))
    lm, m = NgramLM(path), _standin().Model(path)
    rng = np.random.RandomState(3)
    for boundary in (True, False):
        lm.score_boundary = boundary
        ctx, st = lm.start_context(), _standin().State()
        (m.BeginSentenceWrite if boundary else m.NullContextWrite)(st)
        for _ in range(200):
            word = words[rng.randint(12)] if rng.rand() < 0.9 else "oov"
            out = _standin().State()
            want = m.BaseScore(st, word, out)
            v = lm.string_value(word)
            got = float(lm.word_logp(ctx, (v >> 2) - 1 if v >> 2 else lm.unk_id))
            assert got == want, (word, ctx, got, want)
            _, ctx = lm.score(ctx, word)
            st = out


def test_tables_hold_every_prefix_word_and_ngram(tmp_path):
    from speechbrain_amd.decoders.ctc import string_hash
    from speechbrain_amd.decoders.ngram import NgramLM, hash_strings
    from tools.arpa_synth import arpa_text

    words = ["w%d" % i + "xyz"[: i % 4] for i in range(300)] + ["ünï", "abandonment"]
    lm = NgramLM(_write(tmp_path, arpa_text(words, 4, seed=5, two_field=("w7xyz",))), unigrams=words[:200])
    h1, h2 = hash_strings(words)
    assert [(int(a), int(b)) for a, b in zip(h1, h2)] == [(string_hash(w)[0], string_hash(w)[2]) for w in words]
    for i, w in enumerate(words):
        v = lm.string_value(w)
        assert (v >> 2) - 1 == lm.model.word_id[w] and bool(v & 2) == (i < 200) and bool(v & 1) == (i < 200 or w == "w7")
    assert lm.string_value("w1") & 1 and lm.string_value("w1") >> 2 == 0 and lm.string_value("nope") == 0
    for n, (ids, logp, bo) in lm.model.ngrams.items():
        for k in range(0, len(ids), 7):
            hit = lm.ngram(list(ids[k][::-1]))
            assert hit is not None and hit[0] == logp[k] and hit[1] == bo[k]
    assert lm.n_ngrams == sum(len(v[0]) for v in lm.model.ngrams.values())


def test_hash_collision_is_detected(tmp_path):
    from speechbrain_amd.decoders.ngram import NgramLM

    def weak(strings):  # every string of a length hashes alike
        z = np.zeros(len(strings), dtype=np.uint32)
        return z, z

    with pytest.raises(ValueError, match="share both character hashes"):
        NgramLM(_write(tmp_path, TRIGRAM), hash_fn=weak)


def test_refusals(tmp_path):
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher
    from speechbrain_amd.decoders.ngram import NgramLM
    from tools.arpa_synth import arpa_text

    with pytest.raises(ValueError, match="<unk>"):
        NgramLM(_write(tmp_path, HELLO, "hello.arpa"))
    with pytest.raises(NotImplementedError, match="orders above 5"):
        NgramLM(_write(tmp_path, arpa_text(["a", "b", "c"], 6, seed=1), "six.arpa"))
    binary = tmp_path / "lm.bin"
    binary.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\x00\x01\xff\xfe" + bytes(range(256)))
    with pytest.raises(NotImplementedError, match="ARPA"):
        CTCBeamSearcher(blank_index=0, vocab_list=["-", "a", " "], kenlm_model_path=str(binary))
    with pytest.raises(NotImplementedError, match="ARPA"):
        NgramLM(_write(tmp_path, "not a model\n", "text.arpa"))
    # a model file that is not named *.arpa has no unigram set (the reference reads unigrams from *.arpa files only)
    lm = NgramLM(_write(tmp_path, TRIGRAM, "model.txt"))
    assert lm.unigram_set == set() and lm.score_partial_token("a") == -10.0
    assert lm.score(lm.start_context(), "a")[0] == NgramLM(_write(tmp_path, TRIGRAM)).score((lm.bos_id,), "a")[0]
