"""ctc_beam_lm_kernel against the host restatement (tests/ctc_lm_host_ref.py, pinned to the reference's fixture by
tests/test_ctc_lm.py) at shapes the fixture does not cover: a 300-piece vocabulary (the second 256-token chunk), the largest
beam the entry accepts, a long utterance, and a 2 000-word lexicon at order 4 (tables of thousands of slots).  The
posteriors follow sentences over the lexicon (with unknown words), so that the n-gram tables are walked."""
import warnings

import numpy as np
import pytest
import torch

import ctc_lm_host_ref
from tools.arpa_synth import arpa_text

MARGIN = 1e-4
LETTERS = "abcdefghij"


def _lexicon(n, seed):
    rng = np.random.RandomState(seed)
    words = set()
    while len(words) < n:
        words.add("".join(LETTERS[k] for k in rng.randint(0, len(LETTERS), size=rng.randint(1, 10))))
    return sorted(words)


def _spm_vocab(n_pieces, seed):
    rng = np.random.RandomState(seed)
    pieces = {"▁"} | {"▁" + c for c in LETTERS} | set(LETTERS)
    while len(pieces) < n_pieces - 1:
        p = "".join(LETTERS[k] for k in rng.randint(0, len(LETTERS), size=rng.randint(2, 4)))
        pieces.add(("▁" if rng.rand() < 0.4 else "") + p)
    return ["<blank>"] + sorted(pieces)


def _posteriors(vocab, sentences, T, seed, peak, noise):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(len(sentences), T, len(vocab), generator=g) * noise
    for b, toks in enumerate(sentences):
        frames, prev = [], None
        for v in toks:
            if v == prev:
                frames.append(0)
            frames += [v] * (1 + int(torch.randint(0, 2, (1,), generator=g)))
            prev = v
        frames = (frames + [0] * T)[:T]
        z[b, torch.arange(T), torch.tensor(frames)] += peak
    return torch.log_softmax(z, dim=-1)


def _char_sentence(vocab, words, rng, n):
    text = " ".join(words[rng.randint(len(words))] if rng.rand() < 0.8 else "jjjjjjjj"[: rng.randint(2, 9)] for _ in range(n))
    return [vocab.index(c) for c in text]


def _check(backend, tmp_path, vocab, x, lens, words, order, **kw):
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    native, dev = backend
    path = str(tmp_path / "lm.arpa")
    with open(path, "w", encoding="utf-8") as f:
        f.write(arpa_text(words, order, seed=order, per_order=4 * len(words)))
    s = CTCBeamSearcher(blank_index=0, vocab_list=vocab, kenlm_model_path=path, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = s(x.to(dev), None if lens is None else lens.to(dev))
    want = ctc_lm_host_ref.beam_search(x, lens, blank=0, vocab=vocab, lm=s.lm, **kw)
    checked = total = 0
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), b
        fused = [float(h.lm_score) for h in w]
        decided = next((k for k in range(len(w) - 1) if fused[k] - fused[k + 1] <= MARGIN), len(w))
        total += len(w)
        for k in range(decided):
            checked += 1
            assert abs(float(g[k].score) - float(w[k].score)) <= MARGIN, (b, k)
            assert abs(float(g[k].lm_score) - fused[k]) <= MARGIN, (b, k)
            assert g[k].text == w[k].text and g[k].text_frames == w[k].text_frames, (b, k)
    assert checked >= 0.8 * total, (checked, total)
    return want


def test_ctc_lm_three_hundred_pieces(backend, tmp_path):
    vocab = _spm_vocab(300, 1)
    words = _lexicon(40, 2)
    rng = np.random.RandomState(3)
    starts = [v for v, p in enumerate(vocab) if p.startswith("▁") and len(p) > 1]
    inner = [v for v, p in enumerate(vocab) if not p.startswith("▁") and v > 0]
    sentences = [[(starts if rng.rand() < 0.4 else inner)[rng.randint(20)] for _ in range(18)] for _ in range(2)]
    x = _posteriors(vocab, sentences, 36, 4, peak=6.0, noise=1.0)
    _check(backend, tmp_path, vocab, x, torch.tensor([1.0, 0.7]), words, 3, beam_size=12, topk=3, prune_history=True)


def test_ctc_lm_beam_at_the_cap(backend, tmp_path):
    """beam_size 256: 4 * 256 beam records of 128 bytes in LDS (128 KiB), every slot in use on flat posteriors."""
    vocab = ["<blank>", " "] + list(LETTERS)
    words = _lexicon(30, 5)
    rng = np.random.RandomState(6)
    x = _posteriors(vocab, [_char_sentence(vocab, words, rng, 3)], 14, 7, peak=2.5, noise=1.0)
    want = _check(backend, tmp_path, vocab, x, None, words, 5, beam_size=256, topk=256, prune_history=False,
                  token_prune_min_logp=-4.0, beam_prune_logp=-40.0)
    assert len(want[0]) > 100  # (the fused search held more than a hundred distinct texts at the end)
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    native, dev = backend
    s = CTCBeamSearcher(blank_index=0, vocab_list=vocab, kenlm_model_path=str(tmp_path / "lm.arpa"), beam_size=257)
    with pytest.raises(native.SbkError, match="beam_size 257"):
        s(x.to(dev))


def test_ctc_lm_long_utterance(backend, tmp_path):
    vocab = ["<blank>", " "] + list(LETTERS)
    words = _lexicon(60, 8)
    rng = np.random.RandomState(9)
    x = _posteriors(vocab, [_char_sentence(vocab, words, rng, 70)], 600, 10, peak=7.0, noise=1.0)
    _check(backend, tmp_path, vocab, x, torch.tensor([1.0]), words, 3, beam_size=8, topk=2, prune_history=True)


def test_ctc_lm_two_thousand_words_at_order_four(backend, tmp_path):
    vocab = ["<blank>", " "] + list(LETTERS)
    words = _lexicon(2000, 11)
    rng = np.random.RandomState(12)
    x = _posteriors(vocab, [_char_sentence(vocab, words, rng, 9) for _ in range(3)], 64, 13, peak=6.0, noise=1.1)
    _check(backend, tmp_path, vocab, x, torch.tensor([1.0, 0.9, 0.5]), words, 4, beam_size=20, topk=3, prune_history=True)
