"""CTCBeamSearcher with an ARPA n-gram model fused into the device search (csrc/ctc_decode.hip ctc_beam_lm_kernel,
speechbrain_amd/decoders/ngram.py) against the fixture the reference's own search wrote (tools/make_ctc_lm_golden.py), on
the CPU emulator and on the MI355X (the `backend` fixture); the host restatement (tests/ctc_lm_host_ref.py) pinned to the
same fixture; and the search without a language model, which must not have moved."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import ctc_lm_host_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ctc_decode_lm.npz")
PLAIN = os.path.join(HERE, "golden", "ctc_decode.npz")
MARGIN = 1e-4


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    d = tmp_path_factory.mktemp("arpa")
    paths = {}
    for key, text in meta["arpa"].items():
        paths[key] = str(d / f"{key}.arpa")
        with open(paths[key], "w", encoding="utf-8") as f:
            f.write(text)
    return z, meta, paths


def _compare(hyps, case, label, stats, fused=True):
    """score and lm_score within 1e-4; texts and text_frames equal wherever the reference's adjacent top-k gaps (of the
    score it ranks by) exceed the margin."""
    assert len(hyps) == len(case["result"]), label
    for b, (got, ref) in enumerate(zip(hyps, case["result"])):
        assert len(got) == len(ref["text"]), (label, b)
        decided = len(ref["text"])
        for k, gap in enumerate(ref["gaps"]):
            if gap <= MARGIN:
                decided = k
                break
        for k in range(len(ref["text"])):
            stats["total"] += 1
            if k >= decided:
                continue
            stats["checked"] += 1
            assert abs(float(got[k].score) - ref["score"][k]) <= MARGIN, (label, b, k, got[k].score, ref["score"][k])
            if fused:
                assert abs(float(got[k].lm_score) - ref["lm_score"][k]) <= MARGIN, (label, b, k, got[k].lm_score,
                                                                                   ref["lm_score"][k])
            else:
                assert got[k].lm_score == got[k].score
            assert got[k].text == ref["text"][k], (label, b, k)
            assert [[w, list(f)] for w, f in got[k].text_frames] == ref["text_frames"][k], (label, b, k)
            assert got[k].last_lm_state is None


def test_ctc_lm_beam_search_kernel_matches_reference(backend, golden):
    """Every case of the fixture: orders 1, 2, 3 and 5, beams 1, 10 and 100, prune_history on and off with topk 3,
    score_boundary False, explicit unigrams, alpha = 0, two consecutive spaces, an utterance of length 0, posteriors wider
    than the vocabulary; characters and SentencePiece-style pieces."""
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    native, dev = backend
    z, meta, paths = golden
    stats = {"checked": 0, "total": 0}
    for i, case in enumerate(meta["cases"]):
        s = CTCBeamSearcher(blank_index=0, vocab_list=case["vocab"], space_token=" ",
                            kenlm_model_path=paths[case["arpa"]], **case["kwargs"])
        assert s.lm.order == int(case["arpa"][-1])
        x, lens = torch.from_numpy(z[f"case{i}_x"]).to(dev), torch.from_numpy(z[f"case{i}_lens"]).to(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            hyps = s(x, lens)
        _compare(hyps, case, case["name"], stats)
    assert stats["checked"] >= 0.8 * stats["total"], stats


def test_ctc_lm_host_restatement_matches_reference(golden):
    from speechbrain_amd.decoders.ngram import NgramLM

    z, meta, paths = golden
    stats = {"checked": 0, "total": 0}
    for i, case in enumerate(meta["cases"]):
        kw = dict(case["kwargs"])
        lm = NgramLM(paths[case["arpa"]], **{k: kw.pop(k) for k in ("unigrams", "alpha", "beta", "unk_score_offset",
                                                                   "score_boundary") if k in kw})
        hyps = ctc_lm_host_ref.beam_search(z[f"case{i}_x"], z[f"case{i}_lens"], blank=0, vocab=case["vocab"], lm=lm, **kw)
        _compare(hyps, case, case["name"], stats)
    assert stats["checked"] >= 0.8 * stats["total"], stats


def test_ctc_lm_start_state_is_refused(golden):
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    _, meta, paths = golden
    s = CTCBeamSearcher(blank_index=0, vocab_list=meta["cases"][0]["vocab"], kenlm_model_path=paths["char2"])
    with pytest.raises(NotImplementedError, match="lm_start_state"):
        s(torch.zeros(1, 4, 31), None, lm_start_state=object())


def test_ctc_beam_search_without_lm_is_unchanged(backend):
    """sbk_ctc_beam_search_f32 (the kLm = false instantiation of the shared kernel body) on tests/golden/ctc_decode.npz,
    with the comparison of tests/test_ctc_decode.py; passes before and after the fused kernel exists."""
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    native, dev = backend
    z = np.load(PLAIN)
    meta = json.loads(str(z["meta"]))
    stats = {"checked": 0, "total": 0}
    for i, case in enumerate(meta["beam"]):
        x, lens = torch.from_numpy(z[f"beam{i}_x"]).to(dev), torch.from_numpy(z[f"beam{i}_lens"]).to(dev)
        s = CTCBeamSearcher(blank_index=0, vocab_list=case["vocab"], space_token=" ", **case["kwargs"])
        assert s.lm is None
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            hyps = s(x, lens)
        _compare(hyps, case, case["name"], stats, fused=False)
    assert stats["checked"] >= 0.8 * stats["total"], stats
