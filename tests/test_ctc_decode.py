"""CTC decoding (csrc/ctc_decode.hip, speechbrain_amd/decoders/ctc.py) against fixtures the reference wrote
(tools/make_ctc_golden.py), on the CPU emulator and on the MI355X (the `backend` fixture), plus the host restatement
(tests/ctc_host_ref.py) pinned to the same fixtures and the EncoderASR interface."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ctc_host_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ctc_decode.npz")
MARGIN = 1e-4


def _golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def _searcher(case):
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    return CTCBeamSearcher(blank_index=0, vocab_list=case["vocab"], space_token=" ", **case["kwargs"])


def _compare(hyps, case, label, stats):
    """Scores within 1e-4; texts and text_frames equal wherever the reference's adjacent top-k gaps exceed the margin."""
    assert len(hyps) == len(case["result"]), label
    for b, (got, ref) in enumerate(zip(hyps, case["result"])):
        assert len(got) == len(ref["text"]), (label, b)
        decided = len(ref["text"])  # hypotheses whose rank is decided by more than the margin on both sides
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
            assert got[k].text == ref["text"][k], (label, b, k)
            frames = [[w, list(f)] for w, f in got[k].text_frames]
            assert frames == ref["text_frames"][k], (label, b, k)
            assert got[k].lm_score == got[k].score and got[k].last_lm_state is None


def test_ctc_greedy_decode_kernel_matches_reference(backend):
    from speechbrain_amd.decoders.ctc import ctc_greedy_decode

    native, dev = backend
    z, meta = _golden()
    for i, case in enumerate(meta["greedy"]):
        x = torch.from_numpy(z[f"greedy{i}_x"]).to(dev)
        lens = torch.from_numpy(z[f"greedy{i}_lens"]).to(dev)
        blank = case["blank"] % x.shape[-1]
        tokens, count = native.ctc_greedy_decode(x, lens, blank)
        got = [row[:n] for row, n in zip(tokens.cpu().tolist(), count.cpu().tolist())]
        assert got == case["result"], i
        if dev.type == "cuda":
            assert ctc_greedy_decode(x, lens, blank_id=case["blank"]) == case["result"]
        # the host path of the same utility (CPU tensors)
        assert ctc_greedy_decode(x.cpu(), lens.cpu(), blank_id=case["blank"]) == case["result"]


def test_ctc_beam_search_kernel_matches_reference(backend):
    native, dev = backend
    z, meta = _golden()
    stats = {"checked": 0, "total": 0}
    for i, case in enumerate(meta["beam"]):
        x = torch.from_numpy(z[f"beam{i}_x"]).to(dev)
        lens = torch.from_numpy(z[f"beam{i}_lens"]).to(dev)
        with pytest.warns(UserWarning) if x.shape[-1] != len(case["vocab"]) else _nullctx():
            hyps = _searcher(case)(x, lens)
        _compare(hyps, case, case["name"], stats)
    # the margin rule must leave most hypotheses checked
    assert stats["checked"] >= 0.8 * stats["total"], stats


def test_host_restatement_matches_reference():
    """tests/ctc_host_ref.py (no reference code) against the reference's own outputs: tests/test_decode_shapes.py and
    tests/test_ctc_full_size_gpu.py use it as their yardstick at shapes the fixtures do not cover (wide vocabularies,
    beams above 100, long inputs, a blank index other than 0)."""
    z, meta = _golden()
    stats = {"checked": 0, "total": 0}
    for i, case in enumerate(meta["beam"]):
        x, lens = torch.from_numpy(z[f"beam{i}_x"]), torch.from_numpy(z[f"beam{i}_lens"])
        hyps = ctc_host_ref.beam_search(x, lens, blank=0, vocab=case["vocab"], space_token=" ", **case["kwargs"])
        _compare(hyps, case, case["name"], stats)
    assert stats["checked"] >= 0.8 * stats["total"], stats


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def test_ctc_decode_bad_arguments_are_reported(backend):
    native, dev = backend
    lib = native.load()
    x = torch.zeros(1, 4, 5, device=dev)
    tok = torch.zeros(1, 4, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.sbk_ctc_greedy_decode_f32(p(x), None, p(tok), p(cnt), 1, 4, 5, 5, None) == -22
    assert b"blank" in lib.sbk_last_error()
    assert lib.sbk_ctc_greedy_decode_f32(None, None, p(tok), p(cnt), 1, 4, 5, 0, None) == -22
    assert lib.sbk_ctc_greedy_decode_f32(None, None, None, None, 0, 4, 5, 0, None) == 0  # empty batch
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    s = CTCBeamSearcher(blank_index=0, vocab_list=["-", "a", "b", " ", "c"], beam_size=257)
    with pytest.raises(native.SbkError, match="beam_size 257"):
        s(x)
    s = CTCBeamSearcher(blank_index=0, vocab_list=["-", "a", "b", " ", "c"], beam_size=4, topk=5)
    with pytest.raises(native.SbkError, match="topk"):
        s(x)
    cfg = s.config()
    assert lib.sbk_ctc_beam_search_f32(p(x), None, p(tok), 5, None, p(tok), 16, p(tok), p(x), p(cnt), 1, 4, 5, None) == -22
    cfg.topk = 1
    assert lib.sbk_ctc_beam_search_f32(p(x), None, p(tok), 5, ctypes.byref(cfg), p(tok), 4, p(tok), p(x), p(cnt), 1, 4, 5,
                                       None) == -22
    assert b"workspace" in lib.sbk_last_error()
    with pytest.raises(NotImplementedError):
        CTCBeamSearcher(blank_index=0, vocab_list=["-", "a"], kenlm_model_path="lm.arpa")
    with pytest.raises(NotImplementedError):
        s.partial_decode_beams(x, {}, {}, [], 0)


def test_ctc_beam_search_nan_does_not_hang(backend):
    """NaN posteriors neither fault nor hang the search (the result itself is unspecified)."""
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    native, dev = backend
    x = torch.log_softmax(torch.randn(2, 12, 6, generator=torch.Generator().manual_seed(3)), -1)
    x[0, 3:5] = float("nan")
    x[1, :, 2] = float("nan")
    s = CTCBeamSearcher(blank_index=0, vocab_list=["-", "a", "b", " ", "c", "d"], beam_size=8, topk=2,
                        token_prune_min_logp=-50.0)
    hyps = s(x.to(dev))
    assert len(hyps) == 2


# ------------------------------------------------------------------ EncoderASR on a CTC model directory
GOLD = os.path.join(HERE, "golden")
CTC_DIR = os.path.join(GOLD, "pretrained_ctc_tiny")


@pytest.mark.parametrize("yaml,key", [("hyperparams.yaml", "greedy"), ("hyperparams_beam.yaml", "beam")])
def test_encoder_asr_from_hparams_matches_reference(backend, yaml, key):
    """EncoderASR.from_hparams on tests/golden/pretrained_ctc_tiny (the CTC recipe's layout; checkpoints and the
    CTCTextEncoder label file written by the reference's savers, tools/make_ctc_golden.py): the words of the reference's
    EncoderASR on the same batch and files, for the `!name:` partial (greedy) and the bare searcher class (beam 100) forms
    of decoding_function.  The encoder's LogSoftmax runs on sbk_log_softmax_f32."""
    import functools

    from speechbrain_amd.dataio.encoder import CTCTextEncoder
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderASR
    from speechbrain_amd.nnet.activations import NativeLogSoftmax

    native, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_ctc_tiny_expected.npz"))
    asr = EncoderASR.from_hparams(source=CTC_DIR, hparams_file=yaml, run_opts={"device": str(dev)})
    assert isinstance(asr.tokenizer, CTCTextEncoder) and asr.tokenizer.get_blank_index() == 0
    assert len(asr.tokenizer.ind2lab) == 31 and asr.tokenizer.lab2ind[" "] == 30  # the reference's own label order
    assert isinstance(asr.mods.encoder["log_softmax"], NativeLogSoftmax)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    logp = asr.encode_batch(wav, lens).cpu()
    ref = torch.from_numpy(exp["logp"])
    assert float((logp - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))
    words, pred = asr.transcribe_batch(wav, lens)
    assert words == [str(w) for w in exp[f"{key}_words"]]
    if key == "greedy":
        assert isinstance(asr.decoding_function, functools.partial)
        assert pred == [[int(t) for t in row if t >= 0] for row in exp["greedy_tokens"]]
    else:
        assert isinstance(asr.decoding_function, CTCBeamSearcher) and asr.decoding_function.beam_size == 100
        assert asr.decoding_function.space_index == 30
        for h, s in zip(pred, exp["beam_scores"]):
            assert abs(float(h[0].score) - float(s)) <= 1e-4 * max(1.0, abs(float(s)))
    for name, w in zip(exp["file_names"], exp[f"{key}_file_words"]):
        assert asr.transcribe_file(os.path.join(GOLD, str(name))) == str(w)


def test_encoder_asr_precision_scopes_only_the_transformer(backend):
    """run_opts precision applies to the Transformer encoder only, as in EncoderDecoderASR.encode_batch: the front-end,
    the CNN and the CTC head run fp32 (the precision each child saw is recorded by a forward hook)."""
    from speechbrain_amd.inference.ASR import EncoderASR

    native, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_ctc_tiny_expected.npz"))
    seen = {}
    for prec in ("fp32", "bf16"):
        asr = EncoderASR.from_hparams(source=CTC_DIR, run_opts={"device": str(dev), "precision": prec})
        for name, child in asr.mods.encoder.items():
            child.register_forward_hook(lambda m, i, o, name=name, prec=prec: seen.__setitem__((prec, name), native.precision()))
        out = asr.encode_batch(torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])).cpu()
        assert torch.isfinite(out).all()
        if prec == "bf16":
            ref = torch.from_numpy(exp["logp"])  # (bf16 operands in the Transformer's large contractions only)
            assert float((out - ref).abs().max()) <= 0.05 * float(ref.abs().max())
    names = ["compute_features", "normalize", "CNN", "transformer_encoder", "ctc_lin", "log_softmax"]
    assert all(seen[("fp32", n)] == "fp32" for n in names), seen
    assert [seen[("bf16", n)] for n in names] == ["fp32", "fp32", "fp32", "bf16", "fp32", "fp32"], seen


def test_ctc_shim_paths_resolve():
    import subprocess
    import sys

    code = ("import speechbrain_amd.compat as c; c.install(); "
            "from speechbrain.inference.ASR import EncoderASR; from speechbrain.decoders.ctc import CTCBeamSearcher; "
            "from speechbrain.decoders import ctc_greedy_decode; from speechbrain.dataio.encoder import CTCTextEncoder; "
            "import speechbrain_amd as s; assert EncoderASR.__module__.startswith('speechbrain_amd.'); print('ok')")
    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
