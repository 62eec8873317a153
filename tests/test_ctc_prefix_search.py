"""CTC prefix beam search (csrc/ctc_prefix_search.hip, decoders/ctc.py CTCPrefixBeamSearcher) on the CPU emulator and on
the MI355X (the `backend` fixture): against the float64 host restatement (tests/ctc_prefix_host_ref.py) at the shapes where
the kernel changes path, against the reference's records (tools/make_ctc_prefix_golden.py), bit for bit against itself,
and through EncoderASR.

Scores: the kernel is fp32 where the reference adds Python floats.  Its bound is max(4 * d, 1e-5) with d the distance of
the fp32 run of the restatement from the float64 one on the same input (the rule of DESIGN.md's error sections); texts and
text_frames are exact.  Measured on the MI355X and on the emulator: DESIGN.md section 5, "CTC prefix beam search"."""
import json
import os

import numpy as np
import pytest
import torch

import ctc_prefix_host_ref as H

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CHARS = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "-", "."]
WIDE = CHARS + [chr(0x100 + i) for i in range(99)]  # 130 one-character tokens
SPM = ["<blank>", "▁a", "▁ab", "b", "a", "▁", "c", "bc", "▁c", "ab", "▁b", "ca", "▁abc", "d"]


def _x(seed, B, T, V, scale):
    z = torch.randn(B, T, V, generator=torch.Generator().manual_seed(seed)) * scale
    z[:, :, 0] += scale
    return torch.log_softmax(z, dim=-1)


def _case(name):
    """(vocab, x [B,T,V], frame counts, searcher kwargs)"""
    three = lambda T: [1, T - 1, T]  # noqa: E731
    if name == "t1_v3_b1":
        return CHARS[:3], _x(1, 3, 1, 3, 2.0), three(1), dict(beam_size=1)
    if name == "t2_v31_b4":
        return CHARS, _x(2, 3, 2, 31, 2.0), three(2), dict(beam_size=4, topk=3)
    if name == "t65_v31_b64":
        return CHARS, _x(3, 3, 65, 31, 2.0), three(65), dict(beam_size=64, topk=3, token_prune_min_logp=-3.0)
    if name == "t65_v130_b256":
        return WIDE, _x(4, 3, 65, 130, 5.0), three(65), dict(beam_size=256, topk=3, prune_history=False)
    if name == "all_tokens_v130_b256":  # from the second frame on the working set (130 * 131 items, then 256 * 131) lives in the workspace
        return WIDE, _x(5, 3, 3, 130, 1.0), [1, 2, 3], dict(beam_size=256, topk=3, token_prune_min_logp=-1e30,
                                                             beam_prune_logp=-30.0, prune_history=False)
    if name == "all_skipped":
        return CHARS, _x(6, 3, 2, 31, 2.0), three(2), dict(beam_size=4, blank_skip_threshold=1e-30)
    if name == "spm_merge":  # "a" + "▁b" while " a b" is in the list: the reference starts a second beam of that text
        return ["<blank>", "a", "▁b", "▁a"], _x(7, 3, 6, 4, 1.0), [6, 5, 3], dict(beam_size=64, topk=3,
                                                                                  token_prune_min_logp=-1e30)
    if name == "spm_pieces":
        return SPM, _x(8, 3, 65, 14, 2.0), three(65), dict(beam_size=64, topk=3, prune_history=False)
    assert name == "repeat_pb_inf"  # the blank is pruned in frame 0, so "a" meets its repeat with p_b = -inf
    x = torch.tensor([[0.001, 0.9, 0.099], [0.001, 0.9, 0.099], [0.3, 0.3, 0.4]]).log().repeat(3, 1, 1)
    return ["<blank>", "a", "b"], x, [3, 2, 1], dict(beam_size=4, topk=3, token_prune_min_logp=float(np.log(0.01)))


def _searcher(vocab, kw):
    from speechbrain_amd.decoders.ctc import CTCPrefixBeamSearcher

    return CTCPrefixBeamSearcher(blank_index=0, vocab_list=vocab, space_token=" ", **kw)


def _host(s, x, frames, dtype):
    return [H.prefix_search(x[b].numpy(), int(frames[b]), s.vocab_list, 0, beam_size=s.beam_size,
                            beam_prune_logp=s.beam_prune_logp, token_prune_min_logp=s.token_prune_min_logp,
                            prune_history=s.prune_history, log_blank_skip_threshold=s.blank_skip_threshold, topk=s.topk,
                            dtype=dtype) for b in range(x.shape[0])]


def _check(label, hyps, want, want32):
    """texts and frames equal to `want`; scores within max(4 * |fp32 restatement - float64 restatement|, 1e-5)"""
    dist = max([abs(a[1] - b[1]) for ha, hb in zip(want, want32) for a, b in zip(ha, hb)] + [0.0])
    bound = max(4 * dist, 1e-5)
    err = 0.0
    for b, (got, ref) in enumerate(zip(hyps, want)):
        assert [h.text for h in got] == [r[0] for r in ref], (label, b)
        assert [list(h.text_frames) for h in got] == [r[2] for r in ref], (label, b)
        assert all(h.lm_score == h.score and h.last_lm_state is None for h in got)
        err = max([err] + [abs(float(h.score) - r[1]) for h, r in zip(got, ref)])
    print(f"{label}: fp32 restatement {dist:.3g}, bound {bound:.3g}, kernel {err:.3g}")
    assert err <= bound, (label, err, bound)


@pytest.mark.parametrize("name", ["t1_v3_b1", "t2_v31_b4", "t65_v31_b64", "t65_v130_b256", "all_tokens_v130_b256",
                                  "all_skipped", "spm_merge", "spm_pieces", "repeat_pb_inf"])
def test_kernel_matches_host_restatement(backend, name):
    native, dev = backend
    vocab, x, frames, kw = _case(name)
    s = _searcher(vocab, kw)
    want, want32 = _host(s, x, frames, np.float64), _host(s, x, frames, np.float32)
    assert [[h[0] for h in hl] for hl in want] == [[h[0] for h in hl] for hl in want32], "the input hangs on a rounding"
    lens = torch.tensor([(n + 0.5) / x.shape[1] for n in frames])
    _check(name, s(x.to(dev), lens.to(dev)), want, want32)
    if name == "all_skipped":
        assert [[(h.text, float(h.score)) for h in hl] for hl in s(x.to(dev), lens.to(dev))] == [[("", 0.0)]] * 3
    if name == "all_tokens_v130_b256":
        stats = native.ctc_prefix_beam_search(x.to(dev), lens.to(dev), s.prefix_table(), len(vocab), s.config(),
                                              with_stats=True)[3].cpu()
        assert stats[:, 0].tolist() == [1, 2, 3] and stats[:, 3].tolist() == [0, 1, 2], stats  # frames expanded / in workspace
    if name == "spm_merge":
        assert any(len({h[0] for h in hl}) < len(hl) for hl in want), "no hypothesis text occurs twice"


def test_kernel_matches_reference_records(backend):
    native, dev = backend
    z = np.load(os.path.join(GOLD, "ctc_prefix_search.npz"))
    for i, case in enumerate(json.loads(str(z["meta"]))["cases"]):
        x, lens = torch.from_numpy(z[f"case{i}_x"]), torch.from_numpy(z[f"case{i}_lens"])
        s = _searcher(case["vocab"], case["kwargs"])
        frames = (x.shape[1] * lens).numpy().astype(int)
        want = [[(t, sc, [(w, tuple(f)) for w, f in fr]) for t, sc, fr in zip(r["text"], r["score"], r["text_frames"])]
                for r in case["result"]]
        _check(case["name"], _quiet(s, x.to(dev), lens.to(dev)), want, _host(s, x, frames, np.float32))


def _quiet(s, x, lens):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (the vocabulary-size warning of the wide case)
        return s(x, lens)


def test_same_bits_twice_and_on_two_streams(backend):
    native, dev = backend
    vocab, x, frames, kw = _case("spm_pieces")
    s = _searcher(vocab, kw)
    x = x.to(dev)

    def run():
        p, sc, n = native.ctc_prefix_beam_search(x, None, s.prefix_table(), len(vocab), s.config())
        return p.cpu(), sc.cpu(), n.cpu()

    first, runs = run(), [run()]
    if dev.type == "cuda":
        for _ in range(2):
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                runs.append(run())
            stream.synchronize()
    for r in runs:
        assert all(torch.equal(a, b) for a, b in zip(first, r))


def test_encoder_asr_prefix_yaml_and_refusals(backend):
    import subprocess
    import sys

    from speechbrain_amd.decoders.ctc import CTCPrefixBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderASR

    native, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_ctc_tiny_expected.npz"))
    meta = json.loads(str(np.load(os.path.join(GOLD, "ctc_prefix_search.npz"))["meta"]))
    asr = EncoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_ctc_tiny"), hparams_file="hyperparams_prefix.yaml",
                                  run_opts={"device": str(dev)})
    assert isinstance(asr.decoding_function, CTCPrefixBeamSearcher) and asr.decoding_function.beam_size == 40
    words, pred = asr.transcribe_batch(torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"]))
    assert words == meta["yaml_words"]
    for h, sc in zip(pred, meta["yaml_scores"]):
        assert abs(float(h[0].score) - sc) <= 1e-4 * max(1.0, abs(sc))  # (the encoder's own tolerance, as for the beam yaml)
    code = ("import speechbrain_amd.compat as c; c.install(); from speechbrain.decoders.ctc import CTCPrefixBeamSearcher as P; "
            "from speechbrain.decoders import CTCPrefixBeamSearcher as Q; assert P is Q and P.__module__ == "
            "'speechbrain_amd.decoders.ctc'; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
    with pytest.raises(NotImplementedError, match="kenlm_model_path"):
        CTCPrefixBeamSearcher(blank_index=0, vocab_list=CHARS, kenlm_model_path="lm.arpa")
    with pytest.raises(NotImplementedError, match="vocabulary entry 3"):  # white space inside a token's text
        _searcher(CHARS[:3] + ["a b"], {})
    s = _searcher(CHARS, {})
    with pytest.raises(NotImplementedError, match="partial_decode_beams"):
        s.partial_decode_beams(torch.zeros(1, 2, 31), [])
    with pytest.raises(NotImplementedError, match="lm_start_state"):
        s(torch.zeros(1, 2, 31, device=dev), None, lm_start_state=object())
