"""nnet/RNN.py AttentionalRNNDecoder / GRUCell, nnet/attention.py and decoders/seq2seq.py S2SRNNGreedySearcher against the reference's
own (tests/golden/model_s2srnn.npz and the model directory tests/golden/pretrained_crdnn_s2s_tiny, both written by
tools/make_s2srnn_golden.py), on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bounds (the project's): recorded dec_out, attention, logits and scores 5e-5; ids, lengths and text exact.  The generator checked that
the reference's own fp32-vs-fp64 distance is under a quarter of the bound, that its fp64 run decodes the same ids and that the best
two logits of every step are 2e-3 apart in it."""
import functools
import os

import numpy as np
import pytest
import torch

from speechbrain_amd.decoders import S2SRNNBeamSearcher, S2SRNNGreedySearcher
from speechbrain_amd.nnet.attention import ContentBasedAttention, KeyValueAttention, LocationAwareAttention
from speechbrain_amd.nnet.embedding import Embedding
from speechbrain_amd.nnet.linear import Linear
from speechbrain_amd.nnet.RNN import AttentionalRNNDecoder, GRUCell

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
S2S_DIR = os.path.join(GOLD, "pretrained_crdnn_s2s_tiny")
BOUND = 5e-5
CONFIGS = ["location", "single", "never_eos", "min_ratio", "content", "two_layer"]


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(GOLD, "model_s2srnn.npz"))
    return {k: z[k] for k in z.files}


def _cfg(name):
    g = _golden()
    raw = dict(zip((str(k) for k in g[f"{name}/cfg_keys"]), (str(v) for v in g[f"{name}/cfg"])))
    return {k: v if k == "attn" else (float(v) if k in ("min_ratio", "max_ratio", "scaling") else int(v)) for k, v in raw.items()}


def _t(name, key):
    return torch.from_numpy(_golden()[f"{name}/{key}"])


def _state_dict(name):
    pre = f"{name}/sd/"
    return {k[len(pre):]: torch.from_numpy(v) for k, v in _golden().items() if k.startswith(pre)}


def _build(name, dev="cpu", **over):
    """Our embedding, decoder, output layer and searcher with the reference's weights, through strict load_state_dict."""
    c = _cfg(name)
    emb = Embedding(num_embeddings=c["V"], embedding_dim=c["emb"])
    dec = AttentionalRNNDecoder(rnn_type="gru", attn_type=c["attn"], hidden_size=c["H"], attn_dim=c["A"], num_layers=c["layers"],
                                enc_dim=c["E"], input_size=c["emb"], scaling=c["scaling"], channels=c["C"] or None,
                                kernel_size=c["k"] or None, re_init=True, dropout=0.15)
    lin = Linear(input_size=c["H"], n_neurons=c["V"])
    dec.load_state_dict(_state_dict(name), strict=True)
    emb.load_state_dict({"Embedding.weight": _t(name, "emb")}, strict=True)
    lin.load_state_dict({"w.weight": _t(name, "fc_w"), "w.bias": _t(name, "fc_b")}, strict=True)
    kw = dict(bos_index=c["bos"], eos_index=c["eos"], min_decode_ratio=c["min_ratio"], max_decode_ratio=c["max_ratio"])
    kw.update(over)
    searcher = S2SRNNGreedySearcher(embedding=emb, decoder=dec, linear=lin, **kw).to(dev).eval()
    return emb, dec, lin, searcher


def _ids(name):
    return [[int(t) for t in row if t >= 0] for row in _golden()[f"{name}/ids"]]


@pytest.mark.parametrize("name", CONFIGS)
def test_strict_load_and_reference_keys(name):
    """The key sets are the reference's: its state dict loads strictly and nothing of ours is left over."""
    c = _cfg(name)
    _, dec, _, _ = _build(name)
    sd = _state_dict(name)
    assert set(dec.state_dict().keys()) == set(sd.keys())
    for k, v in sd.items():
        assert dec.state_dict()[k].shape == v.shape, k
    want = {"proj.weight", "attn.mlp_enc.weight", "attn.mlp_dec.bias", "attn.mlp_attn.weight", "attn.mlp_out.weight",
            f"rnn.rnn_cells.{c['layers'] - 1}.weight_ih", "rnn.rnn_cells.0.bias_hh"}
    if c["attn"] == "location":
        want |= {"attn.conv_loc.weight", "attn.mlp_loc.weight", "attn.mlp_loc.bias"}
        assert tuple(sd["attn.conv_loc.weight"].shape) == (c["C"], 1, 2 * c["k"] + 1)
        assert isinstance(dec.attn, LocationAwareAttention)
    else:
        assert type(dec.attn) is ContentBasedAttention
    assert want <= set(sd.keys()) and isinstance(dec.rnn, GRUCell)
    with pytest.raises(RuntimeError):
        dec.load_state_dict({k: v for k, v in sd.items() if k != "proj.bias"}, strict=True)


@pytest.mark.parametrize("name", CONFIGS)
def test_forward_step_and_teacher_forced_forward(backend, name):
    """forward_step fed with the reference's greedy tokens, step by step (the attention module keeps enc_h, mask and prev_attn as
    the reference's does), and forward over the same embedded tokens in one call: dec_out, attention and logits of every step."""
    nat, dev = backend
    c = _cfg(name)
    emb, dec, lin, searcher = _build(name, dev)
    enc, wav_len, tokens_in = _t(name, "enc").to(dev), _t(name, "wav_len").to(dev), _t(name, "tokens_in").to(dev)
    ref = {k: _t(name, k) for k in ("dec_out", "attn", "logits")}
    emb_in = emb.Embedding.weight.detach()[tokens_in]
    enc_len = torch.round(enc.shape[1] * wav_len).long()
    dec.attn.reset()
    hs, ctx = None, torch.zeros(enc.shape[0], c["A"], device=dev)
    outs, attns = [], []
    for t in range(tokens_in.shape[1]):
        out, hs, ctx, w = dec.forward_step(emb_in[:, t], hs, ctx, enc, enc_len)
        outs.append(out), attns.append(w)
    assert dec.attn.precomputed_enc_h.shape == (enc.shape[0], enc.shape[1], c["A"]) and dec.attn.mask.shape == enc.shape[:2]
    assert (dec.attn.prev_attn is not None) == (c["attn"] == "location")
    assert tuple(hs.shape) == (c["layers"], enc.shape[0], c["H"])
    step_out, step_attn = torch.stack(outs, 1), torch.stack(attns, 1)
    outputs, attn = dec(emb_in, enc, wav_len)
    with nat.precision_scope("fp32"):
        logits = nat.gemm_nt(outputs.contiguous(), lin.w.weight, lin.w.bias)
    for what, got, want in (("forward_step dec_out", step_out, ref["dec_out"]), ("forward_step attn", step_attn, ref["attn"]),
                            ("forward dec_out", outputs, ref["dec_out"]), ("forward attn", attn, ref["attn"]),
                            ("logits", logits, ref["logits"])):
        err = float((got.cpu() - want).abs().max())
        print(f"s2srnn {name} {what}: max|d| {err:.3e}")
        assert got.shape == want.shape and err <= BOUND, what
    dec.attn.reset()
    assert dec.attn.precomputed_enc_h is None and dec.attn.mask is None and dec.attn.prev_attn is None


@pytest.mark.parametrize("name", CONFIGS)
def test_greedy_ids_lengths_and_scores(backend, name):
    """location: wav_len < 1 in the batch, every utterance ends before the last step; single: B = 1; never_eos: length 1.0, stops at
    max_decode_ratio; min_ratio: min_decode_ratio 0.3; content: the reference doctest's configuration; two_layer."""
    nat, dev = backend
    c = _cfg(name)
    _, _, _, searcher = _build(name, dev)
    enc, wav_len = _t(name, "enc").to(dev), _t(name, "wav_len").to(dev)
    hyps, lengths, scores, log_probs = searcher(enc, wav_len)
    ref_len, ref_sc = _t(name, "lengths"), _t(name, "scores")
    print(f"s2srnn {name} greedy: lengths {[len(h) for h in hyps]} of {scores.shape[-1]} steps, "
          f"scores max|d| {float((scores - ref_sc).abs().max()) if scores.shape == ref_sc.shape else float('nan'):.3e}")
    assert hyps == _ids(name)
    assert log_probs is None
    assert lengths.shape == ref_len.shape and torch.equal(lengths, ref_len)
    assert scores.shape == ref_sc.shape and float((scores - ref_sc).abs().max()) <= BOUND
    steps = int(c["T"] * c["max_ratio"]) - int(c["T"] * c["min_ratio"])
    if name == "never_eos":
        assert scores.shape[-1] == steps and bool((lengths == 1.0).all()) and all(len(h) == steps for h in hyps)
    if name == "location":
        assert scores.shape[-1] < steps and float(wav_len.min()) < 1.0
    if name == "single":
        assert enc.shape[0] == 1
    if name == "min_ratio":
        assert scores.shape[-1] <= steps < c["T"]
    if name == "two_layer":
        assert c["layers"] == 2


def test_an_in_place_weight_update_is_seen(backend):
    """The searcher's weight table is derived through native.Derived: an output layer changed in place changes the result."""
    nat, dev = backend
    c = _cfg("location")
    _, _, lin, searcher = _build("location", dev)
    enc, wav_len = _t("location", "enc").to(dev), _t("location", "wav_len").to(dev)
    assert searcher(enc, wav_len)[0] == _ids("location")
    with torch.no_grad():
        lin.w.bias[c["eos"]] += 1e4  # eos wins the first step of every utterance
    assert searcher(enc, wav_len)[0] == [[] for _ in range(enc.shape[0])]


def test_encoder_decoder_asr_from_hparams_matches_reference(backend):
    """EncoderDecoderASR.from_hparams on a hyperparams directory in the seq2seq recipe's inference layout (CRDNN encoder, embedding,
    GRU attention decoder, output layer, `decoder: !new:speechbrain.decoders.S2SRNNGreedySearcher`) written by the reference: ids and
    text of the batch and of the wav fixtures exact, scores within bound."""
    from speechbrain_amd.inference.ASR import EncoderDecoderASR

    nat, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_crdnn_s2s_tiny_expected.npz"))
    asr = EncoderDecoderASR.from_hparams(source=S2S_DIR, run_opts={"device": str(dev)})
    assert isinstance(asr.mods.decoder, S2SRNNGreedySearcher) and isinstance(asr.mods.decoder.dec, AttentionalRNNDecoder)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    enc_out = asr.encode_batch(wav, lens)
    err = float((enc_out.cpu() - torch.from_numpy(exp["enc_out"])).abs().max())
    print(f"crdnn s2s encoder states: max|d| {err:.3e}")
    assert err <= BOUND
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == [[int(t) for t in row if t >= 0] for row in exp["tokens"]]
    assert words == [str(w) for w in exp["words"]]
    _, lengths, scores, _ = asr.mods.decoder(enc_out, lens.to(enc_out.device))
    assert torch.equal(lengths, torch.from_numpy(exp["lengths"]))
    assert float((scores - torch.from_numpy(exp["scores"])).abs().max()) <= BOUND
    for name, w in zip(exp["file_names"], exp["file_words"]):
        assert asr.transcribe_file(os.path.join(GOLD, str(name))) == str(w)


def test_s2srnn_shim_paths_resolve():
    import subprocess
    import sys

    code = ("import speechbrain_amd.compat as c; c.install(); "
            "from speechbrain.nnet.RNN import AttentionalRNNDecoder, GRUCell; "
            "from speechbrain.nnet.attention import ContentBasedAttention, LocationAwareAttention, KeyValueAttention; "
            "from speechbrain.decoders import S2SRNNGreedySearcher, S2SRNNBeamSearcher; "
            "from speechbrain.decoders.seq2seq import S2SRNNGreedySearcher as G; "
            "assert AttentionalRNNDecoder.__module__ == 'speechbrain_amd.nnet.RNN' and G is S2SRNNGreedySearcher "
            "and LocationAwareAttention.__module__ == 'speechbrain_amd.nnet.attention'; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_refusals_raise_by_name():
    kw = dict(attn_type="location", hidden_size=8, attn_dim=8, num_layers=1, enc_dim=8, input_size=4, channels=2, kernel_size=1)
    for rnn_type in ("lstm", "rnn"):
        with pytest.raises(NotImplementedError, match=rnn_type):
            AttentionalRNNDecoder(rnn_type=rnn_type, **kw)
    with pytest.raises(NotImplementedError, match="KeyValueAttention"):
        AttentionalRNNDecoder(rnn_type="gru", **dict(kw, attn_type="keyvalue"))
    with pytest.raises(NotImplementedError, match="KeyValueAttention"):
        KeyValueAttention(enc_dim=8, dec_dim=8, attn_dim=8, output_dim=8)
    with pytest.raises(ValueError, match="nowhere is not implemented"):
        AttentionalRNNDecoder(rnn_type="gru", **dict(kw, attn_type="nowhere"))
    with pytest.raises(ValueError, match="ligru not implemented"):
        AttentionalRNNDecoder(rnn_type="ligru", **kw)
    emb, dec, lin, _ = _build("location")
    search = dict(bos_index=0, eos_index=0, min_decode_ratio=0.0, max_decode_ratio=1.0)
    with pytest.raises(NotImplementedError, match="temperature"):
        S2SRNNGreedySearcher(embedding=emb, decoder=dec, linear=lin, temperature=0.7, **search)
    with pytest.raises(NotImplementedError, match="S2SRNNGreedySearcher"):
        S2SRNNBeamSearcher(embedding=emb, decoder=dec, linear=lin, beam_size=4, **search)


def test_zero_steps_raise_a_value_error(backend):
    """max_decode_ratio so small that range(int(T * min), int(T * max)) is empty: the reference fails on an empty torch.stack."""
    nat, dev = backend
    _, _, _, searcher = _build("location", dev, max_decode_ratio=0.01)
    with pytest.raises(ValueError, match="no decoding steps"):
        searcher(_t("location", "enc").to(dev), _t("location", "wav_len").to(dev))
