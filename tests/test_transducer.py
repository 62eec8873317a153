"""Transducer greedy decoding (csrc/transducer.hip, speechbrain_amd/decoders/transducer.py) against fixtures the reference
wrote (tools/make_transducer_golden.py), on the CPU emulator and on the MI355X (the `backend` fixture), plus the host
restatement (tests/transducer_host_ref.py) pinned to the same fixtures, the LSTM module, and the refusals."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import transducer_host_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "transducer_decode.npz")
MIN_GAP = 1e-3  # token identity is demanded of decisions the reference made by more than this (fp32 noise is ~1e-6)
ACTS = {"gelu": torch.nn.GELU, "leaky_relu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}


def _golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def _case(z, i):
    p = f"c{i}."
    return {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


def _searcher(cfg, sd, dev, beam_size=1, **kw):
    """The reference's module wiring of the fixture (tools/make_transducer_golden.py build()), from this package."""
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import LSTM
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint

    if cfg["emb"] is None:
        emb = Embedding(num_embeddings=cfg["V"], consider_as_one_hot=True, blank_id=0)
    else:
        emb = Embedding(num_embeddings=cfg["V"], embedding_dim=cfg["emb"])
    dec = LSTM(input_shape=[None, None, emb.embedding_dim], hidden_size=cfg["H"], num_layers=cfg["L"])
    proj = Linear(input_size=cfg["H"], n_neurons=cfg["J"], bias=cfg["proj_bias"])
    lin = Linear(input_size=cfg["J"], n_neurons=cfg["V"], bias=cfg["cls_bias"])
    for prefix, m in (("emb", emb), ("dec", dec), ("proj_dec", proj), ("transducer_lin", lin)):
        m.load_state_dict({k[len(prefix) + 1:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(prefix + ".")})
        m.to(dev)
    tjoint = Transducer_joint(joint="sum", nonlinearity=ACTS[cfg["act"]])
    return TransducerBeamSearcher(decode_network_lst=[emb, dec, proj], tjoint=tjoint, classifier_network=[lin], blank_id=0,
                                  beam_size=beam_size, nbest=1, **kw)


def _close(got, ref, rtol=1e-5, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(1.0, float(np.abs(ref).max()) if ref.size else 1.0)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= rtol * scale, (what, err, scale)


def _run(s, case, sd, dev, frame_block=0):
    """-> tokens, per-utterance scores (from the kernel), (out_pn, h, c), exp-mean score"""
    from speechbrain_amd import native

    cfg = case["cfg"]
    tn = torch.from_numpy(sd["tn"]).to(dev)
    hidden = None
    if cfg["hidden"]:
        hidden = tuple(torch.from_numpy(sd[k]).clone().to(dev) for k in ("out_pn0", "h0", "c0"))  # (updated in place)
        hidden = (hidden[0], (hidden[1], hidden[2]))
    hyps, mean, n1, n2, (out_pn, (h, c)) = s.transducer_greedy_decode(tn, hidden_state=hidden, return_hidden=True,
                                                                      max_symbols_per_step=cfg["S"], frame_block=frame_block)
    assert n1 is None and n2 is None
    # per-utterance scores through the binding (the searcher returns their exp().mean(), as the reference does)
    B, T, J = tn.shape
    L, H = cfg["L"], cfg["H"]
    st = [torch.empty(B, J, device=dev), torch.empty(L, B, H, device=dev), torch.empty(L, B, H, device=dev)]
    start = hidden is None
    if not start:
        st = [hidden_t.clone() for hidden_t in (torch.from_numpy(sd["out_pn0"]).reshape(B, J), torch.from_numpy(sd["h0"]),
                                                 torch.from_numpy(sd["c0"]))]
        st = [t.to(dev).contiguous() for t in st]
    _, _, score = native.transducer_greedy(s._prepare(tn.device), tn, st[0], st[1], st[2], 0, cfg["S"], start_from_blank=start,
                                           act=s.tjoint.act_code, frame_block=frame_block)
    return hyps, score.cpu().numpy(), (out_pn.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()), float(mean)


def test_fixture_margins_make_token_identity_fair():
    z, meta = _golden()
    for i, case in enumerate(meta):
        assert min(case["min_gap"]) >= MIN_GAP, case["name"]
        assert float(_case(z, i)["gaps"].min()) >= MIN_GAP
    names = {c["name"] for c in meta}
    assert {"only_blank", "capped_s5", "capped_s2", "hidden_given", "streaming", "padded_b3", "odd_sizes"} <= names
    # the capped cases emit max_symbols_per_step + 1 tokens at every frame
    for case in meta:
        if case["name"].startswith("capped"):
            cfg = case["cfg"]
            assert all(len(t) == cfg["T"] * (cfg["S"] + 1) for t in case["tokens"])


def test_transducer_greedy_kernel_matches_reference(backend):
    native, dev = backend
    z, meta = _golden()
    for i, case in enumerate(meta):
        if case["cfg"]["chunks"]:
            continue
        sd = _case(z, i)
        s = _searcher(case["cfg"], sd, dev)
        hyps, score, (out_pn, h, c), mean = _run(s, case, sd, dev)
        assert hyps == case["tokens"], case["name"]
        _close(score, sd["score"], what=(case["name"], "score"))
        _close(mean, case["mean_exp_score"], what=(case["name"], "mean"))
        _close(out_pn, sd["out_pn"], what=(case["name"], "out_pn"))
        _close(h, sd["h"], what=(case["name"], "h"))
        _close(c, sd["c"], what=(case["name"], "c"))


def test_transducer_frame_block_is_bit_invariant(backend):
    native, dev = backend
    z, meta = _golden()
    for i, case in enumerate(meta):
        if case["name"] not in ("onehot_l1_gelu", "capped_s2", "hidden_given", "wide_v", "dense_l1_relu_nobias"):
            continue
        sd = _case(z, i)
        s = _searcher(case["cfg"], sd, dev)
        a = _run(s, case, sd, dev, frame_block=0)
        b = _run(s, case, sd, dev, frame_block=1)
        c3 = _run(s, case, sd, dev, frame_block=3)
        for other in (b, c3):
            assert other[0] == a[0], case["name"]
            assert np.array_equal(other[1], a[1]), case["name"]
            for x, y in zip(other[2], a[2]):
                assert np.array_equal(x, y), case["name"]


def test_transducer_streaming_matches_reference(backend):
    from speechbrain_amd.decoders.transducer import TransducerGreedySearcherStreamingContext

    native, dev = backend
    z, meta = _golden()
    (i, case), = [(i, c) for i, c in enumerate(meta) if c["cfg"]["chunks"]]
    sd = _case(z, i)
    s = _searcher(case["cfg"], sd, dev)
    tn = torch.from_numpy(sd["tn"]).to(dev)
    ctx = TransducerGreedySearcherStreamingContext()
    got, t0 = [], 0
    for n in case["cfg"]["chunks"]:
        got.append(s.transducer_greedy_decode_streaming(tn[:, t0:t0 + n], ctx))
        t0 += n
    assert got == case["chunk_tokens"]
    out_pn, (h, c) = ctx.hidden
    assert tuple(out_pn.shape) == (tn.shape[0], 1, tn.shape[2])
    _close(out_pn.cpu().numpy(), sd["out_pn"], what="out_pn")
    _close(h.cpu().numpy(), sd["h"], what="h")
    _close(c.cpu().numpy(), sd["c"], what="c")
    one_shot, _, _, _ = s(tn)
    assert one_shot == case["tokens"]
    assert [sum((chunk[b] for chunk in got), []) for b in range(tn.shape[0])] == one_shot


def test_host_restatement_matches_reference():
    """tests/transducer_host_ref.py (no reference code) against the reference's own outputs: the full-size GPU test uses it
    as its yardstick."""
    z, meta = _golden()
    for i, case in enumerate(meta):
        cfg, sd = case["cfg"], _case(z, i)
        net = transducer_host_ref.Network(sd, cfg["act"])
        st = (sd["out_pn0"][:, 0], sd["h0"], sd["c0"]) if cfg["hidden"] else None
        toks, score, out, h, c, _ = transducer_host_ref.greedy(net, sd["tn"], 0, cfg["S"], st)
        assert toks == case["tokens"], case["name"]
        _close(score, sd["score"], what=(case["name"], "score"))
        _close(out, sd["out_pn"][:, 0], what=(case["name"], "out_pn"))
        _close(h, sd["h"], what=(case["name"], "h"))
        _close(c, sd["c"], what=(case["name"], "c"))


def test_one_hot_embedding_matches_reference_table():
    from speechbrain_amd.nnet.embedding import Embedding

    z, meta = _golden()
    (i, case), = [(i, c) for i, c in enumerate(meta) if c["name"] == "onehot_l1_gelu"]
    ref = _case(z, i)["emb.Embedding.weight"]
    emb = Embedding(num_embeddings=case["cfg"]["V"], consider_as_one_hot=True, blank_id=0)
    assert emb.embedding_dim == case["cfg"]["V"] - 1
    assert np.array_equal(emb.state_dict()["Embedding.weight"].numpy(), ref)
    e3 = Embedding(num_embeddings=5, consider_as_one_hot=True, blank_id=2)  # blank in the middle: its row is zero
    w = e3.Embedding.weight.detach()
    assert torch.equal(w[2], torch.zeros(4)) and torch.equal(w[[0, 1, 3, 4]], torch.eye(4))


def test_lstm_module_matches_torch(backend):
    """LSTM.forward (sbk_gemm_nt_f32 for the input part, sbk_lstm_f32 for the recurrence) against torch.nn.LSTM on the
    host with the same parameters, with and without an initial state, 1 and 2 layers."""
    from speechbrain_amd.nnet.RNN import LSTM

    native, dev = backend
    g = torch.Generator().manual_seed(5)
    for layers, bias, hid, inp in ((1, True, 24, 10), (2, False, 24, 10), (2, True, 23, 9)):  # (23: the scalar path)
        m = LSTM(hidden_size=hid, input_shape=[None, None, inp], num_layers=layers, bias=bias)
        x = torch.randn(3, 7, inp, generator=g)
        hx = (torch.randn(layers, 3, hid, generator=g), torch.randn(layers, 3, hid, generator=g))
        for state in (None, hx):
            with torch.no_grad():
                ref, (rh, rc) = m.rnn(x, state)
            m.to(dev)
            got, (gh, gc) = m(x.to(dev), None if state is None else tuple(t.to(dev) for t in state))
            m.cpu()
            for a, b in ((got, ref), (gh, rh), (gc, rc)):
                assert a.shape == b.shape
                assert float((a.cpu() - b).abs().max()) <= 1e-5
    with pytest.raises(NotImplementedError, match="lengths"):
        m(x, lengths=torch.ones(3))
    with pytest.raises(NotImplementedError, match="bidirectional"):
        LSTM(hidden_size=4, input_size=3, bidirectional=True)(torch.zeros(1, 2, 3))


def test_transducer_bad_arguments_are_reported(backend):
    native, dev = backend
    lib = native.load()
    z, meta = _golden()
    case, sd = meta[0], _case(z, 0)
    s = _searcher(case["cfg"], sd, dev)
    prep = s._prepare(dev)
    B, T, J, H, V = 2, 5, case["cfg"]["J"], case["cfg"]["H"], case["cfg"]["V"]
    tn = torch.zeros(B, T, J, device=dev)
    out_pn, h, c = torch.zeros(B, J, device=dev), torch.zeros(1, B, H, device=dev), torch.zeros(1, B, H, device=dev)
    tok = torch.zeros(B, T * 6, dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    sc = torch.zeros(B, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(cfg, W=prep.W, tn_p=p(tn), B=B):
        return lib.sbk_transducer_greedy_f32(ctypes.byref(W), ctypes.byref(cfg), tn_p, p(out_pn), p(h), p(c), p(tok), p(cnt),
                                             p(sc), B, T, None)

    good = dict(blank=0, max_symbols_per_step=5, start_from_blank=1, frame_block=0, act=native.ACT_GELU)
    assert call(native.TransducerConfig(**good)) == 0
    assert call(native.TransducerConfig(**dict(good, blank=V))) == -22 and b"blank" in lib.sbk_last_error()
    assert call(native.TransducerConfig(**dict(good, act=1))) == -22 and b"activation" in lib.sbk_last_error()
    assert call(native.TransducerConfig(**dict(good, frame_block=9))) == -22 and b"frame_block" in lib.sbk_last_error()
    assert call(native.TransducerConfig(**dict(good, max_symbols_per_step=-1))) == -22
    assert call(native.TransducerConfig(**good), tn_p=None) == -22
    assert call(native.TransducerConfig(**good), tn_p=None, B=0) == 0  # empty batch
    bad = native.TransducerWeights.from_buffer_copy(prep.W)
    bad.n_layers = 5
    assert call(native.TransducerConfig(**good), W=bad) == -22 and b"layers" in lib.sbk_last_error()
    bad = native.TransducerWeights.from_buffer_copy(prep.W)
    bad.n_emb = V - 1
    assert call(native.TransducerConfig(**good), W=bad) == -22
    assert lib.sbk_transducer_greedy_f32(None, None, None, None, None, None, None, None, None, 1, 1, None) == -22
    assert lib.sbk_lstm_f32(None, None, None, None, None, None, None, 1, 1, 1, None) == -22


def test_transducer_nan_input_terminates(backend):
    """NaN transcription-network frames neither fault nor hang the search (every frame is bounded by
    max_symbols_per_step + 1 emissions); the tokens themselves are unspecified."""
    native, dev = backend
    z, meta = _golden()
    case, sd = meta[0], _case(z, 0)
    s = _searcher(case["cfg"], sd, dev)
    tn = torch.from_numpy(sd["tn"]).clone()
    tn[0, 3:9] = float("nan")
    tn[1, :, 2] = float("nan")
    hyps, _, _, _ = s.transducer_greedy_decode(tn.to(dev), max_symbols_per_step=3)
    assert len(hyps) == tn.shape[0] and all(len(h) <= tn.shape[1] * 4 for h in hyps)


def test_unsupported_variants_raise_by_name(backend):
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import GRU, RNN, LiGRU
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher

    native, dev = backend
    z, meta = _golden()
    case, sd = meta[0], _case(z, 0)
    tn = torch.from_numpy(sd["tn"]).to(dev)
    # the recipe's beam searcher (beam 10, an LM) constructs; only the call raises
    lm = torch.nn.Linear(2, 2)
    beam = _searcher(case["cfg"], sd, dev, beam_size=10, lm_module=lm, lm_weight=0.5, state_beam=2.3, expand_beam=2.3)
    with pytest.raises(NotImplementedError, match="transducer beam search"):
        beam(tn)
    greedy_lm = _searcher(case["cfg"], sd, dev, lm_module=lm, lm_weight=0.5)
    with pytest.raises(NotImplementedError, match="LM fusion"):
        greedy_lm(tn)
    with pytest.raises(NotImplementedError, match="concat"):
        Transducer_joint(joint="concat")
    with pytest.raises(NotImplementedError, match="joint_network"):
        Transducer_joint(joint_network=torch.nn.Linear(2, 2), joint="sum")
    j = Transducer_joint(nonlinearity=torch.nn.Sigmoid)
    with pytest.raises(NotImplementedError, match="Sigmoid"):
        j.act_code
    emb = Embedding(num_embeddings=10, consider_as_one_hot=True)
    lin = Linear(input_size=12, n_neurons=10)
    for cls in (GRU, RNN, LiGRU):
        s = TransducerBeamSearcher([emb, cls(hidden_size=8, input_size=9), lin], Transducer_joint(), [lin], 0, beam_size=1)
        with pytest.raises(NotImplementedError, match=cls.__name__):
            s(tn)


def test_transducer_shim_paths_resolve():
    import subprocess
    import sys

    code = ("import speechbrain_amd.compat as c; c.install(); "
            "from speechbrain.decoders.transducer import TransducerBeamSearcher, TransducerGreedySearcherStreamingContext; "
            "from speechbrain.nnet.RNN import LSTM, GRU; from speechbrain.nnet.transducer.transducer_joint import Transducer_joint; "
            "from speechbrain.tokenizers.SentencePiece import SentencePieceDecoderStreamingContext, "
            "spm_decode_preserve_leading_space; import speechbrain.nnet.transducer; "
            "assert TransducerBeamSearcher.__module__.startswith('speechbrain_amd.'); print('ok')")
    root = os.path.dirname(HERE)
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_yaml_binds_the_streaming_decoder_as_a_partial():
    """A reference streaming YAML binds the searcher as ``self`` of transducer_greedy_decode_streaming through
    ``!name:`` with a positional argument; the loader resolves it to a partial over the class attribute."""
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher, TransducerGreedySearcherStreamingContext
    from speechbrain_amd.utils.hpyaml import load_hyperpyyaml

    text = """
ctx: !name:speechbrain.decoders.transducer.TransducerGreedySearcherStreamingContext
fn: !name:speechbrain.decoders.transducer.TransducerBeamSearcher.transducer_greedy_decode_streaming
    - 7
"""
    hp = load_hyperpyyaml(text)
    assert hp["fn"].func is TransducerBeamSearcher.transducer_greedy_decode_streaming and hp["fn"].args == (7,)
    assert isinstance(hp["ctx"](), TransducerGreedySearcherStreamingContext)


def test_spm_streaming_decode_preserves_leading_space():
    import sentencepiece as spm

    from speechbrain_amd.tokenizers.SentencePiece import (SentencePieceDecoderStreamingContext,
                                                           spm_decode_preserve_leading_space)

    path = os.path.join(HERE, "golden", "pretrained_tiny", "tokenizer.ckpt")
    tok = spm.SentencePieceProcessor()
    tok.load(path)
    ids = tok.encode("the cat sat on the mat")
    ctx = SentencePieceDecoderStreamingContext()
    cut = max(1, len(ids) // 2)
    parts = [spm_decode_preserve_leading_space(tok, ids[:cut], ctx), spm_decode_preserve_leading_space(tok, [], ctx),
             spm_decode_preserve_leading_space(tok, ids[cut:], ctx)]
    assert "".join(parts) == tok.decode(ids)
    assert ctx.emitted_symbol_count == len(ids)
