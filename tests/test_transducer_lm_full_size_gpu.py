"""Transducer beam search with RNNLM shallow fusion at the LibriSpeech transducer recipe's decode shape (joint 640, LSTM 512,
1 000 tokens, one-hot embedding, GELU joint; the LM: embedding 128, two LSTM layers of 2 048, one DNN block of 512, LeakyReLU;
beam_size 4), B = 2 x T' = 6, on the MI355X against the host restatement (tests/transducer_lm_host_ref.py, pinned to the
reference's fixture by the CPU suite).  Random weights, the classifier sharpened and the blank row shifted as the existing
full-size beam test does (less far, so that tokens are emitted within six frames); seeds are drawn (at most 20) until the
restatement's search stays under the cap with every decision made by MIN_MARGIN."""
import ctypes

import numpy as np
import pytest
import torch

import transducer_lm_host_ref as host_ref
from test_transducer_beam_full_size_gpu import _case

MIN_MARGIN = 1e-3
LM = dict(V=1000, E=128, H=2048, L=2, D=512)


def _lm_weights():
    """One LM for every seed (200 MB of it): torch's default-scale uniform weights, the output layer sharpened."""
    g = torch.Generator().manual_seed(77)
    u = lambda *shape, k=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * k).numpy()  # noqa: E731
    V, E, H, L, D = LM["V"], LM["E"], LM["H"], LM["L"], LM["D"]
    sd = {"lm.embedding.Embedding.weight": torch.randn(V, E, generator=g).numpy()}
    k = 1.0 / np.sqrt(H)
    for l in range(L):
        sd[f"lm.rnn.rnn.weight_ih_l{l}"] = u(4 * H, E if l == 0 else H, k=k)
        sd[f"lm.rnn.rnn.weight_hh_l{l}"] = u(4 * H, H, k=k)
        sd[f"lm.rnn.rnn.bias_ih_l{l}"], sd[f"lm.rnn.rnn.bias_hh_l{l}"] = u(4 * H, k=k), u(4 * H, k=k)
    sd["lm.dnn.linear.w.weight"], sd["lm.dnn.linear.w.bias"] = u(D, H, k=k), u(D, k=k)
    sd["lm.dnn.norm.norm.weight"], sd["lm.dnn.norm.norm.bias"] = 1.0 + u(D, k=0.2), u(D, k=0.2)
    sd["lm.out.w.weight"], sd["lm.out.w.bias"] = u(V, D, k=3.0 / np.sqrt(D)), u(V, k=0.5)
    return sd


@pytest.mark.gpu
def test_transducer_lm_recipe_shape_matches_host_restatement():
    from test_transducer import _close, _searcher

    from speechbrain_amd import native
    from speechbrain_amd.lobes.models.RNNLM import RNNLM

    cfg = dict(V=1000, emb=None, H=512, L=1, J=640, proj_bias=False, cls_bias=True, act="gelu")
    lsd = _lm_weights()
    hlm = host_ref.LM(lsd, "leaky_relu")
    for seed in range(20):
        sd = _case(700 + seed, B=2, T=6)
        sd["transducer_lin.w.bias"] = sd["transducer_lin.w.bias"].copy()
        sd["transducer_lin.w.bias"][0] -= 8.0  # (the blank's shift 20 -> 12: some tokens within six frames)
        try:
            ref = host_ref.beam_search(host_ref.Network(sd, "gelu"), hlm, 0.5, sd["tn"], 0, 4, 5)
        except host_ref.ExpansionCap:
            continue
        if ref["margin"] >= MIN_MARGIN and int(ref["expansions"].max()) < 16 and any(len(h) > 0 for n in ref["nbest"] for h in n):
            break
    else:
        pytest.fail(f"none of 20 seeds stays under the cap with margins above {MIN_MARGIN}")
    dev = torch.device("cuda:0")
    lm = RNNLM(output_neurons=LM["V"], embedding_dim=LM["E"], rnn_layers=LM["L"], rnn_neurons=LM["H"], dnn_blocks=1,
               dnn_neurons=LM["D"], dropout=0.0, return_hidden=True)
    lm.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in lsd.items()})
    s = _searcher(cfg, sd, dev, beam_size=4, lm_module=lm.to(dev), lm_weight=0.5)
    s.nbest = 5
    tn = torch.from_numpy(sd["tn"]).to(dev)
    # the size function accepts the recipe's shape at beam_size 4 with the default max_expansions
    prep, plm = s._prepare(dev, beam=True), s._prepare_lm(dev)
    bcfg = native.TransducerBeamConfig(blank=0, beam_size=4, nbest=5, state_beam=2.3, expand_beam=2.3, max_expansions=16,
                                       max_tokens=6 * 16, act=native.ACT_GELU)
    assert native.load().sbk_transducer_beam_lm_workspace_bytes(ctypes.byref(prep.W), ctypes.byref(plm.M), ctypes.byref(bcfg),
                                                                2, 6) > 0
    best, mean, nbest, scores = s(tn)
    _, _, _, _, status, expansions, steps = native.transducer_beam_search(prep, tn, 0, 4, 5, act=s.tjoint.act_code, lm=plm,
                                                                          lm_weight=0.5, return_lm_steps=True)
    assert status.cpu().tolist() == [0, 0]
    assert nbest == ref["nbest"] and best == [n[0] for n in ref["nbest"]]
    assert expansions.cpu().tolist() == ref["expansions"].sum(axis=1).tolist()
    assert steps.cpu().tolist() == ref["lm_steps"].tolist()
    assert any(len(h) > 0 for n in nbest for h in n)
    for x, y in zip(scores, ref["scores"]):
        _close(x, y, what="scores")
    _close(float(mean), ref["mean"], what="mean")
