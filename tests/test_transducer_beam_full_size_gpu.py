"""Transducer beam search at the LibriSpeech transducer recipe's decode shape (joint 640, LSTM 512, 1 000 tokens, one-hot
embedding, GELU joint, beam_size 10, nbest 5), B = 2 x T' = 40, on the MI355X against the host restatement
(tests/transducer_beam_host_ref.py, pinned to the reference's fixture by the CPU suite).  Random weights, the classifier
sharpened and the blank row shifted as the fixture's are; seeds are drawn (at most 20) until the restatement's search stays
under the cap with every decision made by MIN_MARGIN."""
import numpy as np
import pytest
import torch

import transducer_beam_host_ref as host_ref

MIN_MARGIN = 1e-3


def _case(seed, V=1000, J=640, H=512, B=2, T=40):
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape, k=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * k).numpy()  # noqa: E731
    k = 2.0 / np.sqrt(H)
    sd = {"emb.Embedding.weight": torch.cat([torch.zeros(1, V - 1), torch.eye(V - 1)]).numpy(),
          "dec.rnn.weight_ih_l0": u(4 * H, V - 1, k=k), "dec.rnn.weight_hh_l0": u(4 * H, H, k=k),
          "dec.rnn.bias_ih_l0": u(4 * H, k=k / 2), "dec.rnn.bias_hh_l0": u(4 * H, k=k / 2),
          "proj_dec.w.weight": u(J, H, k=k / 2), "transducer_lin.w.weight": u(V, J, k=8.0 / np.sqrt(J))}
    bias = u(V, k=1.0 / np.sqrt(J))
    bias[0] += 20.0
    sd["transducer_lin.w.bias"] = bias
    sd["tn"] = torch.randn(B, T, J, generator=g).numpy()
    return sd


@pytest.mark.gpu
def test_transducer_beam_recipe_shape_matches_host_restatement():
    from test_transducer import _close, _searcher

    from speechbrain_amd import native

    cfg = dict(V=1000, emb=None, H=512, L=1, J=640, proj_bias=False, cls_bias=True, act="gelu")
    for seed in range(20):
        sd = _case(500 + seed)
        try:
            ref = host_ref.beam_search(host_ref.Network(sd, "gelu"), sd["tn"], 0, 10, 5)
        except host_ref.ExpansionCap:
            continue
        if ref["margin"] >= MIN_MARGIN and int(ref["expansions"].max()) < 40:
            break
    else:
        pytest.fail(f"none of 20 seeds stays under the cap with margins above {MIN_MARGIN}")
    dev = torch.device("cuda:0")
    s = _searcher(cfg, sd, dev, beam_size=10)
    s.nbest = 5
    tn = torch.from_numpy(sd["tn"]).to(dev)
    best, mean, nbest, scores = s(tn)
    _, _, _, _, status, expansions = native.transducer_beam_search(s._prepare(dev), tn, 0, 10, 5, act=s.tjoint.act_code)
    assert status.cpu().tolist() == [0, 0]
    assert nbest == ref["nbest"] and best == [n[0] for n in ref["nbest"]]
    assert expansions.cpu().tolist() == ref["expansions"].sum(axis=1).tolist()
    assert any(len(h) > 0 for n in nbest for h in n)
    for x, y in zip(scores, ref["scores"]):
        _close(x, y, what="scores")
    _close(float(mean), ref["mean"], what="mean")
