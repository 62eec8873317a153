"""Transducer greedy decoding at the LibriSpeech transducer recipe's shape (joint 640, LSTM 512, 1 000 tokens, one-hot
embedding, GELU joint), B = 32 x T' = 250, on the MI355X against the host restatement (tests/transducer_host_ref.py, pinned
to the reference's fixtures by the CPU suite).  The input mixes blank runs, frames with several emissions and frames that
hit the max_symbols_per_step cap."""
import numpy as np
import pytest
import torch

import transducer_host_ref

MIN_GAP = 1e-3


@pytest.mark.gpu
def test_transducer_greedy_recipe_shape_matches_host_restatement():
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import LSTM
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint

    V, J, H, B, T, S = 1000, 640, 512, 32, 250, 5
    torch.manual_seed(17)
    emb = Embedding(num_embeddings=V, consider_as_one_hot=True, blank_id=0)
    dec = LSTM(input_shape=[None, None, V - 1], hidden_size=H, num_layers=1)
    proj = Linear(input_size=H, n_neurons=J, bias=False)
    lin = Linear(input_size=J, n_neurons=V, bias=True)
    g = torch.Generator().manual_seed(18)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(2.0)
        lin.w.weight.mul_(8.0)
        lin.w.bias.zero_()
        lin.w.bias[0] = 14.0
    tn = torch.randn(B, T, J, generator=g)
    # frames that force one token whatever the PN says: capped at S + 1 emissions
    w = lin.w.weight.detach()
    for b in range(0, B, 3):
        for t in range(7, T, 41):
            k = 1 + (b * 7 + t) % (V - 1)
            tn[b, t] = 30.0 * w[k] / w[k].norm()
    tn[1::4, :, :] *= 0.25  # blank-heavy utterances
    dev = torch.device("cuda:0")
    for m in (emb, dec, proj, lin):
        m.to(dev)
    s = TransducerBeamSearcher([emb, dec, proj], Transducer_joint(nonlinearity=torch.nn.GELU), [lin], 0, beam_size=1)
    hyps, _, _, _, (out_pn, (h, c)) = s.transducer_greedy_decode(tn.to(dev), return_hidden=True, max_symbols_per_step=S)
    sd = {"emb.Embedding.weight": emb.Embedding.weight.cpu().numpy(), "proj_dec.w.weight": proj.w.weight.detach().cpu().numpy(),
          "transducer_lin.w.weight": lin.w.weight.detach().cpu().numpy(), "transducer_lin.w.bias": lin.w.bias.detach().cpu().numpy()}
    for k, v in dec.state_dict().items():
        sd[f"dec.{k}"] = v.cpu().numpy()
    net = transducer_host_ref.Network(sd, "gelu")
    toks, _, r_out, r_h, r_c, gaps = transducer_host_ref.greedy(net, tn.numpy(), 0, S)
    decided = [b for b in range(B) if min(gaps[b]) > MIN_GAP]
    assert len(decided) >= B // 2, len(decided)
    n_emit = [len(t) for t in toks]
    capped = sum(1 for b in range(0, B, 3) if n_emit[b] >= 6 * len(range(7, T, 41)))
    assert capped > 0 and min(n_emit) < T // 4 and max(n_emit) > T // 4, n_emit
    for b in decided:
        assert hyps[b] == toks[b], b
        for got, ref in ((out_pn[b, 0], r_out[b]), (h[:, b], r_h[:, b]), (c[:, b], r_c[:, b])):
            got = got.cpu().numpy()
            assert float(np.abs(got - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max())), b
