"""RNNLMScorer through the public interface, against what the reference wrote (tools/make_rnnlm_scorer_golden.py: its own
S2STransformerBeamSearcher with RNNLMScorer / CTCScorer, tests/golden/s2s_rnnlm.npz and the model directory
tests/golden/pretrained_rnnlm_tiny): the RNNLM step fused into the device search (csrc/search.hip on csrc/rnnlm_step.hip), the
scorer's own step protocol, and the directory through EncoderDecoderASR.from_hparams.  On the CPU emulator (not gpu) and on the
MI355X (-m gpu).  Ids and lengths exact; scores within max(4 x d, 1e-5), d the reference's fp32-to-fp64 distance in the fixture."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = ["beam4", "beam10", "beam4_ctc", "beam10_ctc"]


def _searcher(dev, name, **kw):
    """(fixture, modules, ScorerBuilder, S2STransformerBeamSearcher) of a fixture configuration on the directory's weights."""
    from speechbrain_amd.decoders import CTCScorer, RNNLMScorer, S2STransformerBeamSearcher, ScorerBuilder
    from speechbrain_amd.inference.ASR import EncoderDecoderASR

    g = np.load(os.path.join(GOLD, "s2s_rnnlm.npz"))
    m = EncoderDecoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_rnnlm_tiny"), run_opts={"device": str(dev)}).mods
    beam, ctc_w, lm_w, lm_t, temp = [float(v) for v in g[f"{name}/cfg"]]
    full, weights = [RNNLMScorer(language_model=m.lm_model, temperature=lm_t)], {"rnnlm": lm_w}
    if ctc_w > 0:
        full, weights = full + [CTCScorer(ctc_fc=m.ctc_lin, blank_index=0, eos_index=2)], dict(weights, ctc=ctc_w)
    sb = ScorerBuilder(full_scorers=full, weights=weights)
    opts = dict(dict(min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=int(beam), using_eos_threshold=False,
                     length_normalization=True, temperature=temp), **kw)
    return g, m, sb, S2STransformerBeamSearcher(modules=[m.transformer, m.seq_lin], bos_index=1, eos_index=2, scorer=sb, **opts)


@pytest.mark.parametrize("name", CONFIGS)
@pytest.mark.parametrize("graph_mode", [0, 2])
def test_fixture_configurations(backend, name, graph_mode):
    nat, dev = backend
    g, _, _, bs = _searcher(dev, name)
    bs.graph_mode, bs.overlap_ctc = graph_mode, 0 if graph_mode else bs.overlap_ctc  # (a helper stream turns the device counter off)
    hyps, lens, scores, _ = bs(torch.from_numpy(g["enc_out"]).to(dev), torch.from_numpy(g["lens"]).to(dev))
    err, bound = float((scores.cpu() - torch.from_numpy(g[f"{name}/scores"])).abs().max()), max(4.0 * float(g[f"{name}/d"]), 1e-5)
    print(f"{name} graph_mode {graph_mode}: score max|d| {err:.3e} (bound {bound:.1e})")
    assert hyps == [[int(t) for t in row if t >= 0] for row in g[f"{name}/ids"]]
    assert torch.equal(lens.cpu(), torch.from_numpy(g[f"{name}/lengths"]))
    assert err <= bound


@pytest.mark.parametrize("name", CONFIGS[1:3])
def test_step_protocol_gives_the_search_candidates(backend, name):
    """ScorerBuilder.score / permute_scorer_mem driven by hand for six steps around the decoder's own log-probabilities: the
    hypotheses it ends with are the top-k of the fused search limited to six steps."""
    nat, dev = backend
    g, m, sb, bs = _searcher(dev, name, return_topk=True, topk=4)
    enc, wl = torch.from_numpy(g["enc_out"]).to(dev), torch.from_numpy(g["lens"]).to(dev)
    B, T, _ = enc.shape
    bs.max_decode_ratio = 6.5 / T
    k_hyps, _, k_scores, _ = bs(enc, wl)
    beam, V, temp = bs.beam_size, 40, bs.temperature
    n, off = B * beam, (torch.arange(B) * beam).unsqueeze(1)
    enc_i, len_i = enc.repeat_interleave(beam, 0), torch.round(T * wl).int().repeat_interleave(beam, 0)
    handle = nat.DecoderHandle(m.transformer, m.seq_lin)
    memory = sb.reset_scorer_mem(enc, wl)
    prefix, seqs = torch.ones(n, 1, dtype=torch.long), torch.empty(n, 0, dtype=torch.long)
    seq = torch.full((n,), float("-inf"), dtype=torch.float64)
    seq[off.view(-1)] = 0.0
    done = [[] for _ in range(B)]
    for step in range(6):
        pred = nat.decoder_prefix(handle, prefix.int().to(dev), enc_i, len_i)[:, -1]
        lp = bs.attn_weight * nat.log_softmax(m.seq_lin(pred).contiguous(), temperature=temp)
        lp, new_mem = sb.score(prefix[:, -1].to(dev), memory, None, lp, beam)
        scores, cand = ((seq.unsqueeze(1) + lp.cpu().double()) / (step + 1)).view(B, -1).topk(beam, dim=-1)
        index, tok = (torch.div(cand, V, rounding_mode="floor") + off).view(-1), (cand % V).view(-1)
        prefix, seqs = torch.cat([prefix[index], tok.unsqueeze(1)], 1), torch.cat([seqs[index], tok.unsqueeze(1)], 1)
        ended = tok == 2 if step < 5 else torch.ones(n, dtype=torch.bool)  # (the last step ends what is alive)
        for i in torch.nonzero(ended).flatten().tolist():
            if len(done[i // beam]) < beam:
                done[i // beam].append((float(scores.view(-1)[i]), seqs[i].tolist()))
        seq = (scores.view(-1) * (step + 1)).masked_fill(tok == 2, float("-inf"))
        memory = sb.permute_scorer_mem(new_mem, index.to(dev), cand.to(dev))
    for b in range(B):
        for r, (score, ids) in enumerate(sorted(done[b], key=lambda h: -h[0])[:4]):
            assert k_hyps[b, r, :len(ids)].tolist() == ids and abs(float(k_scores[b, r]) - score) <= 1e-5, (b, r)


def test_model_directory(backend):
    """hyperparams.yaml with !new:speechbrain.decoders.scorer.RNNLMScorer and `lm` among the pretrainer's loadables, unchanged."""
    nat, dev = backend
    from speechbrain_amd.inference.ASR import EncoderDecoderASR

    g = np.load(os.path.join(GOLD, "s2s_rnnlm.npz"))
    asr = EncoderDecoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_rnnlm_tiny"), run_opts={"device": str(dev)})
    assert type(asr.mods.decoder.scorer.full_scorers["rnnlm"]).__module__ == "speechbrain_amd.decoders.scorer"
    words, tokens = asr.transcribe_batch(torch.from_numpy(g["wav"]), torch.from_numpy(g["lens"]))
    assert tokens == [[int(t) for t in row if t >= 0] for row in g[f"{str(g['directory'])}/ids"]]
    assert words == [str(w) for w in g["words"]]


def test_refusals_raise_by_name(backend):
    from speechbrain_amd.decoders import RNNLMScorer, ScorerBuilder, TransformerLMScorer
    from speechbrain_amd.lobes.models.RNNLM import RNNLM

    with pytest.raises(NotImplementedError, match="RNNLM scorer is not implemented for Linear"):
        RNNLMScorer(language_model=torch.nn.Linear(2, 2))
    with pytest.raises(NotImplementedError, match="3 DNN blocks"):
        RNNLMScorer(language_model=RNNLM(output_neurons=10, embedding_dim=4, rnn_neurons=8, dnn_blocks=3, dnn_neurons=8))
    lm = RNNLMScorer(language_model=RNNLM(output_neurons=10, embedding_dim=4, rnn_neurons=8, dnn_neurons=8))
    with pytest.raises(NotImplementedError, match="one LM scorer"):
        ScorerBuilder(full_scorers=[TransformerLMScorer.__new__(TransformerLMScorer), lm], weights={"transformerlm": 0.3, "rnnlm": 0.3})
