"""Model-level parity through the drop-in module surface (speechbrain_amd.*), against the REFERENCE's
outputs stored in tests/golden/model_*.npz.  Runs on the CPU emulator of the kernels (not gpu) and on
the MI355X (``-m gpu``).  Token ids must be bit-exact; floats within the stated fp32 tolerances."""
import os

import numpy as np
import pytest
import torch

from oracle import sb_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def build(tag, dev):
    from speechbrain_amd.inference.builders import build_modules

    g = np.load(os.path.join(GOLD, f"model_{tag}.npz"))
    d_model, nhead, d_ffn, n_enc, n_dec, vocab, beam, eos_thr = [int(v) for v in g["cfg"]]
    m = build_modules(dict(d_model=d_model, nhead=nhead, d_ffn=d_ffn, n_enc=n_enc, n_dec=n_dec, n_fft=512,
                           win_length=32), vocab=vocab)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    mods.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, strict=True)
    return g, mods.to(dev).eval()


def hyps_of(arr):
    return [[int(v) for v in row if v >= 0] for row in arr]


@pytest.mark.parametrize("tag", ["tiny_ctc", "tiny_noctc", "dh36"])
def test_golden_model(backend, tag):
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, S2STransformerGreedySearcher, ScorerBuilder

    g, mods = build(tag, dev)
    beam, eos_thr = int(g["cfg"][6]), bool(g["cfg"][7])
    ctc_w, max_ratio, min_ratio = [float(v) for v in g["cfgf"]]
    feats, wl = torch.from_numpy(g["feats"]).to(dev), torch.from_numpy(g["wav_lens"]).to(dev)
    with torch.no_grad():
        cnn = mods["CNN"](feats)
        assert float((cnn.cpu() - torch.from_numpy(g["cnn_out"])).abs().max()) <= 2e-5
        enc = mods["Transformer"].encode(cnn, wl)
        assert float((enc.cpu() - torch.from_numpy(g["enc_out"])).abs().max()) <= 5e-5
        enc_ref = torch.from_numpy(g["enc_out"]).to(dev)  # searches start from the reference's encoder output
        T = enc_ref.shape[1]
        h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
        pred = nat.decoder_prefix(h, torch.from_numpy(g["dec_tgt"]).int().to(dev), enc_ref, torch.round(T * wl).int())
        assert float((pred.cpu() - torch.from_numpy(g["dec_out"])).abs().max()) <= 5e-5

        gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                          min_decode_ratio=min_ratio, max_decode_ratio=max_ratio)
        hyps, _, scores, _ = gs(enc_ref, wl)
        assert hyps == hyps_of(g["greedy_hyps"])
        assert float((scores[:, 0].cpu() - torch.from_numpy(g["greedy_scores"])[:, : scores.shape[2]]).abs().max()) <= 1e-4

        scorer = None
        if ctc_w > 0:
            scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                                   weights={"ctc": ctc_w})
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=beam,
                                        using_eos_threshold=eos_thr, length_normalization=True, scorer=scorer)
        hyps, lens, scores, _ = bs(enc_ref, wl)
        assert hyps == hyps_of(g["beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g["beam_scores"])).abs().max()) <= 1e-4
        assert float((lens.cpu() - torch.from_numpy(g["beam_lens"])).abs().max()) <= 1e-6

        if "topk_hyps" in g.files:  # return_topk: padded [B,topk,L] tensors in descending score order
            bsk = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                             min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=beam,
                                             using_eos_threshold=eos_thr, length_normalization=True, scorer=scorer,
                                             return_topk=True, topk=3)
            k_hyps, k_lens, k_scores, k_lps = bsk(enc_ref, wl)
            assert torch.equal(k_hyps.cpu(), torch.from_numpy(g["topk_hyps"]))
            assert float((k_lens.cpu() - torch.from_numpy(g["topk_lens"])).abs().max()) <= 1e-6
            assert float((k_scores.cpu() - torch.from_numpy(g["topk_scores"])).abs().max()) <= 1e-4
            assert float((k_lps.cpu() - torch.from_numpy(g["topk_lps"])).abs().max()) <= 1e-4

        bs1 = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                         min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=1,
                                         using_eos_threshold=False, length_normalization=True)
        hyps1, _, s1, _ = bs1(enc_ref, wl)
        assert hyps1 == hyps_of(g["beam1_hyps"])
        assert float((s1.cpu() - torch.from_numpy(g["beam1_scores"])).abs().max()) <= 1e-4


@pytest.mark.parametrize("scale,key", [(1.5, "1p5"), (2, "2")])
def test_golden_partial_ctc_scorer(backend, scale, key):
    """ScorerBuilder(partial_scorers=[CTCScorer]) (scorer.py:1287-1300, ctc.py:168-262 with candidates): only the
    int(beam * scorer_beam_scale) best tokens of every hypothesis and <eos> receive a CTC score.  The reference's
    results (which differ from the full scorer's and between the two scales) must be reproduced exactly."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    g, mods = build("tiny_ctc", dev)
    beam, eos_thr = int(g["cfg"][6]), bool(g["cfg"][7])
    ctc_w, max_ratio, min_ratio = [float(v) for v in g["cfgf"]]
    wl = torch.from_numpy(g["wav_lens"]).to(dev)
    enc_ref = torch.from_numpy(g["enc_out"]).to(dev)
    scorer = ScorerBuilder(partial_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                           weights={"ctc": ctc_w}, scorer_beam_scale=scale)
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=beam,
                                    using_eos_threshold=eos_thr, length_normalization=True, scorer=scorer)
    assert bs.ctc_candidates == int(beam * scale)
    hyps, lens, scores, _ = bs(enc_ref, wl)
    assert hyps == hyps_of(g[f"partial{key}_hyps"])
    assert hyps != hyps_of(g["beam_hyps"])  # (the full scorer decodes something else: the mask matters)
    assert float((scores.cpu() - torch.from_numpy(g[f"partial{key}_scores"])).abs().max()) <= 1e-4
    assert float((lens.cpu() - torch.from_numpy(g[f"partial{key}_lens"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("wsize", [2, 5])
def test_golden_ctc_attention_window(backend, wsize):
    """CTCScorer(ctc_window_size=w) (scorer.py:183-187, ctc.py:189-200): the frames scored at a step are those within w
    of the attention peaks -- arg-max over the decoded positions of the last decoder layer's head-averaged
    cross-attention, min / max over the whole batch, exactly as the reference evaluates it for a transformer decoder.
    The reference's own results (window 2 decodes something else than the unwindowed scorer) must be reproduced."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    g, mods = build("tiny_ctc", dev)
    beam, eos_thr = int(g["cfg"][6]), bool(g["cfg"][7])
    ctc_w, max_ratio, min_ratio = [float(v) for v in g["cfgf"]]
    wl = torch.from_numpy(g["wav_lens"]).to(dev)
    enc_ref = torch.from_numpy(g["enc_out"]).to(dev)
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2, ctc_window_size=wsize)],
                           weights={"ctc": ctc_w})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=beam,
                                    using_eos_threshold=eos_thr, length_normalization=True, scorer=scorer)
    hyps, lens, scores, _ = bs(enc_ref, wl)
    assert hyps == hyps_of(g[f"window{wsize}_hyps"])
    if wsize == 2:
        assert hyps != hyps_of(g["beam_hyps"])  # (the window matters)
    assert float((scores.cpu() - torch.from_numpy(g[f"window{wsize}_scores"])).abs().max()) <= 1e-4
    assert float((lens.cpu() - torch.from_numpy(g[f"window{wsize}_lens"])).abs().max()) <= 1e-6


def test_waveform_to_tokens_vs_oracle(backend):
    """EncoderDecoderASR.transcribe_batch on padded waveforms vs the oracle's whole path."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr, flat_state_dict

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=2, n_dec=2, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=40, seed=3, beam_size=4, ctc_weight=0.4, device=str(dev))
    with torch.no_grad():
        asr.mods.seq_lin.w.weight.mul_(6.0)
        asr.mods.ctc_lin.w.weight.mul_(6.0)
    wav = 0.1 * torch.randn(3, 9600, generator=torch.Generator().manual_seed(1234))
    lens = torch.tensor([1.0, 0.8, 0.6])
    for i, l in enumerate(lens):
        wav[i, int(l * 9600):] = 0
    words, toks = asr.transcribe_batch(wav, lens)
    sd = flat_state_dict(asr)
    fc = O.FbankCfg(n_fft=512, n_mels=80, win_length_ms=32)
    mc = O.ModelCfg(d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=2, d_ffn=64, vocab=40)
    enc = O.encode_batch(wav, lens, sd, fc, mc, torch.zeros(80), torch.ones(80))
    assert float((asr.encode_batch(wav, lens).cpu() - enc).abs().max()) <= 5e-5
    hyps, _, _, _ = O.beam_search(enc, lens, sd, mc, O.SearchCfg(beam=4, ctc_weight=0.4))
    assert toks == hyps
    assert words == [" ".join(str(t) for t in h) for h in hyps]


def test_decoder_long_memory_and_prefix(backend):
    """KV-cached decoder vs the oracle's full-prefix decode with a memory longer than one
    cross-attention split (T' > 128 frames) and a prefix longer than one self-attention batch."""
    nat, dev = backend
    g, mods = build("tiny_ctc", dev)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    d_model, nhead, d_ffn, n_enc, n_dec, vocab = [int(v) for v in g["cfg"][:6]]
    cfg = O.ModelCfg(d_model=d_model, nhead=nhead, num_encoder_layers=n_enc, num_decoder_layers=n_dec, d_ffn=d_ffn,
                     vocab=vocab)
    gen = torch.Generator().manual_seed(77)
    enc = torch.randn(2, 300, d_model, generator=gen)
    enc_len = torch.tensor([300, 170], dtype=torch.int32)
    tgt = torch.randint(0, vocab, (2, 21), generator=gen)
    ref = O.decode(tgt, enc, enc_len, sd, cfg, "Transformer.")
    h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
    pred = nat.decoder_prefix(h, tgt.int().to(dev), enc.to(dev), enc_len.to(dev))
    assert float((pred.cpu() - ref).abs().max()) <= 5e-5


def test_beam_search_long_memory_vs_oracle(backend):
    """Beam 4 + CTC over a 150-frame memory (several 32-frame CTC segments, two cross-attention
    splits, one padded utterance) against the oracle's search: token ids exact, scores 1e-4."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    g, mods = build("tiny_ctc", dev)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    d_model, nhead, d_ffn, n_enc, n_dec, vocab = [int(v) for v in g["cfg"][:6]]
    cfg = O.ModelCfg(d_model=d_model, nhead=nhead, num_encoder_layers=n_enc, num_decoder_layers=n_dec, d_ffn=d_ffn,
                     vocab=vocab)
    enc = torch.randn(2, 150, d_model, generator=torch.Generator().manual_seed(5)) * 2.0
    wl = torch.tensor([1.0, 0.62])
    ratio = 14.5 / 150
    hyps_ref, lens_ref, sc_ref, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=4, ctc_weight=0.4, max_decode_ratio=ratio))
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=ratio, beam_size=4,
                                    using_eos_threshold=False, length_normalization=True, scorer=scorer)
    for overlap in (3, 1, 0):  # helper-stream modes of the CTC scorer must not change the result
        bs.overlap_ctc = overlap
        hyps, lens, sc, _ = bs(enc.to(dev), wl.to(dev))
        assert hyps == hyps_ref
        assert float((sc.cpu() - sc_ref).abs().max()) <= 1e-4
        assert float((lens.cpu() - lens_ref).abs().max()) <= 1e-6


def test_decoder_with_fused_layernorm_vs_oracle(backend):
    """d_model = 128 is eligible for the LayerNorm-fused projection kernel (the 32/72-wide golden models
    are not): decoder outputs and a CTC beam search against the oracle."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder
    from speechbrain_amd.inference.builders import build_modules

    m = build_modules(dict(d_model=128, nhead=4, d_ffn=256, n_enc=1, n_dec=2, n_fft=512, win_length=32), vocab=60, seed=5)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    gen = torch.Generator().manual_seed(9)
    with torch.no_grad():  # non-trivial LayerNorm affines and peaked heads
        for name, p in mods.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
        mods["seq_lin"].w.weight.mul_(5.0)
        mods["ctc_lin"].w.weight.mul_(5.0)
    sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
    mods = mods.to(dev).eval()
    cfg = O.ModelCfg(d_model=128, nhead=4, num_encoder_layers=1, num_decoder_layers=2, d_ffn=256, vocab=60)
    enc = torch.randn(2, 40, 128, generator=gen)
    wl = torch.tensor([1.0, 0.7])
    enc_len = torch.round(40 * wl).int()
    tgt = torch.randint(0, 60, (2, 7), generator=gen)
    h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
    assert h.W.seq_wf and h.layers[0].sa_in_wf  # the folded operands exist for this width
    pred = nat.decoder_prefix(h, tgt.int().to(dev), enc.to(dev), enc_len.to(dev))
    assert float((pred.cpu() - O.decode(tgt, enc, enc_len, sd, cfg, "Transformer.")).abs().max()) <= 5e-5
    ratio = 10.5 / 40
    hyps_ref, _, sc_ref, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=4, ctc_weight=0.4, max_decode_ratio=ratio))
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=ratio, beam_size=4,
                                    using_eos_threshold=False, length_normalization=True, scorer=scorer)
    hyps, _, sc, _ = bs(enc.to(dev), wl.to(dev))
    assert hyps == hyps_ref
    assert float((sc.cpu() - sc_ref).abs().max()) <= 1e-4


def _persist_model(dev, d_model, nhead, d_ffn, n_dec, vocab, seed):
    from speechbrain_amd.inference.builders import build_modules

    m = build_modules(dict(d_model=d_model, nhead=nhead, d_ffn=d_ffn, n_enc=1, n_dec=n_dec, n_fft=512, win_length=32), vocab=vocab, seed=seed)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    gen = torch.Generator().manual_seed(seed + 12)
    with torch.no_grad():
        for name, p in mods.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
        mods["seq_lin"].w.weight.mul_(4.0)
        mods["ctc_lin"].w.weight.mul_(4.0)
    sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
    cfg = O.ModelCfg(d_model=d_model, nhead=nhead, num_encoder_layers=1, num_decoder_layers=n_dec, d_ffn=d_ffn, vocab=vocab)
    return mods.to(dev).eval(), sd, cfg, gen


@pytest.mark.parametrize("shape", ["d128", "d512"])
def test_persistent_few_row_decoding_step_vs_oracle_and_the_launch_per_operation_path(backend, shape):
    """csrc/decoder_persist.hip: the decoder stack of a step with <= 16 hypothesis rows (one utterance's beam -- the
    single-utterance latency regime) as ONE cooperative launch with grid barriers between sub-layers and agent-scope
    hand-over of the activations.  Against the oracle: teacher-forced decoder outputs 5e-5 (3 rows, beam 1), beam search
    with CTC for one utterance at beam 10 and beam 16 (the full 16-row tile) and three utterances at beam 4 (12 rows, ragged
    memory lengths), a 300-frame memory (several 256-frame runs per wave in the cross-attention), the greedy searcher --
    token ids exact, scores 1e-4; and against the launch-per-operation path of the same library (persist = 0): ids equal,
    scores 2e-5.  The profiler's launch names show which path ran; with another grid (persist_grid) the result is the same."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, S2STransformerGreedySearcher, ScorerBuilder

    dm, H, dffn = (128, 2, 256) if shape == "d128" else (512, 8, 2048)
    mods, sd, cfg, gen = _persist_model(dev, dm, H, dffn, 2, 60, 7 if shape == "d128" else 9)

    def searcher(beam, ratio, ctc=0.4):
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": ctc})
        return S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2, min_decode_ratio=0.0,
                                          max_decode_ratio=ratio, beam_size=beam, using_eos_threshold=False,
                                          length_normalization=True, scorer=scorer)

    def run(fn):
        nat.prof_reset()
        nat.prof_enable(True)
        try:
            out = fn()
        finally:
            nat.prof_enable(False)
        return out, nat.prof_report()

    enc = torch.randn(3, 30, dm, generator=gen)
    wl = torch.tensor([1.0, 0.7, 0.9])
    enc_len = torch.round(30 * wl).int()
    tgt = torch.randint(0, 60, (3, 6), generator=gen)
    h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
    pred, rep = run(lambda: nat.decoder_prefix(h, tgt.int().to(dev), enc.to(dev), enc_len.to(dev)))
    assert rep.get("decoder_step_persist", {}).get("count", 0) == tgt.shape[1] and "self_attn_step" not in rep, sorted(rep)
    assert float((pred.cpu() - O.decode(tgt, enc, enc_len, sd, cfg, "Transformer.")).abs().max()) <= 5e-5
    cases = [("one utterance, beam 10", enc[:1], wl[:1], 10, 8.5 / 30), ("three utterances, beam 4", enc, wl, 4, 8.5 / 30)]
    if shape == "d128":
        long_enc = torch.randn(1, 300, dm, generator=gen)
        cases += [("one utterance, beam 16", enc[1:2], torch.ones(1), 16, 6.5 / 30),
                  ("300-frame memory", long_enc, torch.tensor([0.93]), 10, 6.5 / 300)]
    for tag, e, w, beam, ratio in cases:
        ref_h, _, ref_s, _ = O.beam_search(e, w, sd, cfg, O.SearchCfg(beam=beam, ctc_weight=0.4, max_decode_ratio=ratio))
        bs = searcher(beam, ratio)
        (hyps, _, sc, _), rep = run(lambda: bs(e.to(dev), w.to(dev)))
        assert rep.get("decoder_step_persist", {}).get("count", 0) >= 1 and "cross_attn_step" not in rep and "gemm_skinny_ln" not in rep, (tag, sorted(rep))
        assert hyps == ref_h, tag
        assert float((sc.cpu() - ref_s).abs().max()) <= 1e-4, tag
        with nat.knobs(persist=0):
            (hyps0, _, sc0, _), rep0 = run(lambda: bs(e.to(dev), w.to(dev)))
        assert "decoder_step_persist" not in rep0 and ("self_attn_step" in rep0 or "self_attn_anc" in rep0), (tag, sorted(rep0))
        assert hyps0 == hyps and float((sc0 - sc).abs().max()) <= 2e-5, tag
    # another grid: fewer workgroups than column tiles / attention items (every loop over tiles and items runs more than once)
    e, w = enc[:1], wl[:1]
    bs = searcher(10, 8.5 / 30)
    base = bs(e.to(dev), w.to(dev))
    for grid in (3, 1000):
        with nat.knobs(persist_grid=grid):
            got = bs(e.to(dev), w.to(dev))
        assert got[0] == base[0] and torch.equal(got[2], base[2]), grid  # (the arithmetic does not depend on the grid)
    # the grid barriers on a two-level arrival counter (persist_tree): the same results, grid sizes with full, ragged and single sub-counters
    for grid in (128, 3, 13, 1000):
        with nat.knobs(persist_tree=1, persist_grid=grid):
            got = bs(e.to(dev), w.to(dev))
        assert got[0] == base[0] and torch.equal(got[2], base[2]), ("tree", grid)
    gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2, min_decode_ratio=0.0,
                                      max_decode_ratio=8.5 / 30)
    (g_h, _, g_s, _), rep = run(lambda: gs(enc.to(dev), wl.to(dev)))
    assert rep.get("decoder_step_persist", {}).get("count", 0) >= 1, sorted(rep)
    ref_g = O.greedy_search(enc, wl, sd, cfg, O.SearchCfg(beam=1, max_decode_ratio=8.5 / 30))
    assert g_h == ref_g[0]


@pytest.mark.parametrize("ln", [1, 0])
def test_decoder_on_the_x3r_route_vs_oracle(backend, ln):
    """The decode step's projections as sbk_gemm_nt_x3r (csrc/gemm.hip: gemm_x3r_kernel -- fp32 results on the bf16
    matrix pipe from the panel images of the decoder's weights; the route of every step with ~200 hypothesis rows or
    more): d_model 256 / d_ffn 512 are eligible widths (K % 256 == 0), the row threshold is lowered so that this small
    search takes it (x3r_min_rows).  Teacher-forced decoder outputs 5e-5 and a beam search with CTC (ids exact, scores 1e-4)
    against the oracle; with norm1 / norm2 / norm3 and decoder.norm inside the projections they feed (sbk_gemm_ln_nt_x3r,
    x3r_ln = 1: the default -- the profiler's launch names show which route ran) and as launches of their own (0); the
    result does not change when the route is switched off."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder
    from speechbrain_amd.inference.builders import build_modules

    m = build_modules(dict(d_model=256, nhead=4, d_ffn=512, n_enc=1, n_dec=2, n_fft=512, win_length=32), vocab=60, seed=7)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    gen = torch.Generator().manual_seed(19)
    with torch.no_grad():
        for name, p in mods.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
        mods["seq_lin"].w.weight.mul_(4.0)
        mods["ctc_lin"].w.weight.mul_(4.0)
    sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
    mods = mods.to(dev).eval()
    cfg = O.ModelCfg(d_model=256, nhead=4, num_encoder_layers=1, num_decoder_layers=2, d_ffn=512, vocab=60)
    enc = torch.randn(3, 30, 256, generator=gen)
    wl = torch.tensor([1.0, 0.7, 0.9])
    enc_len = torch.round(30 * wl).int()
    tgt = torch.randint(0, 60, (3, 6), generator=gen)
    # (persist: at 12 rows the step would otherwise be the persistent few-row launch, csrc/decoder_persist.hip)
    with nat.knobs(x3r_ln=ln, x3r_min_rows=1, persist=0):
        try:
            h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
            assert h.layers[0].sa_in_wp and h.layers[0].ff2_wp and h.W.seq_wp  # the panel images exist for these widths
            assert h.layers[0].sa_in_wfp and h.layers[0].ca_q_wfp and h.layers[0].ff1_wfp and h.W.seq_wfp  # and the folded ones
            nat.prof_reset()
            nat.prof_enable(True)
            pred = nat.decoder_prefix(h, tgt.int().to(dev), enc.to(dev), enc_len.to(dev))
            nat.prof_enable(False)
            rep = nat.prof_report()
            fused = rep.get("gemm_ln_x3r", {}).get("count", 0)
            assert ("gemm_ln_x3r" in rep) == (ln == 1), sorted(rep)
            # fused: three per layer and position; the LayerNorm launches left are decoder.norm, whose rows are this entry's result
            norms = rep.get("layernorm", {}).get("count", 0)
            assert (fused == 6 * tgt.shape[1] and norms == tgt.shape[1]) if ln else fused == 0, (fused, norms)
            assert float((pred.cpu() - O.decode(tgt, enc, enc_len, sd, cfg, "Transformer.")).abs().max()) <= 5e-5
            ratio = 8.5 / 30
            hyps_ref, _, sc_ref, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=4, ctc_weight=0.4, max_decode_ratio=ratio))
            scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
            bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                            min_decode_ratio=0.0, max_decode_ratio=ratio, beam_size=4,
                                            using_eos_threshold=False, length_normalization=True, scorer=scorer)
            nat.prof_reset()
            nat.prof_enable(True)
            hyps, _, sc, _ = bs(enc.to(dev), wl.to(dev))
            nat.prof_enable(False)
            rep = nat.prof_report()
            if ln:  # a search step: every LayerNorm of the decoder, decoder.norm included, inside a projection
                assert rep["gemm_ln_x3r"]["count"] % 6 == 0 and "layernorm" not in rep, sorted(rep)  # (decoder.norm: the few-row fused kernel at 12 rows)
            assert hyps == hyps_ref
            assert float((sc.cpu() - sc_ref).abs().max()) <= 1e-4
            if ln:
                # decoder.norm inside the vocabulary projection as well: at bench sizes (1 280 rows x 5 000 tokens) the few-row
                # fused kernel does not take that shape; here it is switched off (skinny_off) so that this small search takes the route
                with nat.knobs(skinny_off=1):
                    nat.prof_reset()
                    nat.prof_enable(True)
                    hyps_v, _, sc_v, _ = bs(enc.to(dev), wl.to(dev))
                    nat.prof_enable(False)
                    rep = nat.prof_report()
                assert rep["gemm_ln_x3r"]["count"] % 7 == 0 and "layernorm" not in rep, sorted(rep)
                assert hyps_v == hyps_ref and float((sc_v.cpu() - sc_ref).abs().max()) <= 1e-4
            with nat.knobs(x3r_mode=0):  # the fp32-MFMA route of the same handle
                hyps0, _, sc0, _ = bs(enc.to(dev), wl.to(dev))
            assert hyps0 == hyps and float((sc0 - sc).abs().max()) <= 1e-4
        finally:
            nat.prof_enable(False)


# test_decode_step_launch_plan_per_route: profiler launch name -> count of (decoder_prefix over 3 positions, beam-4 CTC search of
# 8 steps), recorded from the commit BEFORE search.hip's projection router existed (the hand-written ladders of decoder_step)
# on the CPU emulator, which runs the same host code and the same profiler scopes as the GPU build.
_STEP = dict(cross_attn_step=2, embed_pos=1, self_attn_step=2)  # per position / step of a two-layer decoder
_SEARCH = dict(beam_update=8, ctc_advance=7, ctc_score_step=8, log_softmax=1, score_topk=8)


def _plan(prefix, search, persist=False):
    step = {} if persist else _STEP
    return (dict({k: 3 * v for k, v in step.items()}, gemm_nt_32x64=2, **prefix),
            dict({k: 8 * v for k, v in step.items()}, gemm_nt_32x64=3, **_SEARCH, **search))


_LAUNCH_PLANS = {
    # x3r layers with norm1/2/3 inside the projections; decoder.norm: a launch (prefix) / the few-row fused kernel (search)
    "a": _plan(dict(gemm_ln_x3r=18, gemm_x3r=18, layernorm=3), dict(gemm_ln_x3r=48, gemm_x3r=48, gemm_skinny_ln=8)),
    # x3r layers, every LayerNorm of a layer as a launch
    "b": _plan(dict(gemm_x3r=36, layernorm=21), dict(gemm_x3r=96, layernorm=48, gemm_skinny_ln=8)),
    # fp32 layers, LayerNorm folded
    "c": _plan(dict(gemm_skinny=18, gemm_skinny_ln=18, layernorm=3), dict(gemm_skinny=48, gemm_skinny_ln=56)),
    # fp32 layers, no folded weights: every LayerNorm a launch
    "d": _plan(dict(gemm_skinny=36, layernorm=21), dict(gemm_skinny=104, layernorm=56)),
    # d_ffn 384: ff2 has no panel, both layers whole on the fp32 route
    "e": _plan(dict(gemm_skinny=18, gemm_skinny_ln=18, layernorm=3), dict(gemm_skinny=48, gemm_skinny_ln=56)),
    # (a) with decoder.norm inside the panel vocabulary projection
    "f": _plan(dict(gemm_ln_x3r=18, gemm_x3r=18, layernorm=3), dict(gemm_ln_x3r=56, gemm_x3r=48)),
    # the single-launch step
    "g": _plan(dict(decoder_step_persist=3), dict(decoder_step_persist=8), persist=True),
}
_ROUTE_KNOBS = dict(x3r_min_rows=1, persist=0, x3r_ln=1)
_ROUTE_CONFIGS = {  # tag -> (d_ffn, fold, knobs)
    "a": (512, True, _ROUTE_KNOBS),
    "b": (512, True, dict(_ROUTE_KNOBS, x3r_ln=0)),
    "c": (512, True, dict(_ROUTE_KNOBS, x3r_mode=0)),
    "d": (512, False, dict(_ROUTE_KNOBS, x3r_mode=0)),
    "e": (384, True, _ROUTE_KNOBS),
    "f": (512, True, dict(_ROUTE_KNOBS, skinny_off=1)),
    "g": (512, True, dict(x3r_min_rows=1, x3r_ln=1)),
}
_ROUTE_REFS = {}


def _route_model(d_ffn):
    """The decoder of test_decoder_on_the_x3r_route_vs_oracle (d_ffn 512) or one whose ff2 has no panel image (384), its
    inputs and the oracle's results -- computed once per width, shared by the cases, never modified."""
    if d_ffn not in _ROUTE_REFS:
        from speechbrain_amd.inference.builders import build_modules

        m = build_modules(dict(d_model=256, nhead=4, d_ffn=d_ffn, n_enc=1, n_dec=2, n_fft=512, win_length=32), vocab=60, seed=7)
        mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
        gen = torch.Generator().manual_seed(19)
        with torch.no_grad():
            for name, p in mods.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen))
            mods["seq_lin"].w.weight.mul_(4.0)
            mods["ctc_lin"].w.weight.mul_(4.0)
        sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
        cfg = O.ModelCfg(d_model=256, nhead=4, num_encoder_layers=1, num_decoder_layers=2, d_ffn=d_ffn, vocab=60)
        enc = torch.randn(3, 30, 256, generator=gen)
        wl = torch.tensor([1.0, 0.7, 0.9])
        enc_len = torch.round(30 * wl).int()
        tgt = torch.randint(0, 60, (3, 3), generator=gen)
        pred = O.decode(tgt, enc, enc_len, sd, cfg, "Transformer.")
        hyps, _, sc, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=4, ctc_weight=0.4, max_decode_ratio=8.5 / 30))
        _ROUTE_REFS[d_ffn] = (mods, enc, wl, enc_len, tgt, pred, hyps, sc)
    return _ROUTE_REFS[d_ffn]


@pytest.mark.parametrize("config", sorted(_ROUTE_CONFIGS))
def test_decode_step_launch_plan_per_route(backend, config):
    """Which kernels a decode step launches is decided in ONE place (csrc/search.hip, the route table above StepRouter); this
    pins the decision for every route at the smallest decoder that reaches them all (d_model 256, 4 heads, 2 layers, vocabulary
    60, 3 utterances x 30 frames): the exact launch names and counts of a 3-position decoder_prefix and of a beam-4 search with
    CTC 0.4 (_LAUNCH_PLANS: recorded before the router existed), and the outputs against the oracle (prefix 5e-5, ids exact,
    scores 1e-4).  (a) panel kernels with the LayerNorms inside, (b) with LayerNorm launches, (c) fp32 with folded LayerNorms,
    (d) fp32 without folded weights, (e) a layer that lacks one panel (ff2 at d_ffn 384) takes the fp32 route WHOLE, (f) decoder.norm
    inside the panel vocabulary projection, (g) the persistent single-launch step at 12 rows."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    d_ffn, fold, knobs = _ROUTE_CONFIGS[config]
    mods, enc, wl, enc_len, tgt, pred_ref, hyps_ref, sc_ref = _route_model(d_ffn)
    mods = mods.to(dev).eval()

    def run(fn):
        nat.prof_reset()
        nat.prof_enable(True)
        try:
            out = fn()
        finally:
            nat.prof_enable(False)
        return out, {k: v["count"] for k, v in nat.prof_report().items()}

    with nat.knobs(**knobs):
        h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"], fold=fold)
        assert bool(h.layers[0].ff2_wp) == (d_ffn == 512) and bool(h.layers[0].sa_in_wf) == fold
        pred, plan_prefix = run(lambda: nat.decoder_prefix(h, tgt.int().to(dev), enc.to(dev), enc_len.to(dev)))
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=8.5 / 30, beam_size=4,
                                        using_eos_threshold=False, length_normalization=True, scorer=scorer)
        bs._dec_handle = h  # (the searcher would build a folded handle of its own)
        (hyps, _, sc, _), plan_search = run(lambda: bs(enc.to(dev), wl.to(dev)))
    print(config, plan_prefix, plan_search, float((pred.cpu() - pred_ref).abs().max()), float((sc.cpu() - sc_ref).abs().max()))
    want_prefix, want_search = _LAUNCH_PLANS[config]
    assert plan_prefix == want_prefix
    assert plan_search == want_search
    if config == "e":
        assert not any(k.startswith("gemm_x3r") or k.startswith("gemm_ln_x3r") for k in list(plan_prefix) + list(plan_search))
    assert float((pred.cpu() - pred_ref).abs().max()) <= 5e-5
    assert hyps == hyps_ref
    assert float((sc.cpu() - sc_ref).abs().max()) <= 1e-4


def test_search_entries_take_exactly_their_workspace(backend, monkeypatch):
    """Every search entry lays its workspace out once (csrc/search.hip, the *Layout structs): the same carve gives
    sbk_X_workspace_bytes and the entry's pointers.  For each entry -- decoder_prefix, lm_prefix, greedy_search,
    prompted_greedy_search, beam_search with CTC and beam_search with CTC and an LM -- at one tiny shape: a workspace of
    exactly sbk_X_workspace_bytes succeeds; 256 bytes (one carving granule) less fails with the entry's "workspace too small"."""
    nat, dev = backend
    from speechbrain_amd.decoders import (CTCScorer, S2STransformerBeamSearcher, ScorerBuilder, TransformerLMScorer)

    from speechbrain_amd.inference.builders import build_modules

    g = np.load(os.path.join(GOLD, "model_tiny_lm_ctc.npz"))
    d_model, nhead, d_ffn, n_enc, n_dec, vocab, beam, _ = [int(v) for v in g["cfg"]]
    m = build_modules(dict(d_model=d_model, nhead=nhead, d_ffn=d_ffn, n_enc=n_enc, n_dec=n_dec, n_fft=512, win_length=32), vocab=vocab)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    mods.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/") and not k.startswith("sd/LM.")}, strict=True)
    mods = mods.to(dev).eval()
    lm = build_lm(g, dev)
    enc = torch.from_numpy(g["enc_out"]).to(dev)[:2, :9].contiguous()
    enc_len = torch.tensor([9, 6], dtype=torch.int32, device=dev)
    wl = torch.tensor([1.0, 0.7], device=dev)
    tok = torch.tensor([[1, 5, 7], [1, 4, 3]], dtype=torch.int32, device=dev)
    h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
    lmh = nat.LMHandle(lm)

    def searcher(with_lm):
        full, weights = [CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], {"ctc": 0.4}
        if with_lm:
            full, weights = [TransformerLMScorer(language_model=lm, temperature=1.0)] + full, dict(weights, transformerlm=0.3)
        return S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                          min_decode_ratio=0.0, max_decode_ratio=0.34, beam_size=2, using_eos_threshold=False,
                                          length_normalization=True, scorer=ScorerBuilder(full_scorers=full, weights=weights))

    bs_ctc, bs_lm = searcher(False), searcher(True)
    entries = [
        ("sbk_decoder_prefix_workspace_bytes", "decoder_prefix: workspace too small", lambda: nat.decoder_prefix(h, tok, enc, enc_len)),
        ("sbk_lm_prefix_workspace_bytes", "lm_prefix: workspace too small", lambda: nat.lm_prefix(lmh, tok)),
        ("sbk_greedy_search_workspace_bytes", "greedy: workspace too small", lambda: nat.greedy_search(h, enc, enc_len, 0, 3, 1, 2)),
        ("sbk_prompted_greedy_search_workspace_bytes", "prompted_greedy_search: workspace too small",
         lambda: nat.prompted_greedy_search(h, enc, enc_len, tok[:, :2].contiguous(), 2, 2)),
        ("sbk_beam_search_workspace_bytes", "beam_search: workspace too small", lambda: bs_ctc(enc, wl)),
        ("sbk_beam_search_workspace_bytes", "beam_search: workspace too small", lambda: bs_lm(enc, wl)),
    ]
    lib = nat.load()
    with torch.no_grad():
        for sizer, message, call in entries:
            real = getattr(lib, sizer)
            asked = []

            def exact(*a, _real=real):
                asked.append(_real(*a))
                return asked[-1]

            monkeypatch.setattr(lib, sizer, exact, raising=False)
            call()  # the binding hands the entry exactly what the sizer returned
            assert asked and asked[-1] > 256 and asked[-1] % 256 == 0, (sizer, asked)
            monkeypatch.setattr(lib, sizer, lambda *a, _real=real: _real(*a) - 256, raising=False)
            with pytest.raises(nat.SbkError, match=message):
                call()
            monkeypatch.setattr(lib, sizer, real, raising=False)


def build_lm(g, dev):
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM

    lm_d, lm_heads, lm_ffn, lm_layers, pre = [int(v) for v in g["lm_cfg"]]
    lm = TransformerLM(vocab=int(g["cfg"][5]), d_model=lm_d, nhead=lm_heads, num_encoder_layers=lm_layers,
                       num_decoder_layers=0, d_ffn=lm_ffn, dropout=0.0, activation=torch.nn.GELU,
                       normalize_before=bool(pre))
    lm.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/LM.")}, strict=True)
    return lm.to(dev).eval()


@pytest.mark.parametrize("tag", ["tiny_lm_ctc", "tiny_lm_prenorm"])
def test_golden_transformerlm_scorer(backend, tag):
    """a20: TransformerLM.forward and the [transformerlm, ctc] / [transformerlm] searches against the
    reference's outputs (post-norm and pre-norm LM layers, pad-0 key masking, LM temperature)."""
    nat, dev = backend
    from speechbrain_amd.decoders import (CTCScorer, S2STransformerBeamSearcher, ScorerBuilder,
                                          TransformerLMScorer)
    from speechbrain_amd.inference.builders import build_modules

    g = np.load(os.path.join(GOLD, f"model_{tag}.npz"))
    d_model, nhead, d_ffn, n_enc, n_dec, vocab, beam, _ = [int(v) for v in g["cfg"]]
    ctc_w, _, _, lm_w, lm_temp, temp = [float(v) for v in g["cfgf"]]
    m = build_modules(dict(d_model=d_model, nhead=nhead, d_ffn=d_ffn, n_enc=n_enc, n_dec=n_dec, n_fft=512,
                           win_length=32), vocab=vocab)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    mods.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files
                          if k.startswith("sd/") and not k.startswith("sd/LM.")}, strict=True)
    mods = mods.to(dev).eval()
    lm = build_lm(g, dev)
    with torch.no_grad():
        logits = lm(torch.from_numpy(g["lm_tokens"]).to(dev))
        assert float((logits.cpu() - torch.from_numpy(g["lm_logits"])).abs().max()) <= 1e-4
        full, weights = [TransformerLMScorer(language_model=lm, temperature=lm_temp)], {"transformerlm": lm_w}
        if ctc_w > 0:
            full.append(CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2))
            weights["ctc"] = ctc_w
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=beam,
                                        using_eos_threshold=False, length_normalization=True, temperature=temp,
                                        scorer=ScorerBuilder(full_scorers=full, weights=weights))
        enc = torch.from_numpy(g["enc_out"]).to(dev)
        wl = torch.from_numpy(g["wav_lens"]).to(dev)
        hyps, lens, scores, _ = bs(enc, wl)
        assert hyps == hyps_of(g["beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g["beam_scores"])).abs().max()) <= 1e-4
        assert float((lens.cpu() - torch.from_numpy(g["beam_lens"])).abs().max()) <= 1e-6


@pytest.mark.parametrize("beam,partial", [(4, False), (10, False), (3, True)])
def test_scorer_step_protocol_vs_oracle(backend, beam, partial):
    """a18 / a19 as CALLABLE step APIs (VERDICT r5 missing #3): ScorerBuilder.reset_scorer_mem / score / permute_scorer_mem with a
    CTCScorer (scorer.py:1221-1315 -> sbk_ctc_scorer_reset / _score / _permute_f32), driven the way the reference's
    S2SBeamSearcher drives them -- a beam update between the steps chooses (previous path, token) pairs over beam x V of every
    utterance -- against the oracle's CTCPrefixScore restatement step by step: six steps, ragged utterance lengths, repeated
    last tokens; as a full scorer and as the partial scorer of the best int(beam * scorer_beam_scale) tokens."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, ScorerBuilder

    mods, sd, cfg, gen = _persist_model(dev, 128, 2, 256, 1, 50, 21)
    B, T, V = 3, 37, 50
    enc = torch.randn(B, T, 128, generator=gen)
    wl = torch.tensor([1.0, 0.62, 0.85])
    enc_len = torch.round(T * wl).int()
    logp = torch.log_softmax(torch.nn.functional.linear(enc, sd["ctc_lin.w.weight"], sd["ctc_lin.w.bias"]), -1)
    oracle = O.CTCPrefixScorer(logp, enc_len, 0, 2)
    ctc = CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)
    sb = ScorerBuilder(partial_scorers=[ctc], weights={"ctc": 0.4}, scorer_beam_scale=1.5) if partial else \
        ScorerBuilder(full_scorers=[ctc], weights={"ctc": 0.4})
    memory = sb.reset_scorer_mem(enc.to(dev), wl.to(dev))
    state = None
    n = B * beam
    inp = torch.ones(n, dtype=torch.long)  # <bos>
    for step in range(6):
        lp = torch.log_softmax(3.0 * torch.randn(n, V, generator=gen), -1)
        got, new_mem = sb.score(inp.to(dev), memory, None, lp.clone().to(dev), beam)
        delta, st = oracle.step(inp, state, beam)
        ref = lp.clone()
        if partial:
            k = max(1, min(int(beam * 1.5), V))
            cand = ref.topk(k, dim=-1).indices
            keep = torch.zeros(n, V, dtype=torch.bool).scatter_(1, cand, True)
            keep[:, 2] = True
            psi = st[1]
            psi_prev = psi - delta  # (rows constant over V)
            delta = torch.where(keep, delta, torch.full_like(delta, -1e20) - psi_prev)
        else:
            ref[:, 0] = -1e20
        ref = ref + 0.4 * delta
        live = ref > -1e19
        assert torch.equal(got.cpu() > -1e19, live), step
        assert float((got.cpu() - ref)[live].abs().max()) <= 2e-4, step
        assert float((got.cpu()[~live] / ref[~live] - 1.0).abs().max()) <= 1e-5 if (~live).any() else True
        # the beam update: the `beam` best (path, token) pairs of every utterance (at step 0 only the first beam is live)
        flat = ref.view(B, beam * V).clone()
        if step == 0:
            flat[:, V:] = -float("inf")
        cand = flat.topk(beam, dim=-1).indices  # [B, beam]
        if step == 2:  # make a hypothesis repeat its last token: the same-token correction of the scorer (ctc.py:175-186)
            cand[0, 0] = (cand[0, 0] // V) * V + int(inp.view(B, beam)[0, cand[0, 0] // V])
        index = (torch.div(cand, V, rounding_mode="floor") + (torch.arange(B) * beam).unsqueeze(1)).view(-1)
        memory = sb.permute_scorer_mem(new_mem, index.to(dev), cand.to(dev))
        state = oracle.permute(st, cand, beam)
        inp = (cand % V).view(-1)


@pytest.mark.parametrize("tag", ["tiny_lm_ctc"])
def test_transformerlm_scorer_step_protocol_vs_golden(backend, tag):
    """TransformerLMScorer.score / permute_mem as the reference's step protocol (scorer.py:507-560: the prefix is the memory, the
    LM runs over all of it): log-probabilities of the last position against the reference's own LM logits of the golden file."""
    nat, dev = backend
    from speechbrain_amd.decoders import TransformerLMScorer

    g = np.load(os.path.join(GOLD, f"model_{tag}.npz"))
    lm = build_lm(g, dev)
    temp = float(g["cfgf"][4])
    toks = torch.from_numpy(g["lm_tokens"]).long()
    ref = torch.log_softmax(torch.from_numpy(g["lm_logits"]) / temp, -1)
    sc = TransformerLMScorer(language_model=lm, temperature=temp)
    memory = None
    with torch.no_grad():
        for t in range(min(4, toks.shape[1])):
            lp, memory = sc.score(toks[:, t].to(dev), memory, None, None)
            assert float((lp.cpu() - ref[:, t]).abs().max()) <= 2e-4, t
        perm = torch.arange(toks.shape[0] - 1, -1, -1)
        memory = sc.permute_mem(memory, perm.to(dev))
        assert torch.equal(memory.cpu().long(), toks[perm][:, : memory.shape[1]])


@pytest.mark.parametrize("tag", ["rope", "rope_dh36"])
def test_golden_rope_conformer(backend, tag):
    """RoPEMHA encoder (attention_type of the current conformer_large.yaml) against the reference's
    outputs: the attention module with padding, the whole encoder, then beam search + CTC."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder
    from speechbrain_amd.inference.builders import build_modules

    g = np.load(os.path.join(GOLD, f"model_{tag}.npz"))
    d_model, nhead, d_ffn, n_enc, n_dec, vocab, beam, _ = [int(v) for v in g["cfg"]]
    m = build_modules(dict(d_model=d_model, nhead=nhead, d_ffn=d_ffn, n_enc=n_enc, n_dec=n_dec, n_fft=512,
                           win_length=32, attention_type="RoPEMHA"), vocab=vocab)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    res = mods.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}, strict=False)
    assert not res.unexpected_keys and all(k.endswith(".pe") for k in res.missing_keys)
    mods = mods.to(dev).eval()
    wl = torch.from_numpy(g["wav_lens"]).to(dev)
    with torch.no_grad():
        mha = mods["Transformer"].encoder.layers[0].mha_layer
        x = torch.from_numpy(g["mha_x"]).to(dev)
        T = x.shape[1]
        pad = (torch.arange(T)[None, :] >= torch.from_numpy(g["mha_len"])[:, None]).to(dev)
        out, none = mha(x, x, x, key_padding_mask=pad)
        assert none is None
        assert float((out.cpu() - torch.from_numpy(g["mha_out"])).abs().max()) <= 2e-5
        enc = mods["Transformer"].encode(torch.from_numpy(g["cnn_out"]).to(dev), wl)
        assert float((enc.cpu() - torch.from_numpy(g["enc_out"])).abs().max()) <= 5e-5
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                               weights={"ctc": float(g["cfgf"][0])})
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=beam,
                                        using_eos_threshold=False, length_normalization=True, scorer=scorer)
        hyps, _, scores, _ = bs(torch.from_numpy(g["enc_out"]).to(dev), wl)
        assert hyps == hyps_of(g["beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g["beam_scores"])).abs().max()) <= 1e-4


@pytest.mark.parametrize("nhead", [2, 4, 8])
@pytest.mark.parametrize("rows", [0, 3, 4])
def test_cross_attention_kernel_variants(backend, nhead, rows):
    """The frame-per-thread cross-attention kernel (head_dim 64 / 32 / 16) with 128-, 256- and 64-frame splits of a memory
    with ragged lengths (several partial results merged per utterance), through the KV-cached decoder and a 5-beam search
    vs the oracle.  (The register-ring kernel: tests/test_kernels.py::test_cross_attention_register_ring_kernel.)"""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_modules

    m = build_modules(dict(d_model=128, nhead=nhead, d_ffn=128, n_enc=1, n_dec=1, n_fft=512, win_length=32), vocab=30,
                      seed=nhead)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
    mods = mods.to(dev).eval()
    cfg = O.ModelCfg(d_model=128, nhead=nhead, num_encoder_layers=1, num_decoder_layers=1, d_ffn=128, vocab=30)
    gen = torch.Generator().manual_seed(3)
    enc = torch.randn(3, 300, 128, generator=gen)
    enc_len = torch.tensor([300, 171, 5], dtype=torch.int32)
    tgt = torch.randint(0, 30, (3, 4), generator=gen)
    from speechbrain_amd.decoders import S2STransformerBeamSearcher

    with torch.no_grad():
        mods["seq_lin"].w.weight.mul_(6.0)
    sd["seq_lin.w.weight"] = sd["seq_lin.w.weight"] * 6.0
    wl = enc_len.float() / 300
    ratio = 6.5 / 300
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=ratio, beam_size=5,
                                    using_eos_threshold=False, length_normalization=True)
    # cross_fc256: 3 / 4 = 256- / 64-frame splits; persist: 15 rows would otherwise run as the persistent few-row step, which has its own attention
    with nat.knobs(cross_rows=0, cross_fc256={3: 1, 4: 2}.get(rows, 0), persist=0):
        h = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
        pred = nat.decoder_prefix(h, tgt.int().to(dev), enc.to(dev), enc_len.to(dev))
        hyps, _, sc, _ = bs(enc.to(dev), wl.to(dev))  # several beams per (utterance, head) workgroup
    assert float((pred.cpu() - O.decode(tgt, enc, enc_len, sd, cfg, "Transformer.")).abs().max()) <= 5e-5
    hyps_ref, _, sc_ref, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=5, max_decode_ratio=ratio))
    assert hyps == hyps_ref
    assert float((sc.cpu() - sc_ref).abs().max()) <= 1e-4


@pytest.mark.parametrize("beam,ctc_w", [(20, 0.4), (33, 0.0), (17, 0.4)])
def test_wide_beam_vs_oracle(backend, beam, ctc_w):
    """beam > 16 (the recipe's test_search uses 66): radix-select top-k + CTC tables in tiles of 16 beams."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    g, mods = build("tiny_ctc", dev)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    d_model, nhead, d_ffn, n_enc, n_dec, vocab = [int(v) for v in g["cfg"][:6]]
    cfg = O.ModelCfg(d_model=d_model, nhead=nhead, num_encoder_layers=n_enc, num_decoder_layers=n_dec, d_ffn=d_ffn,
                     vocab=vocab)
    enc, wl = torch.from_numpy(g["enc_out"]), torch.from_numpy(g["wav_lens"])
    scorer = None
    if ctc_w > 0:
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                               weights={"ctc": ctc_w})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=beam,
                                    using_eos_threshold=False, length_normalization=True, scorer=scorer)
    hyps, lens, scores, _ = bs(enc.to(dev), wl.to(dev))
    hyps_ref, lens_ref, sc_ref, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=beam, ctc_weight=ctc_w))
    assert hyps == hyps_ref
    assert float((scores.cpu() - sc_ref).abs().max()) <= 1e-4
    assert float((lens.cpu() - lens_ref).abs().max()) <= 1e-6


def test_from_hparams_local_model_directory(backend):
    """EncoderDecoderASR.from_hparams on a model directory in the reference's HuggingFace layout
    (tests/golden/pretrained_tiny: hyperparams.yaml written for ``speechbrain.*`` classes + asr / lm /
    normalizer / tokenizer checkpoints saved by the reference's own savers, oracle/make_golden.py):
    the transcription must equal what the reference's EncoderDecoderASR produced from the same files
    (beam 20 > 16, TransformerLM + CTC scorers, SentencePiece detokenisation)."""
    nat, dev = backend
    from speechbrain_amd.inference.ASR import EncoderDecoderASR

    exp = np.load(os.path.join(GOLD, "pretrained_tiny_expected.npz"))
    asr = EncoderDecoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_tiny"), run_opts={"device": str(dev)})
    assert type(asr.mods.decoder).__module__.startswith("speechbrain_amd.")
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    enc = asr.encode_batch(wav, lens)
    assert float((enc.cpu() - torch.from_numpy(exp["enc_out"])).abs().max()) <= 5e-5
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == hyps_of(exp["tokens"])
    assert words == [str(w) for w in exp["words"]]
    # transcribe_file (inference/ASR.py:96-117): 16-bit PCM mono and stereo (channel mean) wav files
    for name, ref_words in zip(exp["file_names"], exp["file_words"]):
        assert asr.transcribe_file(os.path.join(GOLD, str(name))) == str(ref_words)
    with pytest.raises(FileNotFoundError):
        EncoderDecoderASR.from_hparams(source="speechbrain/asr-conformer-transformerlm-librispeech")


def test_long_utterance_search_vs_oracle(backend):
    """A 44 s utterance (T' = 1100 encoder frames): CTC tables beyond the default 64 KiB LDS window,
    9 cross-attention splits -- beam search + CTC vs the oracle."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    g, mods = build("tiny_ctc", dev)
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    d_model, nhead, d_ffn, n_enc, n_dec, vocab = [int(v) for v in g["cfg"][:6]]
    cfg = O.ModelCfg(d_model=d_model, nhead=nhead, num_encoder_layers=n_enc, num_decoder_layers=n_dec, d_ffn=d_ffn,
                     vocab=vocab)
    enc = torch.randn(2, 1100, d_model, generator=torch.Generator().manual_seed(21))
    wl = torch.tensor([1.0, 0.93])
    ratio = 5.5 / 1100
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                           weights={"ctc": 0.4})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=ratio, beam_size=4,
                                    using_eos_threshold=False, length_normalization=True, scorer=scorer)
    hyps, _, scores, _ = bs(enc.to(dev), wl.to(dev))
    hyps_ref, _, sc_ref, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=4, ctc_weight=0.4, max_decode_ratio=ratio))
    assert hyps == hyps_ref
    assert float((scores.cpu() - sc_ref).abs().max()) <= 1e-4


def test_concurrent_transcriber_matches_sequential(backend):
    """Several batches in flight (one host thread + normal / high-priority HIP streams per batch on the GPU;
    sequential on the CPU emulator) give exactly the token ids of one-at-a-time transcribe_batch calls."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr
    from speechbrain_amd.inference.streams import ConcurrentTranscriber

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=2, n_dec=2, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=40, seed=3, beam_size=4, ctc_weight=0.4, device=str(dev), max_decode_ratio=0.5)
    with torch.no_grad():
        asr.mods.seq_lin.w.weight.mul_(6.0)
        asr.mods.ctc_lin.w.weight.mul_(6.0)
    gen = torch.Generator().manual_seed(5)
    batches = []
    for n, b in ((6400, 2), (9600, 3), (4800, 1), (8000, 2), (7200, 2)):
        wav = 0.1 * torch.randn(b, n, generator=gen)
        lens = torch.linspace(0.7, 1.0, b)
        for i in range(b):
            wav[i, int(lens[i] * n):] = 0
        batches.append((wav.to(dev), lens.to(dev)))
    ref = [asr.transcribe_batch(w, l)[1] for w, l in batches]
    ct = ConcurrentTranscriber(asr, streams=3)
    got = ct.transcribe_batches(batches)
    assert got == ref
    if dev.type == "cuda":  # close(): the workers' streams give their registered library workspaces back
        keys = [(id(nat.load()), s.device.index, s.cuda_stream) for s in ct.enc_streams + [d for d in ct.dec_streams if d is not None]]
        assert any(k in nat._STREAM_WS for k in keys)
        ct.close()
        assert not any(k in nat._STREAM_WS for k in keys)
        assert ConcurrentTranscriber(asr, streams=3).transcribe_batches(batches) == ref  # (fresh streams register again)
    else:
        ct.close()
    seen = []
    got2 = ConcurrentTranscriber(asr, streams=2, prioritise_search=False).transcribe_batches(
        batches, prepare=lambda searcher, wavs: seen.append(wavs.shape[1]))
    assert got2 == ref and sorted(seen) == sorted(w.shape[1] for w, _ in batches)


@pytest.mark.parametrize("tag", ["tiny_ctc", "tiny_noctc", "tiny_lm_ctc"])
@pytest.mark.parametrize("graph_mode", [1, 2])
def test_device_side_step_counter_and_graph_replay(backend, tag, graph_mode):
    """graph_mode 2: the step number lives in device memory (every step-dependent kernel reads it);
    graph_mode 1: two steps captured into a hipGraph and replayed (on the CPU emulator the capture is
    unavailable and the library falls back to mode 2).  Results must equal the reference goldens."""
    nat, dev = backend
    from speechbrain_amd.decoders import (CTCScorer, S2STransformerBeamSearcher, ScorerBuilder,
                                          TransformerLMScorer)
    from speechbrain_amd.inference.builders import build_modules

    g = np.load(os.path.join(GOLD, f"model_{tag}.npz"))
    d_model, nhead, d_ffn, n_enc, n_dec, vocab, beam, eos_thr = [int(v) for v in g["cfg"]]
    cf = [float(v) for v in g["cfgf"]]
    ctc_w, max_ratio, min_ratio = cf[0], cf[1], cf[2]
    m = build_modules(dict(d_model=d_model, nhead=nhead, d_ffn=d_ffn, n_enc=n_enc, n_dec=n_dec, n_fft=512,
                           win_length=32), vocab=vocab)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("CNN", "Transformer", "seq_lin", "ctc_lin")})
    mods.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files
                          if k.startswith("sd/") and not k.startswith("sd/LM.")}, strict=True)
    mods = mods.to(dev).eval()
    full, weights, temp = [], {}, 1.0
    if "lm_cfg" in g.files:
        full.append(TransformerLMScorer(language_model=build_lm(g, dev), temperature=cf[4]))
        weights["transformerlm"], temp = cf[3], cf[5]
    if ctc_w > 0:
        full.append(CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2))
        weights["ctc"] = ctc_w
    scorer = ScorerBuilder(full_scorers=full, weights=weights) if full else None
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=beam,
                                    using_eos_threshold=bool(eos_thr), length_normalization=True, temperature=temp,
                                    scorer=scorer)
    bs.overlap_ctc, bs.graph_mode = 0, graph_mode
    import contextlib
    # capture needs a real stream (the legacy default stream cannot be captured; the library then falls back)
    side = torch.cuda.stream(torch.cuda.Stream(dev)) if dev.type == "cuda" else contextlib.nullcontext()
    for check_every in (8, 1, 0):
        bs.check_every = check_every
        with side:
            hyps, lens, scores, _ = bs(torch.from_numpy(g["enc_out"]).to(dev), torch.from_numpy(g["wav_lens"]).to(dev))
        if dev.type == "cuda" and check_every == 8:  # and once on the default stream: silent fallback to plain launches
            hyps_d, _, _, _ = bs(torch.from_numpy(g["enc_out"]).to(dev), torch.from_numpy(g["wav_lens"]).to(dev))
            assert hyps_d == hyps
        assert hyps == hyps_of(g["beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g["beam_scores"])).abs().max()) <= 1e-4
        assert float((lens.cpu() - torch.from_numpy(g["beam_lens"])).abs().max()) <= 1e-6


def test_degenerate_inputs(backend):
    """Empty batch, a single very short utterance (T' = 3 encoder frames), batch of one, all-padding tails:
    the path returns the shapes the reference would and never faults."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr, flat_state_dict

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=2, n_dec=2, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=40, seed=3, beam_size=4, ctc_weight=0.4, device=str(dev))
    # empty batch through every kernel entry that takes a batch dimension
    assert nat.gemm_nt(torch.zeros(0, 32, device=dev), torch.zeros(8, 32, device=dev)).shape == (0, 8)
    assert nat.layernorm(torch.zeros(0, 32, device=dev), torch.ones(32, device=dev), torch.zeros(32, device=dev), 1e-5).shape == (0, 32)
    enc0 = torch.zeros(0, 7, 32, device=dev)
    hyps, lens, scores, lp = asr.mods.decoder(enc0, torch.zeros(0, device=dev))
    assert hyps == [] and lens.numel() == 0 and scores.numel() == 0
    # 0.07 s of audio -> 8 feature frames -> T' = 2; still decodes (max_decode_ratio 1.0 -> 2 steps)
    wav = 0.1 * torch.randn(1, 1120, generator=torch.Generator().manual_seed(2))
    words, toks = asr.transcribe_batch(wav, torch.ones(1))
    sd = flat_state_dict(asr)
    fc = O.FbankCfg(n_fft=512, n_mels=80, win_length_ms=32)
    mc = O.ModelCfg(d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=2, d_ffn=64, vocab=40)
    enc = O.encode_batch(wav, torch.ones(1), sd, fc, mc, torch.zeros(80), torch.ones(80))
    assert enc.shape[1] == 2
    hyps_ref, _, _, _ = O.beam_search(enc, torch.ones(1), sd, mc, O.SearchCfg(beam=4, ctc_weight=0.4))
    assert toks == hyps_ref
    # an utterance that is almost entirely padding inside a batch
    wav2 = 0.1 * torch.randn(2, 8000, generator=torch.Generator().manual_seed(3))
    lens2 = torch.tensor([1.0, 0.05])
    wav2[1, 400:] = 0
    words2, toks2 = asr.transcribe_batch(wav2, lens2)
    enc2 = O.encode_batch(wav2, lens2, sd, fc, mc, torch.zeros(80), torch.ones(80))
    hyps2, _, _, _ = O.beam_search(enc2, lens2, sd, mc, O.SearchCfg(beam=4, ctc_weight=0.4))
    assert toks2 == hyps2


def test_in_place_weight_update_rebuilds_the_decoder_handle(backend):
    """the searcher caches LayerNorm-folded copies of the projections; an in-place update of the
    source parameters (load_state_dict keeps data_ptr, bumps _version) must invalidate them."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    tiny = dict(d_model=128, nhead=4, d_ffn=128, n_enc=1, n_dec=2, n_fft=512, win_length=32)

    def make(seed):
        asr = build_asr(tiny, vocab=40, seed=seed, beam_size=3, ctc_weight=0.3, device=str(dev))
        with torch.no_grad():  # peaked heads: the comparison below is on token ids
            asr.mods.seq_lin.w.weight.mul_(8.0)
            asr.mods.ctc_lin.w.weight.mul_(8.0)
        return asr

    wav = 0.1 * torch.randn(2, 6400, generator=torch.Generator().manual_seed(3))
    lens = torch.tensor([1.0, 0.8])
    a, b = make(5), make(6)
    _, toks_a = a.transcribe_batch(wav, lens)
    _, toks_b = b.transcribe_batch(wav, lens)
    assert toks_a != toks_b
    h0 = a.mods.decoder._handle()
    assert a.mods.decoder._handle() is h0  # unchanged weights: the cached table is reused
    for name in ("transformer", "seq_lin", "ctc_lin"):
        a.mods[name].load_state_dict(b.mods[name].state_dict())
    a.mods.encoder["model"].load_state_dict(b.mods.encoder["model"].state_dict())
    _, toks_a2 = a.transcribe_batch(wav, lens)
    assert a.mods.decoder._handle() is not h0
    assert toks_a2 == toks_b


@pytest.mark.parametrize("ctc_weight", [0.4, 0.0])
def test_grouped_search_equals_separate_searches(backend, ctc_weight):
    """forward_group: several batches (own padded length, own step limits, EOS reachable) in ONE device search give
    every batch exactly what its own search gives -- the basis for running recipe-sized batches with full GEMMs."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=1, n_dec=2, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=30, seed=21, beam_size=4, ctc_weight=ctc_weight, device=str(dev), using_eos_threshold=True)
    with torch.no_grad():
        asr.mods.seq_lin.w.weight.mul_(7.0)
        asr.mods.ctc_lin.w.weight.mul_(7.0)
        asr.mods.seq_lin.w.bias[2] += 6.0  # EOS (index 2) within reach: some hypotheses end before the step limit
    g = torch.Generator().manual_seed(17)
    shapes = [(3, 9600, (0.0, 0.5)), (2, 5120, (0.2, 1.0)), (1, 12800, (0.0, 0.3)), (2, 7040, (0.0, 0.9))]
    items, ratios = [], []
    dec = asr.mods.decoder
    for B, N, r in shapes:
        wav = 0.1 * torch.randn(B, N, generator=g)
        lens = torch.linspace(0.7, 1.0, B)
        items.append((asr.encode_batch(wav, lens), lens.to(dev)))
        ratios.append(r)
    separate = []
    for (enc, wl), (r_min, r_max) in zip(items, ratios):
        dec.min_decode_ratio, dec.max_decode_ratio = r_min, r_max
        separate.append(dec(enc, wl))
    grouped = dec.forward_group(items, ratios)
    assert len(grouped) == len(separate)
    for (h_g, l_g, s_g, p_g), (h_s, l_s, s_s, p_s) in zip(grouped, separate):
        assert h_g == h_s
        assert float((l_g.cpu() - l_s.cpu()).abs().max()) <= 1e-6
        assert float((s_g.cpu() - s_s.cpu()).abs().max()) <= 2e-5
        assert p_g.shape == p_s.shape and float((p_g.cpu() - p_s.cpu()).abs().max()) <= 2e-5
    early = [len(h) < int(items[i][0].shape[1] * ratios[i][1]) - 1 for i, res in enumerate(separate) for h in res[0]]
    assert any(early), "the case should contain hypotheses that end through EOS before the step limit"
    # return_topk (seq2seq.py:757-760, :1712-1713): every batch's padded [B, topk, max_len] tensors, grouped == separate
    keep_topk = (dec.return_topk, dec.topk)
    dec.return_topk, dec.topk = True, 3
    try:
        sep3 = []
        for (enc, wl), (r_min, r_max) in zip(items, ratios):
            dec.min_decode_ratio, dec.max_decode_ratio = r_min, r_max
            sep3.append(dec(enc, wl))
        for (h_g, l_g, s_g, p_g), (h_s, l_s, s_s, p_s) in zip(dec.forward_group(items, ratios), sep3):
            assert h_g.shape == h_s.shape and torch.equal(h_g.cpu(), h_s.cpu())
            assert float((l_g.cpu() - l_s.cpu()).abs().max()) <= 1e-6 and float((s_g.cpu() - s_s.cpu()).abs().max()) <= 2e-5
            assert p_g.shape == p_s.shape and float((p_g.cpu() - p_s.cpu()).abs().max()) <= 2e-5
    finally:
        dec.return_topk, dec.topk = keep_topk
    # the same grouped search with the step number in device memory (2) and replayed from a captured hipGraph (1: on
    # the GPU, from a real stream; the emulator falls back to 2): per-utterance limits are compared against *step_ptr
    import contextlib

    saved = (dec.overlap_ctc, dec.graph_mode)
    side = torch.cuda.stream(torch.cuda.Stream(dev)) if dev.type == "cuda" else contextlib.nullcontext()
    try:
        for mode in (2, 1):
            dec.overlap_ctc, dec.graph_mode = 0, mode
            with side:
                replay = dec.forward_group(items, ratios)
            for (h_r, l_r, s_r, p_r), (h_g, l_g, s_g, p_g) in zip(replay, grouped):
                assert h_r == h_g
                assert float((s_r.cpu() - s_g.cpu()).abs().max()) <= 2e-5
    finally:
        dec.overlap_ctc, dec.graph_mode = saved


def test_grouped_search_with_a_ctc_attention_window_runs_batch_by_batch(backend):
    """forward_group with CTCScorer(ctc_window_size > 0) (scorer.py:183-187, ctc.py:189-200): the window's frame range is taken over
    the whole batch of a search, so the batches of a group keep their own searches (what the reference, which has no grouped search,
    does) -- every batch gets exactly what forward gives it under its own decode ratios, and the searcher's own ratios are restored."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=1, n_dec=2, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=30, seed=23, beam_size=4, ctc_weight=0.4, device=str(dev), using_eos_threshold=True)
    dec = asr.mods.decoder
    dec.ctc_window_size = 6
    g = torch.Generator().manual_seed(5)
    items, ratios = [], [(0.0, 0.5), (0.1, 0.8), (0.0, 0.3)]
    for B, N in [(2, 9600), (3, 6400), (1, 12800)]:
        wav = 0.1 * torch.randn(B, N, generator=g)
        lens = torch.linspace(0.8, 1.0, B)
        items.append((asr.encode_batch(wav, lens), lens.to(dev)))
    keep = (dec.min_decode_ratio, dec.max_decode_ratio)
    separate = []
    for (enc, wl), r in zip(items, ratios):
        dec.min_decode_ratio, dec.max_decode_ratio = r
        separate.append(dec(enc, wl))
    dec.min_decode_ratio, dec.max_decode_ratio = keep
    grouped = dec.forward_group(items, ratios)
    assert (dec.min_decode_ratio, dec.max_decode_ratio) == keep
    assert len(grouped) == len(separate)
    for (h_g, l_g, s_g, p_g), (h_s, l_s, s_s, p_s) in zip(grouped, separate):
        assert h_g == h_s and torch.equal(s_g.cpu(), s_s.cpu()) and torch.equal(p_g.cpu(), p_s.cpu())


@pytest.mark.parametrize("attention", ["RelPosMHAXL", "RoPEMHA"])
def test_grouped_encoder_equals_batch_by_batch(backend, attention):
    """encode_group: the Conformer encoder over the rows of several independently padded batches laid end to end (one
    launch per projection / feed-forward / LayerNorm for all of them; attention and depthwise convolution per batch)
    gives every batch what encode_batch gives it.  Tolerance 2e-5: a GEMM over more rows may take another tile
    schedule (same products, another summation order)."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=2, n_dec=1, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=30, seed=23, beam_size=2, ctc_weight=0.3, device=str(dev), attention_type=attention)
    g = torch.Generator().manual_seed(3)
    batches = []
    for B, N in [(3, 9600), (2, 5120), (1, 12800), (2, 7040)]:
        batches.append((0.1 * torch.randn(B, N, generator=g), torch.linspace(0.6, 1.0, B) if B > 1 else torch.ones(1)))
    with torch.no_grad():
        one_by_one = [asr.encode_batch(w, l) for w, l in batches]
        together = asr.encode_group(batches)
    assert len(together) == len(one_by_one)
    for a, b in zip(together, one_by_one):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 2e-5
    # and through the workers: grouped encoder + grouped search against plain sequential calls
    from speechbrain_amd.inference.streams import ConcurrentTranscriber

    seq = [asr.transcribe_batch(w, l)[1] for w, l in batches]
    workers = ConcurrentTranscriber(asr, streams=1, group=4)
    workers.group_encoder = True
    got = workers.transcribe_batches(batches)
    workers.pool.shutdown(wait=True)
    assert got == seq


@pytest.mark.parametrize("attention", ["RelPosMHAXL", "RoPEMHA"])
def test_panel_route_serves_both_attention_types_and_the_grouped_encoder(backend, attention):
    """with the both-operands-pre-split route on (the default fp32 path from 2 048 rows on; here the
    thresholds are lowered so that the tiny model takes it) a LayerNorm hands its consumer a native.Panel, not a tensor.
    RoPEMHA.core / core_group and RelPosMHAXL.core_group must accept it: encode_batch and encode_group on the panel route
    against the same model on the fp32-tensor route (2e-5: same products, another summation order)."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    tiny = dict(d_model=32, nhead=4, d_ffn=64, n_enc=2, n_dec=1, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=30, seed=23, beam_size=2, ctc_weight=0.3, device=str(dev), attention_type=attention)
    g = torch.Generator().manual_seed(3)
    batches = [(0.1 * torch.randn(B, N, generator=g), torch.linspace(0.6, 1.0, B) if B > 1 else torch.ones(1))
               for B, N in [(3, 9600), (2, 5120), (1, 12800)]]
    with torch.no_grad():
        plain = [asr.encode_batch(w, l) for w, l in batches]
    old = nat.F32X3, nat.X3P, nat.F32X3_MIN_ROWS, nat.X3P_MIN_TILES
    calls = {"ln": 0}
    ln0 = nat.layernorm_x3p

    def ln(*a, **k):
        calls["ln"] += 1
        return ln0(*a, **k)

    nat.F32X3, nat.X3P, nat.F32X3_MIN_ROWS, nat.X3P_MIN_TILES = True, True, 1, 1
    nat.layernorm_x3p = ln
    try:
        with torch.no_grad():
            one_by_one = [asr.encode_batch(w, l) for w, l in batches]
            n_single = calls["ln"]
            together = asr.encode_group(batches)
    finally:
        nat.F32X3, nat.X3P, nat.F32X3_MIN_ROWS, nat.X3P_MIN_TILES = old
        nat.layernorm_x3p = ln0
    assert n_single > 0 and calls["ln"] > n_single  # (both entry points handed panels to their attention layers)
    for a, b, c in zip(one_by_one, together, plain):
        assert a.shape == c.shape and b.shape == c.shape
        assert float((a - c).abs().max()) <= 2e-5 and float((b - c).abs().max()) <= 2e-5


def test_bf16_precision_is_opt_in_and_close(backend):
    """run_opts precision="bf16": the encoder's large GEMMs take bf16 operands (fp32 accumulation); the default stays
    the fp32 parity path bit for bit.  Stated tolerance for this tiny model: encoder output within 5e-2 absolute of
    the fp32 path (LayerNorm-ed activations of unit scale, 8-bit mantissas through 2 layers)."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    tiny = dict(d_model=64, nhead=4, d_ffn=128, n_enc=2, n_dec=1, n_fft=512, win_length=32)
    a32 = build_asr(tiny, vocab=30, seed=2, beam_size=2, ctc_weight=0.3, device=str(dev))
    a16 = build_asr(tiny, vocab=30, seed=2, beam_size=2, ctc_weight=0.3, device=str(dev))
    a16.eval_precision = "bf16"
    wav = 0.1 * torch.randn(3, 48000, generator=torch.Generator().manual_seed(8))  # 3 x 76 frames = 228 >= 256? no:
    wav = torch.cat([wav, wav], dim=0)                                              # 6 x 76 = 456 rows -> bf16 kernel
    lens = torch.ones(6)
    monkey_rows = nat.BF16A_MIN_ROWS
    nat.BF16A_MIN_ROWS = 256  # (the tiny batch takes the bf16-activation feed-forward path too)
    try:
        e32, e32b, e16 = a32.encode_batch(wav, lens), a32.encode_batch(wav, lens), a16.encode_batch(wav, lens)
    finally:
        nat.BF16A_MIN_ROWS = monkey_rows
    assert torch.equal(e32, e32b)
    d = float((e32 - e16).abs().max())
    assert 0.0 < d <= 5e-2, d
    assert nat.precision() == "fp32"  # the scope does not leak
    # the feed-forward pairs keep their operands in bf16 in memory (LayerNorm / the first contraction write bf16, read by
    # LDS-DMA); with that switched off every contraction reads fp32 activations and rounds them on load -- same roundings
    nat.BF16_ACTIVATIONS = False
    try:
        e16f = a16.encode_batch(wav, lens)
    finally:
        nat.BF16_ACTIVATIONS = True
    assert float((e32 - e16f).abs().max()) <= 5e-2 and float((e16 - e16f).abs().max()) <= 2e-2
    with pytest.raises(NotImplementedError):
        build_asr(tiny, vocab=30, seed=2, device=str(dev)).__class__(modules=dict(a32.mods), hparams={"tokenizer": None},
                                                                     run_opts={"device": str(dev), "precision": "int4"})
    # (fp16 / fp8 are accepted since round 5: inference/interfaces.py, tests/test_whisper.py)


def test_search_projections_on_the_split_operand_kernel(backend):
    """The search's big contractions -- cross-attention key / value rows of the encoder memory, the CTC head over the
    B*T frames, the vocabulary projection of a step -- take sbk_gemm_nt_f32x3 (fp32 on the bf16 matrix pipe) from
    1 024 rows / 192 tiles on.  Knobs 34 / 35 lower those thresholds so that a small model reaches them: token ids equal
    the fp32-MFMA run's and the oracle's, scores within the fp32 tolerance; the handle carries the split images only
    for shapes the kernel takes."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr, flat_state_dict

    tiny = dict(d_model=64, nhead=4, d_ffn=128, n_enc=1, n_dec=2, n_fft=512, win_length=32)
    asr = build_asr(tiny, vocab=52, seed=9, beam_size=4, ctc_weight=0.4, device=str(dev))
    with torch.no_grad():
        asr.mods.seq_lin.w.weight.mul_(7.0)
        asr.mods.ctc_lin.w.weight.mul_(7.0)
    wav = 0.1 * torch.randn(3, 9600, generator=torch.Generator().manual_seed(4))
    lens = torch.tensor([1.0, 0.7, 0.9])
    h = asr.mods.decoder._handle()
    assert h.W.seq_w3 and all(h.layers[l].ca_kv_w3 for l in range(2))
    dec = asr.mods.decoder
    enc = asr.encode_batch(wav, lens)
    ref = dec(enc, lens.to(dev))  # thresholds at their defaults: the fp32-MFMA kernels
    with nat.knobs(x3_route_rows=1, x3_route_tiles=1):
        got = dec(enc, lens.to(dev))
    assert got[0] == ref[0]
    assert float((got[1].cpu() - ref[1].cpu()).abs().max()) <= 1e-4
    sd = flat_state_dict(asr)
    mc = O.ModelCfg(d_model=64, nhead=4, num_encoder_layers=1, num_decoder_layers=2, d_ffn=128, vocab=52)
    hyps, _, _, _ = O.beam_search(enc.cpu(), lens, sd, mc, O.SearchCfg(beam=4, ctc_weight=0.4))
    assert got[0] == hyps
    odd = build_asr(tiny, vocab=50, seed=9, beam_size=4, ctc_weight=0.4, device=str(dev))  # 50 % 4 != 0: rows are not whole vectors
    assert not odd.mods.decoder._handle().W.seq_w3


@pytest.mark.parametrize("tag", ["tiny_ctc", "tiny_noctc", "tiny_lm_ctc"])
def test_fused_scoring_equals_separate_kernels(backend, tag):
    """The step's scoring as ONE pass per hypothesis row (csrc/search.hip:score_topk_row_kernel: log-softmax, eos rules,
    scorer combination, candidate values and the row's top-`beam` from registers; the default) against the launches it
    replaces (log_softmax_row / row_max / ctc_combine or am_only / beam_topk_stage1; score_fused = 0): every expression and
    reduction order is the same, so hypotheses, scores and per-token log-probs must be IDENTICAL, bit for bit -- with
    the CTC scorer, with the eos threshold and without a scorer, with the LM scorer in front of CTC, for top-k lists
    and in a grouped search with per-utterance step limits."""
    nat, dev = backend
    from speechbrain_amd.decoders import (CTCScorer, S2STransformerBeamSearcher, ScorerBuilder, TransformerLMScorer)

    g, mods = build(tag if tag != "tiny_lm_ctc" else "tiny_ctc", dev)
    beam, eos_thr = int(g["cfg"][6]), bool(g["cfg"][7])
    ctc_w, max_ratio, min_ratio = [float(v) for v in g["cfgf"]]
    wl = torch.from_numpy(g["wav_lens"]).to(dev)
    enc = torch.from_numpy(g["enc_out"]).to(dev)
    full, weights = [], {}
    if tag == "tiny_lm_ctc":
        from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM

        torch.manual_seed(3)
        lm = TransformerLM(vocab=int(g["cfg"][5]), d_model=32, nhead=2, num_encoder_layers=2, num_decoder_layers=0,
                           d_ffn=64, dropout=0.0, activation=torch.nn.GELU, normalize_before=False).to(dev).eval()
        full.append(TransformerLMScorer(language_model=lm, temperature=1.3))
        weights["transformerlm"] = 0.5
    if ctc_w > 0:
        full.append(CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2))
        weights["ctc"] = ctc_w
    scorer = ScorerBuilder(full_scorers=full, weights=weights) if full else None

    def run(**kw):
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=min_ratio, max_decode_ratio=max_ratio, beam_size=beam,
                                        using_eos_threshold=eos_thr, length_normalization=True, scorer=scorer, **kw)
        with torch.no_grad():
            return bs(enc, wl)

    out = {}
    for fused in (1, 0):
        with nat.knobs(score_fused=fused):
            out[fused] = (run(), run(return_topk=True, topk=min(3, beam)), run(temperature=1.7))
    for run_no, (a, b) in enumerate(zip(out[1], out[0])):
        for out_no, (x, y) in enumerate(zip(a, b)):
            if torch.is_tensor(x):
                assert torch.equal(x.cpu(), y.cpu()), (run_no, out_no, x.cpu(), y.cpu())
            else:
                assert x == y, (run_no, out_no, x, y)
    if tag == "tiny_ctc":  # (the default path against the reference's own result)
        assert out[1][0][0] == hyps_of(g["beam_hyps"])


@pytest.mark.parametrize("vocab", [1300, 5300])
def test_fused_scoring_large_vocabulary(backend, vocab):
    """The register-list widths the recipe sizes need (20 entries per thread up to V = 5 120, 32 up to 8 192; the golden
    models' vocabularies fit 4): beam 10 + CTC + eos threshold on a random model, fused pass against separate kernels,
    bit for bit; at V = 1 300 also against the oracle's search."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder
    from speechbrain_amd.inference.builders import build_modules

    torch.manual_seed(11)
    m = build_modules(dict(d_model=32, nhead=2, d_ffn=64, n_enc=1, n_dec=2, n_fft=512, win_length=32), vocab=vocab)
    mods = torch.nn.ModuleDict({k: m[k] for k in ("Transformer", "seq_lin", "ctc_lin")}).eval()
    sd = {f"{p}.{k}": v.detach().clone() for p in mods for k, v in mods[p].state_dict().items()}  # (CPU copy for the oracle)
    mods = mods.to(dev)
    enc_h, wl_h = torch.randn(3, 24, 32, generator=torch.Generator().manual_seed(2)) * 1.5, torch.tensor([1.0, 0.7, 0.9])
    enc, wl = enc_h.to(dev), wl_h.to(dev)
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=0.3, beam_size=10, using_eos_threshold=True,
                                    length_normalization=True, scorer=scorer, return_topk=True, topk=4)
    out = {}
    for fused in (1, 0):
        with nat.knobs(score_fused=fused), torch.no_grad():
            out[fused] = bs(enc, wl)
    for x, y in zip(out[1], out[0]):
        assert torch.equal(x.cpu(), y.cpu()) if torch.is_tensor(x) else x == y
    assert int(out[1][0].max()) > 2  # (something was decoded)
    if vocab == 1300:
        # both paths call the same block_topk, so a mistake they share passes the comparison above: the V = 1 300 lists must
        # also be the oracle's.  Fairness of the seed, on the CPU: the oracle in fp64 and in fp32 returns the same lists, and
        # neighbouring fp64 scores lie further apart than the 1e-4 allowed below -- no rank hangs on fp32 rounding.
        cfg = O.ModelCfg(d_model=32, nhead=2, num_encoder_layers=1, num_decoder_layers=2, d_ffn=64, vocab=vocab)
        sc = O.SearchCfg(beam=10, ctc_weight=0.4, using_eos_threshold=True, max_decode_ratio=0.3, return_topk=True, topk=4)
        hyps_ref, lens_ref, sc_ref, _ = O.beam_search(enc_h, wl_h, sd, cfg, sc)
        keep = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)  # (the oracle builds its constants in the default dtype)
        try:
            hyps64, _, sc64, _ = O.beam_search(enc_h.double(), wl_h.double(), {k: v.double() for k, v in sd.items()}, cfg, sc)
        finally:
            torch.set_default_dtype(keep)
        assert torch.equal(hyps_ref, hyps64) and float((sc64[:, :-1] - sc64[:, 1:]).min()) > 1e-4
        hyps, lens, scores, _ = out[1]
        assert hyps.shape == hyps_ref.shape and torch.equal(hyps.cpu(), hyps_ref)
        assert float((scores.cpu() - sc_ref).abs().max()) <= 1e-4
        assert float((lens.cpu() - lens_ref).abs().max()) <= 1e-6


@pytest.mark.parametrize("tag", ["tiny_ctc", "tiny_noctc"])
def test_golden_encoder_on_the_panel_route(backend, tag):
    """The encoder with every eligible contraction on the both-operands-pre-split route (csrc/gemm_x3p.hip; the routing
    thresholds lowered so that the golden models' small shapes take it): LayerNorms write their result directly as the
    next contraction's panel operand (sbk_layernorm_x3p), the feed-forward pair hands its hidden layer over as a panel
    image (no fp32 round trip), the remaining operands are split by sbk_split_x3p -- against the REFERENCE's encoder
    output, 5e-5 as on the default route."""
    nat, dev = backend
    g, mods = build(tag, dev)
    feats, wl = torch.from_numpy(g["feats"]).to(dev), torch.from_numpy(g["wav_lens"]).to(dev)
    old = nat.F32X3, nat.X3P, nat.F32X3_MIN_ROWS, nat.X3P_MIN_TILES
    calls = {"ln": 0, "gemm": 0, "chained": 0}
    ln0, gemm0 = nat.layernorm_x3p, nat.gemm_nt_x3p

    def ln(*a, **k):
        calls["ln"] += 1
        return ln0(*a, **k)

    def gemm(*a, **k):
        calls["gemm"] += 1
        calls["chained"] += bool(k.get("panel_out"))
        return gemm0(*a, **k)

    nat.F32X3, nat.X3P, nat.F32X3_MIN_ROWS, nat.X3P_MIN_TILES = True, True, 1, 1
    nat.layernorm_x3p, nat.gemm_nt_x3p = ln, gemm
    try:
        with torch.no_grad():
            enc = mods["Transformer"].encode(mods["CNN"](feats), wl)
    finally:
        nat.F32X3, nat.X3P, nat.F32X3_MIN_ROWS, nat.X3P_MIN_TILES = old
        nat.layernorm_x3p, nat.gemm_nt_x3p = ln0, gemm0
    assert float((enc.cpu() - torch.from_numpy(g["enc_out"])).abs().max()) <= 5e-5
    n_layers = len(mods["Transformer"].encoder.layers)
    assert calls["ln"] == 5 * n_layers and calls["chained"] == 2 * n_layers and calls["gemm"] >= 7 * n_layers
