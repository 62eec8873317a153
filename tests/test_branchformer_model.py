"""TransformerASR(encoder_module="branchformer") through the drop-in module surface against the REFERENCE's outputs stored in
tests/golden/model_branchformer.npz and tests/golden/pretrained_branchformer_tiny/ (tools/make_branchformer_golden.py).  Runs on
the CPU emulator of the kernels (not gpu) and on the MI355X (-m gpu).  Bounds are those test_model_parity.py applies to the tiny
Conformer goldens: encoder 5e-5, decoder scores 1e-4, token ids exact."""
import os

import numpy as np
import pytest
import torch

import branchformer_host_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_G = {}


def gold():
    if "g" not in _G:
        _G["g"] = np.load(os.path.join(GOLD, "model_branchformer.npz"))
    return _G["g"]


def state_dict(tag):
    g = gold()
    return {k[len(tag) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/sd/")}


def hyps_of(arr):
    return [[int(v) for v in row if v >= 0] for row in arr]


def build(tag, dev):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain_amd.nnet.linear import Linear

    g = gold()
    d, H, n_enc, n_dec, csgu, ksize, vocab, _ = [int(v) for v in g[f"{tag}/cfg"]]
    mods = {"Transformer": TransformerASR(
        input_size=g[f"{tag}/feats"].shape[-1], tgt_vocab=vocab, d_model=d, nhead=H, num_encoder_layers=n_enc,
        num_decoder_layers=n_dec, d_ffn=64, dropout=0.1, activation=torch.nn.GELU, branchformer_activation=torch.nn.GELU,
        encoder_module="branchformer", csgu_linear_units=csgu, kernel_size=ksize, attention_type="RelPosMHAXL",
        normalize_before=True, causal=False)}
    if n_dec:
        mods["seq_lin"], mods["ctc_lin"] = Linear(input_size=d, n_neurons=vocab), Linear(input_size=d, n_neurons=vocab)
    mods = torch.nn.ModuleDict(mods)
    return g, mods, dev


@pytest.mark.parametrize("tag", ["k7", "k31"])
def test_host_restatement_against_the_reference(tag):
    """tests/branchformer_host_ref.py (what the full-size GPU test compares against) reproduces the reference's encoder, layer
    by layer, at 1e-5 in fp32 -- and its fp64 form stays within the same distance of the fp32 reference outputs."""
    g = gold()
    sd = state_dict(tag)
    d, H, n_enc = [int(v) for v in g[f"{tag}/cfg"][:3]]
    feats, wl = torch.from_numpy(g[f"{tag}/feats"]), torch.from_numpy(g[f"{tag}/wav_lens"])
    enc, layers = R.encode(feats, wl, sd, d, H, n_enc, "Transformer.", return_layers=True)
    assert float((enc - torch.from_numpy(g[f"{tag}/enc_out"])).abs().max()) <= 1e-5
    for l, a in enumerate(layers):
        assert float((a - torch.from_numpy(g[f"{tag}/enc_layer{l}"])).abs().max()) <= 1e-5
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    enc64 = R.encode(feats.double(), wl, sd64, d, H, n_enc, "Transformer.")
    assert enc64.dtype == torch.float64
    assert float((enc64 - torch.from_numpy(g[f"{tag}/enc_out"]).double()).abs().max()) <= 1e-5


@pytest.mark.parametrize("tag", ["k7", "k31"])
def test_state_dict_keys_equal_the_reference(tag):
    g, mods, _ = build(tag, None)
    assert set(mods.state_dict().keys()) == set(state_dict(tag).keys())
    ours, theirs = mods.state_dict(), state_dict(tag)
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in theirs.items()}
    for l in range(int(g[f"{tag}/cfg"][2])):
        assert f"Transformer.encoder.layers.{l}.convolution_branch.csgu.conv.conv.weight" in ours
        assert f"Transformer.encoder.layers.{l}.convolution_branch.csgu.norm.norm.bias" in ours
        assert f"Transformer.encoder.layers.{l}.merge_proj.weight" in ours


@pytest.mark.parametrize("tag", ["k7", "k31"])
def test_golden_branchformer_encoder(backend, tag):
    """enc_out and every layer's output (output_hidden_states) at 5e-5.  k7: the shortest utterance is 6 frames short of the
    batch (halo 3), so padded frames reach real ones through the unmasked cgMLP branch; k31: T' = 16 = halo + 1."""
    nat, dev = backend
    g, mods, _ = build(tag, dev)
    mods.load_state_dict(state_dict(tag), strict=True)
    mods = mods.to(dev).eval()
    tr = mods["Transformer"]
    feats, wl = torch.from_numpy(g[f"{tag}/feats"]).to(dev), torch.from_numpy(g[f"{tag}/wav_lens"]).to(dev)
    with torch.no_grad():
        enc = tr.encode(feats, wl)
        assert float((enc.cpu() - torch.from_numpy(g[f"{tag}/enc_out"])).abs().max()) <= 5e-5
        tr.output_hidden_states = tr.encoder.output_hidden_states = True
        enc2, hidden = tr.encode(feats, wl)
        tr.output_hidden_states = tr.encoder.output_hidden_states = False
        assert torch.equal(enc2, enc)
        assert len(hidden) == len(tr.encoder.layers) + 1  # (the encoder's input first, as the reference)
        for l, h in enumerate(hidden[1:]):
            assert float((h.cpu() - torch.from_numpy(g[f"{tag}/enc_layer{l}"])).abs().max()) <= 5e-5
        out, attn = tr.encoder(tr.custom_src_module(feats), pos_embs=tr.positional_encoding(feats))[:2]
        assert len(attn) == len(tr.encoder.layers)


def test_golden_branchformer_decoding(backend):
    """The existing decoder and searchers behind a Branchformer encoder: greedy and beam 4 + CTC 0.4 from the reference's
    enc_out -- token ids exact, scores 1e-4."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, S2STransformerGreedySearcher, ScorerBuilder

    g, mods, _ = build("k7", dev)
    mods.load_state_dict(state_dict("k7"), strict=True)
    mods = mods.to(dev).eval()
    enc_ref, wl = torch.from_numpy(g["k7/enc_out"]).to(dev), torch.from_numpy(g["k7/wav_lens"]).to(dev)
    with torch.no_grad():
        gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                          min_decode_ratio=0.0, max_decode_ratio=1.0)
        hyps, _, scores, _ = gs(enc_ref, wl)
        assert hyps == hyps_of(g["k7/greedy_hyps"])
        assert float((scores[:, 0].cpu() - torch.from_numpy(g["k7/greedy_scores"])[:, : scores.shape[2]]).abs().max()) <= 1e-4
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=int(g["k7/cfg"][7]),
                                        using_eos_threshold=False, length_normalization=True, scorer=scorer)
        hyps, lens, scores, _ = bs(enc_ref, wl)
        assert hyps == hyps_of(g["k7/beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g["k7/beam_scores"])).abs().max()) <= 1e-4
        assert float((lens.cpu() - torch.from_numpy(g["k7/beam_lens"])).abs().max()) <= 1e-6


def test_from_hparams_branchformer_model_directory(backend):
    """EncoderDecoderASR.from_hparams on a directory whose YAML says ``encoder_module: branchformer`` (branchformer_large.yaml's
    structure at tiny sizes, checkpoints written by the reference's savers): enc_out 5e-5, tokens and words equal to what the
    reference's EncoderDecoderASR produced from the same files."""
    nat, dev = backend
    from speechbrain_amd.inference.ASR import EncoderDecoderASR
    from speechbrain_amd.lobes.models.transformer.Branchformer import BranchformerEncoder

    exp = np.load(os.path.join(GOLD, "pretrained_branchformer_tiny_expected.npz"))
    asr = EncoderDecoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_branchformer_tiny"), run_opts={"device": str(dev)})
    assert isinstance(asr.mods.transformer.encoder, BranchformerEncoder)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    enc = asr.encode_batch(wav, lens)
    assert float((enc.cpu() - torch.from_numpy(exp["enc_out"])).abs().max()) <= 5e-5
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == hyps_of(exp["tokens"])
    assert words == [str(w) for w in exp["words"]]


def test_encode_group_equals_batch_by_batch(backend):
    """encode_group of two differently padded batches (the row-wise launches once over all rows, attention and CSGU per batch
    segment) equals encode batch by batch at 2e-5 -- and really takes the grouped path."""
    nat, dev = backend
    g, mods, _ = build("k7", dev)
    mods.load_state_dict(state_dict("k7"), strict=True)
    tr = mods["Transformer"].to(dev).eval()
    gen = torch.Generator().manual_seed(3)
    F_ = g["k7/feats"].shape[-1]
    srcs = [torch.randn(2, 21, F_, generator=gen).to(dev), torch.randn(3, 9, F_, generator=gen).to(dev)]
    wls = [torch.tensor([1.0, 0.6]).to(dev), torch.tensor([0.5, 1.0, 0.8]).to(dev)]
    calls = []
    orig = tr.encoder.forward_group
    tr.encoder.forward_group = lambda *a, **k: calls.append(1) or orig(*a, **k)
    with torch.no_grad():
        grouped = tr.encode_group(srcs, wls)
        single = [tr.encode(s, w) for s, w in zip(srcs, wls)]
    assert calls == [1]
    for a, b in zip(grouped, single):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 2e-5


def test_import_shim_resolves_the_yaml_class_path():
    """The YAML's ``speechbrain.lobes.models.transformer.TransformerASR.TransformerASR`` with ``encoder_module: branchformer``
    builds the Branchformer of this package; ``speechbrain.lobes.models.transformer.Branchformer`` resolves too."""
    import importlib

    import speechbrain_amd.compat

    speechbrain_amd.compat.install()
    mod = importlib.import_module("speechbrain.lobes.models.transformer.TransformerASR")
    tr = mod.TransformerASR(tgt_vocab=20, input_size=24, d_model=32, nhead=4, num_encoder_layers=1, num_decoder_layers=1,
                            d_ffn=64, encoder_module="branchformer", csgu_linear_units=48, kernel_size=7,
                            attention_type="RelPosMHAXL", normalize_before=True, causal=False)
    bf = importlib.import_module("speechbrain.lobes.models.transformer.Branchformer")
    assert isinstance(tr.encoder, bf.BranchformerEncoder)
    assert bf.BranchformerEncoder.__module__ == "speechbrain_amd.lobes.models.transformer.Branchformer"
    conv = importlib.import_module("speechbrain.lobes.models.convolution")
    assert isinstance(tr.encoder.layers[0].convolution_branch.csgu, conv.ConvolutionalSpatialGatingUnit)


def _tiny(**kw):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR

    args = dict(tgt_vocab=20, input_size=24, d_model=32, nhead=4, num_encoder_layers=1, num_decoder_layers=1, d_ffn=64,
                encoder_module="branchformer", csgu_linear_units=48, kernel_size=7, attention_type="RelPosMHAXL",
                normalize_before=True, causal=False)
    args.update(kw)
    return TransformerASR(**args)


def test_refusals_by_name():
    """What is out of scope raises NotImplementedError and says what it is."""
    with pytest.raises(NotImplementedError, match="hypermixing"):
        _tiny(attention_type="hypermixing")
    with pytest.raises(NotImplementedError, match="regularMHA"):
        _tiny(attention_type="regularMHA")
    with pytest.raises(NotImplementedError, match="use_linear_after_conv"):
        _tiny(use_linear_after_conv=True)
    with pytest.raises(NotImplementedError, match="gate_activation"):
        _tiny(gate_activation=torch.nn.Sigmoid)
    with pytest.raises(NotImplementedError, match="kernel_size 9"):
        _tiny(kernel_size=9)
    tr = _tiny()
    with pytest.raises(NotImplementedError, match="streaming"):
        tr.make_streaming_context(object())
    with pytest.raises(NotImplementedError, match="streaming"):
        tr.encode_streaming(torch.zeros(1, 4, 24), None)

    from speechbrain_amd.utils.dynamic_chunk_training import DynChunkTrainConfig

    with pytest.raises(NotImplementedError, match="Dynamic Chunk"):
        tr.encoder(torch.zeros(1, 8, 32), pos_embs=torch.zeros(1, 15, 32), dynchunktrain_config=DynChunkTrainConfig(4, 1))
    with pytest.raises(ValueError, match="positional embeddings"):
        tr.encoder(torch.zeros(1, 8, 32))
    with pytest.raises(ValueError, match=r"T=3 .*\b3\b.*kernel_size=7"):  # (checked before anything is launched)
        tr.encoder.layers[0].convolution_branch.csgu(torch.zeros(1, 3, 48))
