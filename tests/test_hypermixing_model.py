"""TransformerASR(encoder_module="conformer", attention_type="hypermixing") through the drop-in module surface against the
REFERENCE's outputs stored in tests/golden/model_hyperconformer.npz and tests/golden/pretrained_hyperconformer_tiny/
(tools/make_hypermixing_golden.py).  Runs on the CPU emulator of the kernels (not gpu) and on the MI355X (-m gpu).  Bounds are
those of test_branchformer_model.py: encoder 5e-5, decoder scores 1e-4, token ids exact."""
import os

import numpy as np
import pytest
import torch

import hypermixing_host_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_G = {}


def gold():
    if "g" not in _G:
        _G["g"] = np.load(os.path.join(GOLD, "model_hyperconformer.npz"))
    return _G["g"]


def state_dict(with_pe=None):
    """The reference's state dict; its per-layer position tables are not stored (``with_pe``: a module whose own tables fill in)."""
    g = gold()
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    if with_pe is not None:
        for k, v in with_pe.state_dict().items():
            if k.endswith("mha_layer.positional_encoding.pe"):
                sd[k] = v.detach().cpu().clone()
    return sd


def hyps_of(arr):
    return [[int(v) for v in row if v >= 0] for row in arr]


def _tiny(**kw):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR

    args = dict(tgt_vocab=40, input_size=24, d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=2, d_ffn=64,
                dropout=0.1, activation=torch.nn.GELU, encoder_module="conformer", attention_type="hypermixing", kernel_size=7,
                normalize_before=True, causal=False)
    args.update(kw)
    return TransformerASR(**args)


def build():
    from speechbrain_amd.nnet.linear import Linear

    g = gold()
    d, H, n_enc, n_dec, d_ffn, ksize, vocab, _ = [int(v) for v in g["cfg"]]
    tr = _tiny(tgt_vocab=vocab, input_size=g["feats"].shape[-1], d_model=d, nhead=H, num_encoder_layers=n_enc,
               num_decoder_layers=n_dec, d_ffn=d_ffn, kernel_size=ksize)
    return g, torch.nn.ModuleDict({"Transformer": tr, "seq_lin": Linear(input_size=d, n_neurons=vocab),
                                   "ctc_lin": Linear(input_size=d, n_neurons=vocab)})


def loaded(dev):
    g, mods = build()
    mods.load_state_dict(state_dict(with_pe=mods), strict=True)
    return g, mods.to(dev).eval()


def test_host_restatement_against_the_reference():
    """tests/hypermixing_host_ref.py (what the kernel and full-size tests compare against) reproduces the reference's encoder,
    layer by layer, at 1e-5 in fp32 -- and its fp64 form stays within the same distance of the fp32 reference outputs."""
    g = gold()
    sd = state_dict()
    d, H, n_enc, _, _, ksize = [int(v) for v in g["cfg"][:6]]
    feats, wl = torch.from_numpy(g["feats"]), torch.from_numpy(g["wav_lens"])
    enc, layers = R.encode(feats, wl, sd, H, n_enc, ksize, "Transformer.", return_layers=True)
    assert float((enc - torch.from_numpy(g["enc_out"])).abs().max()) <= 1e-5
    for l, a in enumerate(layers):
        assert float((a - torch.from_numpy(g[f"enc_layer{l}"])).abs().max()) <= 1e-5
    enc64 = R.encode(feats.double(), wl, {k: R.cast(v, torch.float64) for k, v in sd.items()}, H, n_enc, ksize, "Transformer.")
    assert enc64.dtype == torch.float64
    assert float((enc64 - torch.from_numpy(g["enc_out"]).double()).abs().max()) <= 1e-5


def test_state_dict_keys_shapes_and_position_table():
    """Keys and shapes equal the reference's, the per-layer ``positional_encoding.pe`` [1,3000,d] included (the golden records
    its shape and rows 0-15 and 2999 instead of 2 x 3000 x d values); strict loading works."""
    g, mods = build()
    ours = mods.state_dict()
    pe_keys = [f"Transformer.encoder.layers.{l}.mha_layer.positional_encoding.pe" for l in range(int(g["cfg"][2]))]
    theirs = state_dict()
    assert set(ours.keys()) == set(theirs.keys()) | set(pe_keys)
    assert {k: tuple(v.shape) for k, v in ours.items() if k not in pe_keys} == {k: tuple(v.shape) for k, v in theirs.items()}
    rows = [int(r) for r in g["pe_rows"]]
    for k in pe_keys:
        assert tuple(ours[k].shape) == tuple(int(v) for v in g["pe_shape"]) == (1, 3000, 32)
        assert float((ours[k][0, rows] - torch.from_numpy(g["pe_values"])).abs().max()) <= 1e-6
    for l in range(int(g["cfg"][2])):
        m = f"Transformer.encoder.layers.{l}.mha_layer."
        assert tuple(ours[m + "hyper.w1_gen.fc1_weights"].shape) == (4, 8, 8)
        assert tuple(ours[m + "hyper.w2_gen.fc2_weights"].shape) == (4, 16, 8)
        assert tuple(ours[m + "hyper.w2_gen.fc2_biases"].shape) == (4, 16)
        assert m + "layer_norm.bias" in ours
    mods.load_state_dict(state_dict(with_pe=mods), strict=True)
    with pytest.raises(RuntimeError, match="positional_encoding.pe"):  # (strict means strict: the tables are part of the dict)
        mods.load_state_dict(state_dict(), strict=True)


def test_golden_hyperconformer_encoder(backend):
    """enc_out and every layer's output (output_hidden_states) at 5e-5."""
    nat, dev = backend
    g, mods = loaded(dev)
    tr = mods["Transformer"]
    feats, wl = torch.from_numpy(g["feats"]).to(dev), torch.from_numpy(g["wav_lens"]).to(dev)
    with torch.no_grad():
        enc = tr.encode(feats, wl)
        err = float((enc.cpu() - torch.from_numpy(g["enc_out"])).abs().max())
        print(f"hyperconformer tiny enc_out: max|d| {err:.3e}")
        assert err <= 5e-5
        tr.output_hidden_states = tr.encoder.output_hidden_states = True
        enc2, hidden = tr.encode(feats, wl)
        tr.output_hidden_states = tr.encoder.output_hidden_states = False
        assert torch.equal(enc2, enc)
        assert len(hidden) == len(tr.encoder.layers) + 1  # (the encoder's input first, as the reference)
        for l, h in enumerate(hidden[1:]):
            assert float((h.cpu() - torch.from_numpy(g[f"enc_layer{l}"])).abs().max()) <= 5e-5
        out, attn = tr.encoder(tr.custom_src_module(feats))[:2]  # no position table is passed
        assert attn == [None] * len(tr.encoder.layers)
        # the module surface of the reference's mixer: (out, None), key_padding_mask True = padded
        mixer = tr.encoder.layers[0].mha_layer
        x = torch.randn(2, 9, 32, generator=torch.Generator().manual_seed(5)).to(dev)
        pad = torch.tensor([[False] * 9, [False] * 5 + [True] * 4]).to(dev)
        y, none = mixer(x, x, x, key_padding_mask=pad)
        assert none is None
        sd = {k: v.cpu() for k, v in mixer.state_dict().items()}
        ref = R.hypermix(x.cpu().double(), torch.tensor([9, 5], dtype=torch.int32), sd["positional_encoding.pe"][0].double(),
                         R.cast(R._generator(sd, "hyper.w1_gen."), torch.float64), R.cast(R._generator(sd, "hyper.w2_gen."), torch.float64),
                         sd["layer_norm.weight"].double(), sd["layer_norm.bias"].double(), 1e-5, 4)
        assert float((y.cpu().double() - ref).abs().max()) <= 1e-5


def test_golden_hyperconformer_decoding(backend):
    """The existing decoder and searchers behind a HyperConformer encoder (the decoder adds the fixed_abs_sine table to the
    targets): greedy and beam 4 + CTC 0.4 from the reference's enc_out -- token ids exact, scores 1e-4."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, S2STransformerGreedySearcher, ScorerBuilder

    g, mods = loaded(dev)
    enc_ref, wl = torch.from_numpy(g["enc_out"]).to(dev), torch.from_numpy(g["wav_lens"]).to(dev)
    with torch.no_grad():
        gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                          min_decode_ratio=0.0, max_decode_ratio=1.0)
        hyps, _, scores, _ = gs(enc_ref, wl)
        assert hyps == hyps_of(g["greedy_hyps"])
        assert float((scores[:, 0].cpu() - torch.from_numpy(g["greedy_scores"])[:, : scores.shape[2]]).abs().max()) <= 1e-4
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=int(g["cfg"][7]),
                                        using_eos_threshold=False, length_normalization=True, scorer=scorer)
        hyps, lens, scores, _ = bs(enc_ref, wl)
        assert hyps == hyps_of(g["beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g["beam_scores"])).abs().max()) <= 1e-4
        assert float((lens.cpu() - torch.from_numpy(g["beam_lens"])).abs().max()) <= 1e-6


def test_from_hparams_hyperconformer_model_directory(backend):
    """EncoderDecoderASR.from_hparams on a directory whose YAML says ``attention_type: hypermixing`` (hyperconformer_22M.yaml's
    structure at tiny sizes, checkpoints written by the reference's savers): enc_out 5e-5, tokens and words equal to what the
    reference's EncoderDecoderASR produced from the same files."""
    nat, dev = backend
    from speechbrain_amd.inference.ASR import EncoderDecoderASR
    from speechbrain_amd.nnet.hypermixing import HyperMixing

    exp = np.load(os.path.join(GOLD, "pretrained_hyperconformer_tiny_expected.npz"))
    asr = EncoderDecoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_hyperconformer_tiny"), run_opts={"device": str(dev)})
    assert isinstance(asr.mods.transformer.encoder.layers[0].mha_layer, HyperMixing)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    enc = asr.encode_batch(wav, lens)
    assert float((enc.cpu() - torch.from_numpy(exp["enc_out"])).abs().max()) <= 5e-5
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == hyps_of(exp["tokens"])
    assert words == [str(w) for w in exp["words"]]


def test_encode_group_equals_batch_by_batch(backend):
    """encode_group of two differently padded batches (the row-wise launches once over all rows, one hypermix call and one
    depthwise convolution per batch segment) is bit-identical to encode batch by batch -- and really takes the grouped path."""
    nat, dev = backend
    g, mods = loaded(dev)
    tr = mods["Transformer"]
    gen = torch.Generator().manual_seed(3)
    F_ = g["feats"].shape[-1]
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
        assert torch.equal(a, b)


def test_import_shim_resolves_the_module_path():
    """``speechbrain.nnet.hypermixing.HyperMixing`` is this package's, and the YAML's TransformerASR class path with
    ``attention_type: hypermixing`` builds it."""
    import importlib

    import speechbrain_amd.compat

    speechbrain_amd.compat.install()
    hm = importlib.import_module("speechbrain.nnet.hypermixing")
    assert hm.HyperMixing.__module__ == "speechbrain_amd.nnet.hypermixing"
    assert {"HyperMixing", "HyperNetwork", "ParallelMLPs"} <= set(dir(hm))
    mod = importlib.import_module("speechbrain.lobes.models.transformer.TransformerASR")
    tr = mod.TransformerASR(tgt_vocab=20, input_size=24, d_model=32, nhead=4, num_encoder_layers=1, num_decoder_layers=1,
                            d_ffn=64, encoder_module="conformer", attention_type="hypermixing", kernel_size=7,
                            normalize_before=True, causal=False)
    assert isinstance(tr.encoder.layers[0].mha_layer, hm.HyperMixing)
    m = hm.HyperMixing(input_output_dim=32, hypernet_size=64, tied=False, num_heads=4, fix_tm_hidden_size=False)
    assert tuple(m.positional_encoding.pe.shape) == (1, 3000, 32) and m.hyper.w1_gen is not m.hyper.w2_gen


def test_refusals_by_name():
    """What is out of scope raises and says what it is, before anything is launched (all of this runs without a device)."""
    from speechbrain_amd.nnet.hypermixing import HyperMixing
    from speechbrain_amd.utils.dynamic_chunk_training import DynChunkTrainConfig

    with pytest.raises(NotImplementedError, match="tied"):
        HyperMixing(32, 64, tied=True, num_heads=4)
    with pytest.raises(NotImplementedError, match="fix_tm_hidden_size"):
        HyperMixing(32, 64, num_heads=4, fix_tm_hidden_size=True)
    with pytest.raises(ValueError, match="max_length"):
        HyperMixing(32, 64, num_heads=4, max_length=8)(torch.zeros(1, 9, 32), None, None)
    with pytest.raises(NotImplementedError, match="transformer.*hypermixing"):
        _tiny(encoder_module="transformer")
    with pytest.raises(NotImplementedError, match="causal"):
        _tiny(causal=True)
    with pytest.raises(NotImplementedError, match="hypermixing"):  # (unchanged: tests/test_branchformer_model.py pins it)
        _tiny(encoder_module="branchformer", csgu_linear_units=48)
    tr = _tiny()
    cfg = DynChunkTrainConfig(4, 1)
    with pytest.raises(NotImplementedError, match="dynchunktrain_config.*hypermixing"):
        tr.encode(torch.zeros(1, 8, 24), dynchunktrain_config=cfg)
    with pytest.raises(NotImplementedError, match="dynchunktrain_config.*hypermixing"):
        tr.encode_group([torch.zeros(1, 8, 24)], [None], dynchunktrain_config=cfg)
    with pytest.raises(NotImplementedError, match="dynchunktrain_config.*hypermixing"):
        tr.encoder.layers[0](torch.zeros(1, 8, 32), dynchunktrain_config=cfg)
    with pytest.raises(NotImplementedError, match="streaming.*hypermixing"):
        tr.make_streaming_context(cfg)
    with pytest.raises(NotImplementedError, match="streaming.*hypermixing"):
        tr.encode_streaming(torch.zeros(1, 4, 24), None)
    with pytest.raises(NotImplementedError, match="streaming.*hypermixing"):
        tr.encoder.layers[0].make_streaming_context(4)
    tr.encoder.layers[0].collect_attention = True
    with pytest.raises(NotImplementedError, match="collect_attention.*hypermixing"):
        tr.encoder.layers[0](torch.zeros(1, 8, 32))
