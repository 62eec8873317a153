"""TransformerASR(encoder_module="transformer", attention_type="regularMHA") -- the transformer.yaml recipe -- through the drop-in
module surface against the REFERENCE's outputs stored in tests/golden/model_transformer.npz and
tests/golden/pretrained_transformer_tiny/ (tools/make_transformer_golden.py).  Runs on the CPU emulator of the kernels (not gpu) and
on the MI355X (-m gpu).  Bounds are those of the tiny Branchformer and Conformer goldens: host restatement 1e-5, encoder 5e-5,
decoder scores 1e-4, token ids exact."""
import os

import numpy as np
import pytest
import torch

import transformer_host_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_G = {}
CNN_KW = dict(num_blocks=3, num_layers_per_block=1, kernel_sizes=(5, 5, 1), strides=(2, 2, 1), residuals=(False, False, True))


def gold():
    if "g" not in _G:
        _G["g"] = np.load(os.path.join(GOLD, "model_transformer.npz"))
    return _G["g"]


def state_dict(tag):
    """h4: as stored; dh128: the parameters redrawn from the recorded seed (3.5 MB are not committed)."""
    g = gold()
    if tag == "h4":
        return {k[len(tag) + 4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(f"{tag}/sd/")}
    shapes = {str(n): [int(v) for v in s if v > 0] for n, s in zip(g[f"{tag}/param_names"], g[f"{tag}/param_shapes"])}
    return R.seeded_state_dict(shapes, int(g[f"{tag}/cfg"][7]))


def hyps_of(arr):
    return [[int(v) for v in row if v >= 0] for row in arr]


def build(tag, normalize_before=True, n_dec=None):
    from speechbrain_amd.lobes.models.convolution import ConvolutionFrontEnd
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain_amd.nnet.linear import Linear

    g = gold()
    d, H, n_enc, dec, d_ffn, vocab, _, _ = [int(v) for v in g[f"{tag}/cfg"]]
    n_dec = dec if n_dec is None else n_dec
    feats = g[f"{tag}/feats"]
    mods = {}
    in_size = feats.shape[-1]
    if f"{tag}/cnn_out" in g.files:
        C = int(g[f"{tag}/cnn_channels"])
        mods["CNN"] = ConvolutionFrontEnd(input_shape=tuple(feats.shape), out_channels=(C, C, C), **CNN_KW)
        in_size = int(np.prod(g[f"{tag}/cnn_out"].shape[2:]))
    mods["Transformer"] = TransformerASR(
        input_size=in_size, tgt_vocab=vocab, d_model=d, nhead=H, num_encoder_layers=n_enc, num_decoder_layers=n_dec, d_ffn=d_ffn,
        dropout=0.1, activation=torch.nn.GELU, encoder_module="transformer", attention_type="regularMHA",
        normalize_before=normalize_before, causal=False)
    mods["seq_lin"], mods["ctc_lin"] = Linear(input_size=d, n_neurons=vocab), Linear(input_size=d, n_neurons=vocab)
    return g, torch.nn.ModuleDict(mods)


def loaded(tag, dev):
    g, mods = build(tag)
    mods.load_state_dict(state_dict(tag), strict=tag == "h4")  # (dh128: parameters only; the position table is a buffer)
    return g, mods.to(dev).eval()


def test_host_restatement_against_the_reference():
    """tests/transformer_host_ref.py reproduces the reference's front end and encoder, block by block and layer by layer, at 1e-5
    in fp32; its fp64 form stays within the same distance; dh128's redrawn parameters reproduce the reference's enc_out."""
    g = gold()
    sd = state_dict("h4")
    d, H, n_enc = [int(v) for v in g["h4/cfg"][:3]]
    feats, wl = torch.from_numpy(g["h4/feats"]), torch.from_numpy(g["h4/wav_lens"])
    src, blocks = R.conv_frontend(feats, sd, "CNN.", return_blocks=True)
    for i, b in enumerate(blocks):
        assert float((b - torch.from_numpy(g[f"h4/cnn_block{i}"])).abs().max()) <= 1e-5
    enc, layers = R.encode(src, wl, sd, "Transformer.", H, n_enc, return_layers=True)
    assert float((enc - torch.from_numpy(g["h4/enc_out"])).abs().max()) <= 1e-5
    for l, a in enumerate(layers):
        assert float((a - torch.from_numpy(g[f"h4/enc_layer{l}"])).abs().max()) <= 1e-5
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    enc64 = R.encode(R.conv_frontend(feats.double(), sd64, "CNN."), wl, sd64, "Transformer.", H, n_enc)
    assert enc64.dtype == torch.float64
    assert float((enc64 - torch.from_numpy(g["h4/enc_out"]).double()).abs().max()) <= 1e-5
    sd, (d, H, n_enc) = state_dict("dh128"), [int(v) for v in g["dh128/cfg"][:3]]
    assert d // H == 128
    enc = R.encode(torch.from_numpy(g["dh128/feats"]), wl, sd, "Transformer.", H, n_enc)
    assert float((enc - torch.from_numpy(g["dh128/enc_out"])).abs().max()) <= 1e-5


@pytest.mark.parametrize("tag", ["h4", "dh128"])
def test_state_dict_keys_equal_the_reference(tag):
    g, mods = build(tag)
    ours = mods.state_dict()
    assert sorted(ours) == [str(k) for k in g[f"{tag}/sd_keys"]]
    if tag == "h4":
        theirs = state_dict(tag)
        assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in theirs.items()}
        for key in ("CNN.convblock_2.convs.conv_0.conv.weight", "CNN.convblock_2.convs.norm_0.norm.weight",
                    "CNN.convblock_2.reduce_conv.conv.conv.weight", "CNN.convblock_2.reduce_conv.norm.norm.bias",
                    "Transformer.encoder.layers.0.self_att.att.in_proj_weight"):
            assert key in ours


def test_golden_transformer_encoder_h4(backend):
    """Every conv block, every encoder layer (output_hidden_states) and enc_out at 5e-5, from the features."""
    nat, dev = backend
    g, mods = loaded("h4", dev)
    tr = mods["Transformer"]
    feats, wl = torch.from_numpy(g["h4/feats"]).to(dev), torch.from_numpy(g["h4/wav_lens"]).to(dev)
    with torch.no_grad():
        x = feats
        for i, block in enumerate(mods["CNN"].values()):
            x = block(x)
            assert float((x.cpu() - torch.from_numpy(g[f"h4/cnn_block{i}"])).abs().max()) <= 5e-5
        fp = mods["CNN"].get_filter_properties()
        assert [fp.window_size, fp.stride, fp.dilation] == [int(v) for v in g["h4/cnn_filter_properties"]]
        enc = tr.encode(x, wl)
        assert float((enc.cpu() - torch.from_numpy(g["h4/enc_out"])).abs().max()) <= 5e-5
        tr.output_hidden_states = tr.encoder.output_hidden_states = True
        enc2, hidden = tr.encode(x, wl)
        tr.output_hidden_states = tr.encoder.output_hidden_states = False
        assert torch.equal(enc2, enc)
        assert len(hidden) == len(tr.encoder.layers) + 1  # (the encoder's input first, as the reference)
        for l, h in enumerate(hidden[1:]):
            assert float((h.cpu() - torch.from_numpy(g[f"h4/enc_layer{l}"])).abs().max()) <= 5e-5
        # attention maps are opt-in: head-averaged [B,T,T] rows that sum to one over the allowed keys
        for layer in tr.encoder.layers:
            layer.collect_attention = True
        src = tr.custom_src_module(x.reshape(x.shape[0], x.shape[1], -1))
        src = src + tr.positional_encoding(src)
        pad = torch.arange(x.shape[1], device=dev)[None] >= torch.round(wl * x.shape[1])[:, None]
        out, attn = tr.encoder(src, src_key_padding_mask=pad)
        assert float((out - enc).abs().max()) <= 2e-5
        assert len(attn) == len(tr.encoder.layers) and attn[0].shape == (3, x.shape[1], x.shape[1])
        assert float((attn[0].sum(-1) - 1).abs().max()) <= 1e-5 and float(attn[0][0, :, -1].abs().max()) == 0.0


def test_golden_transformer_encoder_dh128(backend):
    """Head dim 128: enc_out at 5e-5; asking for attention maps raises by name."""
    nat, dev = backend
    g, mods = loaded("dh128", dev)
    tr = mods["Transformer"]
    feats, wl = torch.from_numpy(g["dh128/feats"]).to(dev), torch.from_numpy(g["dh128/wav_lens"]).to(dev)
    with torch.no_grad():
        enc = tr.encode(feats, wl)
        assert float((enc.cpu() - torch.from_numpy(g["dh128/enc_out"])).abs().max()) <= 5e-5
        tr.encoder.layers[0].collect_attention = True
        with pytest.raises(NotImplementedError, match="collect_attention"):
            tr.encode(feats, wl)


@pytest.mark.parametrize("tag", ["h4", "dh128"])
def test_golden_transformer_decoding(backend, tag):
    """The existing decoder and searchers behind the Transformer encoder: greedy and beam 4 (+ CTC 0.4 for h4) from the
    reference's enc_out -- token ids and lengths exact, scores 1e-4."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, S2STransformerGreedySearcher, ScorerBuilder

    g, mods = loaded(tag, dev)
    enc_ref, wl = torch.from_numpy(g[f"{tag}/enc_out"]).to(dev), torch.from_numpy(g[f"{tag}/wav_lens"]).to(dev)
    with torch.no_grad():
        gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                          min_decode_ratio=0.0, max_decode_ratio=1.0)
        hyps, _, scores, _ = gs(enc_ref, wl)
        assert hyps == hyps_of(g[f"{tag}/greedy_hyps"])
        assert float((scores[:, 0].cpu() - torch.from_numpy(g[f"{tag}/greedy_scores"])[:, : scores.shape[2]]).abs().max()) <= 1e-4
        w = float(g[f"{tag}/ctc_weight"])
        scorer = None
        if w > 0:
            scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": w})
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=int(g[f"{tag}/cfg"][6]),
                                        using_eos_threshold=False, length_normalization=True, scorer=scorer)
        hyps, lens, scores, _ = bs(enc_ref, wl)
        assert hyps == hyps_of(g[f"{tag}/beam_hyps"])
        assert float((scores.cpu() - torch.from_numpy(g[f"{tag}/beam_scores"])).abs().max()) <= 1e-4
        assert float((lens.cpu() - torch.from_numpy(g[f"{tag}/beam_lens"])).abs().max()) <= 1e-6


def test_from_hparams_transformer_model_directory(backend):
    """EncoderDecoderASR.from_hparams on a directory in transformer.yaml's layout (tiny sizes, checkpoints written by the
    reference's savers): enc_out 5e-5, tokens and words equal to what the reference's EncoderDecoderASR produced."""
    nat, dev = backend
    from speechbrain_amd.inference.ASR import EncoderDecoderASR
    from speechbrain_amd.lobes.models.transformer.Transformer import TransformerEncoder

    exp = np.load(os.path.join(GOLD, "pretrained_transformer_tiny_expected.npz"))
    asr = EncoderDecoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_transformer_tiny"), run_opts={"device": str(dev)})
    assert isinstance(asr.mods.transformer.encoder, TransformerEncoder)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    enc = asr.encode_batch(wav, lens)
    assert float((enc.cpu() - torch.from_numpy(exp["enc_out"])).abs().max()) <= 5e-5
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == hyps_of(exp["tokens"])
    assert words == [str(w) for w in exp["words"]]


def test_encode_group_equals_batch_by_batch(backend):
    """encode_group over batches [3, 61] and [2, 40] (front-end output frames; each batch's positions start at 0) equals encode
    batch by batch at 2e-5 -- and really takes the grouped path."""
    nat, dev = backend
    g, mods = loaded("h4", dev)
    tr = mods["Transformer"]
    gen = torch.Generator().manual_seed(3)
    F_ = tr.custom_src_module.layers[0].w.in_features if hasattr(tr.custom_src_module, "layers") else 48
    srcs = [torch.randn(3, 61, F_, generator=gen).to(dev), torch.randn(2, 40, F_, generator=gen).to(dev)]
    wls = [torch.tensor([0.6, 0.8, 1.0]).to(dev), torch.tensor([1.0, 0.5]).to(dev)]
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


def test_post_norm_encoder_only(backend):
    """normalize_before=False, num_decoder_layers=0: encode matches the host restatement's other norm order at 5e-5."""
    nat, dev = backend
    g, mods = build("h4", normalize_before=False, n_dec=0)
    sd = {k: v for k, v in state_dict("h4").items() if k in mods.state_dict()}
    mods.load_state_dict(sd, strict=True)
    tr = mods["Transformer"].to(dev).eval()
    H, n_enc = int(g["h4/cfg"][1]), int(g["h4/cfg"][2])
    src, wl = torch.from_numpy(g["h4/cnn_out"]), torch.from_numpy(g["h4/wav_lens"])
    ref = R.encode(src, wl, sd, "Transformer.", H, n_enc, normalize_before=False)
    pre = R.encode(src, wl, sd, "Transformer.", H, n_enc, normalize_before=True)
    assert float((ref - pre).abs().max()) > 1e-2  # (the two orders differ)
    with torch.no_grad():
        enc = tr.encode(src.to(dev), wl.to(dev))
    assert float((enc.cpu() - ref).abs().max()) <= 5e-5


def test_import_shim_resolves_the_yaml_class_path():
    import importlib

    import speechbrain_amd.compat

    speechbrain_amd.compat.install()
    mod = importlib.import_module("speechbrain.lobes.models.transformer.TransformerASR")
    tr = mod.TransformerASR(tgt_vocab=20, input_size=24, d_model=32, nhead=4, num_encoder_layers=1, num_decoder_layers=1,
                            d_ffn=64, encoder_module="transformer", attention_type="regularMHA", normalize_before=True, causal=False)
    t = importlib.import_module("speechbrain.lobes.models.transformer.Transformer")
    assert isinstance(tr.encoder, t.TransformerEncoder)
    assert t.TransformerEncoder.__module__ == "speechbrain_amd.lobes.models.transformer.Transformer"
    conv = importlib.import_module("speechbrain.lobes.models.convolution")
    cnn = conv.ConvolutionFrontEnd(input_shape=(2, 9, 24), out_channels=(8, 8, 8), **CNN_KW)
    assert cnn["convblock_2"].reduce_conv is not None


def _tiny(**kw):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR

    args = dict(tgt_vocab=20, input_size=24, d_model=32, nhead=4, num_encoder_layers=1, num_decoder_layers=1, d_ffn=64,
                encoder_module="transformer", attention_type="regularMHA", normalize_before=True, causal=False)
    args.update(kw)
    return TransformerASR(**args)


def test_refusals_by_name():
    """What is out of scope raises NotImplementedError and names the argument."""
    from speechbrain_amd.lobes.models.transformer.Transformer import TransformerEncoder
    from speechbrain_amd.utils.dynamic_chunk_training import DynChunkTrainConfig

    with pytest.raises(NotImplementedError, match="normalize_before"):
        _tiny(normalize_before=False)
    _tiny(normalize_before=False, num_decoder_layers=0)  # (a post-norm encoder alone is implemented)
    with pytest.raises(NotImplementedError, match="causal"):
        _tiny(causal=True)
    with pytest.raises(NotImplementedError, match="causal"):
        _tiny(causal=None)  # (TransformerASR's default is causal)
    with pytest.raises(NotImplementedError, match="ffn_type"):
        TransformerEncoder(num_layers=1, nhead=4, d_ffn=64, d_model=32, ffn_type="1dcnn")
    tr = _tiny()
    with pytest.raises(NotImplementedError, match="streaming"):
        tr.make_streaming_context(object())
    with pytest.raises(NotImplementedError, match="streaming"):
        tr.encode_streaming(torch.zeros(1, 4, 24), None)
    with pytest.raises(NotImplementedError, match="dynchunktrain_config"):
        tr.encode(torch.zeros(1, 8, 24), dynchunktrain_config=DynChunkTrainConfig(4, 1))
    with pytest.raises(NotImplementedError, match="dynchunktrain_config"):
        tr.encode_group([torch.zeros(1, 8, 24)], [None], dynchunktrain_config=DynChunkTrainConfig(4, 1))
