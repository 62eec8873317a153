"""integrations/huggingface/wavlm.py and hubert.py against the goldens the reference wrote (tools/make_wavlm_golden.py): the
tiny HuggingFace directories (WavLM group-norm / post-norm with 32 buckets, WavLM layer-norm / stable with the default buckets,
HuBERT without the projection LayerNorm), the wrappers' outputs, their state-dict key lists, and an EncoderASR directory in the
layout of train_hf_wav2vec.yaml with the WavLM wrapper.  ``backend``: the CPU emulator of the kernel sources (not gpu) and the
MI355X (-m gpu).  Neither ``transformers`` nor the reference is imported."""
import json
import os

import numpy as np
import pytest
import torch

import wavlm_host_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DIRS = {"group": "wavlm_group_tiny", "layer": "wavlm_layer_tiny", "hubert": "hubert_tiny"}
VARIANTS = tuple(DIRS)
_G = {}


def gold():
    if "model" not in _G:
        _G["model"] = dict(np.load(os.path.join(GOLD, "wavlm_model.npz")))
    return _G["model"]


def hub(name):
    return os.path.join(GOLD, DIRS.get(name, name))


def host_inputs(name):
    """(state dict without the wrapper's prefix, config, do_normalize) read straight from the fixture directory."""
    from safetensors.torch import load_file

    with open(os.path.join(hub(name), "config.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(hub(name), "preprocessor_config.json")) as f:
        norm = json.load(f)["do_normalize"]
    return {k: v.float() for k, v in load_file(os.path.join(hub(name), "model.safetensors")).items()}, cfg, norm


def wrapper_class(name):
    from speechbrain_amd.integrations.huggingface.hubert import HuBERT
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM

    return HuBERT if name == "hubert" else WavLM


def wrapper(name, dev, **kw):
    return wrapper_class(name)(hub(name), save_path=None, freeze=True, **kw).to(dev)


CASES = [("plain", {}), ("norm", dict(output_norm=True)), ("all", dict(output_all_hiddens=True)),
         ("all_norm", dict(output_all_hiddens=True, output_norm=True))]


@pytest.mark.parametrize("name", VARIANTS)
def test_host_restatement_against_the_reference(name):
    """tests/wavlm_host_ref.py reproduces the reference wrapper at 1e-5 in fp32 (and in fp64), padded frames included."""
    g = gold()
    sd, cfg, norm = host_inputs(name)
    wav, lens = torch.from_numpy(g["wav"]), torch.from_numpy(g["lens"])
    sd64 = {k: v.double() for k, v in sd.items()}
    for tag, kw in CASES:
        want = torch.from_numpy(g[f"{name}_{tag}"])
        got = R.forward(wav, lens, sd, cfg, norm, kw.get("output_norm", False), kw.get("output_all_hiddens", False))
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-5
        got64 = R.forward(wav.double(), lens.double(), sd64, cfg, norm, kw.get("output_norm", False),
                          kw.get("output_all_hiddens", False))
        assert float((got64 - want.double()).abs().max()) <= 1e-5
    assert float((R.forward(wav, None, sd, cfg, norm) - torch.from_numpy(g[f"{name}_nolens"])).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", VARIANTS)
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    want = json.loads(str(gold()[f"{name}_keys"]))
    ours = wrapper(name, "cpu").state_dict()
    assert [[k, list(v.shape)] for k, v in ours.items()] == want
    assert len(want) == {"group": 58, "layer": 77, "hubert": 49}[name]
    assert "model.masked_spec_embed" in ours
    layers = "model.encoder.layers."
    if name == "hubert":
        assert not any("feature_projection.layer_norm" in k or "gru_rel_pos" in k or "rel_attn_embed" in k for k in ours)
    else:
        H = 3 if name == "group" else 4
        assert "model.feature_projection.layer_norm.weight" in ours
        for i in (0, 1):
            assert list(ours[f"{layers}{i}.attention.gru_rel_pos_const"].shape) == [1, H, 1, 1]
            assert list(ours[f"{layers}{i}.attention.gru_rel_pos_linear.weight"].shape) == [8, 32]
        assert list(ours[layers + "0.attention.rel_attn_embed.weight"].shape) == [32 if name == "group" else 320, H]
        assert layers + "1.attention.rel_attn_embed.weight" not in ours


def test_checkpoint_prefix_is_stripped(tmp_path):
    """A task model's checkpoint (``wavlm.`` / ``hubert.`` before every encoder key, a head beside them) loads to the same weights."""
    from safetensors.torch import load_file, save_file

    for name, pre in (("group", "wavlm."), ("hubert", "hubert.")):
        sd = {pre + k: v for k, v in load_file(os.path.join(hub(name), "model.safetensors")).items()}
        sd["lm_head.weight"] = torch.zeros(4, 96, dtype=torch.float16)
        d = tmp_path / name
        d.mkdir()
        save_file(sd, str(d / "model.safetensors"))
        for f in ("config.json", "preprocessor_config.json"):
            (d / f).write_bytes(open(os.path.join(hub(name), f), "rb").read())
        a, b = wrapper(name, "cpu").state_dict(), wrapper_class(name)(str(d), save_path=None).state_dict()
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a if k != "model.masked_spec_embed")


@pytest.mark.parametrize("name", VARIANTS)
def test_golden_wrapper_outputs(backend, name):
    """output_norm on / off, output_all_hiddens: 5e-5 on every frame, padded frames included (the tiny-encoder bound of
    tests/test_wav2vec2_model.py; the reference's own fp32-vs-fp64 distance on these models is in the fixture: 1.8e-6 .. 4.0e-6)."""
    nat, dev = backend
    g = gold()
    wav, lens = torch.from_numpy(g["wav"]).to(dev), torch.from_numpy(g["lens"]).to(dev)
    for tag, kw in CASES:
        got = wrapper(name, dev, **kw)(wav, lens).cpu()
        want = torch.from_numpy(g[f"{name}_{tag}"])
        assert got.shape == want.shape
        err = float((got - want).abs().max())
        print(f"{name} {tag}: max|d| {err:.3e} (reference fp32 vs fp64 {float(g[f'{name}_{tag}_ref32v64']):.2e})")
        assert err <= 5e-5
    err = float((wrapper(name, dev)(wav).cpu() - torch.from_numpy(g[f"{name}_nolens"])).abs().max())
    assert err <= 5e-5


def test_no_square_tensor_on_the_wavlm_path(backend, monkeypatch):
    """Nothing with two T' axes is allocated by the WavLM forward: every tensor the kernels are handed or return has at most
    one axis of T' (or 2T'-1) frames.  T' = 18 and no other dimension of the tiny model is 18 or 35."""
    nat, dev = backend
    g = gold()
    w = wrapper("group", dev)
    seen = []
    for fn in ("gemm_nt", "gemm_nt_rows", "layernorm", "w2v_posconv", "wavlm_attention", "wavlm_bias_table"):
        real = getattr(nat, fn)

        def spy(*a, _real=real, **k):
            out = _real(*a, **k)
            seen.extend(tuple(t.shape) for t in list(a) + [out] if torch.is_tensor(t))
            return out

        monkeypatch.setattr(nat, fn, spy)
    y = w(torch.from_numpy(g["wav"]).to(dev), torch.from_numpy(g["lens"]).to(dev))
    T = y.shape[1]
    assert T == 18 and any(s == (3, 2 * T - 1) for s in seen)  # the table: [H, 2T'-1]
    assert not [s for s in seen if sum(1 for n in s if n in (T, 2 * T - 1)) > 1]


def test_hubert_with_projection_layer_norm_from_config(backend):
    """feat_proj_layer_norm=True (HuggingFace's default; hubert-large): 51 keys, the LayerNorm runs -- against the host
    restatement on the model's own random weights, at the wrapper bound."""
    nat, dev = backend
    from speechbrain_amd.integrations.huggingface.hubert import HuBERT

    _, cfg, _ = host_inputs("hubert")
    cfg = {**cfg, "feat_proj_layer_norm": True}
    w = HuBERT.from_config(cfg, seed=5)
    with torch.no_grad():
        ln = w.model.feature_projection.layer_norm
        ln.weight.add_(0.2 * torch.randn(ln.weight.shape))
        ln.bias.add_(0.2 * torch.randn(ln.bias.shape))
    sd = {k[len("model."):]: v.detach().clone() for k, v in w.state_dict().items()}
    assert len(sd) == 51 and "feature_projection.layer_norm.weight" in sd
    g = gold()
    wav, lens = torch.from_numpy(g["wav"]), torch.from_numpy(g["lens"])
    want = R.forward(wav.double(), lens.double(), {k: v.double() for k, v in sd.items()}, cfg, False)
    off = R.forward(wav.double(), lens.double(), {k: v.double() for k, v in sd.items()}, {**cfg, "feat_proj_layer_norm": False}, False)
    assert float((want - off).abs().max()) > 1e-2  # (the switch matters on these weights)
    got = w.to(dev)(wav.to(dev), lens.to(dev)).cpu()
    err = float((got.double() - want).abs().max())
    print(f"hubert feat_proj_layer_norm=True: max|d| {err:.3e}")
    assert err <= 5e-5


def _asr(dev, yaml="hyperparams.yaml"):
    from speechbrain_amd.inference.ASR import EncoderASR

    return EncoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_wavlm_ctc_tiny"), hparams_file=yaml,
                                   overrides={"wav2vec2_hub": hub("group")}, run_opts={"device": str(dev)})


def _tokens(padded):
    return [[int(t) for t in row if t >= 0] for row in padded]


def test_from_hparams_wavlm_ctc_directory(backend):
    """A hyperparams.yaml with !new:speechbrain.integrations.huggingface.wavlm.WavLM: wav2vec2.ckpt / model.ckpt / tokenizer.ckpt
    written by the reference's savers load through the Pretrainer; log-probs 1e-4, greedy ids exact, beam-search text equal."""
    nat, dev = backend
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM

    exp = np.load(os.path.join(GOLD, "pretrained_wavlm_ctc_tiny_expected.npz"))
    asr = _asr(dev)
    enc = asr.mods.encoder
    assert type(enc.wav2vec2) is WavLM
    model = torch.nn.ModuleList([enc.enc, enc.ctc_lin])
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(exp["model_keys"]))
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    logp = asr.encode_batch(wav, lens).cpu()
    err = float((logp - torch.from_numpy(exp["logp"])).abs().max())
    print(f"WavLM CTC log-probs: max|d| {err:.3e}")
    assert err <= 1e-4
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == _tokens(exp["greedy_tokens"]) and list(words) == [str(w) for w in exp["greedy_words"]]
    path = os.path.join(GOLD, "ref_spk1_snt1.wav")
    sig = asr.load_audio(path)
    flogp = asr.encode_batch(sig[None], torch.ones(1)).cpu()
    assert float((flogp - torch.from_numpy(exp["file_logp"])).abs().max()) <= 1e-4
    fwords, ftokens = asr.transcribe_batch(sig[None], torch.ones(1))
    assert ftokens == _tokens(exp["file_greedy_tokens"]) and list(fwords) == [str(w) for w in exp["file_greedy_words"]]
    assert asr.transcribe_file(path) == str(exp["greedy_file_words"][0])
    beam = _asr(dev, "hyperparams_beam.yaml")
    bwords, _ = beam.transcribe_batch(wav, lens)
    assert list(bwords) == [str(w) for w in exp["beam_words"]]
    assert beam.transcribe_file(path) == str(exp["beam_file_words"][0])


def test_import_shim_resolves_the_yaml_class_paths():
    from speechbrain_amd.integrations.huggingface.hubert import HuBERT
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM
    from speechbrain_amd.utils.hpyaml import load_hyperpyyaml

    h = load_hyperpyyaml("a: !name:speechbrain.integrations.huggingface.wavlm.WavLM\n"
                         "b: !name:speechbrain.integrations.huggingface.hubert.HuBERT\n")
    for key, cls in (("a", WavLM), ("b", HuBERT)):
        assert (h[key].func if hasattr(h[key], "func") else h[key]) is cls


def _cfg(name, **over):
    with open(os.path.join(hub(name), "config.json")) as f:
        return {**json.load(f), **over}


@pytest.mark.parametrize("name,over,word", [
    ("group", dict(add_adapter=True), "WavLM with add_adapter"),
    ("group", dict(hidden_act="relu"), "hidden_act"),
    ("group", dict(feat_extract_activation="relu"), "feat_extract_activation"),
    ("group", dict(hidden_size=80, num_conv_pos_embedding_groups=5, num_attention_heads=4), r"head dim 80/4.*\(16, 32, 64\)"),
    ("group", dict(hidden_size=256, num_conv_pos_embedding_groups=4, num_attention_heads=2), "head dim 256/2"),  # 128: plain only
    ("hubert", dict(conv_pos_batch_norm=True), "conv_pos_batch_norm"),
    ("hubert", dict(add_adapter=True), "HuBERT with add_adapter"),
    ("hubert", dict(hidden_size=1280, num_conv_pos_embedding_groups=20, num_attention_heads=16), "head dim 1280/16"),  # xlarge: 80
])
def test_unsupported_configs_raise_by_name(name, over, word):
    with pytest.raises(NotImplementedError, match=word):
        wrapper_class(name).from_config(_cfg(name, **over))


def test_wrappers_accept_their_own_model_type_only():
    from speechbrain_amd.integrations.huggingface.hubert import HuBERT
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM

    w2v = os.path.join(GOLD, "wav2vec2_group_tiny")
    with pytest.raises(NotImplementedError, match=r"WavLM: model_type 'wav2vec2' — load it with .*wav2vec2\.Wav2Vec2"):
        WavLM(w2v, None)
    with pytest.raises(NotImplementedError, match=r"HuBERT: model_type 'wavlm' — load it with .*wavlm\.WavLM"):
        HuBERT(hub("group"), None)
    with pytest.raises(NotImplementedError, match=r"WavLM: model_type 'hubert' — load it with .*hubert\.HuBERT"):
        WavLM(hub("hubert"), None)
    with pytest.raises(NotImplementedError, match=r"Wav2Vec2: model_type 'wavlm' — load it with .*wavlm\.WavLM"):
        Wav2Vec2(hub("group"), None)
    with pytest.raises(NotImplementedError, match=r"Wav2Vec2: model_type 'hubert' — load it with .*hubert\.HuBERT"):
        Wav2Vec2(hub("hubert"), None)
    for cls, name in ((WavLM, "group"), (HuBERT, "hubert")):
        with pytest.raises(NotImplementedError, match="output_attentions"):
            cls(hub(name), None, output_attentions=True)
        with pytest.raises(NotImplementedError, match="apply_spec_augment"):
            cls(hub(name), None, apply_spec_augment=True)
