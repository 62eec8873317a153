"""integrations/huggingface/wav2vec2.py against the goldens the reference wrote (tools/make_wav2vec2_golden.py): the two tiny
HuggingFace directories (group-norm / post-norm and layer-norm / stable), the wrapper's outputs, its state-dict key list, and
an EncoderASR directory in the layout of train_hf_wav2vec.yaml.  ``backend``: the CPU emulator of the kernel sources (not gpu)
and the MI355X (-m gpu).  Neither ``transformers`` nor the reference is imported."""
import json
import os

import numpy as np
import pytest
import torch

import wav2vec2_host_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VARIANTS = ("group", "layer")
_G = {}


def gold():
    if "model" not in _G:
        _G["model"] = dict(np.load(os.path.join(GOLD, "wav2vec2_model.npz")))
    return _G["model"]


def hub(name):
    return os.path.join(GOLD, f"wav2vec2_{name}_tiny")


def host_inputs(name):
    """(state dict without the wrapper's prefix, config, do_normalize) read straight from the fixture directory."""
    from safetensors.torch import load_file

    with open(os.path.join(hub(name), "config.json")) as f:
        cfg = json.load(f)
    with open(os.path.join(hub(name), "preprocessor_config.json")) as f:
        norm = json.load(f)["do_normalize"]
    return {k: v.float() for k, v in load_file(os.path.join(hub(name), "model.safetensors")).items()}, cfg, norm


def wrapper(name, dev, **kw):
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2

    return Wav2Vec2(hub(name), save_path=None, freeze=True, **kw).to(dev)


CASES = [("plain", {}), ("norm", dict(output_norm=True)), ("all", dict(output_all_hiddens=True)),
         ("all_norm", dict(output_all_hiddens=True, output_norm=True))]


@pytest.mark.parametrize("name", VARIANTS)
def test_host_restatement_against_the_reference(name):
    """tests/wav2vec2_host_ref.py reproduces the reference wrapper at 1e-5 in fp32 (and in fp64), padded frames included."""
    g = gold()
    sd, cfg, norm = host_inputs(name)
    wav, lens = torch.from_numpy(g["wav"]), torch.from_numpy(g["lens"])
    for tag, kw in CASES:
        want = torch.from_numpy(g[f"{name}_{tag}"])
        got = R.forward(wav, lens, sd, cfg, norm, kw.get("output_norm", False), kw.get("output_all_hiddens", False))
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-5
        sd64 = {k: v.double() for k, v in sd.items()}
        got64 = R.forward(wav.double(), lens.double(), sd64, cfg, norm, kw.get("output_norm", False),
                          kw.get("output_all_hiddens", False))
        assert float((got64 - want.double()).abs().max()) <= 1e-5
    assert float((R.forward(wav, None, sd, cfg, norm) - torch.from_numpy(g[f"{name}_nolens"])).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", VARIANTS)
def test_state_dict_keys_and_shapes_equal_the_reference(name):
    want = json.loads(str(gold()[f"{name}_keys"]))
    ours = wrapper(name, "cpu").state_dict()
    assert [[k, list(v.shape)] for k, v in ours.items()] == want
    assert len(want) == (51 if name == "group" else 70)
    assert "model.masked_spec_embed" in ours
    assert "model.encoder.pos_conv_embed.conv.parametrizations.weight.original0" in ours
    assert "model.encoder.pos_conv_embed.conv.parametrizations.weight.original1" in ours


def test_old_weight_norm_spelling_loads_to_the_same_effective_weight(tmp_path):
    """``weight_g`` / ``weight_v`` (checkpoints written by older torch): in a HuggingFace directory and in a wrapper state dict."""
    from safetensors.torch import load_file, save_file

    pre = "encoder.pos_conv_embed.conv."
    sd = load_file(os.path.join(hub("group"), "model.safetensors"))
    sd[pre + "weight_g"] = sd.pop(pre + "parametrizations.weight.original0")
    sd[pre + "weight_v"] = sd.pop(pre + "parametrizations.weight.original1")
    d = tmp_path / "old"
    d.mkdir()
    save_file(sd, str(d / "model.safetensors"))
    for f in ("config.json", "preprocessor_config.json"):
        (d / f).write_bytes(open(os.path.join(hub("group"), f), "rb").read())
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2

    new, old = wrapper("group", "cpu"), Wav2Vec2(str(d), save_path=None)
    want = R.pos_weight({k: v.float() for k, v in load_file(os.path.join(hub("group"), "model.safetensors")).items()})
    tap_major = want.permute(0, 2, 1).reshape(want.shape[0], -1)
    for w in (new, old):
        assert torch.equal(w.model.encoder.pos_conv_embed.conv.effective(), tap_major)
    wsd = {("model." + k): v.float() for k, v in sd.items()}
    fresh = Wav2Vec2.from_config(json.load(open(os.path.join(hub("group"), "config.json"))), seed=3)
    res = fresh.load_state_dict(wsd, strict=False)
    assert not res.unexpected_keys and res.missing_keys == []
    assert torch.equal(fresh.model.encoder.pos_conv_embed.conv.effective(), tap_major)


@pytest.mark.parametrize("name", VARIANTS)
def test_golden_wrapper_outputs(backend, name):
    """output_norm on / off, output_all_hiddens: 5e-5 on every frame, padded frames included (the tiny-encoder bound of
    tests/test_model_parity.py; the reference's own fp32-vs-fp64 distance on these models is 2.4e-6 .. 3.4e-6)."""
    nat, dev = backend
    g = gold()
    wav, lens = torch.from_numpy(g["wav"]).to(dev), torch.from_numpy(g["lens"]).to(dev)
    for tag, kw in CASES:
        got = wrapper(name, dev, **kw)(wav, lens).cpu()
        want = torch.from_numpy(g[f"{name}_{tag}"])
        assert got.shape == want.shape
        err = float((got - want).abs().max())
        print(f"wav2vec2 {name} {tag}: max|d| {err:.3e}")
        assert err <= 5e-5
    err = float((wrapper(name, dev)(wav).cpu() - torch.from_numpy(g[f"{name}_nolens"])).abs().max())
    assert err <= 5e-5


def _asr(dev, yaml="hyperparams.yaml"):
    from speechbrain_amd.inference.ASR import EncoderASR

    return EncoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_wav2vec2_ctc_tiny"), hparams_file=yaml,
                                   overrides={"wav2vec2_hub": hub("group")}, run_opts={"device": str(dev)})


def _tokens(padded):
    return [[int(t) for t in row if t >= 0] for row in padded]


def test_from_hparams_wav2vec2_ctc_directory(backend):
    """A hyperparams.yaml in train_hf_wav2vec.yaml's layout: wav2vec2.ckpt / model.ckpt / tokenizer.ckpt written by the
    reference's savers load through the Pretrainer; log-probs 1e-4, greedy ids exact, beam-search text and transcribe_file equal."""
    nat, dev = backend
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2
    from speechbrain_amd.lobes.models.VanillaNN import VanillaNN
    from speechbrain_amd.nnet.activations import Softmax

    exp = np.load(os.path.join(GOLD, "pretrained_wav2vec2_ctc_tiny_expected.npz"))
    asr = _asr(dev)
    enc = asr.mods.encoder
    assert isinstance(enc.wav2vec2, Wav2Vec2) and isinstance(enc.enc, VanillaNN) and isinstance(enc.log_softmax, Softmax)
    model = torch.nn.ModuleList([enc.enc, enc.ctc_lin])
    assert [[k, list(v.shape)] for k, v in model.state_dict().items()] == json.loads(str(exp["model_keys"]))
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    logp = asr.encode_batch(wav, lens).cpu()
    err = float((logp - torch.from_numpy(exp["logp"])).abs().max())
    print(f"wav2vec2 CTC log-probs: max|d| {err:.3e}")
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


def test_native_log_softmax_replacement_still_works():
    """EncoderASR swaps torch.nn.LogSoftmax children; the recipe's Softmax(apply_log=True) is already on the kernel and stays."""
    from speechbrain_amd.nnet.activations import NativeLogSoftmax, Softmax

    seq = torch.nn.Sequential(torch.nn.LogSoftmax(dim=-1), Softmax(apply_log=True))
    assert NativeLogSoftmax.replace_in(seq) == 1
    assert isinstance(seq[0], NativeLogSoftmax) and isinstance(seq[1], Softmax)
    assert Softmax(apply_log=True).state_dict() == {}


def test_import_shim_resolves_the_yaml_class_paths():
    from speechbrain_amd.utils.hpyaml import load_hyperpyyaml

    text = ("a: !name:speechbrain.integrations.huggingface.wav2vec2.Wav2Vec2\n"
            "b: !name:speechbrain.lobes.models.VanillaNN.VanillaNN\n"
            "c: !new:speechbrain.nnet.activations.Softmax\n    apply_log: True\n")
    h = load_hyperpyyaml(text)
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2

    assert h["a"].func is Wav2Vec2 if hasattr(h["a"], "func") else h["a"] is Wav2Vec2


def _cfg(**over):
    with open(os.path.join(hub("group"), "config.json")) as f:
        return {**json.load(f), **over}


@pytest.mark.parametrize("over,word", [
    (dict(add_adapter=True), "add_adapter"),
    (dict(hidden_act="relu"), "hidden_act"),
    (dict(feat_extract_activation="relu"), "feat_extract_activation"),
    (dict(num_conv_pos_embedding_groups=1), "group width"),            # 96 channels in one group
    (dict(hidden_size=80, num_conv_pos_embedding_groups=5, num_attention_heads=4), "head dim"),  # cg 16, head dim 20
])
def test_unsupported_configs_raise_by_name(over, word):
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2

    with pytest.raises(NotImplementedError, match=word):
        Wav2Vec2.from_config(_cfg(**over))


def test_unsupported_wrappers_raise_by_name():
    from speechbrain_amd.integrations.huggingface.hubert import HuBERT
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2, Wav2Vec2Pretrain
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM

    with pytest.raises(NotImplementedError, match="output_attentions"):
        Wav2Vec2(hub("group"), None, output_attentions=True)
    with pytest.raises(NotImplementedError, match="Wav2Vec2Pretrain"):
        Wav2Vec2Pretrain(hub("group"), None)
    with pytest.raises(NotImplementedError, match="HuBERT"):
        HuBERT(hub("group"), None)
    with pytest.raises(NotImplementedError, match="WavLM"):
        WavLM(hub("group"), None)
