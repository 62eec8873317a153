"""Write the WavLM / HuBERT fixtures under tests/golden/ with the REFERENCE's own wrappers, savers and EncoderASR:

  wavlm_group_tiny/, wavlm_layer_tiny/     local HuggingFace directories (config.json, preprocessor_config.json, model.safetensors)
                                           of two random 2-layer WavLM models: the base / base-plus variant (group norm, post-norm;
                                           num_buckets 32, max_bucket_distance 12, so that the 18 frames of the inputs reach the
                                           exact, the logarithmic and the saturated buckets on both signs) and the large variant
                                           (layer norm, stable layer norm; the default 320 / 800 buckets)
  hubert_tiny/                             a random 2-layer HuBERT (group norm, feat_proj_layer_norm false)
  wavlm_model.npz                          inputs [3, 6000] with wav_lens, the reference wrappers' outputs (output_norm on / off,
                                           output_all_hiddens, no lengths), their state-dict key lists with shapes, the reference's
                                           fp32-vs-fp64 distance per case, and transformers' _relative_positions_bucket on
                                           [-2000, 2000] for both bucket settings
  pretrained_wavlm_ctc_tiny/               hyperparams.yaml in the layout of recipes/LibriSpeech/ASR/CTC/hparams/train_hf_wav2vec.yaml
                                           with the WavLM wrapper (as the downsampled/train_hf_wavlm_*.yaml recipes name it),
                                           wav2vec2.ckpt / model.ckpt / tokenizer.ckpt
  pretrained_wavlm_ctc_tiny_expected.npz   the reference EncoderASR's log-probs, greedy ids and beam-search text

HuggingFace initialises the relative-position embedding and the gate so that the bias barely moves the output; here
``rel_attn_embed`` is drawn at unit scale and ``gru_rel_pos_linear`` / ``gru_rel_pos_const`` are perturbed by O(0.3), and the
generator ASSERTS on the reference itself that zeroing the table, and mirroring it (r -> -r), each move the output by more than
100 x the tests' bound, and that the gates of the batch span at least 0.2: a wrong table or a constant gate cannot pass.

Runs only where the reference checkout (SB_REFERENCE, default: `reference` next to this repository) and ``transformers`` are
available, on the CPU, offline.  The weights are drawn in fp32, rounded to fp16-representable values and stored as fp16.

    python tools/make_wavlm_golden.py
"""
import functools
import json
import os
import shutil
import sys
import tempfile

os.environ.setdefault("HF_HUB_OFFLINE", "1")
os.environ.setdefault("TRANSFORMERS_OFFLINE", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SB_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_stubs"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_wav2vec2_golden as W2V  # noqa: E402  (the tiny sizes, the CTC directory's writer)

OUT = W2V.OUT
WRAPPER_BOUND = 5e-5  # tests/test_wavlm_model.py::test_golden_wrapper_outputs
COMMON, GROUP, LAYER = W2V.COMMON, W2V.VARIANTS["group"], W2V.VARIANTS["layer"]
# name -> (directory, model family, config, do_normalize, seed)
MODELS = {
    "group": ("wavlm_group_tiny", "wavlm", dict(GROUP, num_buckets=32, max_bucket_distance=12), False, 51),
    "layer": ("wavlm_layer_tiny", "wavlm", dict(LAYER), True, 52),
    "hubert": ("hubert_tiny", "hubert", dict(GROUP, feat_proj_layer_norm=False), False, 53),
}
BUCKETS = ((320, 800), (32, 12))


def make_hf_dir(name):
    from transformers import HubertConfig, HubertModel, Wav2Vec2FeatureExtractor, WavLMConfig, WavLMModel

    folder, family, cfg, do_normalize, seed = MODELS[name]
    path = os.path.join(OUT, folder)
    shutil.rmtree(path, ignore_errors=True)
    torch.manual_seed(seed)
    model = (WavLMModel(WavLMConfig(**COMMON, **cfg)) if family == "wavlm" else HubertModel(HubertConfig(**COMMON, **cfg))).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "rel_attn_embed" in n:  # unit scale: the bias is of the scores' size
                p.copy_(torch.randn(p.shape, generator=g))
            elif "gru_rel_pos" in n:   # O(0.3) around the initialisation: gates that differ between frames, heads and layers
                p.add_(0.3 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 or "norm" in n:  # random norm affines / biases, so that they are exercised
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            p.copy_(p.half().float())
    model.half().save_pretrained(path, safe_serialization=True)
    Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=do_normalize,
                             return_attention_mask=do_normalize).save_pretrained(path)
    keep = {"config.json", "preprocessor_config.json", "model.safetensors"}
    for f in os.listdir(path):
        if f not in keep:
            os.remove(os.path.join(path, f))
    return path


def ref_wrapper(name, path, **kw):
    from speechbrain.integrations.huggingface.hubert import HuBERT
    from speechbrain.integrations.huggingface.wavlm import WavLM

    cls = WavLM if MODELS[name][1] == "wavlm" else HuBERT
    w = cls(source=path, save_path=tempfile.mkdtemp(), freeze=True, **kw).float().eval()
    assert all(p.dtype == torch.float32 for p in w.parameters())
    return w


def sensitivity_promise(name, path, wav, lens):
    """On the reference: the table and its orientation matter by > 100 x the wrapper bound, and the gates are not a constant."""
    w = ref_wrapper(name, path)
    att0 = w.model.encoder.layers[0].attention
    gates = []

    def hook(mod, args, out, const):  # out: gru_rel_pos_linear(x) [B,H,T,8]
        ga, gb = torch.sigmoid(out.view(out.shape[:-1] + (2, 4)).sum(-1)).chunk(2, dim=-1)
        gates.append(ga * (gb * const - 1.0) + 2.0)

    hooks = [L.attention.gru_rel_pos_linear.register_forward_hook(functools.partial(hook, const=L.attention.gru_rel_pos_const))
             for L in w.model.encoder.layers]
    with torch.no_grad():
        base = w(wav, lens)
        for h in hooks:
            h.remove()
        keep = att0.rel_attn_embed.weight.clone()
        att0.rel_attn_embed.weight.zero_()
        zeroed = float((w(wav, lens) - base).abs().max())
        half = keep.shape[0] // 2  # bucket(r) = half * (r > 0) + f(|r|): r -> -r swaps the halves; r = 0 keeps bucket 0
        att0.rel_attn_embed.weight.copy_(torch.cat([keep[half:], keep[:half]]))
        att0.rel_attn_embed.weight[0] = keep[0]
        mirrored = float((w(wav, lens) - base).abs().max())
    span = min(float(g.max() - g.min()) for g in gates)
    print(f"  {name}: zeroed table moves the reference by {zeroed:.2e}, mirrored table by {mirrored:.2e}, gate span {span:.2f}")
    assert zeroed > 100 * WRAPPER_BOUND and mirrored > 100 * WRAPPER_BOUND, "the relative-position bias barely matters"
    assert span >= 0.2, "the gates are (almost) a constant"


def recorded_buckets():
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention

    out = {}
    r = torch.arange(-2000, 2001)
    for nb, md in BUCKETS:
        att = WavLMAttention(embed_dim=16, num_heads=2, num_buckets=nb, max_distance=md)
        out[f"buckets_{nb}_{md}"] = att._relative_positions_bucket(r).numpy().astype(np.int64)
    return out


def model_golden(paths):
    g = torch.Generator().manual_seed(41)
    wav = 0.3 * torch.randn(3, 6000, generator=g)
    lens = torch.tensor([1.0, 0.62, 0.4])
    for i in range(3):
        wav[i, int(round(float(lens[i]) * 6000)):] = 0
    out = dict(wav=wav.numpy(), lens=lens.numpy(), **recorded_buckets())
    for name, path in paths.items():
        with torch.no_grad():
            for tag, kw in (("plain", {}), ("norm", dict(output_norm=True)), ("all", dict(output_all_hiddens=True)),
                            ("all_norm", dict(output_all_hiddens=True, output_norm=True))):
                w = ref_wrapper(name, path, **kw)
                out[f"{name}_{tag}"] = w(wav, lens).numpy()
                y64 = w.double()(wav.double(), lens.double())
                dist = float((torch.from_numpy(out[f"{name}_{tag}"]).double() - y64).abs().max())
                out[f"{name}_{tag}_ref32v64"] = np.array(dist)
                print(f"  {name} {tag}: {tuple(out[f'{name}_{tag}'].shape)}, reference fp32 vs fp64 {dist:.2e}")
            out[f"{name}_nolens"] = ref_wrapper(name, path)(wav).numpy()
        sd = ref_wrapper(name, path).state_dict()
        out[f"{name}_keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))
        print(f"  {name}: {len(sd)} state-dict keys")
        if MODELS[name][1] == "wavlm":
            sensitivity_promise(name, path, wav, lens)
            T = out[f"{name}_plain"].shape[1]
            nb, md = MODELS[name][2].get("num_buckets", 320), MODELS[name][2].get("max_bucket_distance", 800)
            seen = sorted(set(out[f"buckets_{nb}_{md}"][2000 - (T - 1): 2000 + T].tolist()))
            print(f"  {name}: T' = {T}, buckets reached {seen}")
    np.savez_compressed(os.path.join(OUT, "wavlm_model.npz"), **out)


def ctc_yaml():
    """make_wav2vec2_golden's hyperparams.yaml with the WavLM wrapper (the downsampled/train_hf_wavlm_*.yaml recipes' spelling)."""
    y = W2V.CTC_YAML.replace("speechbrain.integrations.huggingface.wav2vec2.Wav2Vec2", "speechbrain.integrations.huggingface.wavlm.WavLM")
    y = y.replace("tests/golden/wav2vec2_group_tiny", "tests/golden/wavlm_group_tiny")
    y = y.replace("tools/make_wav2vec2_golden.py", "tools/make_wavlm_golden.py")
    assert "wavlm.WavLM" in y and "wavlm_group_tiny" in y
    return y


def main():
    paths = {name: make_hf_dir(name) for name in MODELS}
    for p in paths.values():
        for f in sorted(os.listdir(p)):
            print(f"  {os.path.basename(p)}/{f}: {os.path.getsize(os.path.join(p, f)) / 1024:.0f} KiB")
    model_golden(paths)
    W2V.pretrained_ctc_tiny(paths["group"], family="wavlm", wrapper=functools.partial(ref_wrapper, "group"), yaml=ctc_yaml(),
                            seeds=(27, 28))


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
