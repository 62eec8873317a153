"""Write the wav2vec 2.0 fixtures under tests/golden/ with the REFERENCE's own wrapper, savers and EncoderASR:

  wav2vec2_group_tiny/, wav2vec2_layer_tiny/   local HuggingFace directories (config.json, preprocessor_config.json,
                                               model.safetensors) of two random 2-layer models: the wav2vec2-base variant
                                               (group norm, post-norm, no conv bias, do_normalize false) and the large-lv60 /
                                               xlsr variant (layer norm, stable layer norm, conv bias, do_normalize true)
  wav2vec2_model.npz                           inputs [3, 6000] with wav_lens, the reference wrapper's outputs (output_norm on /
                                               off, output_all_hiddens) and its state-dict key list with shapes
  pretrained_wav2vec2_ctc_tiny/                hyperparams.yaml in the layout of recipes/LibriSpeech/ASR/CTC/hparams/
                                               train_hf_wav2vec.yaml (wav2vec2 -> VanillaNN -> ctc_lin -> log-softmax),
                                               wav2vec2.ckpt / model.ckpt / tokenizer.ckpt
  pretrained_wav2vec2_ctc_tiny_expected.npz    the reference EncoderASR's log-probs, greedy ids and beam-search text

Runs only where the reference checkout (SB_REFERENCE, default: `reference` next to this repository) and ``transformers`` are available, on the CPU,
offline; it puts the reference and oracle/ref_stubs on sys.path the way tools/make_ctc_golden.py does.  The weights are drawn in
fp32 and rounded to fp16-representable values, and stored as fp16: the same numbers in half the bytes.

    python tools/make_wav2vec2_golden.py
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CHARS = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "-", "."]  # V = 31, as the CTC fixtures

COMMON = dict(conv_dim=[32] * 7, conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_kernel=[10, 3, 3, 3, 3, 2, 2], num_hidden_layers=2,
              hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, feat_proj_dropout=0.0, layerdrop=0.0,
              final_dropout=0.0, vocab_size=32)
VARIANTS = {
    "group": dict(hidden_size=96, num_attention_heads=3, intermediate_size=64, num_conv_pos_embeddings=32,
                  num_conv_pos_embedding_groups=2, feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False),
    "layer": dict(hidden_size=128, num_attention_heads=4, intermediate_size=64, num_conv_pos_embeddings=16,
                  num_conv_pos_embedding_groups=2, feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True),
}
DO_NORMALIZE = {"group": False, "layer": True}


def make_hf_dir(name, seed):
    from transformers import Wav2Vec2Config, Wav2Vec2FeatureExtractor, Wav2Vec2Model

    path = os.path.join(OUT, f"wav2vec2_{name}_tiny")
    shutil.rmtree(path, ignore_errors=True)
    torch.manual_seed(seed)
    model = Wav2Vec2Model(Wav2Vec2Config(**COMMON, **VARIANTS[name])).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in model.named_parameters():  # random norm affines / biases, so that they are exercised
            if p.dim() == 1 or "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            p.copy_(p.half().float())
    model.half().save_pretrained(path, safe_serialization=True)
    Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=DO_NORMALIZE[name],
                             return_attention_mask=DO_NORMALIZE[name]).save_pretrained(path)
    keep = {"config.json", "preprocessor_config.json", "model.safetensors"}
    for f in os.listdir(path):
        if f not in keep:
            os.remove(os.path.join(path, f))
    return path


def ref_wrapper(path, **kw):
    from speechbrain.integrations.huggingface.wav2vec2 import Wav2Vec2

    w = Wav2Vec2(source=path, save_path=tempfile.mkdtemp(), freeze=True, **kw).float().eval()
    assert all(p.dtype == torch.float32 for p in w.parameters())
    return w


def model_golden(paths):
    g = torch.Generator().manual_seed(41)
    wav = 0.3 * torch.randn(3, 6000, generator=g)
    lens = torch.tensor([1.0, 0.62, 0.4])
    for i in range(3):
        wav[i, int(round(float(lens[i]) * 6000)):] = 0
    out = dict(wav=wav.numpy(), lens=lens.numpy())
    for name, path in paths.items():
        with torch.no_grad():
            for tag, kw in (("plain", {}), ("norm", dict(output_norm=True)), ("all", dict(output_all_hiddens=True)),
                            ("all_norm", dict(output_all_hiddens=True, output_norm=True))):
                w = ref_wrapper(path, **kw)
                out[f"{name}_{tag}"] = w(wav, lens).numpy()
                y64 = w.double()(wav.double(), lens.double())
                print(f"  {name} {tag}: {tuple(out[f'{name}_{tag}'].shape)}, reference fp32 vs fp64 "
                      f"{float((torch.from_numpy(out[f'{name}_{tag}']).double() - y64).abs().max()):.2e}")
            out[f"{name}_nolens"] = ref_wrapper(path)(wav).numpy()
        sd = ref_wrapper(path).state_dict()
        out[f"{name}_keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))
        print(f"  {name}: {len(sd)} state-dict keys")
    np.savez_compressed(os.path.join(OUT, "wav2vec2_model.npz"), **out)


CTC_YAML = """# Layout of recipes/LibriSpeech/ASR/CTC/hparams/train_hf_wav2vec.yaml at tiny sizes, as an inference hyperparams.yaml for
# EncoderASR.  Written by tools/make_wav2vec2_golden.py.  wav2vec2_hub: a LOCAL HuggingFace directory (pass it in `overrides`).
wav2vec2_hub: tests/golden/wav2vec2_group_tiny
wav2vec2_folder: wav2vec2_checkpoint
sample_rate: 16000

activation: !name:torch.nn.LeakyReLU
dnn_layers: 2
dnn_neurons: 48
freeze_wav2vec: True
output_neurons: 31
blank_index: 0

enc: !new:speechbrain.lobes.models.VanillaNN.VanillaNN
    input_shape: [null, null, 96]
    activation: !ref <activation>
    dnn_blocks: !ref <dnn_layers>
    dnn_neurons: !ref <dnn_neurons>

wav2vec2: !new:speechbrain.integrations.huggingface.wav2vec2.Wav2Vec2
    source: !ref <wav2vec2_hub>
    output_norm: True
    freeze: !ref <freeze_wav2vec>
    save_path: !ref <wav2vec2_folder>

ctc_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <dnn_neurons>
    n_neurons: !ref <output_neurons>

log_softmax: !new:speechbrain.nnet.activations.Softmax
    apply_log: True

tokenizer: !new:speechbrain.dataio.encoder.CTCTextEncoder

encoder: !new:speechbrain.nnet.containers.LengthsCapableSequential
    wav2vec2: !ref <wav2vec2>
    enc: !ref <enc>
    ctc_lin: !ref <ctc_lin>
    log_softmax: !ref <log_softmax>

%DECODING%

modules:
    encoder: !ref <encoder>

model: !new:torch.nn.ModuleList
    - [!ref <enc>, !ref <ctc_lin>]

pretrainer: !new:speechbrain.utils.parameter_transfer.Pretrainer
    loadables:
        wav2vec2: !ref <wav2vec2>
        model: !ref <model>
        tokenizer: !ref <tokenizer>
"""
GREEDY_DECODING = """decoding_function: !name:speechbrain.decoders.ctc.ctc_greedy_decode
    blank_id: !ref <blank_index>"""
BEAM_SETTINGS = dict(beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2, prune_history=False)
BEAM_DECODING = """test_beam_search:
    blank_index: !ref <blank_index>
    beam_size: 100
    beam_prune_logp: -12.0
    token_prune_min_logp: -1.2
    prune_history: False

decoding_function: !name:speechbrain.decoders.ctc.CTCBeamSearcher"""


def pretrained_ctc_tiny(hub, family="wav2vec2", wrapper=None, yaml=CTC_YAML, seeds=(23, 24)):
    """pretrained_<family>_ctc_tiny/ and its _expected.npz around the reference wrapper ``wrapper(hub, output_norm=True)``
    (default: ``ref_wrapper``); ``seeds``: of the head's initialisation and of the batch's noise."""
    from speechbrain.dataio.encoder import CTCTextEncoder
    from speechbrain.decoders.ctc import CTCBeamSearcher, ctc_greedy_decode
    from speechbrain.inference.ASR import EncoderASR
    from speechbrain.lobes.models.VanillaNN import VanillaNN
    from speechbrain.nnet.activations import Softmax
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear

    out_dir = os.path.join(OUT, f"pretrained_{family}_ctc_tiny")
    shutil.rmtree(out_dir, ignore_errors=True)
    os.makedirs(out_dir)
    w2v = (wrapper or ref_wrapper)(hub, output_norm=True)
    torch.manual_seed(seeds[0])
    enc = VanillaNN(input_shape=[None, None, 96], activation=torch.nn.LeakyReLU, dnn_blocks=2, dnn_neurons=48)
    ctc_lin = Linear(input_size=48, n_neurons=31)
    model = torch.nn.ModuleList([enc, ctc_lin]).eval()
    import speechbrain.dataio.dataio as sbio

    sig = sbio.read_audio(os.path.join(OUT, "ref_spk1_snt1.wav"))
    g = torch.Generator().manual_seed(seeds[1])
    n = 12000
    wav = torch.zeros(3, n)
    lens = torch.tensor([1.0, 0.8, 0.55])
    for i in range(3):  # one ragged batch of three: shifted cuts of the recording over a little noise, zero padded
        m = int(round(float(lens[i]) * n))
        wav[i, :m] = sig[2000 * i: 2000 * i + m] + 0.01 * torch.randn(m, generator=g)
    tok = CTCTextEncoder()
    tok.update_from_iterable(CHARS[1:], sequence_input=False)
    tok.insert_blank(index=0)
    encoder = LengthsCapableSequential(wav2vec2=w2v, enc=enc, ctc_lin=ctc_lin, log_softmax=Softmax(apply_log=True))
    with torch.no_grad():
        for _, p in model.named_parameters():
            p.copy_(p.half().float())
        # a random head mostly reads the features' common direction (one label everywhere): project it out of the first
        # block's input, as training would, and scale the head so that the ids do not hinge on fp32 reassociation
        feats = w2v(torch.cat([wav, sig[None, :n]]))
        mu = feats.mean(dim=(0, 1))
        w0 = enc.linear.w.weight
        w0.sub_(torch.outer(w0 @ mu, mu) / mu.dot(mu))
        w0.mul_(3.0)
        for scale in (8.0, 2.0, 2.0, 2.0):
            ctc_lin.w.weight.mul_(scale)
            logp = torch.cat([encoder(sig[None]), encoder(wav).reshape(1, -1, 31)], dim=1)
            top2 = logp.topk(2, dim=-1).values
            margin = float((top2[..., 0] - top2[..., 1]).min())
            if margin >= 1e-3:
                break
        for _, p in model.named_parameters():
            p.copy_(p.half().float())
    half = lambda sd: {k: v.half() for k, v in sd.items()}  # noqa: E731  (exact: every value is fp16-representable)
    torch.save(half(w2v.state_dict()), os.path.join(out_dir, "wav2vec2.ckpt"))
    torch.save(half(model.state_dict()), os.path.join(out_dir, "model.ckpt"))
    tok.save(os.path.join(out_dir, "tokenizer.ckpt"))
    for name, dec in (("hyperparams.yaml", GREEDY_DECODING), ("hyperparams_beam.yaml", BEAM_DECODING)):
        with open(os.path.join(out_dir, name), "w", encoding="utf-8") as f:
            f.write(yaml.replace("%DECODING%", dec))

    greedy = EncoderASR(modules={"encoder": encoder}, hparams={
        "tokenizer": tok, "decoding_function": functools.partial(ctc_greedy_decode, blank_id=0)}, run_opts={"device": "cpu"})
    beam = EncoderASR(modules={"encoder": encoder}, hparams={
        "tokenizer": tok, "decoding_function": CTCBeamSearcher, "test_beam_search": dict(blank_index=0, **BEAM_SETTINGS)},
        run_opts={"device": "cpu"})
    one = torch.ones(1)
    with torch.no_grad():
        logp = greedy.encode_batch(wav, lens)
        file_logp = greedy.encode_batch(sig[None], one)
        # the generator's promise: the reference's top-1 / top-2 margin on every valid frame, so that exact ids are a fair demand
        # (EncoderASR hands the container no lengths -- the wrapper's argument is `wav_lens`, not `lengths` -- so every frame counts)
        for lp in (logp, file_logp):
            top2 = lp.topk(2, dim=-1).values
            margin = float((top2[..., 0] - top2[..., 1]).min())
            assert margin >= 1e-3, f"top-1/top-2 log-prob margin {margin:.2e} < 1e-3"
        g_words, g_tokens = greedy.transcribe_batch(wav, lens)
        b_words, b_hyps = beam.transcribe_batch(wav, lens)
        f_words, f_tokens = greedy.transcribe_batch(sig[None], one)
        fb_words, _ = beam.transcribe_batch(sig[None], one)
        g_file = greedy.transcribe_file(os.path.join(OUT, "ref_spk1_snt1.wav"))
        b_file = beam.transcribe_file(os.path.join(OUT, "ref_spk1_snt1.wav"))
    print("  margin", margin)
    print("  greedy:", g_words, [g_file])
    print("  beam:  ", b_words, [b_file])
    assert len(set(t for ts in g_tokens + f_tokens for t in ts)) > 3, "the head emits (almost) one label"
    pad = lambda toks, T: np.array([t + [-1] * (T - len(t)) for t in toks], dtype=np.int64)  # noqa: E731
    model_keys = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    print("  model.ckpt keys:", [k for k, _ in model_keys])
    np.savez_compressed(os.path.join(OUT, f"pretrained_{family}_ctc_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        logp=logp.numpy(), greedy_words=np.array(g_words), greedy_tokens=pad(g_tokens, logp.shape[1]),
                        beam_words=np.array(b_words), file_logp=file_logp.numpy(), file_greedy_words=np.array(f_words),
                        file_greedy_tokens=pad(f_tokens, file_logp.shape[1]), file_beam_words=np.array(fb_words),
                        greedy_file_words=np.array([g_file]), beam_file_words=np.array([b_file]),
                        model_keys=np.array(json.dumps(model_keys)))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


def main():
    paths = {name: make_hf_dir(name, seed) for name, seed in (("group", 31), ("layer", 32))}
    for p in paths.values():
        for f in sorted(os.listdir(p)):
            print(f"  {os.path.basename(p)}/{f}: {os.path.getsize(os.path.join(p, f)) / 1024:.0f} KiB")
    model_golden(paths)
    pretrained_ctc_tiny(paths["group"])


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
