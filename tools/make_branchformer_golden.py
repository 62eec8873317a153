"""Write tests/golden/model_branchformer.npz and the Branchformer model directory tests/golden/pretrained_branchformer_tiny/
(with tests/golden/pretrained_branchformer_tiny_expected.npz) with the REFERENCE's own TransformerASR(encoder_module=
"branchformer"), searchers, savers and EncoderDecoderASR.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_branchformer_golden.py

model_branchformer.npz holds two tiny models.  "k7/": d 32, 4 heads, 2 encoder + 2 decoder layers, csgu_linear_units 48,
kernel 7; features [3,16,24] with relative lengths 0.6 / 0.8 / 1.0 (the shortest utterance is 6 frames short of the batch,
twice the halo: padded frames reach real ones through the reflect-padded convolution of the unmasked cgMLP branch); the state
dict, the output of every encoder layer, enc_out, and the reference's greedy and beam + CTC searches from enc_out.  "k31/":
kernel 31 at T' = 16, the smallest legal length (the reflection spans the whole sequence), encoder only.  Before anything is
written, tests/branchformer_host_ref.py (the plain-torch restatement the GPU tests compare against) is checked against the
reference on both.

The model directory has branchformer_large.yaml's structure at tiny sizes in the inference layout of pretrained_tiny (the
reference cannot parse YAML here -- oracle/ref_stubs/hyperpyyaml is an import stub -- so its EncoderDecoderASR is built
from modules wired exactly as the committed YAML describes); checkpoints are written by the reference's own savers, the
SentencePiece model is pretrained_tiny's.
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SB_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_stubs"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)
OUT = os.path.join(ROOT, "tests", "golden")
VOCAB, FEAT = 40, 24


def check(name, ref, got, tol):
    d = float((ref - got).abs().max())
    print(f"  {name:44s} max|d| = {d:.3e}  (tol {tol:g})")
    assert d <= tol, name


def pad_hyps(hyps):
    return np.array([h + [-1] * (64 - len(h)) for h in hyps], dtype=np.int64)


def randomise(mods, seed, sharpen):
    """Random LayerNorm affines and biases (default init is 1 / 0), a CSGU filter that filters (the reference draws it with
    std 1e-6), peaked output heads (EOS and non-trivial beams appear)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mods.named_parameters():
            if n.endswith("csgu.conv.conv.weight"):
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1 or "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for k in ("seq_lin", "ctc_lin"):
            if k in mods:
                mods[k].w.weight.mul_(sharpen)


def build_transformer(input_size, d_model, nhead, n_enc, n_dec, csgu_units, ksize):
    from speechbrain.lobes.models.transformer.TransformerASR import TransformerASR

    return TransformerASR(input_size=input_size, tgt_vocab=VOCAB, d_model=d_model, nhead=nhead, num_encoder_layers=n_enc,
                          num_decoder_layers=n_dec, d_ffn=64, dropout=0.1, activation=torch.nn.GELU,
                          branchformer_activation=torch.nn.GELU, encoder_module="branchformer",
                          csgu_linear_units=csgu_units, kernel_size=ksize, attention_type="RelPosMHAXL",
                          normalize_before=True, causal=False)


def encode_with_layers(tr, feats, wav_lens):
    outs = []
    hooks = [layer.register_forward_hook(lambda m, i, o: outs.append(o[0].detach().clone())) for layer in tr.encoder.layers]
    enc = tr.encode(feats, wav_lens)
    for h in hooks:
        h.remove()
    return enc, outs


def golden_model():
    import branchformer_host_ref as R
    from speechbrain.decoders import S2STransformerBeamSearcher, S2STransformerGreedySearcher
    from speechbrain.decoders.scorer import CTCScorer, ScorerBuilder
    from speechbrain.nnet.linear import Linear

    out = {}
    wav_lens = torch.tensor([0.6, 0.8, 1.0])
    for tag, ksize, n_dec, seed in (("k7", 7, 2, 11), ("k31", 31, 0, 12)):
        print(f"[model_branchformer {tag}]")
        torch.manual_seed(seed)
        mods = {"Transformer": build_transformer(FEAT, 32, 4, 2, n_dec, 48, ksize)}
        if n_dec:
            mods["seq_lin"], mods["ctc_lin"] = Linear(input_size=32, n_neurons=VOCAB), Linear(input_size=32, n_neurons=VOCAB)
        mods = torch.nn.ModuleDict(mods).eval()
        randomise(mods, seed + 1, 6.0)
        sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
        feats = torch.randn(3, 16, FEAT, generator=torch.Generator().manual_seed(4321 + seed))
        with torch.no_grad():
            enc_ref, layers_ref = encode_with_layers(mods["Transformer"], feats, wav_lens)
            enc_got, layers_got = R.encode(feats, wav_lens, sd, 32, 4, 2, "Transformer.", return_layers=True)
            check("host restatement, enc_out", enc_ref, enc_got, 1e-5)
            for l, (a, b) in enumerate(zip(layers_ref, layers_got)):
                check(f"host restatement, layer {l}", a, b, 1e-5)
            # the padded frames matter: the same utterance alone (no padded frames behind it) encodes differently
            n0 = int(round(0.6 * 16))
            if n0 > (ksize - 1) // 2:  # (kernel 31 cannot filter 10 frames at all)
                alone = mods["Transformer"].encode(feats[:1, :n0], torch.ones(1))
                gap = float((alone - enc_ref[:1, :n0]).abs().max())
                print(f"  utterance 0 alone vs inside the padded batch: max|d| = {gap:.3e}")
                assert gap > 1e-3
            out[f"{tag}/feats"], out[f"{tag}/wav_lens"], out[f"{tag}/enc_out"] = feats.numpy(), wav_lens.numpy(), enc_ref.numpy()
            for l, a in enumerate(layers_ref):
                out[f"{tag}/enc_layer{l}"] = a.numpy()
            if n_dec:
                gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                                  min_decode_ratio=0.0, max_decode_ratio=1.0)
                hyps, _, scores, _ = gs(enc_ref, wav_lens)
                print("  greedy hyps lens:", [len(h) for h in hyps])
                out[f"{tag}/greedy_hyps"], out[f"{tag}/greedy_scores"] = pad_hyps(hyps), scores.squeeze(1).numpy()
                scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                                       weights={"ctc": 0.4})
                bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                                min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=4,
                                                using_eos_threshold=False, length_normalization=True, scorer=scorer)
                hyps, lens, scores, _ = bs(enc_ref.clone(), wav_lens)
                print("  beam hyps lens:", [len(h) for h in hyps])
                out[f"{tag}/beam_hyps"], out[f"{tag}/beam_scores"], out[f"{tag}/beam_lens"] = pad_hyps(hyps), scores.numpy(), lens.numpy()
        out[f"{tag}/cfg"] = np.array([32, 4, 2, n_dec, 48, ksize, VOCAB, 4], dtype=np.int64)  # d, H, enc, dec, csgu, k, V, beam
        for k, v in sd.items():
            out[f"{tag}/sd/{k}"] = v.numpy()
    path = os.path.join(OUT, "model_branchformer.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


PRETRAINED_YAML = """\
# Layout of recipes/LibriSpeech/ASR/transformer/hparams/branchformer_large.yaml (inference form), tiny sizes.
sample_rate: 16000
n_fft: 400
n_mels: 80

d_model: 32
nhead: 4
num_encoder_layers: 2
num_decoder_layers: 2
d_ffn: 64  # (the decoder's; branchformer_large.yaml leaves it at the default 2048)
csgu_linear_units: 48
csgu_kernel_size: 7
transformer_dropout: 0.0
activation: !name:torch.nn.GELU
output_neurons: 40

blank_index: 0
bos_index: 1
eos_index: 2

min_decode_ratio: 0.0
max_decode_ratio: 1.0
valid_beam_size: 10
ctc_weight_decode: 0.40

CNN: !new:speechbrain.lobes.models.convolution.ConvolutionFrontEnd
    input_shape: (8, 10, 80)
    num_blocks: 2
    num_layers_per_block: 1
    out_channels: (64, 32)
    kernel_sizes: (3, 3)
    strides: (2, 2)
    residuals: (False, False)

Transformer: !new:speechbrain.lobes.models.transformer.TransformerASR.TransformerASR
    input_size: 640
    tgt_vocab: !ref <output_neurons>
    d_model: !ref <d_model>
    nhead: !ref <nhead>
    num_encoder_layers: !ref <num_encoder_layers>
    num_decoder_layers: !ref <num_decoder_layers>
    d_ffn: !ref <d_ffn>
    dropout: !ref <transformer_dropout>
    activation: !ref <activation>
    branchformer_activation: !ref <activation>
    encoder_module: branchformer
    csgu_linear_units: !ref <csgu_linear_units>
    kernel_size: !ref <csgu_kernel_size>
    attention_type: RelPosMHAXL
    normalize_before: True
    causal: False

ctc_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <d_model>
    n_neurons: !ref <output_neurons>

seq_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <d_model>
    n_neurons: !ref <output_neurons>

ctc_scorer: !new:speechbrain.decoders.scorer.CTCScorer
    eos_index: !ref <eos_index>
    blank_index: !ref <blank_index>
    ctc_fc: !ref <ctc_lin>

scorer: !new:speechbrain.decoders.scorer.ScorerBuilder
    full_scorers: [!ref <ctc_scorer>]
    weights:
        ctc: !ref <ctc_weight_decode>

decoder: !new:speechbrain.decoders.S2STransformerBeamSearcher
    modules: [!ref <Transformer>, !ref <seq_lin>]
    bos_index: !ref <bos_index>
    eos_index: !ref <eos_index>
    min_decode_ratio: !ref <min_decode_ratio>
    max_decode_ratio: !ref <max_decode_ratio>
    beam_size: !ref <valid_beam_size>
    using_eos_threshold: False
    length_normalization: True
    scorer: !ref <scorer>

log_softmax: !new:torch.nn.LogSoftmax
    dim: -1

normalizer: !new:speechbrain.processing.features.InputNormalization
    norm_type: global

compute_features: !new:speechbrain.lobes.features.Fbank
    sample_rate: !ref <sample_rate>
    n_fft: !ref <n_fft>
    n_mels: !ref <n_mels>

tokenizer: !new:sentencepiece.SentencePieceProcessor

Tencoder: !new:speechbrain.lobes.models.transformer.TransformerASR.EncoderWrapper
    transformer: !ref <Transformer>

encoder: !new:speechbrain.nnet.containers.LengthsCapableSequential
    input_shape: [null, null, !ref <n_mels>]
    compute_features: !ref <compute_features>
    normalize: !ref <normalizer>
    cnn: !ref <CNN>
    transformer_encoder: !ref <Tencoder>

asr_model: !new:torch.nn.ModuleList
    - [!ref <CNN>, !ref <Transformer>, !ref <seq_lin>, !ref <ctc_lin>]

modules:
    pre_transformer: !ref <CNN>
    transformer: !ref <Transformer>
    seq_lin: !ref <seq_lin>
    ctc_lin: !ref <ctc_lin>
    normalizer: !ref <normalizer>
    encoder: !ref <encoder>
    compute_features: !ref <compute_features>
    model: !ref <asr_model>
    decoder: !ref <decoder>

pretrainer: !new:speechbrain.utils.parameter_transfer.Pretrainer
    loadables:
        normalizer: !ref <normalizer>
        asr: !ref <asr_model>
        tokenizer: !ref <tokenizer>
"""


def golden_pretrained():
    import sentencepiece as spm
    from speechbrain.decoders import S2STransformerBeamSearcher
    from speechbrain.decoders.scorer import CTCScorer, ScorerBuilder
    from speechbrain.inference.ASR import EncoderDecoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.lobes.models.convolution import ConvolutionFrontEnd
    from speechbrain.lobes.models.transformer.TransformerASR import EncoderWrapper
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear
    from speechbrain.processing.features import InputNormalization

    print("[pretrained_branchformer_tiny]")
    out_dir = os.path.join(OUT, "pretrained_branchformer_tiny")
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(21)
    cnn = ConvolutionFrontEnd(input_shape=(8, 10, 80), num_blocks=2, num_layers_per_block=1, out_channels=(64, 32),
                              kernel_sizes=(3, 3), strides=(2, 2), residuals=(False, False))
    mods = torch.nn.ModuleDict({"CNN": cnn, "Transformer": build_transformer(640, 32, 4, 2, 2, 48, 7),
                                "seq_lin": Linear(input_size=32, n_neurons=VOCAB),
                                "ctc_lin": Linear(input_size=32, n_neurons=VOCAB)}).eval()
    randomise(mods, 22, 6.0)
    shutil.copyfile(os.path.join(OUT, "pretrained_tiny", "tokenizer.ckpt"), os.path.join(out_dir, "tokenizer.ckpt"))
    tok = spm.SentencePieceProcessor()
    tok.load(os.path.join(out_dir, "tokenizer.ckpt"))
    g = torch.Generator().manual_seed(23)
    norm = InputNormalization(norm_type="global")
    norm.glob_mean = -30.0 + 5.0 * torch.randn(80, generator=g)
    norm.glob_std = 8.0 + torch.rand(80, generator=g)
    norm.count = 1000
    norm._save(os.path.join(out_dir, "normalizer.ckpt"))
    asr_model = torch.nn.ModuleList([mods["CNN"], mods["Transformer"], mods["seq_lin"], mods["ctc_lin"]])
    torch.save(asr_model.state_dict(), os.path.join(out_dir, "asr.ckpt"))
    with open(os.path.join(out_dir, "hyperparams.yaml"), "w") as f:
        f.write(PRETRAINED_YAML)

    # the reference pipeline, wired exactly as the YAML describes
    encoder = LengthsCapableSequential(input_shape=[None, None, 80],
                                       compute_features=Fbank(sample_rate=16000, n_fft=400, n_mels=80), normalize=norm,
                                       cnn=mods["CNN"], transformer_encoder=EncoderWrapper(mods["Transformer"]))
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
    decoder = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                         min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=10,
                                         using_eos_threshold=False, length_normalization=True, scorer=scorer)
    asr = EncoderDecoderASR(modules={"encoder": encoder, "decoder": decoder, "transformer": mods["Transformer"]},
                            hparams={"tokenizer": tok}, run_opts={"device": "cpu"})
    wav = 0.1 * torch.randn(3, 12000, generator=g)
    lens = torch.tensor([1.0, 0.8, 0.55])
    for i in range(3):
        wav[i, int(lens[i] * 12000):] = 0
    with torch.no_grad():
        words_ref, tokens_ref = asr.transcribe_batch(wav, lens)
        enc_ref = asr.encode_batch(wav, lens)
    print("  enc_out", tuple(enc_ref.shape), "tokens:", [len(t) for t in tokens_ref], "words[0]:", repr(words_ref[0][:60]))
    np.savez_compressed(os.path.join(OUT, "pretrained_branchformer_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        enc_out=enc_ref.numpy(), tokens=pad_hyps(tokens_ref), words=np.array(words_ref))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    golden_model()
    golden_pretrained()
