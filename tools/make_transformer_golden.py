"""Write tests/golden/model_transformer.npz and the Transformer-encoder model directory tests/golden/pretrained_transformer_tiny/
(with tests/golden/pretrained_transformer_tiny_expected.npz) with the REFERENCE's own TransformerASR(encoder_module=
"transformer", attention_type="regularMHA"), ConvolutionFrontEnd, searchers, savers and EncoderDecoderASR.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_transformer_golden.py

model_transformer.npz holds two tiny models.  "h4/": d 32, 4 heads (head dim 8), 2 encoder + 2 decoder layers, d_ffn 64, vocab
40; features [3,61,24] with relative lengths 0.6 / 0.8 / 1.0 through transformer.yaml's three-block front end (kernel sizes 5, 5,
1; strides 2, 2, 1; residuals F, F, T; 8 channels): every conv block's output, every encoder layer's output, enc_out, the
reference's greedy and beam-4 + CTC 0.4 searches, the state-dict key list, the front end's filter properties.  "dh128/": d 256, 2
heads (head dim 128), 1 + 1 layers, features [3,40,24] straight into custom_src_module: enc_out, greedy and beam-4 searches; its
state dict (3.5 MB) is not stored: the parameters are drawn from the recorded seed by transformer_host_ref.seeded_state_dict,
which the tests call again.

Before anything is written the generator asserts
  * tests/transformer_host_ref.py (the plain-torch restatement the GPU tests compare against) is within 1e-5 of the reference on
    every recorded tensor;
  * the recorded searches are decided by margins > 1e-3, so that equality of ids is a fair demand: at every step of the greedy
    hypotheses the chosen token leads the runner-up by more than 1e-3 in log-probability (the reference's decoder, teacher-forced
    on its own hypothesis), and the best beam hypothesis leads the second best by more than 1e-3 in final score -- another seed is
    tried when not;
  * utterance 0 encoded alone (its own frames of the front end's output) differs from its rows in the padded batch by less than
    1e-5: key masking is what the model relies on.

The model directory has transformer.yaml's structure at tiny sizes in the inference layout of pretrained_tiny (the reference
cannot parse YAML here -- oracle/ref_stubs/hyperpyyaml is an import stub -- so its EncoderDecoderASR is built from modules wired
exactly as the committed YAML describes); checkpoints are written by the reference's own savers, the SentencePiece model is
pretrained_tiny's.
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
CNN_KW = dict(num_blocks=3, num_layers_per_block=1, kernel_sizes=(5, 5, 1), strides=(2, 2, 1), residuals=(False, False, True))


def check(name, ref, got, tol):
    d = float((ref - got).abs().max())
    print(f"  {name:44s} max|d| = {d:.3e}  (tol {tol:g})")
    assert d <= tol, name


def pad_hyps(hyps):
    return np.array([h + [-1] * (64 - len(h)) for h in hyps], dtype=np.int64)


def randomise(mods, seed, sharpen):
    """Random LayerNorm affines and biases (default init is 1 / 0), peaked output heads (EOS and non-trivial beams appear)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in mods.named_parameters():
            if p.dim() == 1 or "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for k in ("seq_lin", "ctc_lin"):
            if k in mods:
                mods[k].w.weight.mul_(sharpen)


def build_transformer(input_size, d_model, nhead, n_enc, n_dec):
    from speechbrain.lobes.models.transformer.TransformerASR import TransformerASR

    return TransformerASR(input_size=input_size, tgt_vocab=VOCAB, d_model=d_model, nhead=nhead, num_encoder_layers=n_enc,
                          num_decoder_layers=n_dec, d_ffn=64, dropout=0.1, activation=torch.nn.GELU,
                          encoder_module="transformer", attention_type="regularMHA", normalize_before=True, causal=False)


def build_cnn(input_shape, channels):
    from speechbrain.lobes.models.convolution import ConvolutionFrontEnd

    return ConvolutionFrontEnd(input_shape=input_shape, out_channels=(channels,) * 3, **CNN_KW)


def run_with_outputs(modules, fn):
    """fn() with the output of every module in ``modules`` recorded (tuples: their first element)."""
    outs = []
    hooks = [m.register_forward_hook(lambda m, i, o: outs.append((o[0] if isinstance(o, tuple) else o).detach().clone()))
             for m in modules]
    res = fn()
    for h in hooks:
        h.remove()
    return res, outs


def greedy_margin(tr, seq_lin, enc, wav_lens, hyps):
    """Smallest lead of the chosen token over the runner-up along the greedy hypotheses (teacher-forced reference decoder)."""
    worst = float("inf")
    for b, hyp in enumerate(hyps):
        n = int(round(float(wav_lens[b]) * enc.shape[1]))
        toks = torch.tensor([[1] + list(hyp)])
        pred, _ = tr.decode(toks, enc[b: b + 1, :n], None)
        lp = torch.log_softmax(seq_lin(pred), dim=-1)[0]
        for step, want in enumerate(list(hyp) + [2]):
            if step >= lp.shape[0]:
                break
            top = torch.topk(lp[step], 2)
            if int(top.indices[0]) != want:  # (a hypothesis cut by max_decode_ratio ends without EOS)
                continue
            worst = min(worst, float(top.values[0] - top.values[1]))
    return worst


def golden_model():
    import transformer_host_ref as R
    from speechbrain.decoders import S2STransformerBeamSearcher, S2STransformerGreedySearcher
    from speechbrain.decoders.scorer import CTCScorer, ScorerBuilder
    from speechbrain.nnet.linear import Linear

    out = {}
    wav_lens = torch.tensor([0.6, 0.8, 1.0])
    for tag, d, H, n_lay, T, with_cnn, ctc_w, seeds in (("h4", 32, 4, 2, 61, True, 0.4, range(11, 40)),
                                                        ("dh128", 256, 2, 1, 40, False, 0.0, range(51, 80))):
        for seed in seeds:
            print(f"[model_transformer {tag}] seed {seed}")
            torch.manual_seed(seed)
            feats = torch.randn(3, T, FEAT, generator=torch.Generator().manual_seed(4321 + seed))
            mods = {}
            if with_cnn:
                mods["CNN"] = build_cnn(tuple(feats.shape), 8)
            in_size = 6 * 8 if with_cnn else FEAT
            mods["Transformer"] = build_transformer(in_size, d, H, n_lay, n_lay)
            mods["seq_lin"], mods["ctc_lin"] = Linear(input_size=d, n_neurons=VOCAB), Linear(input_size=d, n_neurons=VOCAB)
            mods = torch.nn.ModuleDict(mods).eval()
            rec = {}
            if with_cnn:
                randomise(mods, seed + 1, 6.0)
            else:  # a state dict too large to commit: parameters drawn from the seed, rebuilt by the tests
                shapes = {k: tuple(v.shape) for k, v in mods.named_parameters()}
                mods.load_state_dict(R.seeded_state_dict(shapes, seed), strict=False)
                rec["param_names"] = np.array(sorted(shapes))
                rec["param_shapes"] = np.array([list(shapes[k]) + [0] * (2 - len(shapes[k])) for k in sorted(shapes)], dtype=np.int64)
            tr = mods["Transformer"]
            sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
            with torch.no_grad():
                src = feats
                if with_cnn:
                    src, blocks = run_with_outputs(list(mods["CNN"].children()), lambda: mods["CNN"](feats))
                    _, blocks_got = R.conv_frontend(feats, sd, "CNN.", return_blocks=True)
                    for i, (a, b) in enumerate(zip(blocks, blocks_got)):
                        check(f"host restatement, conv block {i}", a, b, 1e-5)
                        rec[f"cnn_block{i}"] = a.numpy()
                    rec["cnn_out"] = src.numpy()
                    fp = mods["CNN"].get_filter_properties()
                    rec["cnn_filter_properties"] = np.array([fp.window_size, fp.stride, fp.dilation], dtype=np.int64)
                    rec["cnn_channels"] = np.array(8, dtype=np.int64)
                enc_ref, layers_ref = run_with_outputs(list(tr.encoder.layers), lambda: tr.encode(src, wav_lens))
                enc_got, layers_got = R.encode(src, wav_lens, sd, "Transformer.", H, n_lay, return_layers=True)
                check("host restatement, enc_out", enc_ref, enc_got, 1e-5)
                for l, (a, b) in enumerate(zip(layers_ref, layers_got)):
                    check(f"host restatement, layer {l}", a, b, 1e-5)
                    rec[f"enc_layer{l}"] = a.numpy()
                # key masking is all that separates an utterance from its padding
                n0 = int(round(0.6 * src.shape[1]))
                alone = tr.encode(src[:1, :n0], torch.ones(1))
                check("utterance 0 alone vs inside the padded batch", alone, enc_ref[:1, :n0], 1e-5)
                rec["feats"], rec["wav_lens"], rec["enc_out"] = feats.numpy(), wav_lens.numpy(), enc_ref.numpy()
                gs = S2STransformerGreedySearcher(modules=[tr, mods["seq_lin"]], bos_index=1, eos_index=2,
                                                  min_decode_ratio=0.0, max_decode_ratio=1.0)
                hyps, _, scores, _ = gs(enc_ref, wav_lens)
                margin = greedy_margin(tr, mods["seq_lin"], enc_ref, wav_lens, hyps)
                print("  greedy hyps lens:", [len(h) for h in hyps], f"smallest step margin {margin:.3e}")
                rec["greedy_hyps"], rec["greedy_scores"] = pad_hyps(hyps), scores.squeeze(1).numpy()
                kw = dict(modules=[tr, mods["seq_lin"]], bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0,
                          beam_size=4, using_eos_threshold=False, length_normalization=True)

                def scorer():
                    if ctc_w == 0.0:
                        return None
                    return ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)],
                                         weights={"ctc": ctc_w})

                hyps, lens, scores, _ = S2STransformerBeamSearcher(scorer=scorer(), **kw)(enc_ref.clone(), wav_lens)
                _, _, top2, _ = S2STransformerBeamSearcher(scorer=scorer(), topk=2, return_topk=True, **kw)(enc_ref.clone(), wav_lens)
                top2 = top2.view(3, 2)
                beam_margin = float((top2[:, 0] - top2[:, 1]).min())
                print("  beam hyps lens:", [len(h) for h in hyps], f"best vs second hypothesis {beam_margin:.3e}")
                rec["beam_hyps"], rec["beam_scores"], rec["beam_lens"] = pad_hyps(hyps), scores.numpy(), lens.numpy()
            if margin > 1e-3 and beam_margin > 1e-3 and min(len(h) for h in hyps) > 0 and rec["greedy_hyps"][:, 0].min() >= 0:
                break
            print("  margins too small (or an empty hypothesis) for this seed: trying the next")
        else:
            raise AssertionError(f"{tag}: no seed with search margins > 1e-3")
        rec["cfg"] = np.array([d, H, n_lay, n_lay, 64, VOCAB, 4, seed], dtype=np.int64)  # d, H, enc, dec, d_ffn, V, beam, seed
        rec["ctc_weight"] = np.array(ctc_w, dtype=np.float32)
        rec["sd_keys"] = np.array(sorted(sd))
        for k, v in rec.items():
            out[f"{tag}/{k}"] = v
        if with_cnn:
            for k, v in sd.items():
                out[f"{tag}/sd/{k}"] = v.numpy()
    path = os.path.join(OUT, "model_transformer.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")
    assert os.path.getsize(path) < 1024 * 1024


PRETRAINED_YAML = """\
# Layout of recipes/LibriSpeech/ASR/transformer/hparams/transformer.yaml (inference form), tiny sizes.
sample_rate: 16000
n_fft: 400
n_mels: 80

d_model: 32
nhead: 4
num_encoder_layers: 2
num_decoder_layers: 2
d_ffn: 64
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
    num_blocks: 3
    num_layers_per_block: 1
    out_channels: (8, 8, 8)
    kernel_sizes: (5, 5, 1)
    strides: (2, 2, 1)
    residuals: (False, False, True)

Transformer: !new:speechbrain.lobes.models.transformer.TransformerASR.TransformerASR
    input_size: 160
    tgt_vocab: !ref <output_neurons>
    d_model: !ref <d_model>
    nhead: !ref <nhead>
    num_encoder_layers: !ref <num_encoder_layers>
    num_decoder_layers: !ref <num_decoder_layers>
    d_ffn: !ref <d_ffn>
    dropout: !ref <transformer_dropout>
    activation: !ref <activation>
    encoder_module: transformer
    attention_type: regularMHA
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
    from speechbrain.lobes.models.transformer.TransformerASR import EncoderWrapper
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear
    from speechbrain.processing.features import InputNormalization

    print("[pretrained_transformer_tiny]")
    out_dir = os.path.join(OUT, "pretrained_transformer_tiny")
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(21)
    cnn = build_cnn((8, 10, 80), 8)
    mods = torch.nn.ModuleDict({"CNN": cnn, "Transformer": build_transformer(160, 32, 4, 2, 2),
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
    np.savez_compressed(os.path.join(OUT, "pretrained_transformer_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        enc_out=enc_ref.numpy(), tokens=pad_hyps(tokens_ref), words=np.array(words_ref))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    golden_model()
    golden_pretrained()
