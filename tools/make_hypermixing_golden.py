"""Write tests/golden/model_hyperconformer.npz and the HyperConformer model directory tests/golden/pretrained_hyperconformer_tiny/
(with tests/golden/pretrained_hyperconformer_tiny_expected.npz) with the REFERENCE's own TransformerASR(encoder_module=
"conformer", attention_type="hypermixing"), searchers, savers and EncoderDecoderASR.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_hypermixing_golden.py

model_hyperconformer.npz: d 32, 4 heads, d_ffn 64 (head width 8, hypernet width per head 16), kernel 7, 2 encoder + 2 decoder
layers, vocabulary 40; features [3,16,24] with relative lengths 0.6 / 0.8 / 1.0; the state dict WITHOUT the per-layer
``positional_encoding.pe`` buffers (3000 x d each, a pure function of the sizes: rows 0-15 and 2999 of one are recorded instead),
the output of every encoder layer, enc_out, and the reference's greedy and beam 4 + CTC 0.4 searches from enc_out.  Before
anything is written, tests/hypermixing_host_ref.py (the plain-torch restatement the kernel tests compare against) is checked
against the reference layer by layer at 1e-5, and the reference's own fp64 run must give the token ids of its fp32 run (the
seed is advanced until it does, so that the exact-id tests are not decided by rounding).

The model directory has hyperconformer_22M.yaml's structure at tiny sizes in the inference layout of pretrained_tiny (the
reference cannot parse YAML here -- oracle/ref_stubs/hyperpyyaml is an import stub -- so its EncoderDecoderASR is built from
modules wired exactly as the committed YAML describes); ONE encoder layer, so that the checkpoint -- which, written by the
reference's savers, does carry the mixer's 3000-row table -- stays under 1 MiB (max_length 500 for the decoder's table too); the SentencePiece model is pretrained_tiny's.
"""
import copy
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
VOCAB, FEAT, D, H, DFFN, KSIZE = 40, 24, 32, 4, 64, 7


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
            if (p.dim() == 1 or "norm" in n) and "hyper." not in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        for k in ("seq_lin", "ctc_lin"):
            if k in mods:
                mods[k].w.weight.mul_(sharpen)


def build_transformer(input_size, n_enc, n_dec, max_length=2500):
    from speechbrain.lobes.models.transformer.TransformerASR import TransformerASR

    return TransformerASR(input_size=input_size, tgt_vocab=VOCAB, d_model=D, nhead=H, num_encoder_layers=n_enc,
                          num_decoder_layers=n_dec, d_ffn=DFFN, dropout=0.1, activation=torch.nn.GELU,
                          encoder_module="conformer", attention_type="hypermixing", kernel_size=KSIZE, normalize_before=True,
                          causal=False, max_length=max_length)


def encode_with_layers(tr, feats, wav_lens):
    outs = []
    hooks = [layer.register_forward_hook(lambda m, i, o: outs.append(o[0].detach().clone())) for layer in tr.encoder.layers]
    enc = tr.encode(feats, wav_lens)
    for h in hooks:
        h.remove()
    return enc, outs


def searches(mods, enc, wav_lens):
    from speechbrain.decoders import S2STransformerBeamSearcher, S2STransformerGreedySearcher
    from speechbrain.decoders.scorer import CTCScorer, ScorerBuilder

    gs = S2STransformerGreedySearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                      min_decode_ratio=0.0, max_decode_ratio=1.0)
    ghyps, _, gscores, _ = gs(enc, wav_lens)
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                    min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=4, using_eos_threshold=False,
                                    length_normalization=True, scorer=scorer)
    bhyps, blens, bscores, _ = bs(enc.clone(), wav_lens)
    return ghyps, gscores, bhyps, blens, bscores


def golden_model():
    import hypermixing_host_ref as R
    from speechbrain.nnet.linear import Linear

    wav_lens = torch.tensor([0.6, 0.8, 1.0])
    for seed in range(11, 40):
        print(f"[model_hyperconformer, seed {seed}]")
        torch.manual_seed(seed)
        mods = torch.nn.ModuleDict({"Transformer": build_transformer(FEAT, 2, 2), "seq_lin": Linear(input_size=D, n_neurons=VOCAB),
                                    "ctc_lin": Linear(input_size=D, n_neurons=VOCAB)}).eval()
        randomise(mods, seed + 1, 6.0)
        feats = torch.randn(3, 16, FEAT, generator=torch.Generator().manual_seed(4321 + seed))
        with torch.no_grad():
            enc_ref, layers_ref = encode_with_layers(mods["Transformer"], feats, wav_lens)
            ghyps, gscores, bhyps, blens, bscores = searches(mods, enc_ref, wav_lens)
            mods64 = copy.deepcopy(mods).double()
            # the reference's tables are made in the default dtype; its look-ahead mask is cast to fp32 by name
            import speechbrain.lobes.models.transformer.TransformerASR as ref_asr

            lookahead = ref_asr.get_lookahead_mask
            ref_asr.get_lookahead_mask = lambda t: lookahead(t).double()
            torch.set_default_dtype(torch.float64)
            try:
                enc64 = mods64["Transformer"].encode(feats.double(), wav_lens.double())
                g64, _, b64, _, _ = searches(mods64, enc64, wav_lens.double())
            finally:
                torch.set_default_dtype(torch.float32)
                ref_asr.get_lookahead_mask = lookahead
        print("  greedy hyps lens:", [len(h) for h in ghyps], " beam hyps lens:", [len(h) for h in bhyps])
        if g64 == ghyps and b64 == bhyps and all(len(h) > 1 for h in bhyps):
            break
        print("  the fp64 run of the reference gives other token ids (or an empty hypothesis): next seed")
    else:
        raise SystemExit("no seed found")
    sd = {k: v.detach().clone() for k, v in mods.state_dict().items()}
    pe_keys = [k for k in sd if k.endswith("positional_encoding.pe") and ".mha_layer." in k]
    assert len(pe_keys) == 2 and all(torch.equal(sd[k], sd[pe_keys[0]]) for k in pe_keys)
    with torch.no_grad():
        enc_got, layers_got = R.encode(feats, wav_lens, sd, H, 2, KSIZE, "Transformer.", return_layers=True)
    check("host restatement, enc_out", enc_ref, enc_got, 1e-5)
    for l, (a, b) in enumerate(zip(layers_ref, layers_got)):
        check(f"host restatement, layer {l}", a, b, 1e-5)
    check("the reference in fp64, enc_out", enc_ref.double(), enc64, 1e-5)
    out = {"feats": feats.numpy(), "wav_lens": wav_lens.numpy(), "enc_out": enc_ref.numpy(),
           "greedy_hyps": pad_hyps(ghyps), "greedy_scores": gscores.squeeze(1).numpy(), "beam_hyps": pad_hyps(bhyps),
           "beam_scores": bscores.numpy(), "beam_lens": blens.numpy(),
           "cfg": np.array([D, H, 2, 2, DFFN, KSIZE, VOCAB, 4], dtype=np.int64),  # d, H, enc, dec, d_ffn, k, V, beam
           "pe_rows": np.array(list(range(16)) + [2999], dtype=np.int64),
           "pe_values": sd[pe_keys[0]][0, list(range(16)) + [2999]].numpy(), "pe_shape": np.array(sd[pe_keys[0]].shape)}
    for l, a in enumerate(layers_ref):
        out[f"enc_layer{l}"] = a.numpy()
    for k, v in sd.items():
        if k not in pe_keys:
            out[f"sd/{k}"] = v.numpy()
    path = os.path.join(OUT, "model_hyperconformer.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


PRETRAINED_YAML = """\
# Layout of recipes/LibriSpeech/ASR/transformer/hparams/hyperconformer_22M.yaml (inference form), tiny sizes.
sample_rate: 16000
n_fft: 400
n_mels: 80

d_model: 32
nhead: 4
num_encoder_layers: 1
num_decoder_layers: 2
d_ffn: 64
transformer_dropout: 0.0
activation: !name:torch.nn.GELU
encoder_module: conformer
attention_type: hypermixing
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
    encoder_module: !ref <encoder_module>
    attention_type: !ref <attention_type>
    kernel_size: 7
    max_length: 500  # (the decoder's position table; the recipe leaves the default 2500 -- kept short so that the checkpoint is small)
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

    print("[pretrained_hyperconformer_tiny]")
    out_dir = os.path.join(OUT, "pretrained_hyperconformer_tiny")
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(31)
    cnn = ConvolutionFrontEnd(input_shape=(8, 10, 80), num_blocks=2, num_layers_per_block=1, out_channels=(64, 32),
                              kernel_sizes=(3, 3), strides=(2, 2), residuals=(False, False))
    mods = torch.nn.ModuleDict({"CNN": cnn, "Transformer": build_transformer(640, 1, 2, max_length=500),
                                "seq_lin": Linear(input_size=D, n_neurons=VOCAB),
                                "ctc_lin": Linear(input_size=D, n_neurons=VOCAB)}).eval()
    randomise(mods, 32, 6.0)
    shutil.copyfile(os.path.join(OUT, "pretrained_tiny", "tokenizer.ckpt"), os.path.join(out_dir, "tokenizer.ckpt"))
    tok = spm.SentencePieceProcessor()
    tok.load(os.path.join(out_dir, "tokenizer.ckpt"))
    g = torch.Generator().manual_seed(33)
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
    np.savez_compressed(os.path.join(OUT, "pretrained_hyperconformer_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        enc_out=enc_ref.numpy(), tokens=pad_hyps(tokens_ref), words=np.array(words_ref))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    golden_model()
    golden_pretrained()
