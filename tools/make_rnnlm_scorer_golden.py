"""Write tests/golden/s2s_rnnlm.npz and the model directory tests/golden/pretrained_rnnlm_tiny/ with the REFERENCE's own
S2STransformerBeamSearcher, RNNLMScorer (score + permute_mem on the LM's carried state), CTCScorer, RNNLM, savers and
EncoderDecoderASR on the CPU.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_rnnlm_scorer_golden.py

One tiny Transformer ASR (conformer encoder, d_model 16) and one tiny RNNLM (embedding 6, 2 x 13 LSTM, one DNN block of 9) serve
the four configurations of CONFIGS -- beam 4 and 10, full_scorers [rnnlm] and [rnnlm, ctc] -- and the model directory, whose
hyperparams.yaml describes the configuration DIRECTORY; the weights live in the directory's asr.ckpt / lm.ckpt only, the npz holds
the wavs, the encoder states and, per configuration, the reference's ids, lengths, scores and d = the distance of its fp32 scores
from its fp64 run.  A seed is kept only if, for all four configurations, the reference's fp64 run returns the same ids and at every
step of every utterance the fp64 gap between the last kept and the first dropped candidate is at least MIN_GAP; the seed is
advanced until one passes.  The tokenizer is pretrained_tiny's SentencePiece model."""
import copy
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SB_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_stubs"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(8)
OUT = os.path.join(ROOT, "tests", "golden")
MIN_GAP = 1e-3
V, D_MODEL, LM_W, LM_T, TEMP, CTC_W = 40, 16, 0.5, 1.25, 1.15, 0.4
CONFIGS = {"beam4": (4, 0.0), "beam10": (10, 0.0), "beam4_ctc": (4, CTC_W), "beam10_ctc": (10, CTC_W)}
DIRECTORY = "beam10_ctc"

YAML = """# A Transformer ASR with RNNLM shallow fusion (the reference's rnnlm_scorer + ctc_scorer pairing) at tiny sizes, as an inference
# hyperparams.yaml for EncoderDecoderASR.  Written by tools/make_rnnlm_scorer_golden.py.
sample_rate: 16000
n_fft: 400
n_mels: 80
d_model: 16
output_neurons: 40
blank_index: 0
bos_index: 1
eos_index: 2
lm_weight: 0.5
ctc_weight_decode: 0.4

CNN: !new:speechbrain.lobes.models.convolution.ConvolutionFrontEnd
    input_shape: (8, 10, 80)
    num_blocks: 2
    num_layers_per_block: 1
    out_channels: (8, 4)
    kernel_sizes: (3, 3)
    strides: (2, 2)
    residuals: (False, False)

Transformer: !new:speechbrain.lobes.models.transformer.TransformerASR.TransformerASR
    input_size: 80
    tgt_vocab: !ref <output_neurons>
    d_model: !ref <d_model>
    nhead: 2
    num_encoder_layers: 1
    num_decoder_layers: 1
    d_ffn: 32
    dropout: 0.0
    activation: !name:torch.nn.GELU
    encoder_module: conformer
    attention_type: RelPosMHAXL
    normalize_before: True
    causal: False

ctc_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <d_model>
    n_neurons: !ref <output_neurons>

seq_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <d_model>
    n_neurons: !ref <output_neurons>

lm_model: !new:speechbrain.lobes.models.RNNLM.RNNLM
    output_neurons: !ref <output_neurons>
    embedding_dim: 6
    activation: !name:torch.nn.LeakyReLU
    dropout: 0.0
    rnn_layers: 2
    rnn_neurons: 13
    dnn_blocks: 1
    dnn_neurons: 9
    return_hidden: True

rnnlm_scorer: !new:speechbrain.decoders.scorer.RNNLMScorer
    language_model: !ref <lm_model>
    temperature: 1.25

ctc_scorer: !new:speechbrain.decoders.scorer.CTCScorer
    eos_index: !ref <eos_index>
    blank_index: !ref <blank_index>
    ctc_fc: !ref <ctc_lin>

scorer: !new:speechbrain.decoders.scorer.ScorerBuilder
    full_scorers: [!ref <rnnlm_scorer>, !ref <ctc_scorer>]
    weights:
        rnnlm: !ref <lm_weight>
        ctc: !ref <ctc_weight_decode>

decoder: !new:speechbrain.decoders.S2STransformerBeamSearcher
    modules: [!ref <Transformer>, !ref <seq_lin>]
    bos_index: !ref <bos_index>
    eos_index: !ref <eos_index>
    min_decode_ratio: 0.0
    max_decode_ratio: 1.0
    beam_size: 10
    temperature: 1.15
    using_eos_threshold: False
    length_normalization: True
    scorer: !ref <scorer>

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
    transformer: !ref <Transformer>
    seq_lin: !ref <seq_lin>
    ctc_lin: !ref <ctc_lin>
    encoder: !ref <encoder>
    lm_model: !ref <lm_model>
    decoder: !ref <decoder>

pretrainer: !new:speechbrain.utils.parameter_transfer.Pretrainer
    loadables:
        normalizer: !ref <normalizer>
        asr: !ref <asr_model>
        lm: !ref <lm_model>
        tokenizer: !ref <tokenizer>
"""


def build(seed):
    """The reference's modules as the YAML above describes them, with random weights of a useful size."""
    from speechbrain.lobes.models.convolution import ConvolutionFrontEnd
    from speechbrain.lobes.models.RNNLM import RNNLM
    from speechbrain.lobes.models.transformer.TransformerASR import TransformerASR
    from speechbrain.nnet.linear import Linear

    torch.manual_seed(seed)
    cnn = ConvolutionFrontEnd(input_shape=(8, 10, 80), num_blocks=2, num_layers_per_block=1, out_channels=(8, 4), kernel_sizes=(3, 3),
                              strides=(2, 2), residuals=(False, False))
    tr = TransformerASR(input_size=80, tgt_vocab=V, d_model=D_MODEL, nhead=2, num_encoder_layers=1, num_decoder_layers=1, d_ffn=32,
                        dropout=0.0, activation=torch.nn.GELU, encoder_module="conformer", attention_type="RelPosMHAXL",
                        normalize_before=True, causal=False)
    mods = torch.nn.ModuleDict({"CNN": cnn, "Transformer": tr, "seq_lin": Linear(input_size=D_MODEL, n_neurons=V),
                                "ctc_lin": Linear(input_size=D_MODEL, n_neurons=V)})
    lm = RNNLM(output_neurons=V, embedding_dim=6, activation=torch.nn.LeakyReLU, dropout=0.0, rnn_layers=2, rnn_neurons=13,
               dnn_blocks=1, dnn_neurons=9, return_hidden=True)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in (mods, lm):  # biases and LayerNorm affines off their initial 0 / 1
            for _, p in m.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        mods["seq_lin"].w.weight.mul_(10.0)
        mods["ctc_lin"].w.weight.mul_(10.0)
        for p in lm.rnn.parameters():
            p.mul_(2.0)
        lm.out.w.weight.mul_(4.0)  # a language model with opinions
    return mods.eval(), lm.eval()


def searcher(mods, lm, beam, ctc_w):
    from speechbrain.decoders import S2STransformerBeamSearcher
    from speechbrain.decoders.scorer import CTCScorer, RNNLMScorer, ScorerBuilder

    full, weights = [RNNLMScorer(language_model=lm, temperature=LM_T)], {"rnnlm": LM_W}
    if ctc_w > 0:
        full, weights = full + [CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], dict(weights, ctc=ctc_w)
    return S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2, min_decode_ratio=0.0,
                                      max_decode_ratio=1.0, beam_size=beam, temperature=TEMP, using_eos_threshold=False,
                                      length_normalization=True, scorer=ScorerBuilder(full_scorers=full, weights=weights))


def run64(mods, lm, beam, ctc_w, enc, lens):
    """The reference's search in fp64 and the smallest gap, over every step and utterance, between the last candidate its beam
    update keeps and the first it drops (read off the scores the update itself ranks)."""
    torch.set_default_dtype(torch.float64)  # (the scorers make their own tensors in the default dtype)
    try:
        mods64 = copy.deepcopy(mods).double()
        # (the reference builds its look-ahead mask with .float() whatever the module's type: the fp64 copy casts it)
        up = lambda t: t.double() if torch.is_tensor(t) and t.dtype == torch.float32 else t  # noqa: E731
        mods64["Transformer"].decoder.register_forward_pre_hook(
            lambda m, args, kw: (tuple(up(a) for a in args), {k: up(v) for k, v in kw.items()}), with_kwargs=True)
        s = searcher(mods64, copy.deepcopy(lm).double(), beam, ctc_w)
        gaps, inner = [], s._compute_scores_and_next_inp_tokens

        def watched(alived_hyps, log_probs, step):
            scores = alived_hyps.sequence_scores.unsqueeze(1) + log_probs
            if s.length_normalization:
                scores = scores / (step + 1)
            top = scores.view(s.batch_size, -1).topk(beam + 1, dim=-1).values
            gaps.append(float((top[:, beam - 1] - top[:, beam]).min()))
            return inner(alived_hyps, log_probs, step)

        s._compute_scores_and_next_inp_tokens = watched
        with torch.no_grad():
            hyps, _, scores, _ = s(enc.double(), lens.double())
    finally:
        torch.set_default_dtype(torch.float32)
    return hyps, scores, min(gaps)


def main():
    import sentencepiece as spm
    from speechbrain.inference.ASR import EncoderDecoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.lobes.models.transformer.TransformerASR import EncoderWrapper
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.processing.features import InputNormalization

    out_dir = os.path.join(OUT, "pretrained_rnnlm_tiny")
    os.makedirs(out_dir, exist_ok=True)
    shutil.copyfile(os.path.join(OUT, "pretrained_tiny", "tokenizer.ckpt"), os.path.join(out_dir, "tokenizer.ckpt"))
    tok = spm.SentencePieceProcessor()
    tok.load(os.path.join(out_dir, "tokenizer.ckpt"))
    assert tok.vocab_size() == V
    g = torch.Generator().manual_seed(99)
    norm = InputNormalization(norm_type="global")
    norm.glob_mean, norm.glob_std, norm.count = -30.0 + 5.0 * torch.randn(80, generator=g), 8.0 + torch.rand(80, generator=g), 1000
    wav, lens = 0.1 * torch.randn(3, 6400, generator=g), torch.tensor([1.0, 0.8, 0.55])
    for i in range(3):
        wav[i, int(lens[i] * 6400):] = 0
    feats = Fbank(sample_rate=16000, n_fft=400, n_mels=80)
    for seed in range(11, 6000):
        mods, lm = build(seed)
        encoder = LengthsCapableSequential(input_shape=[None, None, 80], compute_features=feats, normalize=norm, cnn=mods["CNN"],
                                           transformer_encoder=EncoderWrapper(mods["Transformer"]))
        rec, ok = {}, True
        with torch.no_grad():
            enc = encoder(wav, lens)
            for name, (beam, ctc_w) in CONFIGS.items():
                hyps, lengths, scores, _ = searcher(mods, lm, beam, ctc_w)(enc, lens)
                hyps64, scores64, gap = run64(mods, lm, beam, ctc_w, enc, lens)
                d = float((scores.double() - scores64).abs().max())
                print(f"[seed {seed}, {name}] lengths {[len(h) for h in hyps]}, min gap {gap:.2e}, d {d:.1e}, same ids {hyps == hyps64}")
                # the configuration is kept only if the reference's own fp64 run agrees and no beam update is a near-tie
                if not (hyps == hyps64 and gap >= MIN_GAP and all(len(h) > 1 for h in hyps) and len({tuple(h) for h in hyps}) > 1):
                    ok = False
                    break
                pad = max(len(h) for h in hyps)
                rec.update({f"{name}/ids": np.array([h + [-1] * (pad - len(h)) for h in hyps], dtype=np.int64),
                            f"{name}/lengths": lengths.numpy(), f"{name}/scores": scores.numpy(), f"{name}/d": np.array(d),
                            f"{name}/cfg": np.array([beam, ctc_w, LM_W, LM_T, TEMP])})
        if ok:
            break
    else:
        raise SystemExit("no seed found")
    for name in CONFIGS:
        assert rec[f"{name}/ids"].size and float(rec[f"{name}/d"]) < 1e-4, name
    beam, ctc_w = CONFIGS[DIRECTORY]
    asr = EncoderDecoderASR(modules={"encoder": encoder, "decoder": searcher(mods, lm, beam, ctc_w), "transformer": mods["Transformer"]},
                            hparams={"tokenizer": tok}, run_opts={"device": "cpu"})
    with torch.no_grad():
        words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == [[int(t) for t in row if t >= 0] for row in rec[f"{DIRECTORY}/ids"]]
    print("  words:", words)
    norm._save(os.path.join(out_dir, "normalizer.ckpt"))
    torch.save(torch.nn.ModuleList([mods["CNN"], mods["Transformer"], mods["seq_lin"], mods["ctc_lin"]]).state_dict(),
               os.path.join(out_dir, "asr.ckpt"))
    torch.save(lm.state_dict(), os.path.join(out_dir, "lm.ckpt"))
    with open(os.path.join(out_dir, "hyperparams.yaml"), "w", encoding="utf-8") as f:
        f.write(YAML)
    np.savez_compressed(os.path.join(OUT, "s2s_rnnlm.npz"), configs=np.array(list(CONFIGS)), directory=np.array(DIRECTORY),
                        wav=wav.numpy(), lens=lens.numpy(), enc_out=enc.numpy(), words=np.array(words), seed=np.array(seed), **rec)
    for f in sorted(os.listdir(out_dir)) + ["../s2s_rnnlm.npz"]:
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
