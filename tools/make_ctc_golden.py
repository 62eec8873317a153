"""Write tests/golden/ctc_decode.npz and the CTC model directory tests/golden/pretrained_ctc_tiny/ (with
tests/golden/pretrained_ctc_tiny_expected.npz) with the REFERENCE's own CTC decoders, savers and EncoderASR.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_ctc_golden.py

Every case stores its log-probabilities, relative lengths and the reference's outputs: greedy token lists, and for
CTCBeamSearcher the texts, scores and text_frames of each hypothesis with the adjacent top-k score gaps (the tests check
texts only where the reference's own ranking is decided by more than their margin).

The model directory has the LibriSpeech CTC recipe's layout at tiny sizes (Fbank, normalisation, CNN, Conformer through
EncoderWrapper, ctc_lin, LogSoftmax; a CTCTextEncoder label file), its checkpoints written by the reference's savers, and
the reference EncoderASR's words for the greedy (hyperparams.yaml) and CTCBeamSearcher (hyperparams_beam.yaml) forms of
decoding_function.  The reference cannot parse YAML here (oracle/ref_stubs/hyperpyyaml is an import stub), so its
EncoderASR is built from modules wired exactly as the committed YAML describes.
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SB_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_stubs"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

CHARS = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "-", "."]  # V = 31, as the CTC recipe
SPM = ["<blank>", "▁a", "▁ab", "b", "a", "▁", "c", "bc", "▁c", "ab", "▁b", "ca", "▁abc", "d"]


def posteriors(seed, B, T, V, scale, blank=0, blank_bias=2.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, T, V, generator=g) * scale
    z[:, :, blank] += blank_bias * scale / 3
    return torch.log_softmax(z, dim=-1)


def beam_cases():
    """(name, vocab, log_probs, wav_lens, searcher kwargs)"""
    cases = []
    lens3 = torch.tensor([1.0, 0.8, 0.55])
    for scale, tag in ((6.0, "peaky"), (1.0, "flat")):
        for beam, tmin, ph, topk in ((10, -5.0, False, 3), (100, -1.2, False, 1), (100, -1.2, False, 3), (1, -5.0, False, 1),
                                     (10, -1e30, False, 3), (10, -5.0, True, 1), (100, -1.2, True, 3)):
            name = f"char_{tag}_b{beam}_t{tmin:g}_ph{int(ph)}_k{topk}"
            x = posteriors(len(cases) + 100, 3, 48, 31, scale)
            cases.append((name, CHARS, x, lens3, dict(beam_size=beam, token_prune_min_logp=tmin, prune_history=ph,
                                                      topk=topk, beam_prune_logp=-12.0)))
    x = posteriors(301, 3, 48, 31, 3.0)
    cases.append(("char_blankskip", CHARS, x, lens3, dict(beam_size=10, token_prune_min_logp=-5.0, prune_history=False,
                                                          topk=3, blank_skip_threshold=0.5)))
    x = posteriors(302, 3, 48, 34, 3.0)  # V > len(vocab_list): the last three columns are never expanded
    cases.append(("char_wide_v", CHARS, x, lens3, dict(beam_size=10, token_prune_min_logp=-5.0, prune_history=False,
                                                       topk=3)))
    x = posteriors(303, 3, 48, 31, 4.0)
    x[0, 5:9, 3:10] = -math.inf
    x[1, :, 20] = -math.inf
    x[2, 10, 1:] = -math.inf
    x[2, 10, 0] = 0.0
    cases.append(("char_neg_inf", CHARS, x, lens3, dict(beam_size=10, token_prune_min_logp=-5.0, prune_history=False,
                                                        topk=3)))
    # finalize: two same-text groups whose merged scores interleave with their members' (the merged 'a' passes 'b')
    x = torch.tensor([[[0.02, 0.03, 0.5, 0.45], [0.35, 0.05, 0.31, 0.29]]]).log()
    cases.append(("finalize_interleave", ["<blank>", " ", "a", "b"], x, torch.tensor([1.0]), dict(beam_size=10, topk=4)))
    # small random sweep: short utterances, topk up to the beam, both prune_history settings
    g = torch.Generator().manual_seed(501)
    for i in range(9):
        vocab = [CHARS[:5], CHARS[:8], SPM[:8]][i % 3]
        beam = [3, 8, 20][i // 3]
        x = torch.log_softmax(torch.randn(4, 10, len(vocab), generator=g) * (1 + i % 4), dim=-1)
        cases.append((f"sweep{i}_b{beam}", vocab, x, None, dict(beam_size=beam, topk=min(beam, 4), prune_history=bool(i % 2),
                                                                 token_prune_min_logp=-5.0, beam_prune_logp=-10.0)))
    for i, (scale, beam, tmin, ph, topk) in enumerate(((3.0, 10, -5.0, False, 3), (1.0, 10, -1e30, False, 3),
                                                      (3.0, 100, -1.2, True, 3), (1.0, 10, -5.0, True, 1),
                                                      (6.0, 100, -5.0, False, 3))):
        x = posteriors(400 + i, 3, 40, len(SPM), scale)
        name = f"spm_s{scale:g}_b{beam}_t{tmin:g}_ph{int(ph)}_k{topk}"
        cases.append((name, SPM, x, lens3, dict(beam_size=beam, token_prune_min_logp=tmin, prune_history=ph, topk=topk,
                                                beam_prune_logp=-12.0)))
    return cases


def main():
    from speechbrain.decoders.ctc import CTCBeamSearcher, ctc_greedy_decode

    out = {}
    meta = []
    for i, (name, vocab, x, lens, kw) in enumerate(beam_cases()):
        s = CTCBeamSearcher(blank_index=0, vocab_list=vocab, space_token=" ", **kw)
        hyps = s(x, lens)
        res = []
        for hl in hyps:
            scores = [float(h.score) for h in hl]
            res.append(dict(text=[h.text for h in hl], score=scores,
                            text_frames=[[[w, list(f)] for w, f in h.text_frames] for h in hl],
                            gaps=[scores[k] - scores[k + 1] for k in range(len(scores) - 1)]))
        out[f"beam{i}_x"] = x.numpy()
        out[f"beam{i}_lens"] = (torch.ones(x.shape[0]) if lens is None else lens).numpy()
        meta.append(dict(name=name, vocab=vocab, kwargs=kw, result=res))
        print(f"  {name:36s} {[r['text'][0][:30] for r in res]}")
    greedy = []
    g = torch.Generator().manual_seed(7)
    for i, (B, T, V, blank) in enumerate(((4, 50, 31, 0), (4, 64, 31, -1), (3, 33, 7, 2))):
        x = torch.log_softmax(torch.randn(B, T, V, generator=g) * 2.0, dim=-1)
        if i == 2:
            x[0, 3, 4] = x[0, 3, 5] = x[0, 3].max()  # equal maxima: the first index wins
            x[1, 4, 5] = float("nan")  # NaN counts as the maximum
        lens = torch.tensor([1.0, 0.5, 0.25, 0.75][:B])  # T = 50: 12.5 -> 12, 37.5 -> 38; T = 33: 16.5 -> 16
        res = ctc_greedy_decode(x, lens, blank_id=blank)
        out[f"greedy{i}_x"] = x.numpy()
        out[f"greedy{i}_lens"] = lens.numpy()
        greedy.append(dict(blank=blank, result=res))
    out["meta"] = np.array(json.dumps(dict(beam=meta, greedy=greedy)))
    np.savez_compressed(os.path.join(OUT, "ctc_decode.npz"), **out)
    print("wrote", os.path.join(OUT, "ctc_decode.npz"))
    pretrained_ctc_tiny()


CTC_YAML = """# Layout of the LibriSpeech CTC recipe (recipes/LibriSpeech/ASR/CTC/hparams/conformer_large.yaml) at tiny sizes,
# as an inference hyperparams.yaml for EncoderASR.  Written by tools/make_ctc_golden.py.
sample_rate: 16000
n_fft: 400
n_mels: 80
d_model: 32
output_neurons: 31
blank_index: 0

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
    nhead: 4
    num_encoder_layers: 2
    num_decoder_layers: 0
    d_ffn: 64
    dropout: 0.0
    activation: !name:torch.nn.GELU
    encoder_module: conformer
    attention_type: RelPosMHAXL
    normalize_before: True
    causal: False

ctc_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <d_model>
    n_neurons: !ref <output_neurons>

log_softmax: !new:torch.nn.LogSoftmax
    dim: -1

normalize: !new:speechbrain.processing.features.InputNormalization
    norm_type: global

compute_features: !new:speechbrain.lobes.features.Fbank
    sample_rate: !ref <sample_rate>
    n_fft: !ref <n_fft>
    n_mels: !ref <n_mels>

tokenizer: !new:speechbrain.dataio.encoder.CTCTextEncoder

Tencoder: !new:speechbrain.lobes.models.transformer.TransformerASR.EncoderWrapper
    transformer: !ref <Transformer>

encoder: !new:speechbrain.nnet.containers.LengthsCapableSequential
    input_shape: [null, null, !ref <n_mels>]
    compute_features: !ref <compute_features>
    normalize: !ref <normalize>
    CNN: !ref <CNN>
    transformer_encoder: !ref <Tencoder>
    ctc_lin: !ref <ctc_lin>
    log_softmax: !ref <log_softmax>

%DECODING%

modules:
    encoder: !ref <encoder>

model: !new:torch.nn.ModuleList
    - [!ref <CNN>, !ref <Transformer>, !ref <ctc_lin>]

pretrainer: !new:speechbrain.utils.parameter_transfer.Pretrainer
    loadables:
        model: !ref <model>
        normalize: !ref <normalize>
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


def pretrained_ctc_tiny():
    import functools

    from speechbrain.dataio.encoder import CTCTextEncoder
    from speechbrain.decoders.ctc import CTCBeamSearcher, ctc_greedy_decode
    from speechbrain.inference.ASR import EncoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.lobes.models.convolution import ConvolutionFrontEnd
    from speechbrain.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear
    from speechbrain.processing.features import InputNormalization

    out_dir = os.path.join(OUT, "pretrained_ctc_tiny")
    os.makedirs(out_dir, exist_ok=True)
    torch.manual_seed(17)
    cnn = ConvolutionFrontEnd(input_shape=(8, 10, 80), num_blocks=2, num_layers_per_block=1, out_channels=(64, 32),
                              kernel_sizes=(3, 3), strides=(2, 2), residuals=(False, False))
    tr = TransformerASR(input_size=640, tgt_vocab=31, d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=0,
                        d_ffn=64, dropout=0.0, activation=torch.nn.GELU, encoder_module="conformer",
                        attention_type="RelPosMHAXL", normalize_before=True, causal=False)
    ctc_lin = Linear(input_size=32, n_neurons=31)
    model = torch.nn.ModuleList([cnn, tr, ctc_lin]).eval()
    g = torch.Generator().manual_seed(18)
    with torch.no_grad():
        for n, p in model.named_parameters():  # random LayerNorm affines / biases, so that they are exercised
            if p.dim() == 1 or "norm" in n:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
        ctc_lin.w.weight.mul_(12.0)  # peaked posteriors: the words do not hinge on fp32 reassociation
        ctc_lin.w.bias.mul_(0.1)
    # tones that change every 40 ms over noise: frame-to-frame variety, so that the decoders emit more than one label
    n = 24000
    steps = torch.arange(n) // 640
    freq = 200.0 + 3000.0 * torch.rand(3, int(steps[-1]) + 1, generator=g)
    phase = torch.cumsum(2 * math.pi * freq[:, steps] / 16000.0, dim=1)
    wav = 0.3 * torch.sin(phase) * torch.rand(3, int(steps[-1]) + 1, generator=g)[:, steps] + 0.02 * torch.randn(3, n,
                                                                                                             generator=g)
    lens = torch.tensor([1.0, 0.8, 0.55])
    for i in range(3):
        wav[i, int(lens[i] * n):] = 0
    # normalisation statistics as a trained model carries them: the moments of its features
    feats = Fbank(sample_rate=16000, n_fft=400, n_mels=80)(wav)
    norm = InputNormalization(norm_type="global")
    norm.glob_mean = feats.mean(dim=(0, 1))
    norm.glob_std = feats.std(dim=(0, 1))
    norm.count = 1000
    # a random head mostly reads the encoder's common direction (one label everywhere): project it out, as training would
    with torch.no_grad():
        enc = tr.encode(cnn(norm(feats, torch.ones(3))), torch.ones(3))
        mu = enc.mean(dim=(0, 1))
        w = ctc_lin.w.weight
        w.sub_(torch.outer(w @ mu, mu) / mu.dot(mu))
    norm._save(os.path.join(out_dir, "normalize.ckpt"))
    tok = CTCTextEncoder()
    tok.update_from_iterable(CHARS[1:], sequence_input=False)
    tok.insert_blank(index=0)
    tok.save(os.path.join(out_dir, "tokenizer.ckpt"))
    torch.save(model.state_dict(), os.path.join(out_dir, "model.ckpt"))
    for name, dec in (("hyperparams.yaml", GREEDY_DECODING), ("hyperparams_beam.yaml", BEAM_DECODING)):
        with open(os.path.join(out_dir, name), "w", encoding="utf-8") as f:
            f.write(CTC_YAML.replace("%DECODING%", dec))
    assert sorted(tok.lab2ind.values()) == list(range(31)) and tok.get_blank_index() == 0

    encoder = LengthsCapableSequential(input_shape=[None, None, 80], compute_features=Fbank(sample_rate=16000, n_fft=400,
                                                                                            n_mels=80),
                                       normalize=norm, CNN=cnn, transformer_encoder=EncoderWrapper(tr), ctc_lin=ctc_lin,
                                       log_softmax=torch.nn.LogSoftmax(dim=-1))
    greedy = EncoderASR(modules={"encoder": encoder}, hparams={
        "tokenizer": tok, "decoding_function": functools.partial(ctc_greedy_decode, blank_id=0)}, run_opts={"device": "cpu"})
    beam = EncoderASR(modules={"encoder": encoder}, hparams={
        "tokenizer": tok, "decoding_function": CTCBeamSearcher, "test_beam_search": dict(blank_index=0, **BEAM_SETTINGS)},
        run_opts={"device": "cpu"})
    with torch.no_grad():
        logp = greedy.encode_batch(wav, lens)
        g_words, g_tokens = greedy.transcribe_batch(wav, lens)
        b_words, b_hyps = beam.transcribe_batch(wav, lens)
        files = ["sample_mono.wav", "sample_stereo.wav"]
        g_file = [greedy.transcribe_file(os.path.join(OUT, f)) for f in files]
        b_file = [beam.transcribe_file(os.path.join(OUT, f)) for f in files]
    print("  greedy:", g_words, g_file)
    print("  beam:  ", b_words, b_file)
    np.savez_compressed(os.path.join(OUT, "pretrained_ctc_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        logp=logp.numpy(), greedy_words=np.array(g_words),
                        greedy_tokens=np.array([t + [-1] * (logp.shape[1] - len(t)) for t in g_tokens], dtype=np.int64),
                        beam_words=np.array(b_words), beam_scores=np.array([float(h[0].score) for h in b_hyps]),
                        file_names=np.array(files), greedy_file_words=np.array(g_file), beam_file_words=np.array(b_file))
    size = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))
    print(f"  wrote {out_dir} ({size / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
