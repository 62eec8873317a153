"""Write tests/golden/model_s2srnn.npz and the CRDNN seq2seq model directory tests/golden/pretrained_crdnn_s2s_tiny/ (with
tests/golden/pretrained_crdnn_s2s_tiny_expected.npz) with the REFERENCE's own AttentionalRNNDecoder, S2SRNNGreedySearcher, savers
and EncoderDecoderASR.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_s2srnn_golden.py

model_s2srnn.npz holds, per configuration of CONFIGS (a tiny GRU attention decoder with its embedding and output layer): the
state dicts, encoder states and relative lengths, the reference's greedy result (ids, lengths, scores), and -- teacher forced
with the greedy tokens -- dec_out, the attention and the logits of every step.  Before anything is written the host
restatement tests/attn_rnn_host_ref.py is checked against the reference step by step at 1e-5, and the reference's own fp64 run
must decode the same ids with a margin of MIN_GAP between the best two logits of every step (the seed is advanced until it does,
so that the exact-id tests are not decided by rounding).  The reference builds its first prev_attn in fp32 whatever the
module's type (enc_len.float()), so the fp64 copy casts conv_loc's input to double; everything else of it is the reference's.

The model directory has train_BPE_1000.yaml's encoder, embedding, decoder and output layer at tiny sizes in the inference
layout of the reference's published CRDNN models, with S2SRNNGreedySearcher as the decoder (the reference cannot parse YAML
here -- oracle/ref_stubs/hyperpyyaml is an import stub -- so its EncoderDecoderASR is built from modules wired exactly as the
committed YAML describes).  The wavs are pretrained_crdnn_ctc_tiny's signal; the tokenizer is pretrained_tiny's SentencePiece
model (EncoderDecoderASR decodes with decode_ids, which the CTC directory's label encoder does not have).
"""
import copy
import math
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
MIN_GAP = 2e-3  # (40 x the model tests' bound) between the best two logits of every decoding step, in the reference's fp64 run
BASE = dict(attn="location", emb=6, H=16, A=12, E=10, V=21, C=4, k=3, layers=1, B=3, T=23, wav_len=(1.0, 0.7, 0.4), bos=0, eos=0,
            min_ratio=0.0, max_ratio=1.0, scaling=1.0, eos_bias=2.0, want="early_stop")
CONFIGS = {
    "location": BASE,                                                          # every utterance ends before the last step
    "single": dict(BASE, B=1, wav_len=(1.0,), want="eos"),                     # B = 1
    "never_eos": dict(BASE, eos_bias=-100.0, max_ratio=0.5, want="no_eos"),      # no eos: length 1.0, stops at max_decode_ratio
    "min_ratio": dict(BASE, min_ratio=0.3, want="eos"),                        # range(int(T * 0.3), T)
    "content": dict(BASE, attn="content", emb=3, H=3, A=3, E=7, V=5, C=0, k=0, B=2, T=6, wav_len=(1.0, 1.0), bos=0, eos=1,
                    eos_bias=0.0, want="any"),                                 # the reference doctest's configuration
    "two_layer": dict(BASE, layers=2, scaling=2.0, want="eos"),                # a two-layer GRU, sharpened attention
}
MODEL_KEYS = ("attn", "emb", "H", "A", "E", "V", "C", "k", "layers", "B", "T", "bos", "eos", "min_ratio", "max_ratio", "scaling")


def check(name, ref, got, tol):
    d = float((ref - got).abs().max())
    print(f"  {name:44s} max|d| = {d:.3e}  (tol {tol:g})")
    assert d <= tol, name


def build(cfg, seed):
    """The reference's embedding, decoder, output layer and searcher with random weights of a useful size."""
    from speechbrain.decoders.seq2seq import S2SRNNGreedySearcher
    from speechbrain.nnet.embedding import Embedding
    from speechbrain.nnet.linear import Linear
    from speechbrain.nnet.RNN import AttentionalRNNDecoder

    torch.manual_seed(seed)
    emb = Embedding(num_embeddings=cfg["V"], embedding_dim=cfg["emb"])
    dec = AttentionalRNNDecoder(rnn_type="gru", attn_type=cfg["attn"], hidden_size=cfg["H"], attn_dim=cfg["A"],
                                num_layers=cfg["layers"], enc_dim=cfg["E"], input_size=cfg["emb"], scaling=cfg["scaling"],
                                channels=cfg["C"] or None, kernel_size=cfg["k"] or None, re_init=True, dropout=0.15)
    lin = Linear(input_size=cfg["H"], n_neurons=cfg["V"])
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in dec.named_parameters():  # biases of both signs, b_ih != b_hh; an attention that looks somewhere
            if p.dim() == 1:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
        dec.attn.mlp_attn.weight.mul_(6.0)
        if cfg["C"]:
            dec.attn.conv_loc.weight.mul_(8.0)
        lin.w.weight.mul_(8.0)  # sharpened: the reference's own decisions have wide margins
        lin.w.bias[cfg["eos"]] += cfg["eos_bias"]
    for m in (emb, dec, lin):
        m.eval()
    searcher = S2SRNNGreedySearcher(embedding=emb, decoder=dec, linear=lin, bos_index=cfg["bos"], eos_index=cfg["eos"],
                                    min_decode_ratio=cfg["min_ratio"], max_decode_ratio=cfg["max_ratio"])
    return emb, dec, lin, searcher.eval()


def to_double(searcher):
    s64 = copy.deepcopy(searcher).double()
    if hasattr(s64.dec.attn, "conv_loc"):
        s64.dec.attn.conv_loc.register_forward_pre_hook(lambda m, inp: (inp[0].to(m.weight.dtype),))
    return s64


def teacher_forced(searcher, enc, wav_len, tokens_in):
    """The reference's forward_step over given input tokens [B,L] -> dec_out [B,L,H], attn [B,L,T], logits [B,L,V]."""
    enc_len = torch.round(enc.shape[1] * wav_len).long()
    hs, c = searcher.reset_mem(enc.shape[0], enc.device)
    outs, attns, logits = [], [], []
    for t in range(tokens_in.shape[1]):
        out, hs, c, w = searcher.dec.forward_step(searcher.emb(tokens_in[:, t]), hs, c, enc, enc_len)
        outs.append(out), attns.append(w), logits.append(searcher.fc(out))
    return torch.stack(outs, 1), torch.stack(attns, 1), torch.stack(logits, 1)


def run(searcher, enc, wav_len, cfg):
    """(hyps, lengths [B,1], scores [B,1,L], tokens_in [B,L]) of the reference's search."""
    hyps, lengths, scores, _ = searcher(enc, wav_len)
    L = scores.shape[-1]
    tokens_in = torch.full((enc.shape[0], L), cfg["eos"], dtype=torch.long)
    tokens_in[:, 0] = cfg["bos"]
    for b, h in enumerate(hyps):  # the inputs of the greedy run: bos, then its own tokens, eos once it has ended
        n = min(len(h), L - 1)
        tokens_in[b, 1:1 + n] = torch.tensor(h[:n], dtype=torch.long)
    return hyps, lengths, scores, tokens_in


def decoded_ok(cfg, hyps, L, steps):
    if cfg["want"] == "early_stop":
        return L < steps and all(len(h) > 0 for h in hyps) and len({len(h) for h in hyps}) > 1 and sum(len(h) for h in hyps) >= 9
    if cfg["want"] == "eos":
        return any(2 < len(h) < L for h in hyps)
    if cfg["want"] == "no_eos":
        return all(len(h) == L for h in hyps) and L == steps
    return True


def golden_model():
    import attn_rnn_host_ref as R

    rec = {"configs": np.array(list(CONFIGS))}
    for ci, (name, cfg) in enumerate(CONFIGS.items()):
        wav_len = torch.tensor(cfg["wav_len"])
        steps = int(cfg["T"] * cfg["max_ratio"]) - int(cfg["T"] * cfg["min_ratio"])
        for seed in range(1000 * ci + 11, 1000 * ci + 1000):
            emb, dec, lin, searcher = build(cfg, seed)
            enc = torch.randn(cfg["B"], cfg["T"], cfg["E"], generator=torch.Generator().manual_seed(500 + seed))
            with torch.no_grad():
                hyps, lengths, scores, tokens_in = run(searcher, enc, wav_len, cfg)
                s64 = to_double(searcher)
                hyps64, _, _, _ = run(s64, enc.double(), wav_len.double(), cfg)
                _, _, logits64 = teacher_forced(s64, enc.double(), wav_len.double(), tokens_in)
                own = float((teacher_forced(searcher, enc, wav_len, tokens_in)[2].double() - logits64).abs().max())
            top2 = logits64.topk(2, dim=-1).values
            gap = float((top2[..., 0] - top2[..., 1]).min())
            L = scores.shape[-1]
            print(f"[{name}, seed {seed}] lengths {[len(h) for h in hyps]} of {L} (at most {steps}) steps, min gap {gap:.3f}, "
                  f"the reference's fp32 logits against its fp64 ones {own:.1e}")
            # (own: the reference's own rounding must sit under a quarter of the model tests' bound, 5e-5, on this draw)
            if hyps64 == hyps and gap >= MIN_GAP and own <= 5e-5 / 4 and decoded_ok(cfg, hyps, L, steps):
                break
        else:
            raise SystemExit(f"{name}: no seed found")
        with torch.no_grad():
            dec_out, attn, logits = teacher_forced(searcher, enc, wav_len, tokens_in)
            emb_in = emb(tokens_in)
            dec.attn.reset()
            outputs, attn_fw = dec(emb_in, enc, wav_len)  # AttentionalRNNDecoder.forward: the same numbers by the other entry
        check("reference forward against its forward_step", dec_out, outputs, 1e-6)
        check("reference forward attention", attn, attn_fw, 1e-6)
        # the host restatement against the reference, step by step
        sd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
        enc_len = torch.round(cfg["T"] * wav_len).int()
        host = R.HostDecoder(sd, cfg["scaling"], torch.float32)
        h_out, h_attn, _, _ = host.forward(emb_in, enc, enc_len)
        check("host restatement, dec_out", dec_out, h_out, 1e-5)
        check("host restatement, attention", attn, h_attn, 1e-5)
        check("host restatement, logits", logits, h_out @ lin.w.weight.T + lin.w.bias, 1e-5)
        g_tok, g_sc, _ = R.greedy(R.HostDecoder(sd, cfg["scaling"], torch.float32), emb.Embedding.weight.detach(),
                                  lin.w.weight.detach(), lin.w.bias.detach(), enc, enc_len, steps, cfg["bos"], cfg["eos"])
        assert R.hyps_of(g_tok, cfg["eos"])[0] == hyps, (R.hyps_of(g_tok, cfg["eos"])[0], hyps)
        check("host restatement, greedy scores", scores[:, 0], g_sc, 1e-5)
        check("the reference in fp64, logits", logits.double(), logits64, 5e-5 / 4)
        pad = max(1, max(len(h) for h in hyps))
        rec.update({f"{name}/enc": enc.numpy(), f"{name}/wav_len": wav_len.numpy(), f"{name}/tokens_in": tokens_in.numpy(),
                    f"{name}/dec_out": dec_out.numpy(), f"{name}/attn": attn.numpy(), f"{name}/logits": logits.numpy(),
                    f"{name}/ids": np.array([h + [-1] * (pad - len(h)) for h in hyps], dtype=np.int64),
                    f"{name}/lengths": lengths.numpy(), f"{name}/scores": scores.numpy(),
                    f"{name}/emb": emb.Embedding.weight.detach().numpy(), f"{name}/fc_w": lin.w.weight.detach().numpy(),
                    f"{name}/fc_b": lin.w.bias.detach().numpy(),
                    f"{name}/cfg_keys": np.array(MODEL_KEYS), f"{name}/cfg": np.array([str(cfg[k]) for k in MODEL_KEYS])})
        for k, v in sd.items():
            rec[f"{name}/sd/{k}"] = v.numpy()
    path = os.path.join(OUT, "model_s2srnn.npz")
    np.savez_compressed(path, **rec)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


S2S_YAML = """\
# The encoder, embedding, decoder and output layer of recipes/LibriSpeech/ASR/seq2seq/hparams/train_BPE_1000.yaml at tiny sizes,
# as an inference hyperparams.yaml for EncoderDecoderASR with greedy decoding.  Written by tools/make_s2srnn_golden.py.
sample_rate: 16000
n_fft: 400
n_mels: 40
activation: !name:torch.nn.LeakyReLU
dropout: 0.15
cnn_blocks: 2
cnn_channels: (4, 8)
inter_layer_pooling_size: (2, 2)
cnn_kernelsize: (3, 3)
time_pooling_size: 4
rnn_class: !name:speechbrain.nnet.RNN.LSTM
rnn_layers: 2
rnn_neurons: 12
rnn_bidirectional: True
dnn_blocks: 2
dnn_neurons: 16
emb_size: 8
dec_neurons: 24
output_neurons: 40
bos_index: 1
eos_index: 2
min_decode_ratio: 0.0
max_decode_ratio: 1.0

enc: !new:speechbrain.lobes.models.CRDNN.CRDNN
    input_shape: [null, null, !ref <n_mels>]
    activation: !ref <activation>
    dropout: !ref <dropout>
    cnn_blocks: !ref <cnn_blocks>
    cnn_channels: !ref <cnn_channels>
    cnn_kernelsize: !ref <cnn_kernelsize>
    inter_layer_pooling_size: !ref <inter_layer_pooling_size>
    time_pooling: True
    using_2d_pooling: False
    time_pooling_size: !ref <time_pooling_size>
    rnn_class: !ref <rnn_class>
    rnn_layers: !ref <rnn_layers>
    rnn_neurons: !ref <rnn_neurons>
    rnn_bidirectional: !ref <rnn_bidirectional>
    rnn_re_init: True
    dnn_blocks: !ref <dnn_blocks>
    dnn_neurons: !ref <dnn_neurons>
    use_rnnp: False

emb: !new:speechbrain.nnet.embedding.Embedding
    num_embeddings: !ref <output_neurons>
    embedding_dim: !ref <emb_size>

dec: !new:speechbrain.nnet.RNN.AttentionalRNNDecoder
    enc_dim: !ref <dnn_neurons>
    input_size: !ref <emb_size>
    rnn_type: gru
    attn_type: location
    hidden_size: !ref <dec_neurons>
    attn_dim: 20
    num_layers: 1
    scaling: 1.0
    channels: 10
    kernel_size: 100
    re_init: True
    dropout: !ref <dropout>

seq_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <dec_neurons>
    n_neurons: !ref <output_neurons>

normalize: !new:speechbrain.processing.features.InputNormalization
    norm_type: global

compute_features: !new:speechbrain.lobes.features.Fbank
    sample_rate: !ref <sample_rate>
    n_fft: !ref <n_fft>
    n_mels: !ref <n_mels>

tokenizer: !new:sentencepiece.SentencePieceProcessor

encoder: !new:speechbrain.nnet.containers.LengthsCapableSequential
    input_shape: [null, null, !ref <n_mels>]
    compute_features: !ref <compute_features>
    normalize: !ref <normalize>
    model: !ref <enc>

decoder: !new:speechbrain.decoders.S2SRNNGreedySearcher
    embedding: !ref <emb>
    decoder: !ref <dec>
    linear: !ref <seq_lin>
    bos_index: !ref <bos_index>
    eos_index: !ref <eos_index>
    min_decode_ratio: !ref <min_decode_ratio>
    max_decode_ratio: !ref <max_decode_ratio>

modules:
    encoder: !ref <encoder>
    decoder: !ref <decoder>

model: !new:torch.nn.ModuleList
    - [!ref <enc>, !ref <emb>, !ref <dec>, !ref <seq_lin>]

pretrainer: !new:speechbrain.utils.parameter_transfer.Pretrainer
    loadables:
        model: !ref <model>
        normalize: !ref <normalize>
        tokenizer: !ref <tokenizer>
"""
S2S = dict(attn="location", emb=8, H=24, A=20, E=16, V=40, C=10, k=100, layers=1, bos=1, eos=2, min_ratio=0.0, max_ratio=1.0,
           scaling=1.0, eos_bias=1.0)


def golden_pretrained():
    import sentencepiece as spm
    from make_crdnn_golden import N_MELS, build_crdnn, randomise
    from speechbrain.inference.ASR import EncoderDecoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear
    from speechbrain.processing.features import InputNormalization

    print("[pretrained_crdnn_s2s_tiny]")
    out_dir = os.path.join(OUT, "pretrained_crdnn_s2s_tiny")
    os.makedirs(out_dir, exist_ok=True)
    shutil.copyfile(os.path.join(OUT, "pretrained_tiny", "tokenizer.ckpt"), os.path.join(out_dir, "tokenizer.ckpt"))
    sp = spm.SentencePieceProcessor()
    sp.load(os.path.join(out_dir, "tokenizer.ckpt"))
    assert sp.vocab_size() == S2S["V"]
    # tones that change every 40 ms over noise (the signal of pretrained_crdnn_ctc_tiny): frame-to-frame variety
    g = torch.Generator().manual_seed(58)
    n = 24000
    steps = torch.arange(n) // 640
    freq = 200.0 + 3000.0 * torch.rand(3, int(steps[-1]) + 1, generator=g)
    phase = torch.cumsum(2 * math.pi * freq[:, steps] / 16000.0, dim=1)
    wav = 0.3 * torch.sin(phase) * torch.rand(3, int(steps[-1]) + 1, generator=g)[:, steps] + 0.02 * torch.randn(3, n, generator=g)
    lens = torch.tensor([1.0, 0.8, 0.55])
    for i in range(3):
        wav[i, int(lens[i] * n):] = 0
    fbank = Fbank(sample_rate=16000, n_fft=400, n_mels=N_MELS)
    feats = fbank(wav)
    norm = InputNormalization(norm_type="global")
    norm.glob_mean, norm.glob_std, norm.count = feats.mean(dim=(0, 1)), feats.std(dim=(0, 1)), 1000
    files = ["sample_mono.wav", "sample_stereo.wav"]
    for seed in range(71, 400):
        torch.manual_seed(seed)
        enc = build_crdnn()
        enc(feats)
        enc.eval()
        randomise(enc, Linear(input_size=16, n_neurons=2), seed + 1, 1.0)
        emb, dec, lin, searcher = build(S2S, seed + 2)
        encoder = LengthsCapableSequential(input_shape=[None, None, N_MELS], compute_features=fbank, normalize=norm, model=enc)
        asr = EncoderDecoderASR(modules={"encoder": encoder, "decoder": searcher}, hparams={"tokenizer": sp},
                                run_opts={"device": "cpu"})
        with torch.no_grad():
            enc_out = asr.encode_batch(wav, lens)
            # a random decoder mostly reads the encoder's common direction (the same text for every input): project it out of
            # the two layers that read the encoder and give what is left unit scale, as training would
            mu = enc_out.mean(dim=(0, 1))
            for w in (dec.attn.mlp_enc.weight, dec.attn.mlp_out.weight):
                w.sub_(torch.outer(w @ mu, mu) / mu.dot(mu))
                w.mul_(1.0 / float((enc_out - mu).std()))
            words, tokens = asr.transcribe_batch(wav, lens)
            _, lengths, scores, _ = searcher(enc_out, lens)
            file_words = [asr.transcribe_file(os.path.join(OUT, f)) for f in files]
            # the reference's fp64 decoder from the same fp32 encoder states (the encoder is not what this fixture is about)
            s64 = to_double(searcher)
            hyps64, _, _, tokens_in = run(s64, enc_out.double(), lens.double(), S2S)
            _, _, logits64 = teacher_forced(s64, enc_out.double(), lens.double(), tokens_in)
        top2 = logits64.topk(2, dim=-1).values
        gap = float((top2[..., 0] - top2[..., 1]).min())
        L = scores.shape[-1]
        print(f"  seed {seed}: lengths {[len(t) for t in tokens]} of {L} steps ({enc_out.shape[1]} frames), min gap {gap:.3f}, {words}")
        if (hyps64 == tokens and gap >= MIN_GAP and all(0 < len(t) for t in tokens) and any(len(t) < L for t in tokens) and len({tuple(t) for t in tokens}) == 3
                and all(len(w) > 0 for w in file_words)):
            break
        print("    the fp64 run of the reference decodes differently, a margin is thin, a hypothesis is empty or two are equal: next seed")
    else:
        raise SystemExit("no seed found")
    norm._save(os.path.join(out_dir, "normalize.ckpt"))
    torch.save(torch.nn.ModuleList([enc, emb, dec, lin]).state_dict(), os.path.join(out_dir, "model.ckpt"))
    with open(os.path.join(out_dir, "hyperparams.yaml"), "w", encoding="utf-8") as f:
        f.write(S2S_YAML)
    pad = max(len(t) for t in tokens)
    np.savez_compressed(os.path.join(OUT, "pretrained_crdnn_s2s_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        enc_out=enc_out.numpy(), words=np.array(words),
                        tokens=np.array([t + [-1] * (pad - len(t)) for t in tokens], dtype=np.int64),
                        lengths=lengths.numpy(), scores=scores.numpy(), file_names=np.array(files),
                        file_words=np.array(file_words), min_gap=np.array([gap], dtype=np.float32))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    golden_model()
    golden_pretrained()
