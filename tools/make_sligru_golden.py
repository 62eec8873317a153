"""Write tests/golden/model_sligru.npz and the CRDNN(SLiGRU) + CTC model directory tests/golden/pretrained_crdnn_sligru_ctc_tiny/
(with tests/golden/pretrained_crdnn_sligru_ctc_tiny_expected.npz) with the REFERENCE's own SLiGRU, CRDNN, savers, greedy CTC
decoder and EncoderASR.  The sibling of tools/make_crdnn_golden.py, whose helpers and YAML text it uses.

Runs only where the reference checkout is available (SB_REFERENCE, as for make_crdnn_golden.py), and AFTER the tools whose
fixtures it reads: tests/golden/pretrained_ctc_tiny/tokenizer.ckpt (tools/make_ctc_golden.py) and
tests/golden/pretrained_crdnn_ctc_tiny_expected.npz (tools/make_crdnn_golden.py: the waveforms, which this tool checks and does
not store again).

    python tools/make_sligru_golden.py

model_sligru.npz: a 2-layer bidirectional SLiGRU, H 12, input 10, B 3, T 9, batchnorm with random affines and non-trivial running
statistics, recurrent_elementwise_affine with random affines; the state dict, the input, each layer's output and hh.
The model directory is pretrained_crdnn_ctc_tiny's with ``rnn_class: !name:speechbrain.nnet.RNN.SLiGRU`` (the encoder of
train_BPE_1000_sligru.yaml at tiny sizes); its expected file holds the CTC log-probabilities, the greedy ids and the text.
Before anything is written the reference's own fp64 run must decode the ids of its fp32 run (the seed is advanced until it
does) and its fp32-vs-fp64 distance has to stay under a quarter of the tests' bounds (5e-5 on the layers, 1e-4 on the log-probs).
"""
import copy
import functools
import math
import os
import shutil

import make_crdnn_golden as C  # (puts the reference and oracle/ref_stubs on sys.path)
import numpy as np
import torch

OUT = C.OUT
H, IN, B, T, LAYERS = 12, 10, 3, 9, 2


def golden_model():
    from speechbrain.nnet.RNN import SLiGRU

    print("[model_sligru]")
    torch.manual_seed(71)
    x = torch.randn(B, T, IN, generator=torch.Generator().manual_seed(72))
    m = SLiGRU(hidden_size=H, input_shape=[B, T, IN], num_layers=LAYERS, bidirectional=True, recurrent_elementwise_affine=True).eval()
    g = torch.Generator().manual_seed(73)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
            elif n.endswith("num_batches_tracked"):
                b.fill_(1000)

    def run(mod, inp):
        outs = []
        hooks = [lay.register_forward_hook(lambda _m, _i, o: outs.append(o.detach().clone())) for lay in mod.rnn]
        with torch.no_grad():
            out, hh = mod(inp)
        for h in hooks:
            h.remove()
        return out, hh, outs

    out, hh, outs = run(m, x)
    out64, hh64, outs64 = run(copy.deepcopy(m).double(), x.double())
    for i, (a, b) in enumerate(zip(outs, outs64)):
        C.check(f"the reference in fp64, layer {i}", a.double(), b, C.STAGE_BOUND / 4)
    C.check("the reference in fp64, hh", hh.double(), hh64, C.STAGE_BOUND / 4)
    assert torch.equal(out, outs[-1])
    rec = {"x": x.numpy(), "hh": hh.numpy(), "cfg": np.array([H, IN, B, T, LAYERS], dtype=np.int64)}
    for i, o in enumerate(outs):
        rec[f"layer{i}"] = o.numpy()
    for k, v in m.state_dict().items():
        rec[f"sd/{k}"] = v.numpy()
    path = os.path.join(OUT, "model_sligru.npz")
    np.savez_compressed(path, **rec)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def build_crdnn():
    from speechbrain.lobes.models.CRDNN import CRDNN
    from speechbrain.nnet.RNN import SLiGRU

    return CRDNN(input_shape=[None, None, C.N_MELS], activation=torch.nn.LeakyReLU, dropout=0.15, cnn_blocks=2,
                 cnn_channels=list(C.CHANNELS), cnn_kernelsize=(3, 3), inter_layer_pooling_size=list(C.POOLS), time_pooling=True,
                 using_2d_pooling=False, time_pooling_size=C.TIME_POOL, rnn_class=SLiGRU, rnn_layers=C.RNN_LAYERS,
                 rnn_neurons=C.RNN_NEURONS, rnn_bidirectional=True, rnn_re_init=True, dnn_blocks=C.DNN_BLOCKS,
                 dnn_neurons=C.DNN_NEURONS, use_rnnp=False)


def golden_pretrained():
    from speechbrain.dataio.encoder import CTCTextEncoder
    from speechbrain.decoders.ctc import ctc_greedy_decode
    from speechbrain.inference.ASR import EncoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear
    from speechbrain.processing.features import InputNormalization

    print("[pretrained_crdnn_sligru_ctc_tiny]")
    out_dir = os.path.join(OUT, "pretrained_crdnn_sligru_ctc_tiny")
    os.makedirs(out_dir, exist_ok=True)
    shutil.copyfile(os.path.join(OUT, "pretrained_ctc_tiny", "tokenizer.ckpt"), os.path.join(out_dir, "tokenizer.ckpt"))
    tok = CTCTextEncoder()
    tok.load(os.path.join(out_dir, "tokenizer.ckpt"))
    # the signal of pretrained_crdnn_ctc_tiny: tones that change every 40 ms over noise
    g = torch.Generator().manual_seed(58)
    n = 24000
    steps = torch.arange(n) // 640
    freq = 200.0 + 3000.0 * torch.rand(3, int(steps[-1]) + 1, generator=g)
    phase = torch.cumsum(2 * math.pi * freq[:, steps] / 16000.0, dim=1)
    wav = 0.3 * torch.sin(phase) * torch.rand(3, int(steps[-1]) + 1, generator=g)[:, steps] + 0.02 * torch.randn(3, n, generator=g)
    lens = torch.tensor([1.0, 0.8, 0.55])
    for i in range(3):
        wav[i, int(lens[i] * n):] = 0
    fbank = Fbank(sample_rate=16000, n_fft=400, n_mels=C.N_MELS)
    feats = fbank(wav)
    norm = InputNormalization(norm_type="global")
    norm.glob_mean, norm.glob_std, norm.count = feats.mean(dim=(0, 1)), feats.std(dim=(0, 1)), 1000
    for seed in range(57, 100):
        print(f"  seed {seed}")
        torch.manual_seed(seed)
        enc = build_crdnn()
        enc(feats)  # (the reference instantiates its layers at the first call)
        ctc_lin = Linear(input_size=C.DNN_NEURONS, n_neurons=C.VOCAB)
        enc.eval(), ctc_lin.eval()
        C.randomise(enc, ctc_lin, seed + 1, 8.0)
        with torch.no_grad():
            mu = enc(norm(feats, torch.ones(3))).mean(dim=(0, 1))  # (project the common direction out, as training would)
            w = ctc_lin.w.weight
            w.sub_(torch.outer(w @ mu, mu) / mu.dot(mu))
        encoder = LengthsCapableSequential(input_shape=[None, None, C.N_MELS], compute_features=fbank, normalize=norm, enc=enc,
                                           ctc_lin=ctc_lin, log_softmax=torch.nn.LogSoftmax(dim=-1))
        asr = EncoderASR(modules={"encoder": encoder}, run_opts={"device": "cpu"},
                         hparams={"tokenizer": tok, "decoding_function": functools.partial(ctc_greedy_decode, blank_id=0)})
        enc64 = copy.deepcopy(encoder).double()
        with torch.no_grad():
            logp = asr.encode_batch(wav, lens)
            words, tokens = asr.transcribe_batch(wav, lens)
            f32 = norm(fbank(wav), lens)
            logp64 = torch.log_softmax(enc64.ctc_lin(enc64.enc(f32.double())), dim=-1)
            t64 = ctc_greedy_decode(logp64, lens.double(), blank_id=0)
        print("    greedy:", words)
        if t64 == tokens and all(len(t) > 1 for t in tokens):
            break
        print("    the fp64 run of the reference decodes differently (or an empty hypothesis): next seed")
    else:
        raise SystemExit("no seed found")
    C.check("the reference in fp64, log-probs", logp.double(), logp64, C.LOGP_BOUND / 4)
    norm._save(os.path.join(out_dir, "normalize.ckpt"))
    torch.save(torch.nn.ModuleList([enc, ctc_lin]).state_dict(), os.path.join(out_dir, "model.ckpt"))
    yaml = C.CRDNN_YAML.replace("%DECODING%", C.GREEDY_DECODING).replace("speechbrain.nnet.RNN.LSTM", "speechbrain.nnet.RNN.SLiGRU")
    yaml = yaml.replace("train_BPE_1000.yaml", "train_BPE_1000_sligru.yaml").replace("make_crdnn_golden", "make_sligru_golden")
    with open(os.path.join(out_dir, "hyperparams.yaml"), "w", encoding="utf-8") as f:
        f.write(yaml)
    # the waveforms are pretrained_crdnn_ctc_tiny_expected.npz's (wav, lens): not stored twice
    lstm = np.load(os.path.join(OUT, "pretrained_crdnn_ctc_tiny_expected.npz"))
    assert np.array_equal(lstm["wav"], wav.numpy()) and np.array_equal(lstm["lens"], lens.numpy())
    np.savez_compressed(os.path.join(OUT, "pretrained_crdnn_sligru_ctc_tiny_expected.npz"),
                        logp=logp.numpy(), greedy_words=np.array(words),
                        greedy_tokens=np.array([t + [-1] * (logp.shape[1] - len(t)) for t in tokens], dtype=np.int64))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    golden_model()
    golden_pretrained()
