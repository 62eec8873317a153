"""Write tests/golden/model_crdnn.npz and the CRDNN + CTC model directory tests/golden/pretrained_crdnn_ctc_tiny/ (with
tests/golden/pretrained_crdnn_ctc_tiny_expected.npz) with the REFERENCE's own CRDNN, savers, CTC decoders and EncoderASR.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference); it puts the reference and
oracle/ref_stubs on sys.path the way oracle/make_golden.py does and changes nothing under oracle/.

    python tools/make_crdnn_golden.py

model_crdnn.npz: n_mels 40, channels (4, 8), frequency pooling 2 / 2, time pooling 4, LSTM 2 x 12 bidirectional, DNN 2 x 16,
vocabulary 31; features [3,37,40] with relative lengths 0.6 / 0.8 / 1.0 (frames past a length are zeros: CRDNN itself takes no
lengths); the state dict, the output of each CNN block, of the time pooling, of each LSTM layer and of each DNN block, the
ctc_lin log-probabilities and the reference's greedy ids.  LayerNorm / BatchNorm affines are random and the running statistics
non-trivial.  Before anything is written, tests/crdnn_host_ref.py (the plain-torch restatement the kernel tests compare against)
is checked against the reference stage by stage at 1e-5, and the reference's own fp64 run must give the ids of its fp32 run (the
seed is advanced until it does, so that the exact-id tests are not decided by rounding); the reference's fp32-vs-fp64 distance is
printed per stage (it has to stay under a quarter of the tests' bounds: 5e-5 on the stages, 1e-4 on the log-probabilities).

The model directory has train_BPE_1000.yaml's encoder and CTC head at the same tiny sizes in the inference layout of
pretrained_ctc_tiny (the reference cannot parse YAML here -- oracle/ref_stubs/hyperpyyaml is an import stub -- so its EncoderASR
is built from modules wired exactly as the committed YAML describes); tokenizer and wav fixtures are pretrained_ctc_tiny's.
The beam searcher's hypotheses carry text, not ids: ``beam_ids`` are the label indices of the best hypotheses' characters.
"""
import copy
import functools
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
N_MELS, CHANNELS, POOLS, TIME_POOL, RNN_LAYERS, RNN_NEURONS, DNN_BLOCKS, DNN_NEURONS, VOCAB = 40, (4, 8), (2, 2), 4, 2, 12, 2, 16, 31
STAGE_BOUND, LOGP_BOUND = 5e-5, 1e-4


def check(name, ref, got, tol):
    d = float((ref - got).abs().max())
    print(f"  {name:44s} max|d| = {d:.3e}  (tol {tol:g})")
    assert d <= tol, name


def build_crdnn():
    from speechbrain.lobes.models.CRDNN import CRDNN
    from speechbrain.nnet.RNN import LSTM

    return CRDNN(input_shape=[None, None, N_MELS], activation=torch.nn.LeakyReLU, dropout=0.15, cnn_blocks=2,
                 cnn_channels=list(CHANNELS), cnn_kernelsize=(3, 3), inter_layer_pooling_size=list(POOLS), time_pooling=True,
                 using_2d_pooling=False, time_pooling_size=TIME_POOL, rnn_class=LSTM, rnn_layers=RNN_LAYERS,
                 rnn_neurons=RNN_NEURONS, rnn_bidirectional=True, rnn_re_init=True, dnn_blocks=DNN_BLOCKS,
                 dnn_neurons=DNN_NEURONS, use_rnnp=False)


def randomise(model, ctc_lin, seed, sharpen):
    """Random LayerNorm / BatchNorm affines and biases (default init is 1 / 0), non-trivial running statistics, a peaked head."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 1 or "norm" in n:
                p.add_(0.2 * torch.randn(p.shape, generator=g))
        for n, b in model.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
            elif n.endswith("num_batches_tracked"):
                b.fill_(1000)
        ctc_lin.w.weight.mul_(sharpen)


def stages_of(enc, ctc_lin, feats):
    """The reference's own intermediates, by forward hooks on its children."""
    got = {}
    hooks = []

    def rec(name):
        return lambda m, i, o: got.__setitem__(name, (o[0] if isinstance(o, tuple) else o).detach().clone())

    for i in range(2):
        hooks.append(enc.CNN[f"block_{i}"].register_forward_hook(rec(f"cnn_block{i}")))
    hooks.append(enc.time_pooling.register_forward_hook(rec("time_pooling")))
    for i in range(DNN_BLOCKS):
        hooks.append(enc.DNN[f"block_{i}"].register_forward_hook(rec(f"dnn_block{i}")))
    out = enc(feats)
    for h in hooks:
        h.remove()
    # torch.nn.LSTM does not expose its layers: layer l's output is the output of the same weights cut to l + 1 layers
    x = got["time_pooling"]
    x = x.reshape(x.shape[0], x.shape[1], -1)
    rnn = enc.RNN.rnn
    for l in range(RNN_LAYERS):
        one = torch.nn.LSTM(rnn.input_size if l == 0 else 2 * RNN_NEURONS, RNN_NEURONS, 1, batch_first=True, bidirectional=True)
        one = one.to(x.dtype)
        one.load_state_dict({k.replace(f"_l{l}", "_l0"): v for k, v in rnn.state_dict().items() if f"_l{l}" in k})
        x = one(x)[0]
        got[f"lstm_layer{l}"] = x.detach().clone()
    logp = torch.log_softmax(ctc_lin(out), dim=-1)
    return out, logp, got


def greedy_ids(logp, lens):
    from speechbrain.decoders.ctc import ctc_greedy_decode

    return ctc_greedy_decode(logp, lens, blank_id=0)


def golden_model():
    import crdnn_host_ref as R
    from speechbrain.nnet.linear import Linear

    lens = torch.tensor([0.6, 0.8, 1.0])
    for seed in range(41, 80):
        print(f"[model_crdnn, seed {seed}]")
        torch.manual_seed(seed)
        feats = torch.randn(3, 37, N_MELS, generator=torch.Generator().manual_seed(987 + seed))
        for b in range(3):
            feats[b, int(round(float(lens[b]) * 37)):] = 0
        enc = build_crdnn()
        enc(feats)  # (the reference instantiates its layers at the first call)
        ctc_lin = Linear(input_size=DNN_NEURONS, n_neurons=VOCAB)
        enc.eval(), ctc_lin.eval()
        randomise(enc, ctc_lin, seed + 1, 8.0)
        with torch.no_grad():
            out, logp, st = stages_of(enc, ctc_lin, feats)
            ids = greedy_ids(logp, lens)
            enc64, lin64 = copy.deepcopy(enc).double(), copy.deepcopy(ctc_lin).double()
            out64, logp64, st64 = stages_of(enc64, lin64, feats.double())
            ids64 = greedy_ids(logp64, lens.double())
        print("  greedy ids lens:", [len(h) for h in ids])
        if ids64 == ids and all(len(h) > 1 for h in ids):
            break
        print("  the fp64 run of the reference gives other ids (or an empty hypothesis): next seed")
    else:
        raise SystemExit("no seed found")
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        got, got_st = R.crdnn(feats, sd, POOLS, TIME_POOL, RNN_LAYERS, True, DNN_BLOCKS)
    for k in st:
        check(f"host restatement, {k}", st[k], got_st[k], 1e-5)
    check("host restatement, output", out, got, 1e-5)
    for k in st:
        check(f"the reference in fp64, {k}", st[k].double(), st64[k], STAGE_BOUND / 4)
    check("the reference in fp64, log-probs", logp.double(), logp64, LOGP_BOUND / 4)
    rec = {"feats": feats.numpy(), "wav_lens": lens.numpy(), "output": out.numpy(), "logp": logp.numpy(),
           "greedy_ids": np.array([h + [-1] * (logp.shape[1] - len(h)) for h in ids], dtype=np.int64),
           "ctc_lin/w.weight": ctc_lin.w.weight.detach().numpy(), "ctc_lin/w.bias": ctc_lin.w.bias.detach().numpy(),
           "cfg": np.array([N_MELS, *CHANNELS, *POOLS, TIME_POOL, RNN_LAYERS, RNN_NEURONS, DNN_BLOCKS, DNN_NEURONS, VOCAB], dtype=np.int64)}
    for k, v in st.items():
        rec[k] = v.numpy()
    for k, v in sd.items():
        rec[f"sd/{k}"] = v.numpy()
    path = os.path.join(OUT, "model_crdnn.npz")
    np.savez_compressed(path, **rec)
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


CRDNN_YAML = """\
# The encoder and CTC head of recipes/LibriSpeech/ASR/seq2seq/hparams/train_BPE_1000.yaml at tiny sizes, as an inference
# hyperparams.yaml for EncoderASR (the layout of pretrained_ctc_tiny).  Written by tools/make_crdnn_golden.py.
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
output_neurons: 31
blank_index: 0

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

ctc_lin: !new:speechbrain.nnet.linear.Linear
    input_size: !ref <dnn_neurons>
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

encoder: !new:speechbrain.nnet.containers.LengthsCapableSequential
    input_shape: [null, null, !ref <n_mels>]
    compute_features: !ref <compute_features>
    normalize: !ref <normalize>
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


def golden_pretrained():
    from speechbrain.dataio.encoder import CTCTextEncoder
    from speechbrain.decoders.ctc import CTCBeamSearcher, ctc_greedy_decode
    from speechbrain.inference.ASR import EncoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.linear import Linear
    from speechbrain.processing.features import InputNormalization

    print("[pretrained_crdnn_ctc_tiny]")
    out_dir = os.path.join(OUT, "pretrained_crdnn_ctc_tiny")
    os.makedirs(out_dir, exist_ok=True)
    shutil.copyfile(os.path.join(OUT, "pretrained_ctc_tiny", "tokenizer.ckpt"), os.path.join(out_dir, "tokenizer.ckpt"))
    tok = CTCTextEncoder()
    tok.load(os.path.join(out_dir, "tokenizer.ckpt"))
    assert sorted(tok.lab2ind.values()) == list(range(VOCAB)) and tok.get_blank_index() == 0
    # tones that change every 40 ms over noise (the signal of pretrained_ctc_tiny): frame-to-frame variety
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
    norm.glob_mean = feats.mean(dim=(0, 1))
    norm.glob_std = feats.std(dim=(0, 1))
    norm.count = 1000
    files = ["sample_mono.wav", "sample_stereo.wav"]
    for seed in range(57, 100):
        print(f"  seed {seed}")
        torch.manual_seed(seed)
        enc = build_crdnn()
        enc(feats)
        ctc_lin = Linear(input_size=DNN_NEURONS, n_neurons=VOCAB)
        enc.eval(), ctc_lin.eval()
        randomise(enc, ctc_lin, seed + 1, 8.0)
        with torch.no_grad():
            # a random head mostly reads the encoder's common direction (one label everywhere): project it out, as training would
            mu = enc(norm(feats, torch.ones(3))).mean(dim=(0, 1))
            w = ctc_lin.w.weight
            w.sub_(torch.outer(w @ mu, mu) / mu.dot(mu))
        encoder = LengthsCapableSequential(input_shape=[None, None, N_MELS], compute_features=fbank, normalize=norm, enc=enc,
                                           ctc_lin=ctc_lin, log_softmax=torch.nn.LogSoftmax(dim=-1))
        mk = lambda e, hp: EncoderASR(modules={"encoder": e}, hparams={"tokenizer": tok, **hp}, run_opts={"device": "cpu"})  # noqa: E731
        hp_g = {"decoding_function": functools.partial(ctc_greedy_decode, blank_id=0)}
        hp_b = {"decoding_function": CTCBeamSearcher, "test_beam_search": dict(blank_index=0, **BEAM_SETTINGS)}
        greedy, beam = mk(encoder, hp_g), mk(encoder, hp_b)
        enc64 = copy.deepcopy(encoder).double()
        enc64.normalize.glob_mean, enc64.normalize.glob_std = norm.glob_mean.double(), norm.glob_std.double()
        with torch.no_grad():
            logp = greedy.encode_batch(wav, lens)
            g_words, g_tokens = greedy.transcribe_batch(wav, lens)
            b_words, b_hyps = beam.transcribe_batch(wav, lens)
            g_file = [greedy.transcribe_file(os.path.join(OUT, f)) for f in files]
            b_file = [beam.transcribe_file(os.path.join(OUT, f)) for f in files]
            # the reference's fp64 run from the same fp32 features (the front end is not what this fixture is about)
            f32 = norm(fbank(wav), lens)
            logp64 = torch.log_softmax(enc64.ctc_lin(enc64.enc(f32.double())), dim=-1)
            g64 = ctc_greedy_decode(logp64, lens.double(), blank_id=0)
            b64 = CTCBeamSearcher(blank_index=0, vocab_list=[tok.ind2lab[i] for i in range(VOCAB)], **BEAM_SETTINGS)(logp64.float(), lens)
        b64_words = [h[0].text for h in b64]
        print("    greedy:", g_words, g_file)
        print("    beam:  ", b_words, b_file)
        ok = g64 == g_tokens and b64_words == b_words and all(len(t) > 1 for t in g_tokens) and all(len(w) > 0 for w in g_file)
        if ok:
            break
        print("    the fp64 run of the reference decodes differently (or an empty hypothesis): next seed")
    else:
        raise SystemExit("no seed found")
    check("the reference in fp64, log-probs", logp.double(), logp64, LOGP_BOUND / 4)
    norm._save(os.path.join(out_dir, "normalize.ckpt"))
    torch.save(torch.nn.ModuleList([enc, ctc_lin]).state_dict(), os.path.join(out_dir, "model.ckpt"))
    for name, dec in (("hyperparams.yaml", GREEDY_DECODING), ("hyperparams_beam.yaml", BEAM_DECODING)):
        with open(os.path.join(out_dir, name), "w", encoding="utf-8") as f:
            f.write(CRDNN_YAML.replace("%DECODING%", dec))
    np.savez_compressed(os.path.join(OUT, "pretrained_crdnn_ctc_tiny_expected.npz"), wav=wav.numpy(), lens=lens.numpy(),
                        logp=logp.numpy(), greedy_words=np.array(g_words),
                        greedy_tokens=np.array([t + [-1] * (logp.shape[1] - len(t)) for t in g_tokens], dtype=np.int64),
                        beam_words=np.array(b_words), beam_scores=np.array([float(h[0].score) for h in b_hyps]),
                        beam_ids=np.array([[tok.lab2ind[c] for c in h[0].text] + [-1] * (logp.shape[1] - len(h[0].text))
                                           for h in b_hyps], dtype=np.int64),
                        file_names=np.array(files), greedy_file_words=np.array(g_file), beam_file_words=np.array(b_file))
    for f in sorted(os.listdir(out_dir)):
        print(f"  {f}: {os.path.getsize(os.path.join(out_dir, f)) / 1024:.0f} KiB")


if __name__ == "__main__":
    golden_model()
    golden_pretrained()
