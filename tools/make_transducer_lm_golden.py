"""Write tests/golden/transducer_beam_lm.npz and the model directory tests/golden/pretrained_transducer_lm_tiny with the
REFERENCE's own TransducerBeamSearcher.transducer_beam_search_decode (beam_size > 1) fused with the reference's own
lobes.models.RNNLM.RNNLM (lm_weight > 0) on the CPU.

Runs only where the reference checkout is available (SB_REFERENCE, as tools/make_transducer_golden.py resolves it).  The module wiring and the
steering of the blank row come from tools/make_transducer_golden.py, the expansion guard and the reference run from
tools/make_transducer_beam_golden.py, both by import; those tools' own fixtures are not regenerated.

    python tools/make_transducer_lm_golden.py [--model-directory-only]

Every case stores the weights of its transducer and of its LM (under ``lm.``, by the reference's state_dict names), `tn`, the
reference's n-best token lists and scores, the mean, the expansions of every frame, the LM's logits over a short token
sequence (for the RNNLM module's own test) and the smallest decision margin.  The margin is the one of
tools/make_transducer_beam_golden.py, measured by tests/transducer_lm_host_ref.py on the scores the hypotheses actually hold
(so it covers the LM terms) after that restatement has been checked to take the reference's path.  Seeds are drawn until the
reference stays under the cap with margin >= MIN_MARGIN, at most 100 per case.  The case `lm_decides` is also run with the
LM switched off and must then give another best hypothesis: the LM term demonstrably decides something.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_transducer_golden as G  # noqa: E402  (puts the reference and the stubs on sys.path)
import make_transducer_beam_golden as BG  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import transducer_lm_host_ref as R  # noqa: E402

OUT = G.OUT
MIN_MARGIN = BG.MIN_MARGIN
MODEL_MIN_MARGIN = BG.MODEL_MIN_MARGIN


def cases():
    base = dict(B=3, T=16, J=12, H=16, L=1, V=10, emb=None, act="gelu", cls_bias=True, proj_bias=True, S=5, seed=0,
                sharpen=3.0, blank_shift=4.0, hidden=False, pad=False, chunks=None, beam=4, nbest=5, state_beam=2.3,
                expand_beam=2.3, lm_weight=0.3, lm_E=6, lm_H=12, lm_L=1, lm_dnn=1, lm_D=8, lm_act="leaky_relu", lm_V=None,
                lm_sharpen=2.0, differs=False)
    out = []

    def add(name, **kw):
        c = dict(base, **kw)
        c["seed"] = 5000 + len(out)
        out.append((name, c))

    add("w03_l1_leaky_relu")
    add("w10_l2_relu", lm_weight=1.0, lm_L=2, lm_act="relu", lm_H=16)
    add("dnn2_gelu", lm_dnn=2, lm_act="gelu", lm_E=8, lm_H=24, lm_D=12)
    add("odd_sizes_tanh", lm_act="tanh", lm_H=15, lm_D=13, lm_dnn=2, lm_E=7, J=13, H=15, V=11, emb=5, L=2, T=12, B=2,
        sharpen=4.0)  # K % 4 != 0: the scalar path of the kernel's products, in the PN and in the LM
    add("wide_v70", V=70, J=20, H=24, B=2, T=8, lm_H=24, lm_D=16, lm_E=8)  # more than a wave, not a multiple of 64
    add("lm_vocab_larger", lm_V=17, lm_L=2)  # the LM's log-softmax runs over outputs the classifier does not have
    add("beam10_whole_row", beam=10, T=8, B=2)  # beam_size == V
    add("padded_b3", pad=True, lm_weight=1.0)
    add("lm_decides", lm_weight=1.0, lm_sharpen=6.0, blank_shift=3.0, differs=True)
    return out


def build_lm(c):
    from speechbrain.lobes.models.RNNLM import RNNLM

    torch.manual_seed(c["seed"] + 13)
    lm = RNNLM(output_neurons=c["lm_V"] or c["V"], embedding_dim=c["lm_E"], activation=G.ACTS[c["lm_act"]], dropout=0.0,
               rnn_layers=c["lm_L"], rnn_neurons=c["lm_H"], return_hidden=True, dnn_blocks=c["lm_dnn"],
               dnn_neurons=c["lm_D"]).eval()
    with torch.no_grad():
        for p in lm.rnn.parameters():
            p.mul_(2.0)
        lm.out.w.weight.mul_(c["lm_sharpen"])
        for name, p in lm.dnn.named_parameters():  # (LayerNorm's affine part off its identity initialisation)
            if ".norm." in name:
                p.add_(0.3 * torch.randn_like(p))
    return lm


def run_case(c):
    searcher, state = G.build(c)
    lm = build_lm(c)
    g = torch.Generator().manual_seed(c["seed"] + 7)
    tn = torch.randn(c["B"], c["T"], c["J"], generator=g)
    if c["pad"]:
        tn[1, c["T"] * 2 // 3:] = 0.0
        tn[2, c["T"] // 2:] = 0.0
    plain = None
    if c["differs"]:
        plain = BG.run_reference(searcher, tn, c["beam"], c["nbest"], c["state_beam"], c["expand_beam"])
        if plain is None:
            return "a frame reached the cap without the LM"
        searcher, _ = G.build(c)  # (a fresh guard)
    searcher.lm, searcher.lm_weight = lm, c["lm_weight"]
    ref = BG.run_reference(searcher, tn, c["beam"], c["nbest"], c["state_beam"], c["expand_beam"])
    if ref is None:
        return "a frame reached the cap"
    best, mean, nb, nbs, counts = ref
    if plain is not None and plain[0] == best:
        return "the best hypothesis is the one without the LM"
    if max(len(x) for x in best) < 2 or counts.mean() < 1.2:
        return "too few tokens or expansions to test anything"
    arrays = {k: v.numpy() for k, v in state.items()}
    arrays.update({f"lm.{k}": v.numpy() for k, v in lm.state_dict().items()})
    arrays["tn"] = tn.numpy()
    # the LM alone: logits of a short sequence, as the module's own test reads them
    toks = torch.randint(0, c["V"], (2, 5), generator=g)
    with torch.no_grad():
        logits, _ = lm(toks)
    arrays["lm_tokens"], arrays["lm_logits"] = toks.numpy().astype(np.int64), logits.numpy()
    net, hlm = R.Network(arrays, c["act"]), R.LM(arrays, c["lm_act"])
    try:
        host = R.beam_search(net, hlm, c["lm_weight"], arrays["tn"], 0, c["beam"], c["nbest"], c["state_beam"], c["expand_beam"])
    except R.ExpansionCap:
        return "the restatement reached the cap"
    same = host["nbest"] == nb and np.array_equal(host["expansions"], counts) and all(
        np.allclose(x, y, rtol=1e-5, atol=1e-5) for x, y in zip(host["scores"], nbs))
    res = dict(cfg=c, nbest=nb, scores=nbs, mean=mean, margin=host["margin"] if same else 0.0, path_agrees=bool(same),
               max_expansions=int(counts.max()), best_without_lm=None if plain is None else plain[0])
    arrays["expansions"] = counts.astype(np.int32)
    return res, arrays


def draw(item):
    name, c = item
    torch.set_num_threads(1)
    why = []
    for attempt in range(100):
        got = run_case(dict(c, seed=c["seed"] + 100 * attempt))
        if not isinstance(got, str) and got[0]["margin"] >= MIN_MARGIN:
            return got
        why.append(got if isinstance(got, str) else f"margin {got[0]['margin']:.5f} (path agrees: {got[0]['path_agrees']})")
    return f"{name}: no seed stays under the cap with margins above {MIN_MARGIN}: {why[:10]}"


def fixture():
    import multiprocessing

    out, meta = {}, []
    with multiprocessing.get_context("fork").Pool(8) as pool:
        drawn = pool.map(draw, cases(), chunksize=1)
    failed = [d for d in drawn if isinstance(d, str)]
    if failed:
        raise RuntimeError("\n".join(failed))
    for i, ((name, c), (res, arrays)) in enumerate(zip(cases(), drawn)):
        res["name"] = name
        out.update({f"c{i}.{k}": v for k, v in arrays.items()})
        meta.append(res)
        print(f"  {name:20s} seed {res['cfg']['seed']} best {[len(x[0]) for x in res['nbest']]} expansions mean "
              f"{arrays['expansions'].mean():.2f} max {res['max_expansions']} margin {res['margin']:.4f}", flush=True)
    assert any(m["best_without_lm"] is not None and m["best_without_lm"] != [n[0] for n in m["nbest"]] for m in meta)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "transducer_beam_lm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


LM_YAML = """lm_model: !new:speechbrain.lobes.models.RNNLM.RNNLM
    output_neurons: !ref <output_neurons>
    embedding_dim: 8
    activation: !name:torch.nn.LeakyReLU
    dropout: 0.0
    rnn_layers: 2
    rnn_neurons: 24
    dnn_blocks: 1
    dnn_neurons: 16
    return_hidden: True

Beamsearcher: !new:speechbrain.decoders.transducer.TransducerBeamSearcher
    decode_network_lst: [!ref <emb>, !ref <dec>, !ref <proj_dec>]
    tjoint: !ref <Tjoint>
    classifier_network: [!ref <transducer_lin>]
    blank_id: !ref <blank_index>
    beam_size: 4
    nbest: 3
    lm_module: !ref <lm_model>
    lm_weight: 0.5
    state_beam: 2.3
    expand_beam: 2.3

"""
LM_CFG = dict(V=40, lm_V=None, lm_E=8, lm_act="leaky_relu", lm_L=2, lm_H=24, lm_dnn=1, lm_D=16, lm_sharpen=4.0)


def model_directory():
    """tests/golden/pretrained_transducer_lm_tiny: pretrained_transducer_beam_tiny (its layout, inputs, normalizer,
    tokenizer and model.ckpt) with an RNNLM as the beam searcher's lm_module (lm_weight 0.5) and `lm` among the pretrainer's
    loadables.  The LM's weights are drawn (at most 100 seeds) until the reference's transcribe_batch stays under the cap with
    every decision made by MODEL_MIN_MARGIN.  (This acoustic model is blank-dominated: the LM moves the scores and the
    order below the best hypothesis; the fixture's `lm_decides` case is where it changes the best one.)"""
    import shutil

    import sentencepiece as spm
    from speechbrain.decoders.transducer import TransducerBeamSearcher
    from speechbrain.inference.ASR import EncoderDecoderASR
    from speechbrain.lobes.features import Fbank
    from speechbrain.lobes.models.convolution import ConvolutionFrontEnd
    from speechbrain.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    from speechbrain.nnet.containers import LengthsCapableSequential
    from speechbrain.nnet.embedding import Embedding
    from speechbrain.nnet.linear import Linear
    from speechbrain.nnet.RNN import LSTM
    from speechbrain.nnet.transducer.transducer_joint import Transducer_joint
    from speechbrain.processing.features import InputNormalization

    src = os.path.join(OUT, "pretrained_transducer_beam_tiny")
    d = os.path.join(OUT, "pretrained_transducer_lm_tiny")
    text = G.TRANSDUCER_YAML.replace("%INTERFACE%", G.OFFLINE)
    text = text.replace("# tiny sizes, as an inference hyperparams file.  Written by tools/make_transducer_golden.py.",
                        "# tiny sizes, as an inference hyperparams file with a beam searcher fused with an RNNLM as the decoder.\n"
                        "# Written by tools/make_transducer_lm_golden.py.")
    text = text.replace("tokenizer: !new:sentencepiece", LM_YAML + "tokenizer: !new:sentencepiece")
    text = text.replace("decoder: !ref <Greedysearcher>", "decoder: !ref <Beamsearcher>")
    text = text.replace("        model: !ref <model>\n", "        model: !ref <model>\n        lm: !ref <lm_model>\n")
    assert "lm: !ref <lm_model>" in text and "decoder: !ref <Beamsearcher>" in text and "lm_module: !ref <lm_model>" in text
    exp = np.load(os.path.join(OUT, "pretrained_transducer_tiny_expected.npz"))
    plain = np.load(os.path.join(OUT, "pretrained_transducer_beam_tiny_expected.npz"))
    plain_tokens = [[int(t) for t in row if t >= 0] for row in plain["tokens"]]
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    V, J, H = 40, 24, 32
    fb = Fbank(sample_rate=16000, n_fft=512, win_length=32, n_mels=80)
    norm = InputNormalization(norm_type="global")
    norm._load(os.path.join(src, "normalize.ckpt"), end_of_epoch=False)
    sp = spm.SentencePieceProcessor()
    sp.load(os.path.join(src, "tokenizer.ckpt"))
    cnn = ConvolutionFrontEnd(input_shape=(8, 10, 80), num_blocks=2, num_layers_per_block=1, out_channels=(64, 32),
                              kernel_sizes=(3, 3), strides=(2, 2), residuals=(False, False))
    tr = TransformerASR(input_size=640, tgt_vocab=V, d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=0,
                        d_ffn=64, dropout=0.0, activation=torch.nn.GELU, encoder_module="conformer",
                        attention_type="RelPosMHAXL", normalize_before=True, causal=False)
    enc = EncoderWrapper(tr)
    proj_enc = Linear(input_size=32, n_neurons=J, bias=False)
    emb = Embedding(num_embeddings=V, consider_as_one_hot=True, blank_id=0)
    dec = LSTM(input_shape=[None, None, V - 1], hidden_size=H, num_layers=1, re_init=True)
    proj_dec = Linear(input_size=H, n_neurons=J, bias=False)
    lin = Linear(input_size=J, n_neurons=V, bias=False)
    model = torch.nn.ModuleList([cnn, enc, emb, dec, proj_enc, proj_dec, lin]).eval()
    model.load_state_dict(torch.load(os.path.join(src, "model.ckpt"), map_location="cpu"))
    encoder = LengthsCapableSequential(input_shape=[None, None, 80], compute_features=fb, normalize=norm, CNN=cnn,
                                       enc=enc, proj_enc=proj_enc)
    why = []
    for attempt in range(100):
        lm = build_lm(dict(LM_CFG, seed=7100 + attempt))
        searcher = TransducerBeamSearcher(decode_network_lst=[emb, dec, proj_dec],
                                          tjoint=Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU),
                                          classifier_network=[lin], blank_id=0, beam_size=4, nbest=3, lm_module=lm,
                                          lm_weight=0.5, state_beam=2.3, expand_beam=2.3)
        asr = EncoderDecoderASR(modules={"encoder": encoder, "decoder": searcher},
                                hparams={"tokenizer": sp, "transducer_beam_search": True}, run_opts={"device": "cpu"})
        with torch.no_grad():
            tn = asr.encode_batch(wav, lens)
        counts = BG.guard(searcher, tn, 4 * searcher.beam_size)
        try:
            with torch.no_grad():
                words, tokens = asr.transcribe_batch(wav, lens)
        except BG.TooManyExpansions as e:
            why.append(str(e))
            continue
        arrays = {"emb.Embedding.weight": emb.state_dict()["Embedding.weight"].numpy()}
        for prefix, m in (("dec", dec), ("proj_dec", proj_dec), ("transducer_lin", lin), ("lm", lm)):
            arrays.update({f"{prefix}.{k}": v.numpy() for k, v in m.state_dict().items()})
        try:
            host = R.beam_search(R.Network(arrays, "gelu"), R.LM(arrays, "leaky_relu"), 0.5, tn.numpy(), 0, 4, 3, 2.3, 2.3)
        except R.ExpansionCap:
            why.append("the restatement reached the cap")
            continue
        agrees = [n[0] for n in host["nbest"]] == tokens and np.array_equal(host["expansions"], counts)
        n_tok = [len(t) for t in tokens]
        print(f"  LM seed {7100 + attempt}: tokens {n_tok}, expansions mean {counts.mean():.2f} max {counts.max()}, "
              f"margin {host['margin']:.4f}, path agrees {agrees}, best as without the LM {tokens == plain_tokens}", flush=True)
        if agrees and host["margin"] >= MODEL_MIN_MARGIN and max(n_tok) > 0:
            break
        why.append(f"margin {host['margin']:.5f}, tokens {n_tok}")
    else:
        raise RuntimeError(f"no LM seed stays under the cap with margins above {MODEL_MIN_MARGIN}: {why[:10]}")
    os.makedirs(d, exist_ok=True)
    for name in ("normalize.ckpt", "tokenizer.ckpt", "model.ckpt"):
        shutil.copyfile(os.path.join(src, name), os.path.join(d, name))
    torch.save(lm.state_dict(), os.path.join(d, "lm.ckpt"))
    with open(os.path.join(d, "hyperparams.yaml"), "w", encoding="utf-8") as f:
        f.write(text)
    pad = max(len(t) for t in tokens)
    np.savez_compressed(os.path.join(OUT, "pretrained_transducer_lm_tiny_expected.npz"), tn=tn.numpy(), words=np.array(words),
                        tokens=np.array([t + [-1] * (pad - len(t)) for t in tokens], dtype=np.int64),
                        margin=np.array([host["margin"]], dtype=np.float32), expansions=counts.astype(np.int32))
    print(f"  words {words}; wrote {d}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if "--model-directory-only" not in sys.argv:
        fixture()
    model_directory()
