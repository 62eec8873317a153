"""Write tests/golden/transducer_beam.npz and the model directory tests/golden/pretrained_transducer_beam_tiny with the
REFERENCE's own TransducerBeamSearcher.transducer_beam_search_decode (beam_size > 1, no LM) on the CPU.

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference).  The module wiring, the
steering of the blank row and the model directory's YAML come from tools/make_transducer_golden.py by import; that tool's
own fixtures are not regenerated.

    python tools/make_transducer_beam_golden.py [--model-directory-only]

The reference's loop over the expansions of a frame has no bound: it never leaves a frame whose blank stays out of the top
beam_size.  Every run of the reference here therefore goes through a wrapper of its joint step that counts the expansions
of each frame and raises out of the search once a frame reaches the cap (4 * beam_size, the kernel's default); such a seed is
dropped.  Every case stores its weights, `tn`, the reference's n-best token lists and scores, the mean, the expansions of
every frame and its smallest decision margin.  The margin is the minimum over the whole search of: the gap between the k-th
and (k+1)-th log-probability of every top-k; |logp_j - (best_logp - expand_beam)| of every non-blank candidate;
|b_best - state_beam - a_best| at every check; the gap between the two best keys of A at every selection; the gaps between
adjacent keys of the final sort.  It is measured by tests/transducer_beam_host_ref.py after that restatement has been
checked to take the reference's path (the same tokens, scores and expansions).  Seeds are drawn until the margin is at least
MIN_MARGIN, at most 100 per case.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_transducer_golden as G  # noqa: E402  (puts the reference and the stubs on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import transducer_beam_host_ref as R  # noqa: E402

OUT = G.OUT
MIN_MARGIN = 2e-3
MODEL_MIN_MARGIN = 2e-3


class TooManyExpansions(RuntimeError):
    pass


def cases():
    base = dict(B=3, T=24, J=12, H=16, L=1, V=10, emb=None, act="gelu", cls_bias=True, proj_bias=True, S=5, seed=0,
                sharpen=3.0, blank_shift=5.0, hidden=False, pad=False, chunks=None, beam=4, nbest=5, state_beam=2.3,
                expand_beam=2.3, same_as_greedy=False)
    out = []

    def add(name, **kw):
        c = dict(base, **kw)
        c["seed"] = 3000 + len(out)
        out.append((name, c))

    add("beam2_gelu", beam=2)
    add("beam4_leaky_relu", act="leaky_relu")
    add("beam10_whole_row_tanh", beam=10, act="tanh")  # beam_size == V: the top-k takes the whole row
    add("beam4_relu_nbest1", act="relu", nbest=1)
    add("dense_l2_nobias", emb=6, L=2, cls_bias=False, proj_bias=False, blank_shift=40.0, T=12)  # (the shift acts through mean(z))
    add("dense_l1_beam10", emb=5, beam=10)
    add("wide_v40", V=40, J=20, H=24, B=2, T=8)
    add("wide_v70", V=70, J=20, H=24, B=2, T=8)  # more than one wave of tokens, not a multiple of 64
    add("odd_sizes", J=13, H=15, V=11, emb=5, L=2, act="tanh", T=12, B=2, sharpen=4.0)  # K % 4 != 0: the scalar path of the kernel's products
    add("one_frame", T=1, beam=4)
    add("blank_dominated", blank_shift=10.0, sharpen=4.0, same_as_greedy=True)  # the state_beam exit fires after one expansion
    add("blank_near_zero", blank_shift=0.5, sharpen=1.0, T=6, B=2)  # many expansions per frame
    add("padded_b3", pad=True)
    add("tight_beams", state_beam=0.5, expand_beam=0.5)  # both prunings bite
    add("loose_beams", state_beam=10.0, expand_beam=10.0, T=6, B=2)  # neither does
    return out


def guard(searcher, tn, cap):
    """Count the expansions of every (utterance, frame) through the searcher's joint step; raise once a frame reaches cap."""
    B, T, J = tn.shape
    counts = np.zeros((B, T), np.int64)
    inner = searcher._joint_forward_step
    base = tn.storage_offset()

    def step(h_i, out_PN):
        idx = (h_i.storage_offset() - base) // J
        counts[idx // T, idx % T] += 1
        if counts[idx // T, idx % T] >= cap:
            raise TooManyExpansions(f"frame {idx % T} of utterance {idx // T}: {cap} expansions")
        return inner(h_i, out_PN)

    searcher._joint_forward_step = step
    return counts


def run_reference(searcher, tn, beam, nbest, state_beam, expand_beam):
    """-> (best, mean, nbest tokens, nbest scores, expansions [B,T]) or None when a frame reached the cap"""
    searcher.beam_size, searcher.nbest = beam, nbest
    searcher.state_beam, searcher.expand_beam = state_beam, expand_beam
    counts = guard(searcher, tn, 4 * beam)
    try:
        with torch.no_grad():
            best, mean, nb, nbs = searcher.transducer_beam_search_decode(tn)
    except TooManyExpansions:
        return None
    return best, float(mean), nb, [[float(s) for s in row] for row in nbs], counts


def run_case(c):
    searcher, state = G.build(c)
    g = torch.Generator().manual_seed(c["seed"] + 7)
    tn = torch.randn(c["B"], c["T"], c["J"], generator=g)
    if c["pad"]:
        tn[1, c["T"] * 2 // 3:] = 0.0
        tn[2, c["T"] // 2:] = 0.0
    greedy = None
    if c["same_as_greedy"]:
        with torch.no_grad():
            greedy = searcher.transducer_greedy_decode(tn)[0]
    ref = run_reference(searcher, tn, c["beam"], c["nbest"], c["state_beam"], c["expand_beam"])
    if ref is None:
        return "a frame reached the cap"
    best, mean, nb, nbs, counts = ref
    if greedy is not None and greedy != best:
        return "the best hypothesis is not greedy's"
    if not c["same_as_greedy"] and (max(len(x) for x in best) < 2 or counts.mean() < 1.2):
        return "too few tokens or expansions to test anything"
    arrays = {k: v.numpy() for k, v in state.items()}
    arrays["tn"] = tn.numpy()
    # the margin, from the restatement once it is seen to take the reference's path
    net = R.Network(arrays, c["act"])
    try:
        host = R.beam_search(net, arrays["tn"], 0, c["beam"], c["nbest"], c["state_beam"], c["expand_beam"])
    except R.ExpansionCap:
        return "the restatement reached the cap"
    same = host["nbest"] == nb and np.array_equal(host["expansions"], counts) and all(
        np.allclose(x, y, rtol=1e-5, atol=1e-5) for x, y in zip(host["scores"], nbs))
    res = dict(cfg=c, nbest=nb, scores=nbs, mean=mean, margin=host["margin"] if same else 0.0, path_agrees=bool(same),
               max_expansions=int(counts.max()))
    arrays["expansions"] = counts.astype(np.int32)
    return res, arrays


def draw(item):
    """The first of at most 100 seeds of one case that stays under the cap with every decision made by MIN_MARGIN."""
    name, c = item
    torch.set_num_threads(1)
    why = []
    for attempt in range(100):
        got = run_case(dict(c, seed=c["seed"] + 100 * attempt))
        if not isinstance(got, str) and got[0]["margin"] >= MIN_MARGIN:
            return got
        why.append(got if isinstance(got, str) else f"margin {got[0]['margin']:.5f} (path agrees: {got[0]['path_agrees']})")
    return f"{name}: no seed stays under the cap with margins above {MIN_MARGIN}: {why[:10]}"


def main():
    if "--model-directory-only" not in sys.argv:
        fixture()
    model_directory()


def fixture():
    import multiprocessing

    out, meta = {}, []
    with multiprocessing.get_context("fork").Pool(8) as pool:  # (the cases are independent: one process each)
        drawn = pool.map(draw, cases(), chunksize=1)
    failed = [d for d in drawn if isinstance(d, str)]
    if failed:
        raise RuntimeError("\n".join(failed))
    for i, ((name, c), (res, arrays)) in enumerate(zip(cases(), drawn)):
        res["name"] = name
        out.update({f"c{i}.{k}": v for k, v in arrays.items()})
        meta.append(res)
        print(f"  {name:24s} seed {res['cfg']['seed']} best {[len(x[0]) for x in res['nbest']]} n-best "
              f"{[len(x) for x in res['nbest']]} expansions mean {arrays['expansions'].mean():.2f} max "
              f"{res['max_expansions']} margin {res['margin']:.4f}", flush=True)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, "transducer_beam.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


BEAM_SEARCHER = """Beamsearcher: !new:speechbrain.decoders.transducer.TransducerBeamSearcher
    decode_network_lst: [!ref <emb>, !ref <dec>, !ref <proj_dec>]
    tjoint: !ref <Tjoint>
    classifier_network: [!ref <transducer_lin>]
    blank_id: !ref <blank_index>
    beam_size: 4
    nbest: 3
    state_beam: 2.3
    expand_beam: 2.3

"""


MODEL_BLANK_BOOST = 2.0  # added to the blank row of the classifier (it has no bias): with the 2.0 of pretrained_transducer_tiny
# the reference's own beam search at beam_size 4 does not leave frame 4 of utterance 1 within 16 expansions


def model_directory():
    """tests/golden/pretrained_transducer_beam_tiny: the layout, sizes, inputs, normalizer and tokenizer of
    pretrained_transducer_tiny with a beam searcher (beam_size 4, nbest 3) as `decoder`, and model weights of its own, drawn
    (at most 100 seeds) until the reference's transcribe_batch stays under the cap with every decision made by
    MODEL_MIN_MARGIN and some utterance gets tokens.  The checkpoints of pretrained_transducer_tiny itself cannot serve:
    see MODEL_BLANK_BOOST."""
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

    src = os.path.join(OUT, "pretrained_transducer_tiny")
    d = os.path.join(OUT, "pretrained_transducer_beam_tiny")
    text = G.TRANSDUCER_YAML.replace("%INTERFACE%", G.OFFLINE)
    text = text.replace("# tiny sizes, as an inference hyperparams file.  Written by tools/make_transducer_golden.py.",
                        "# tiny sizes, as an inference hyperparams file with a beam searcher as the decoder.\n"
                        "# Written by tools/make_transducer_beam_golden.py.")
    text = text.replace("tokenizer: !new:sentencepiece", BEAM_SEARCHER + "tokenizer: !new:sentencepiece")
    text = text.replace("decoder: !ref <Greedysearcher>", "decoder: !ref <Beamsearcher>")
    assert "Written by tools/make_transducer_beam_golden.py" in text and "decoder: !ref <Beamsearcher>" in text
    exp = np.load(os.path.join(OUT, "pretrained_transducer_tiny_expected.npz"))
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    V, J, H = 40, 24, 32
    fb = Fbank(sample_rate=16000, n_fft=512, win_length=32, n_mels=80)
    norm = InputNormalization(norm_type="global")
    norm._load(os.path.join(src, "normalize.ckpt"), end_of_epoch=False)
    sp = spm.SentencePieceProcessor()
    sp.load(os.path.join(src, "tokenizer.ckpt"))
    why = []
    for attempt in range(100):
        torch.manual_seed(2100 + attempt)
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
        with torch.no_grad():
            z = proj_enc(tr.encode(cnn(norm(fb(wav), torch.ones(3))), torch.ones(3)))
            proj_enc.w.weight.mul_(2.0 / float(z.std()))  # joint inputs of unit scale
            lin.w.weight.mul_(10.0)
            lin.w.weight[0] += MODEL_BLANK_BOOST
        searcher = TransducerBeamSearcher(decode_network_lst=[emb, dec, proj_dec],
                                          tjoint=Transducer_joint(joint="sum", nonlinearity=torch.nn.GELU),
                                          classifier_network=[lin], blank_id=0, beam_size=4, nbest=3, state_beam=2.3,
                                          expand_beam=2.3)
        encoder = LengthsCapableSequential(input_shape=[None, None, 80], compute_features=fb, normalize=norm, CNN=cnn,
                                           enc=enc, proj_enc=proj_enc)
        asr = EncoderDecoderASR(modules={"encoder": encoder, "decoder": searcher},
                                hparams={"tokenizer": sp, "transducer_beam_search": True}, run_opts={"device": "cpu"})
        with torch.no_grad():
            tn = asr.encode_batch(wav, lens)
        counts = guard(searcher, tn, 4 * searcher.beam_size)
        try:
            with torch.no_grad():
                words, tokens = asr.transcribe_batch(wav, lens)
        except TooManyExpansions as e:
            why.append(str(e))
            continue
        arrays = {"emb.Embedding.weight": emb.state_dict()["Embedding.weight"].numpy()}
        for prefix, m in (("dec", dec), ("proj_dec", proj_dec), ("transducer_lin", lin)):
            arrays.update({f"{prefix}.{k}": v.numpy() for k, v in m.state_dict().items()})
        try:
            host = R.beam_search(R.Network(arrays, "gelu"), tn.numpy(), 0, 4, 3, 2.3, 2.3)
        except R.ExpansionCap:
            why.append("the restatement reached the cap")
            continue
        agrees = [n[0] for n in host["nbest"]] == tokens and np.array_equal(host["expansions"], counts)
        n_tok = [len(t) for t in tokens]
        print(f"  model seed {2100 + attempt}: tokens {n_tok}, expansions mean {counts.mean():.2f} max {counts.max()}, "
              f"margin {host['margin']:.4f}, path agrees {agrees}", flush=True)
        if agrees and host["margin"] >= MODEL_MIN_MARGIN and max(n_tok) > 0 and counts.mean() >= 1.2:
            break
        why.append(f"margin {host['margin']:.5f}, tokens {n_tok}")
    else:
        raise RuntimeError(f"no model seed stays under the cap with margins above {MODEL_MIN_MARGIN}: {why[:10]}")
    os.makedirs(d, exist_ok=True)
    for name in ("normalize.ckpt", "tokenizer.ckpt"):
        shutil.copyfile(os.path.join(src, name), os.path.join(d, name))
    torch.save(model.state_dict(), os.path.join(d, "model.ckpt"))
    with open(os.path.join(d, "hyperparams.yaml"), "w", encoding="utf-8") as f:
        f.write(text)
    pad = max(len(t) for t in tokens)
    np.savez_compressed(os.path.join(OUT, "pretrained_transducer_beam_tiny_expected.npz"), tn=tn.numpy(),
                        words=np.array(words), tokens=np.array([t + [-1] * (pad - len(t)) for t in tokens], dtype=np.int64),
                        margin=np.array([host["margin"]], dtype=np.float32), expansions=counts.astype(np.int32))
    print(f"  words {words}; wrote {d}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
