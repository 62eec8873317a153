"""The CTC and transducer decode kernels (csrc/ctc_decode.hip, csrc/transducer.hip) at the shapes where their strided loops
go round more than once: T past the 256-frame compaction chunk, vocabularies past 64 lanes and past the 256-token chunk of
the beam search, beams of 101..256, prediction networks with K % 4 != 0, H > 512, 2..4 LSTM layers, a frame block that has
to shrink to fit in LDS.  Inputs are generated from seeds; the references are a numpy arg-max collapse, the host
restatements tests/ctc_host_ref.py and tests/transducer_host_ref.py (pinned to the reference's fixtures by
test_ctc_decode.py / test_transducer.py) and torch.nn.LSTM in float64.  Every case runs on the CPU emulator and on the
MI355X through the `backend` fixture; the sizes the emulator cannot finish in about 10 s are GPU-only siblings (`*_full_size`)
of a smaller case that runs on both."""
import copy

import numpy as np
import pytest
import torch

import ctc_host_ref
import transducer_host_ref
from test_ctc_decode import MARGIN, _compare
from test_transducer_full_size_gpu import MIN_GAP


def _hip():
    """The shipped library on cuda:0, for the GPU-only siblings (what the `backend` fixture does for its 'hip' leg)."""
    import emu_utils
    from speechbrain_amd import native

    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    emu_utils.detach()
    native.load()
    return native, torch.device("cuda:0")


# ====================================================================================================== 1. CTC greedy
def _greedy_ref(x, rel, blank):
    """arg-max per frame over the first round(rel * T) frames (fp32 product, half to even, clamped to [0, T]), collapse
    repeats, drop blanks."""
    x = np.asarray(x, dtype=np.float32)
    B, T, _ = x.shape
    out = []
    for b in range(B):
        n = T if rel is None else int(min(max(np.rint(np.float32(rel[b]) * np.float32(T)), 0), T))
        path = x[b, :n].argmax(-1).tolist()  # (numpy: the first of equal maxima)
        out.append([t for j, t in enumerate(path) if t != blank and (j == 0 or path[j - 1] != t)])
    return out


def _greedy_random(seed, B, T, V, blank):
    """Noise plus a peak on a path of short runs over a handful of tokens and the blank, so that repeats, blanks and kept
    tokens all occur at every position modulo 256."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    pool = torch.cat([torch.randint(0, V, (6,), generator=g), torch.tensor([blank, blank])])
    pick = pool[torch.randint(0, len(pool), (B, T), generator=g)]
    hold = torch.rand(B, T, generator=g) < 0.4  # a frame repeats its predecessor's token
    for t in range(1, T):
        pick[:, t] = torch.where(hold[:, t], pick[:, t - 1], pick[:, t])
    x.scatter_add_(2, pick[..., None], torch.full((B, T, 1), 9.0))
    return x


def _check_greedy(backend, x, rel, blank, blank_arg=None, expect=None):
    """native.ctc_greedy_decode and decoders.ctc.ctc_greedy_decode (device and host tensors) against _greedy_ref."""
    from speechbrain_amd.decoders.ctc import ctc_greedy_decode

    native, dev = backend
    ref = _greedy_ref(x.numpy(), None if rel is None else rel.numpy(), blank)
    if expect is not None:
        assert ref == expect
    tokens, count = native.ctc_greedy_decode(x.to(dev), None if rel is None else rel.to(dev), blank)
    got = [row[:n] for row, n in zip(tokens.cpu().tolist(), count.cpu().tolist())]
    assert got == ref
    if rel is not None:  # (the utility takes a tensor of lengths, as the reference's does)
        blank_arg = blank if blank_arg is None else blank_arg
        if dev.type == "cuda":
            assert ctc_greedy_decode(x.to(dev), rel.to(dev), blank_id=blank_arg) == ref
        assert ctc_greedy_decode(x, rel, blank_id=blank_arg) == ref
    return ref


# every T of {255, 256, 257, 511, 512, 513, 1100} and every V of {1, 2, 63, 64, 65, 300, 5000}; blank first, last, middle
GREEDY_SHAPES = [(255, 1, 0), (256, 65, 64), (257, 300, 7), (511, 63, 0), (512, 64, 63), (513, 2, 1), (1100, 5, 4),
                 (256, 2, 0), (257, 64, 32), (513, 300, 150), (512, 5000, 4999), (1100, 5000, 2500), (255, 65, 0)]


@pytest.mark.parametrize("T,V,blank", GREEDY_SHAPES)
def test_ctc_greedy_chunk_and_lane_edges(backend, T, V, blank):
    """ctc_greedy_kernel at T > 256 (the second and later passes of the in-place compaction and the s_carry hand-over
    between them) and V > 64 (the second pass of the per-lane arg-max loop), blank at 0, V - 1 and in the middle, ragged
    relative lengths and None, blank_id = -1 through the Python utility."""
    B = 3
    x = _greedy_random(1000 + T + V, B, T, V, blank)
    rel = torch.tensor([1.0, 0.37, (256.0 if T > 256 else 130.0) / T])  # (the third ends on / near a chunk edge)
    ref = _check_greedy(backend, x, rel, blank, blank_arg=-1 if blank == V - 1 else None)
    _check_greedy(backend, x, None, blank)
    if V > 2:
        assert len(ref[0]) > T // 8 and len(ref[0]) < T  # the path both keeps and drops frames


def _one_hot_rows(paths, V):
    x = torch.full((len(paths), len(paths[0]), V), -10.0)
    for b, p in enumerate(paths):
        x[b, torch.arange(len(p)), torch.tensor(p)] = 0.0
    return x


def test_ctc_greedy_hand_made_rows_on_the_chunk_boundary(backend):
    """A repeat or a blank lying on a 256-frame boundary of ctc_greedy_kernel: a token repeated across frames 250..262
    emits once, twice with a blank at frame 255 or 256 inside the run; an all-blank utterance; one that emits at every
    frame (the compaction writes as far forward as it can); a token in frame 256 whose predecessor in frame 255 is the
    same token (the s_carry hand-over of the previous chunk's last arg-max)."""
    T, V, blank = 600, 7, 3
    run = [blank] * 250 + [5] * 13 + [blank] * (T - 263)
    with255, with256 = list(run), list(run)
    with255[255], with256[256] = blank, blank
    alternating = [1 + (t & 1) for t in range(T)]
    # frames 0..255 all kept, so the running count sits at the chunk edge; frame 256 repeats frame 255, frame 512 repeats 511
    carry = [1 + (t & 1) for t in range(255)] + [6, 6] + [blank if t % 3 else 4 for t in range(257, 511)] + [2, 2] + \
        [blank] * (T - 513)
    paths = [run, with255, with256, [blank] * T, alternating, carry]
    expect = [[5], [5, 5], [5, 5], [], alternating, _greedy_ref(_one_hot_rows([carry], V).numpy(), None, blank)[0]]
    assert expect[5][255:257] == [6, 4] and expect[5][-1] == 2 and expect[5].count(2) == 128  # (127 in 0..254, one at 511)
    _check_greedy(backend, _one_hot_rows(paths, V), torch.ones(len(paths)), blank, expect=expect)
    _check_greedy(backend, _one_hot_rows(paths, V), None, blank, expect=expect)


def test_ctc_greedy_half_frame_lengths_ties_and_many_workgroups(backend):
    """ctc_greedy_kernel's length rule where rel * T lands on .5 (12.5 -> 12, 13.5 -> 14: half to even), at 0, 1, slightly
    above 1; exact ties inside a frame (the first index wins, also when the equal maxima sit in different passes of the
    per-lane loop, V > 64); B = 1 and B = 70 workgroups."""
    T, V, blank = 256, 300, 0
    x = _greedy_random(5, 8, T, V, blank)
    rel = torch.tensor([12.5 / T, 13.5 / T, 0.0, 1.0, 1.0 + 1.0 / 1024, 0.5 / T, 1.5 / T, 255.5 / T])
    assert [int(np.rint(np.float32(r) * np.float32(T))) for r in rel.numpy()] == [12, 14, 0, 256, 256, 0, 2, 256]
    ref = _check_greedy(backend, x, rel, blank)
    assert ref[2] == [] and ref[5] == []
    # ties: two equal maxima per frame, at (lane, pass) pairs that differ in the lane, in the pass, or in both
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 257, V, generator=g)
    pairs = [(3, 67), (70, 200), (64, 128), (1, 2), (130, 299), (63, 64), (5, 261)]
    for t in range(257):
        i, j = pairs[t % len(pairs)]
        x[:, t, i] = x[:, t, j] = 7.0 + (t % 3)
    ref = _check_greedy(backend, x, torch.ones(2), blank)
    assert ref[0][:4] == [3, 70, 64, 1]
    for B in (1, 70):
        _check_greedy(backend, _greedy_random(7 + B, B, 300, 40, 39), torch.linspace(0.5, 1.0, B), 39, blank_arg=-1)


# ====================================================================================================== 2. CTC beam search
def _chars(n, blank=0):
    """A character vocabulary of n unique single characters with the blank at `blank` and the space right after it."""
    letters = [chr(ord("a") + i) for i in range(26)] + ["'"] + [chr(0x100 + i) for i in range(n)]  # (none is whitespace)
    v = letters[:n]
    v[blank] = "<b>"
    v[(blank + 1) % n] = " "
    return v


def _pieces(n, blank=0):
    """A SentencePiece-style vocabulary of n unique pieces, about a third of them word-initial (leading U+2581), of one to
    three letters, so that different piece paths spell the same text."""
    out, i = [], 0
    while len(out) < n:
        s, k = "", i
        while True:
            s = chr(ord("a") + k % 26) + s
            k = k // 26 - 1
            if k < 0:
                break
        out.append(("▁" if i % 3 == 0 else "") + s)
        i += 1
    out[blank] = "<blank>"
    return out


def _beam_logp(seed, B, T, V, Vl, blank, peak=(4.0, 6.0), blank_share=0.5):
    """log_softmax of noise plus a peak of 4 to 6 on a random target, about half of the frames blank."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g)
    tgt = torch.randint(0, Vl, (B, T), generator=g)
    tgt[torch.rand(B, T, generator=g) < blank_share] = blank
    pk = peak[0] + (peak[1] - peak[0]) * torch.rand(B, T, generator=g)
    x.scatter_add_(2, tgt[..., None], pk[..., None])
    return torch.log_softmax(x, -1)


def _check_beam(backend, x, lens, vocab, blank, stats=None, **kw):
    """CTCBeamSearcher.__call__ against ctc_host_ref.beam_search, compared as test_ctc_decode._compare does.  The
    restatement runs with one hypothesis more than topk, so that the last returned hypothesis, too, is only compared when
    its rank is decided by more than the margin.  Asserts that >= 80 % of the hypotheses and every utterance's best one
    were compared; returns the reference and the share compared."""
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher

    native, dev = backend
    topk = kw.get("topk", 1)
    ref = ctc_host_ref.beam_search(x, lens, blank=blank, vocab=vocab, **dict(kw, topk=topk + 1))
    result = []
    for hl in ref:
        scores = [float(h.score) for h in hl]
        gaps = [scores[k] - scores[k + 1] for k in range(len(scores) - 1)][:topk]
        hl = hl[:topk]
        result.append(dict(text=[h.text for h in hl], score=scores[:topk], gaps=gaps,
                           text_frames=[[[w, list(f)] for w, f in h.text_frames] for h in hl]))
        assert not gaps or gaps[0] > MARGIN, "the inputs must decide every utterance's best hypothesis"
    s = CTCBeamSearcher(blank_index=blank, vocab_list=vocab, **kw)
    if x.shape[-1] != len(vocab):
        with pytest.warns(UserWarning):
            hyps = s(x.to(dev), None if lens is None else lens.to(dev))
    else:
        hyps = s(x.to(dev), None if lens is None else lens.to(dev))
    own = {"checked": 0, "total": 0}
    _compare(hyps, dict(result=result), kw, own)
    print(f"\n[decode-shapes] beam {kw} V={x.shape[-1]} Vl={len(vocab)} T={x.shape[1]}: compared "
          f"{own['checked']}/{own['total']}")
    assert own["checked"] >= 0.8 * own["total"], own
    if stats is not None:
        stats["checked"] += own["checked"]
        stats["total"] += own["total"]
    return ref, own


@pytest.mark.parametrize("beam,prune_history", [(128, False), (256, True)])
def test_ctc_beam_second_vocabulary_chunk_and_wide_beams(backend, beam, prune_history):
    """ctc_beam_kernel at Vl > 256 (the second vocabulary chunk c0 += 256, s_tok / s_scan re-used across chunks, the
    per-thread arg-max loop going round twice) with beam 101..256: a character vocabulary padded to 300 entries at beam
    128 (prune_history off) and 256 (on)."""
    x = _beam_logp(31 + beam, 2, 60, 300, 300, 0)
    _check_beam(backend, x, torch.tensor([1.0, 0.8]), _chars(300), 0, beam_size=beam, topk=4, prune_history=prune_history)


@pytest.mark.gpu
@pytest.mark.parametrize("beam,prune_history", [(128, True), (256, False)])
def test_ctc_beam_second_vocabulary_chunk_and_wide_beams_full_size(beam, prune_history):
    """The sibling of test_ctc_beam_second_vocabulary_chunk_and_wide_beams with prune_history the other way round, T = 120
    and B = 4."""
    x = _beam_logp(41 + beam, 4, 120, 300, 300, 0)
    _check_beam(_hip(), x, torch.tensor([1.0, 0.8, 0.55, 0.3]), _chars(300), 0, beam_size=beam, topk=4,
                prune_history=prune_history)


@pytest.mark.parametrize("n,beam,T,peak,floor", [(600, 101, 40, (4.0, 6.0), -5.0), (1000, 200, 30, (4.0, 6.0), -5.0),
                                                 (5000, 10, 120, (6.0, 8.0), -7.0)])
def test_ctc_beam_sentencepiece_vocabulary_of_realistic_size(backend, n, beam, T, peak, floor):
    """ctc_beam_kernel on a SentencePiece vocabulary of realistic size (pieces with and without a leading U+2581): 600
    pieces / beam 101, 1 000 pieces / beam 200, 5 000 pieces / beam 10 (the CTC-BPE setting: twenty vocabulary chunks).  The
    noise of 5 000 entries alone weighs e^9, so there the peak is 6 to 8 and token_prune_min_logp -7: with these the
    restatement's beam is full (10 of 10) at every frame, with the default -5 it holds two hypotheses on average."""
    x = _beam_logp(50 + n, 2, T, n, n, 0, peak=peak)
    _check_beam(backend, x, torch.tensor([1.0, 0.7]), _pieces(n), 0, beam_size=beam, topk=3, token_prune_min_logp=floor)


@pytest.mark.gpu
@pytest.mark.parametrize("n,beam,T,peak,floor", [(600, 101, 300, (4.0, 6.0), -5.0), (1000, 200, 120, (4.0, 6.0), -5.0),
                                                 (5000, 10, 300, (6.0, 8.0), -7.0)])
def test_ctc_beam_sentencepiece_vocabulary_of_realistic_size_full_size(n, beam, T, peak, floor):
    """The sibling of test_ctc_beam_sentencepiece_vocabulary_of_realistic_size at T up to 300."""
    x = _beam_logp(60 + n, 2, T, n, n, 0, peak=peak)
    _check_beam(_hip(), x, torch.tensor([1.0, 0.7]), _pieces(n), 0, beam_size=beam, topk=3, token_prune_min_logp=floor)


def test_ctc_beam_topk_equal_to_beam_size_fills_slots_above_100(backend):
    """ctc_beam_kernel with topk == beam_size = 160 on a flat input and a low token_prune_min_logp: the restatement itself
    returns more than 100 hypotheses, so beam slots above 100 were live and are compared."""
    g = torch.Generator().manual_seed(16)  # (of seeds 1..39 the restatement leaves all 257 hypotheses decided at 16, 22, 27)
    x = torch.log_softmax(0.7 * torch.randn(2, 9, 7, generator=g), -1)
    vocab = ["<b>", " ", "a", "b", "c", "d", "e"]
    ref, own = _check_beam(backend, x, None, vocab, 0, beam_size=160, topk=160, beam_prune_logp=-40.0,
                           token_prune_min_logp=-20.0, prune_history=False)
    assert max(len(hl) for hl in ref) > 100, [len(hl) for hl in ref]
    assert own["checked"] > 100


@pytest.mark.parametrize("V,Vl,blank", [(256, 256, 0), (257, 257, 5), (512, 512, 511), (320, 300, 299)])
def test_ctc_beam_chunk_edges_wide_logits_and_blank_index(backend, V, Vl, blank):
    """ctc_beam_kernel at Vl exactly 256, 257 and 512 (the edges of the 256-token chunk), Vl < V (logits wider than the
    vocabulary: 300 of 320) and a blank index other than 0 (5, Vl - 1).  The reference's CTCBeamSearcher treats the blank
    by index in the frame skip and in the blank branch of the expansion only, which is where the restatement uses it."""
    x = _beam_logp(70 + V, 2, 40, V, Vl, blank)
    if blank == Vl - 1:  # the last entry of the last chunk also as a frame's arg-max and as a kept regular neighbour
        x[0, 3, Vl - 2] = x[0, 3].max() + 0.5
    _check_beam(backend, x, torch.tensor([1.0, 0.6]), _chars(Vl, blank), blank, beam_size=32, topk=4)


def test_ctc_beam_argmax_in_second_chunk_below_the_token_floor(backend):
    """ctc_beam_kernel keeps the arg-max token of a frame although it lies in the second vocabulary chunk and below
    token_prune_min_logp (kept only because it is the arg-max)."""
    x = _beam_logp(81, 2, 40, 300, 300, 0)
    g = torch.Generator().manual_seed(82)
    flat = [4, 5, 17, 30]
    for t in flat:
        row = 0.05 * torch.randn(2, 300, generator=g)
        row[0, 256 + t] += 0.5
        row[1, 299] += 0.5
        x[:, t] = torch.log_softmax(row, -1)
    for t in flat:  # the precondition: nothing passes the floor, the arg-max is in the second chunk
        assert float(x[:, t].max()) < -5.0 and int(x[0, t].argmax()) == 256 + t and int(x[1, t].argmax()) == 299
    ref, _ = _check_beam(backend, x, None, _chars(300), 0, beam_size=40, topk=3, token_prune_min_logp=-5.0)
    assert chr(0x100 + 299 - 27) in ref[1][0].text


def test_ctc_beam_ragged_lengths_and_forty_workgroups(backend):
    """ctc_beam_kernel with B = 40 workgroups and ragged lengths, among them utterances whose int(T * rel) is 0 (the empty
    hypothesis with score 0)."""
    B, T = 40, 24
    x = _beam_logp(91, B, T, 40, 40, 0)
    lens = torch.linspace(0.0, 1.0, B)
    lens[7] = 0.9 / T
    ref, _ = _check_beam(backend, x, lens, _chars(40), 0, beam_size=12, topk=2)
    assert ref[0][0].text == "" and float(ref[0][0].score) == 0.0 and ref[7][0].text == ""


def test_ctc_beam_blank_skip_crosses_runs_of_frames(backend):
    """ctc_beam_kernel with blank_skip_threshold < 1 on a long input (T = 600): whole runs of frames are skipped and the
    backtrack crosses them (fproc / the -1 entries of the path)."""
    B, T, V = 2, 600, 31
    x = _beam_logp(95, B, T, V, V, 0, peak=(7.0, 9.0), blank_share=0.7)
    skipped = (x[:, :, 0] > float(np.log(0.9))).float().mean()
    assert 0.4 < float(skipped) < 0.9, skipped
    ref, _ = _check_beam(backend, x, torch.tensor([1.0, 0.75]), _chars(V), 0, beam_size=24, topk=3,
                         blank_skip_threshold=0.9)
    assert len(ref[0][0].text) > 50


# ====================================================================================================== 3. transducer, LSTM
ACTS = {"gelu": torch.nn.GELU, "leaky_relu": torch.nn.LeakyReLU, "tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}


def _transducer(V, J, H, L, emb_dim, act, blank, seed):
    """The full-size test's construction (test_transducer_full_size_gpu.py) at any size: LSTM weights x 2, classifier x 8
    with a bias of 14 on the blank.  -> (modules, state dict by the reference's names for the host restatement)."""
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import LSTM

    torch.manual_seed(seed)
    if emb_dim is None:
        emb = Embedding(num_embeddings=V, consider_as_one_hot=True, blank_id=blank)
    else:
        emb = Embedding(num_embeddings=V, embedding_dim=emb_dim)
    dec = LSTM(input_shape=[None, None, emb.embedding_dim], hidden_size=H, num_layers=L)
    proj = Linear(input_size=H, n_neurons=J, bias=False)
    lin = Linear(input_size=J, n_neurons=V, bias=True)
    with torch.no_grad():
        for p in dec.parameters():
            p.mul_(2.0)
        lin.w.weight.mul_(8.0)
        lin.w.bias.zero_()
        lin.w.bias[blank] = 14.0
    sd = {"emb.Embedding.weight": emb.Embedding.weight.detach().numpy().copy(),
          "proj_dec.w.weight": proj.w.weight.detach().numpy().copy(),
          "transducer_lin.w.weight": lin.w.weight.detach().numpy().copy(),
          "transducer_lin.w.bias": lin.w.bias.detach().numpy().copy()}
    for k, v in dec.state_dict().items():
        sd[f"dec.{k}"] = v.numpy().copy()
    return (emb, dec, proj, lin), sd


def _tn(seed, B, T, J, lin_w, V, blank, every):
    """The full-size test's input: noise, frames that force one token whatever the PN says (every third utterance, every
    `every` frames: they hit the cap), and blank-heavy utterances."""
    g = torch.Generator().manual_seed(seed)
    tn = torch.randn(B, T, J, generator=g)
    forced = list(range(min(7, T - 1), T, every))
    for b in range(0, B, 3):
        for t in forced:
            k = (blank + 1 + (b * 7 + t) % (V - 1)) % V
            tn[b, t] = 30.0 * lin_w[k] / lin_w[k].norm()
    tn[1::4, :, :] *= 0.25
    return tn, forced


def _searcher(mods, act, blank, dev):
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint

    for m in mods:
        m.to(dev)
    emb, dec, proj, lin = mods
    return TransducerBeamSearcher([emb, dec, proj], Transducer_joint(nonlinearity=ACTS[act]), [lin], blank, beam_size=1)


def _check_transducer(backend, V, J, H, L, emb_dim, act, blank, B, T, S=5, every=41, seed=17, carried=False, frame_block=0,
                      mix=True):
    """The device search against transducer_host_ref.greedy as test_transducer_full_size_gpu.py compares them: tokens
    equal for utterances whose smallest decision gap exceeds MIN_GAP, final out_pn / h / c within 1e-4 * max(1, |ref|), at
    least half of the utterances decided, and the emission mix of the input (capped frames, blank-heavy and busy
    utterances).  `carried`: the search starts from a given state (start_from_blank = False)."""
    native, dev = backend
    mods, sd = _transducer(V, J, H, L, emb_dim, act, blank, seed)
    tn, forced = _tn(seed + 1, B, T, J, mods[3].w.weight.detach(), V, blank, every)
    net = transducer_host_ref.Network(sd, act)
    state, hidden = None, None
    if carried:
        g = torch.Generator().manual_seed(seed + 2)
        st = [0.5 * torch.randn(B, 1, J, generator=g), 0.5 * torch.randn(L, B, H, generator=g).tanh(),
              torch.randn(L, B, H, generator=g)]
        state = (st[0][:, 0].numpy(), st[1].numpy(), st[2].numpy())
        hidden = (st[0].clone().to(dev), (st[1].clone().to(dev), st[2].clone().to(dev)))
    toks, r_score, r_out, r_h, r_c, gaps = transducer_host_ref.greedy(net, tn.numpy(), blank, S, state)
    decided = [b for b in range(B) if min(gaps[b]) > MIN_GAP]
    n_emit = [len(t) for t in toks]
    print(f"\n[decode-shapes] transducer V={V} J={J} H={H} L={L} B={B} T={T} S={S}: decided {len(decided)}/{B}, "
          f"emissions {n_emit}")
    assert 2 * len(decided) >= B, (len(decided), B)
    if mix:
        capped = sum(1 for b in range(0, B, 3) if n_emit[b] >= (S + 1) * len(forced))
        assert capped > 0 and min(n_emit) < T // 4 and max(n_emit) > T // 4, n_emit
    s = _searcher(mods, act, blank, dev)
    hyps, _, _, _, (out_pn, (h, c)) = s.transducer_greedy_decode(tn.to(dev), hidden_state=hidden, return_hidden=True,
                                                                 max_symbols_per_step=S, frame_block=frame_block)
    for m in mods:
        m.cpu()
    assert all(len(hy) <= T * (S + 1) for hy in hyps)
    for b in decided:
        assert hyps[b] == toks[b], b
        for got, ref in ((out_pn[b, 0], r_out[b]), (h[:, b], r_h[:, b]), (c[:, b], r_c[:, b])):
            got = got.cpu().numpy()
            assert float(np.abs(got - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max())), b
    return hyps


def test_transducer_odd_sizes_take_the_scalar_gemv_path(backend):
    """transducer_greedy_kernel with J 645, H 515, V 1003, 2 LSTM layers, a dense embedding of width 77 and tanh: the
    scalar path of gemv_rows (K % 4 != 0) with every lane looping more than once (K > 64), V not a multiple of 64, H > 512
    (lstm_update looping), a dense embedding at size."""
    _check_transducer(backend, V=1003, J=645, H=515, L=2, emb_dim=77, act="tanh", blank=0, B=2, T=20, every=11)


@pytest.mark.gpu
def test_transducer_odd_sizes_take_the_scalar_gemv_path_full_size():
    """The sibling of test_transducer_odd_sizes_take_the_scalar_gemv_path at B = 32, T = 250."""
    _check_transducer(_hip(), V=1003, J=645, H=515, L=2, emb_dim=77, act="tanh", blank=0, B=32, T=250)


def test_transducer_four_layers_h1024(backend):
    """transducer_greedy_kernel with H 1024 (lstm_update and the state copies looping), 4 LSTM layers at recipe size
    (layer_ptr's every case), J 512, V 500 (not a multiple of 64), one-hot embedding."""
    _check_transducer(backend, V=500, J=512, H=1024, L=4, emb_dim=None, act="gelu", blank=0, B=1, T=4, S=2, every=11, mix=False)


@pytest.mark.gpu
def test_transducer_four_layers_h1024_full_size():
    """The sibling of test_transducer_four_layers_h1024 at B = 32, T = 250, with the emission mix asserted."""
    _check_transducer(_hip(), V=500, J=512, H=1024, L=4, emb_dim=None, act="gelu", blank=0, B=32, T=250)


def _run_binding(s, tn, dev, frame_block, S=None):
    """One search through native.transducer_greedy -> tokens, scores, out_pn, h, c (the searcher returns no scores)."""
    from speechbrain_amd import native

    prep = s._prepare(dev)
    (B, T, J), L, H = tn.shape, prep.W.n_layers, prep.W.hidden
    st = [torch.empty(B, J, device=dev), torch.empty(L, B, H, device=dev), torch.empty(L, B, H, device=dev)]
    tokens, count, score = native.transducer_greedy(prep, tn.to(dev), st[0], st[1], st[2], s.blank_id, s.S if S is None else S,
                                                    start_from_blank=True, act=s.tjoint.act_code, frame_block=frame_block)
    hyps = [row[:n] for row, n in zip(tokens.cpu().tolist(), count.cpu().tolist())]
    return (hyps, score.cpu().numpy()) + tuple(t.cpu().numpy() for t in st)


def _run_block(s, tn, dev, frame_block, S=5):
    hyps, _, _, _, (out_pn, (h, c)) = s.transducer_greedy_decode(tn.to(dev), return_hidden=True, max_symbols_per_step=S,
                                                                 frame_block=frame_block)
    return hyps, out_pn.cpu().numpy(), h.cpu().numpy(), c.cpu().numpy()


def _check_block_shrink(backend, B, T, every, S, blocks, emb_dim=None):
    # td_lds_bytes = 4 * (F * J + F * V + J + 2 * L * H + 8 * H) = 4 * (6 024 F + 1 024 + 2 560 + 5 120) at J 1024, V 5000,
    # H 640, L 2: F = 8 -> 227 584 B, F = 6 -> 179 392 B, F = 5 -> 155 296 B.  The kernel may use 160 KiB less its 80 B of
    # static LDS = 163 760 B, so the launcher has to shrink the default block of 8 to 5, and 155 296 B is above 64 KiB.
    V, J, H, L = 5000, 1024, 640, 2
    lds = lambda F: 4 * (F * J + F * V + J + 2 * L * H + 8 * H)  # noqa: E731
    assert lds(8) == 227584 and lds(6) > 160 * 1024 - 80 >= lds(5) == 155296 > 64 * 1024
    native, dev = backend
    hyps = _check_transducer(backend, V=V, J=J, H=H, L=L, emb_dim=emb_dim, act="relu", blank=0, B=B, T=T, S=S, every=every, seed=23,
                             mix=S == 5)
    mods, _ = _transducer(V, J, H, L, emb_dim, "relu", 0, 23)
    tn, _ = _tn(24, B, T, J, mods[3].w.weight.detach(), V, 0, every)
    s = _searcher(mods, "relu", 0, dev)
    s.S = S
    # the work the launcher reports counts one pass over the classifier per frame block: ceil(T / 5) passes
    native.prof_reset()
    native.prof_enable(True)
    a = _run_binding(s, tn, dev, 0)
    native.prof_enable(False)
    rep = native.prof_report()["transducer_greedy"]
    expect = 4.0 * B * T * J + 4.0 * J * V * B * (-(-T // 5)) + 4.0 * (4.0 * H) * H * L * B
    assert rep["count"] == 1 and abs(rep["bytes"] - expect) <= 1e-5 * expect, (rep, expect)  # (printed with 7 digits)
    assert a[0] == hyps
    for fb in blocks:  # tokens, scores and the final state, bit for bit
        other = _run_binding(s, tn, dev, fb)
        assert other[0] == a[0], fb
        for x, y in zip(other[1:], a[1:]):
            assert np.array_equal(x, y), fb


def test_transducer_frame_block_shrinks_to_fit_lds(backend):
    """transducer_greedy_kernel at V 5000, J 1024, H 640, 2 layers: the shrinking of the frame block when F * (J + V) does
    not fit in LDS (8 -> 5) and the more-than-64-KiB LDS request (155 296 B).  Tokens, final state and scores are bit-equal
    to the same search with frame_block = 1 (and 8, 5), and agree with the host restatement."""
    _check_block_shrink(backend, B=1, T=6, every=6, S=1, blocks=(1,), emb_dim=32)  # (dense: folding a 5000-wide one-hot is slow on the emulator)


@pytest.mark.gpu
def test_transducer_frame_block_shrinks_to_fit_lds_full_size():
    """The sibling of test_transducer_frame_block_shrinks_to_fit_lds at B = 32, T = 250."""
    _check_block_shrink(_hip(), B=32, T=250, every=41, S=5, blocks=(1, 8, 5, 3))


@pytest.mark.parametrize("T,frame_block,S", [(9, 0, 5), (1, 0, 5), (17, 3, 5), (17, 7, 1), (17, 8, 0)])
def test_transducer_ragged_frame_blocks_and_symbol_caps(backend, T, frame_block, S):
    """transducer_greedy_kernel with T not a multiple of the frame block (T = 1, 9, and 17 with blocks 3, 7, 8) and
    max_symbols_per_step 0 and 1, at J 645 / H 515 / V 1003 (the scalar gemv_rows path)."""
    _check_transducer(backend, V=1003, J=645, H=515, L=1, emb_dim=None, act="leaky_relu", blank=0, B=2, T=T, S=S, every=5,
                      frame_block=frame_block, mix=False, seed=29)


@pytest.mark.gpu
@pytest.mark.parametrize("frame_block,S", [(3, 5), (7, 1), (8, 0)])
def test_transducer_ragged_frame_blocks_and_symbol_caps_full_size(frame_block, S):
    """The sibling of test_transducer_ragged_frame_blocks_and_symbol_caps at T = 250 (250 = 83 * 3 + 1 = 35 * 7 + 5 =
    31 * 8 + 2), B = 16."""
    _check_transducer(_hip(), V=1003, J=645, H=515, L=1, emb_dim=None, act="leaky_relu", blank=0, B=16, T=250, S=S,
                      frame_block=frame_block, mix=S == 5, seed=29)


def test_transducer_blank_in_the_middle_and_carried_state(backend):
    """transducer_greedy_kernel with a blank index other than 0 (one-hot embedding whose zero row is the blank's; 501 of
    1003) and with carried state (start_from_blank = False) at size: J 645, H 515, V 1003, 3 layers."""
    _check_transducer(backend, V=1003, J=645, H=515, L=3, emb_dim=None, act="gelu", blank=501, B=2, T=8, every=4, seed=31)
    _check_transducer(backend, V=1003, J=645, H=515, L=3, emb_dim=64, act="gelu", blank=1002, B=2, T=8, every=4, seed=33,
                      carried=True)


@pytest.mark.gpu
def test_transducer_blank_in_the_middle_and_carried_state_full_size():
    """The sibling of test_transducer_blank_in_the_middle_and_carried_state at B = 32, T = 250."""
    hip = _hip()
    _check_transducer(hip, V=1003, J=645, H=515, L=3, emb_dim=None, act="gelu", blank=501, B=32, T=250, seed=31)
    _check_transducer(hip, V=1003, J=645, H=515, L=3, emb_dim=64, act="gelu", blank=1002, B=32, T=250, seed=33, carried=True)


def _check_streaming(backend, B, T, every, V=1003, J=645, H=515):
    from speechbrain_amd.decoders.transducer import TransducerGreedySearcherStreamingContext

    native, dev = backend
    L = 2
    mods, _ = _transducer(V, J, H, L, 77, "tanh", 0, 37)
    tn, _ = _tn(38, B, T, J, mods[3].w.weight.detach(), V, 0, every)
    s = _searcher(mods, "tanh", 0, dev)
    tn = tn.to(dev)
    offline = _run_block(s, tn, dev, 0)
    assert sum(len(hy) for hy in offline[0]) > T // 2
    for n in (1, 8, 13):
        ctx = TransducerGreedySearcherStreamingContext()
        got = [[] for _ in range(B)]
        for t0 in range(0, T, n):
            for b, part in enumerate(s.transducer_greedy_decode_streaming(tn[:, t0:t0 + n], ctx)):
                got[b] += part
        assert got == offline[0], n
        out_pn, (h, c) = ctx.hidden
        for x, y in zip((out_pn, h, c), offline[1:]):
            assert np.array_equal(x.cpu().numpy(), y), n


def test_transducer_streaming_at_size_is_bit_equal_to_offline(backend):
    """transducer_greedy_kernel's carried state (start_from_blank = False) at size: the same utterances in chunks of 1, 8
    and 13 frames through transducer_greedy_decode_streaming give the offline tokens and final state bit for bit (2 layers, dense
    embedding; J 133, H 131, V 203 here, J 645, H 515, V 1003 in the GPU-only sibling)."""
    _check_streaming(backend, B=2, T=27, every=6, V=203, J=133, H=131)


@pytest.mark.gpu
def test_transducer_streaming_at_size_is_bit_equal_to_offline_full_size():
    """The sibling of test_transducer_streaming_at_size_is_bit_equal_to_offline at B = 8, T = 250."""
    _check_streaming(_hip(), B=8, T=250, every=41)


def _check_lstm(backend, H, L, B, T, inp=77):
    from speechbrain_amd.nnet.RNN import LSTM

    native, dev = backend
    torch.manual_seed(100 + H + L)
    m = LSTM(hidden_size=H, input_shape=[None, None, inp], num_layers=L)
    g = torch.Generator().manual_seed(200 + H + L)
    x = torch.randn(B, T, inp, generator=g)
    hx = (torch.randn(L, B, H, generator=g).tanh(), torch.randn(L, B, H, generator=g))
    ref64 = copy.deepcopy(m.rnn).double()
    for state in (None, hx):
        with torch.no_grad():
            r64 = ref64(x.double(), None if state is None else tuple(t.double() for t in state))
            r32 = m.rnn(x, state)
        r64 = (r64[0], r64[1][0], r64[1][1])
        r32 = (r32[0], r32[1][0], r32[1][1])
        m.to(dev)
        got, (gh, gc) = m(x.to(dev), None if state is None else tuple(t.to(dev) for t in state))
        m.cpu()
        for name, a, b32, b64 in zip(("out", "h", "c"), (got, gh, gc), r32, r64):
            assert a.shape == b64.shape
            own = float((b32.double() - b64).abs().max())
            err = float((a.cpu().double() - b64).abs().max())
            print(f"\n[decode-shapes] lstm H={H} L={L} T={T} given={state is not None} {name}: torch fp32 vs fp64 {own:.3e}, "
                  f"kernel vs fp64 {err:.3e}")
            # Bound: 4 x the error of torch's own float32 LSTM against the float64 one on the same input (both are fp32
            # recurrences of the same length; the factor covers a different summation order).  Measured on the host
            # at H 1024 / 3 layers / T 300, given state, `out`: torch fp32 vs fp64 3.01e-07; the kernel on the MI355X
            # 1.31e-07 (over all GPU cases: torch 3.2e-08 .. 3.0e-07, the kernel 1.9e-08 .. 1.3e-07, ratio <= 1.15).
            assert err <= 4.0 * own, (name, H, L, err, own)


def test_lstm_h515_against_float64(backend):
    """lstm_layer_kernel at H > 512 and H not a multiple of 4 (H 515: the scalar gemv_rows path, lstm_update looping),
    against torch.nn.LSTM in float64, given and default initial state."""
    _check_lstm(backend, H=515, L=1, B=1, T=24)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [515, 1024])
@pytest.mark.parametrize("L", [1, 3])
def test_lstm_long_sequences_against_float64_full_size(H, L):
    """lstm_layer_kernel at H in {515, 1024}, T of a few hundred (300), 1 and 3 layers, against a float64 LSTM, given and
    default initial state."""
    _check_lstm(_hip(), H=H, L=L, B=4, T=300)
