"""csrc/search.hip with an RNNLMScorer -- the RNNLM step (csrc/rnnlm_step.hip) inside the attention beam search -- beyond the
fixture shapes of tests/test_rnnlm_scorer_model.py, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

The random models of tests/test_search_shapes.py (history-dependent logits, B = 2 ragged utterances) with a random RNNLM per
vocabulary, through the public S2STransformerBeamSearcher with ScorerBuilder(full_scorers=[RNNLMScorer, CTCScorer]), against
oracle.sb_oracle.beam_search with a stateful full scorer built on tests/rnnlm_host_ref.py.  Hypotheses equal, lengths within 1e-6,
scores within 1e-4 of the fp32 oracle: the bounds of tests/test_search_shapes.py for this comparison.

What the rows reach (n = 2 * beam hypothesis rows):
  V 257  beam 16   score_topk_row_kernel<4> with the LM's `extra`, one 32-row tile of the LSTM kernel
  V 257  beam 17   the large-beam select; am_only / ctc_combine_kernel with `extra`; two row tiles
  V 257  beam 33   four row tiles, one row group
  V 257  beam 65   the second row group (blockIdx.y = 1); predecessor maps across row 128
  V 1025 beam 16   score_topk_row_kernel<20>, the LM's 16-byte loads (rnn_neurons 16)
  V 5121 beam 16   score_topk_row_kernel<32>
  V 8193 beam 5    no fused pass: am_only with `extra` and the two-stage top-k
The beam-16 rows also run with the fused pass switched off (am_only / ctc_combine + two-stage top-k with `extra`).

CPU-only tests hold the inputs to conditions: the fp32 and the fp64 oracle agree on every list and no rank hangs on rounding; the
LM changes every list; reading the LM state by row instead of through the predecessors changes every list of both utterances; a
predecessor taken modulo 128 changes the beam-65 lists, whose maps do send rows >= 128 to rows < 128.

Measured worst |score - fp32 oracle score| per row of the table over its CTC weights and its runs (fused, separate launches, device
step counter), bound 1e-4, on the emulator / on the MI355X:
  V 257 beam 16  1.43e-6 / 1.43e-6    V 257 beam 17  1.43e-6 / 1.43e-6    V 257 beam 33   1.43e-6 / 1.43e-6
  V 257 beam 65  1.43e-6 / 1.43e-6    V 1025 beam 16 1.91e-6 / 1.91e-6    V 5121 beam 16  1.91e-6 / 2.86e-6
  V 8193 beam 5  1.91e-6 / 1.91e-6
(the fp32 oracle itself lies within 1.7e-6 of its fp64 run on these lists).  Every hypothesis and length agreed on both."""
import ctypes

import pytest
import torch

import rnnlm_host_ref as R
import test_search_shapes as S
from oracle import sb_oracle as O

LM_WEIGHT, LM_TEMPERATURE = 0.5, 1.25
TABLE = [(257, 16, (0.0, 0.4)), (257, 17, (0.0, 0.4)), (257, 33, (0.0, 0.4)), (257, 65, (0.0, 0.4)), (1025, 16, (0.0, 0.4)),
         (5121, 16, (0.0,)), (8193, 5, (0.0,))]
CASES = [(V, beam, w) for V, beam, ws in TABLE for w in ws]
GRAPH_CASES = [(257, 16, 0.4), (257, 65, 0.0)]
MAX_FUSED_BEAM = 16  # kMaxBeam of csrc/search.hip: the fused scoring pass runs up to this beam (and up to 8 192 tokens)
# per vocabulary: (seed of the LM, factor on its output weights).  Chosen so that the conditions of the CPU-only tests below hold
# for every row of TABLE; the factor makes the LM's log-probabilities spread enough to reorder the lists.  Rows 128 and 129 hold the
# two lowest-ranked hypotheses of the second utterance, so few LMs let one of their descendants into the eight best of both beam-65
# lists (about one seed in thirty per list): seed and factor of V = 257 come from a scan for the LMs that do.
LM_SEEDS = {257: (6, 6.25), 1025: (12, 8.0), 5121: (13, 8.0), 8193: (14, 8.0)}
_LMS, _ORACLE = {}, {}


def random_lm(V, dev=None):
    """A random RNNLM over V tokens (CPU; with ``dev`` a copy there): embedding 6, 2 x 13 LSTM (16 at V = 1025: the 16-byte loads),
    two DNN blocks of 9."""
    from speechbrain_amd.lobes.models.RNNLM import RNNLM

    key = (V, "cpu" if dev is None else dev.type)
    if key not in _LMS:
        seed, scale = LM_SEEDS[V]
        keep = torch.random.get_rng_state()
        torch.manual_seed(seed)
        lm = RNNLM(output_neurons=V, embedding_dim=6, rnn_neurons=16 if V == 1025 else 13, rnn_layers=2, dnn_blocks=2,
                   dnn_neurons=9).eval()
        torch.random.set_rng_state(keep)
        with torch.no_grad():
            lm.out.w.weight.mul_(scale)
        _LMS[(V, "cpu")] = lm
        if key[1] != "cpu":
            import copy

            _LMS[key] = copy.deepcopy(lm).to(dev)
    return _LMS[key]


def lm_weights(lm, dtype):
    """The module's weights by the names of tests/rnnlm_host_ref.py, in ``dtype``."""
    t = lambda p: None if p is None else p.detach().to(dtype)  # noqa: E731
    dnn = [(t(lin.w.weight), t(lin.w.bias), t(ln.norm.weight), t(ln.norm.bias), ln.eps) for lin, ln, _ in lm.blocks()]
    return dict(emb=t(lm.embedding.Embedding.weight), lstm=[tuple(t(w) for w in layer) for layer in lm.rnn.layer_weights()], dnn=dnn,
                out_w=t(lm.out.w.weight), out_b=t(lm.out.w.bias))


class HostRNNLMScorer:
    """RNNLMScorer on the host restatement for oracle.sb_oracle.beam_search(full_scorer=...): memory is (state, the predecessors
    the last beam update chose), read through the map by the next step -- or read wrongly under a planted mistake."""

    def __init__(self, lm, dtype, mistakes=()):
        self.lm, self.mistakes = lm_weights(lm, dtype), mistakes

    def score(self, tokens, memory):
        state, parent = (None, None) if memory is None else memory
        out, state = R.step(self.lm, "leaky_relu", tokens, parent, state, LM_WEIGHT, LM_TEMPERATURE, self.mistakes)
        return out, (state, None)

    def permute(self, memory, preds):
        return memory[0], preds


def topk_of(beam):
    return min(S.RANDOM_TOPK, beam)  # the eight best, as RANDOM_CASES; a list holds no more than the beam


def oracle_search(V, beam, ctc_w, double=False, mistakes=(), trace=None, lm=True):
    """The oracle's best hypotheses per utterance with the RNNLM (``lm`` False: without it, S.oracle_search where that has the
    list's width)."""
    if not lm and topk_of(beam) == S.RANDOM_TOPK:
        return S.oracle_search(V, beam, ctc_w, double)
    key = (V, beam, ctc_w, double, mistakes, lm)
    if key not in _ORACLE or trace is not None:
        _, sd, cfg, enc, wl = S.random_model(V)
        sc = O.SearchCfg(bos=S.BOS, eos=S.EOS, beam=beam, ctc_weight=ctc_w, using_eos_threshold=True, max_decode_ratio=0.5,
                         return_topk=True, topk=topk_of(beam))
        dtype = torch.float64 if double else torch.float32
        scorer = HostRNNLMScorer(random_lm(V), dtype, mistakes) if lm else None
        with S.default_dtype(dtype):
            _ORACLE[key] = O.beam_search(enc.to(dtype), wl.to(dtype), {k: v.to(dtype) for k, v in sd.items()}, cfg, sc, trace=trace,
                                         full_scorer=scorer)
    return _ORACLE[key]


def _same_lists(a, b, utt=None):
    rows = slice(None) if utt is None else utt
    return torch.equal(a[0][rows], b[0][rows]) and float((a[2][rows].double() - b[2][rows].double()).abs().max()) <= 1e-4


# ------------------------------------------------------------------------------------------------- conditions on the inputs
@pytest.mark.parametrize("V,beam,ctc_w", CASES)
def test_seeds_are_fair(V, beam, ctc_w):
    """CPU only, the rule of test_search_shapes.test_random_model_seeds_are_fair: the oracle in fp64 and in fp32 returns the same
    eight hypotheses per utterance, their scores agree within 2e-6, and neighbouring fp64 scores lie more than 1e-4 apart."""
    h32, l32, s32, _ = oracle_search(V, beam, ctc_w)
    h64, l64, s64, _ = oracle_search(V, beam, ctc_w, double=True)
    print(f"V={V} beam={beam} ctc={ctc_w}: fp32-fp64 score max|d| {float((s32.double() - s64).abs().max()):.2e}, "
          f"smallest gap between neighbours {float((s64[:, :-1] - s64[:, 1:]).min()):.2e}")
    assert torch.equal(h32, h64) and float((l32.double() - l64).abs().max()) <= 1e-6
    assert float((s32.double() - s64).abs().max()) <= 2e-6
    assert float((s64[:, :-1] - s64[:, 1:]).min()) > 1e-4


@pytest.mark.parametrize("V,beam,ctc_w", CASES)
def test_the_lm_and_its_state_gather_matter(V, beam, ctc_w):
    """CPU only: the list with the RNNLM is not the list without it, and an LM state read by row instead of through the
    predecessors gives other lists for BOTH utterances (a parent taken per utterance instead of per batch would show in the
    second)."""
    good = oracle_search(V, beam, ctc_w)
    assert not _same_lists(good, oracle_search(V, beam, ctc_w, lm=False))
    by_row = oracle_search(V, beam, ctc_w, mistakes=("state_by_row",))
    for utt in (0, 1):
        assert not _same_lists(good, by_row, utt), utt


@pytest.mark.parametrize("ctc_w", [0.0, 0.4])
def test_beam_65_maps_cross_row_128(ctc_w):
    """CPU only: at beam 65 (130 rows) some step's predecessors send a row >= 128 to a row < 128, and a predecessor taken modulo
    128 gives another list."""
    trace = O.SearchTrace()
    good = oracle_search(257, 65, ctc_w, trace=trace)
    crossing = [s for s, p in enumerate(trace.preds) if bool((p[128:] < 128).any())]
    print(f"beam 65 ctc={ctc_w}: steps whose map sends a row >= 128 below row 128: {crossing} of {len(trace.preds)}")
    assert crossing and crossing[0] + 1 < len(trace.preds)  # (a later step reads through that map)
    assert not _same_lists(good, oracle_search(257, 65, ctc_w, mistakes=("parent_mod_128",)))


# ------------------------------------------------------------------------------------------------------- the device search
def _searcher(dev, V, beam, ctc_w, lm=None):
    from speechbrain_amd.decoders import CTCScorer, RNNLMScorer, S2STransformerBeamSearcher, ScorerBuilder

    mods = S.random_model(V, dev)[0]
    full, weights = [RNNLMScorer(language_model=lm or random_lm(V, dev), temperature=LM_TEMPERATURE)], {"rnnlm": LM_WEIGHT}
    if ctc_w > 0:
        full, weights = full + [CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=S.EOS)], dict(weights, ctc=ctc_w)
    return S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=S.BOS, eos_index=S.EOS,
                                      min_decode_ratio=0.0, max_decode_ratio=0.5, beam_size=beam, using_eos_threshold=True,
                                      length_normalization=True, scorer=ScorerBuilder(full_scorers=full, weights=weights),
                                      return_topk=True, topk=topk_of(beam))


def _run(nat, dev, V, beam, ctc_w, what, **attrs):
    _, _, _, enc, wl = S.random_model(V, dev)
    bs = _searcher(dev, V, beam, ctc_w)
    for k, v in attrs.items():
        setattr(bs, k, v)
    hyps, lens, scores, _ = bs(enc.to(dev), wl.to(dev))
    hyps_ref, lens_ref, sc_ref, _ = oracle_search(V, beam, ctc_w)
    err = float((scores.cpu() - sc_ref).abs().max()) if scores.shape == sc_ref.shape else float("nan")
    print(f"rnnlm search V={V} beam={beam} ctc={ctc_w} {what} on {dev.type}: score max|d| {err:.3e} (bound 1.0e-04)")
    assert hyps.shape == hyps_ref.shape and torch.equal(hyps.cpu(), hyps_ref), what
    assert float((lens.cpu() - lens_ref).abs().max()) <= 1e-6, what
    assert err <= 1e-4, what


@pytest.mark.parametrize("V,beam,ctc_w", CASES)
def test_search_vs_oracle(backend, V, beam, ctc_w):
    nat, dev = backend
    _run(nat, dev, V, beam, ctc_w, "")


@pytest.mark.parametrize("V,beam,ctc_w", [c for c in CASES if c[1] <= MAX_FUSED_BEAM and c[0] <= 8192])
def test_search_vs_oracle_without_the_fused_pass(backend, V, beam, ctc_w):
    """The rows the fused pass takes, on the separate launches: am_only / ctc_combine_kernel and the two-stage top-k with the
    LM's log-probabilities at every vocabulary width."""
    nat, dev = backend
    with nat.knobs(score_fused=0):
        _run(nat, dev, V, beam, ctc_w, "score_fused=0")


@pytest.mark.parametrize("V,beam,ctc_w", GRAPH_CASES)
def test_search_vs_oracle_on_the_device_step_counter(backend, V, beam, ctc_w):
    """graph_mode 2: the step number in device memory, the RNNLM step the same launch list at every step (a helper stream turns
    the device counter off, hence overlap_ctc = 0)."""
    nat, dev = backend
    _run(nat, dev, V, beam, ctc_w, "graph_mode=2", graph_mode=2, overlap_ctc=0)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_with_an_rnnlm_are_named(backend):
    nat, dev = backend
    from speechbrain_amd.lobes.models.RNNLM import RNNLM
    from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM

    V, beam = 257, 16
    _, _, _, enc, wl = S.random_model(V, dev)
    enc, wl = enc.to(dev).contiguous(), wl.to(dev)
    enc_len = torch.round(enc.shape[1] * wl).int()

    # graph_mode 1: by the searcher before anything runs, and by the entry itself
    bs = _searcher(dev, V, beam, 0.0)
    bs.graph_mode, bs.overlap_ctc = 1, 0
    with pytest.raises(NotImplementedError, match="RNNLM scorer with graph_mode 1 is not implemented"):
        bs(enc, wl)
    bs.graph_mode = 2
    cfg = bs.config(enc.shape[1])
    cfg.graph_mode = 1
    with pytest.raises(nat.SbkError, match="RNNLM scorer with graph_mode 1 is not implemented"):
        nat.beam_search(bs._handle(), cfg, enc, enc_len)

    # a TransformerLM beside the RNNLM, handed to the entry
    tlm = TransformerLM(vocab=V, d_model=32, nhead=2, num_encoder_layers=1, num_decoder_layers=0, d_ffn=64, dropout=0.0,
                        activation=torch.nn.GELU, normalize_before=False).to(dev).eval()
    handle = nat.LMHandle(tlm)
    cfg = bs.config(enc.shape[1])
    cfg.lm, cfg.lm_weight, cfg.lm_temperature = ctypes.pointer(handle.W), 0.3, 1.0
    with pytest.raises(nat.SbkError, match="TransformerLM scorer and the RNNLM scorer together are not implemented"):
        nat.beam_search(bs._handle(), cfg, enc, enc_len)

    # an LM over another vocabulary
    other = RNNLM(output_neurons=V + 43, embedding_dim=6, rnn_neurons=13, rnn_layers=2, dnn_blocks=1, dnn_neurons=9).to(dev)
    with pytest.raises(nat.SbkError, match=f"the RNNLM scores {V + 43} tokens, the decoder {V}"):
        _searcher(dev, V, beam, 0.0, lm=other)(enc, wl)

    # more hypothesis rows than the RNNLM step takes: the entry's own check with B = 512 and beam 128 on the operands of a
    # two-utterance search (it refuses before it lays out its workspace or launches anything, so nothing of that size exists)
    bs = _searcher(dev, V, 128, 0.0)
    cfg = bs.config(enc.shape[1])
    few = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device=dev)  # noqa: E731
    ws, tok, ln, sc, lp = few(torch.uint8, 4096), few(torch.int32, 8), few(torch.int32, 8), few(torch.float32, 8), few(torch.float32, 8)
    steps = ctypes.c_int32(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = nat.load().sbk_beam_search_f32(ctypes.byref(bs._handle().W), ctypes.byref(cfg), p(enc), p(enc_len), None, None, p(ws),
                                        ws.numel(), p(tok), p(ln), p(sc), p(lp), None, None, None, ctypes.byref(steps), 512,
                                        enc.shape[1], None)
    assert rc != 0
    assert "65536 hypothesis rows exceed the RNNLM step's 65535" in nat.load().sbk_last_error().decode()
