"""csrc/decoder_persist.hip -- the decoder stack of one step for <= 16 hypothesis rows as one cooperative launch -- against an
fp64 decoder (tests/decoder_host_ref.py) at the edges of its loops, on the CPU emulator of the kernel sources (not gpu) and on
the MI355X (-m gpu).

Every model is built with DecoderHandle.from_tensors from seeded random tensors: matrices with the builder's xavier-normal
scale, biases 0.1 N(0,1), the vocabulary projection x 4 (as _persist_model of tests/test_model_parity.py; part B: see there), LayerNorm
gamma = 1 + 0.3 N(0,1), beta = 0.3 N(0,1), so that the fold of the LayerNorm affine into the next projection carries weight.

THE BOUND (parts A, B, C, E).  The yardstick is the SAME host restatement run in float32 on the same inputs: its error against
the float64 run is what one more fp32 evaluation of the function costs at these shapes and weights.  A kernel row may be off
by at most K_RATIO x the root mean square of that fp32 error over the case (errors are normalised per row, below).  K_RATIO = 5
was chosen once: at least 2 x the largest kernel / fp32 ratio any case gives on either backend (1.65, CASE RATIOS below), at
most half of what the mildest planted mistake gives (PLANTED MISTAKES below).

Each case runs twice: on the persistent step (the profiler's launch names prove it ran, once per step, and that no
self_attn_* / cross_attn_* launch did) and, knob persist = 0, on the launch-per-operation kernels -- same reference, same bound.

A. Teacher forced (native.decoder_prefix), error per (row, position) = RMS over d of (got - ref64) / RMS over d of ref64:
   a1  d128 H2, d_ffn 64 (ONE 16-deep operand group per wave: nb = 1), 1 layer, relu, 1 row, 3 positions, a 1-frame memory.
   a2  d128 H2, d_ffn 320 (nb = 5), 3 layers, gelu, 5 rows, 70 positions: self-attention lengths 17 / 33 / 49 (first key of
       waves 1 / 2 / 3) and 65, 66 (second 64-position pass, running-max rescale); memory lengths 70, 65, 64, 63, 1.
   a3  d256 H4, d_ffn 1088 (nb = 17: one group into the second 16-group block of the operand ring), 2 layers, swish, a full
       16-row tile, 18 positions (length 17 with 16 rows), 260-frame memory with lengths at every wave (64 frames) and pass
       (256 frames) edge of the cross-attention: 260, 257, 256, 255, 193, 192, 129, 128, 127, 66, 65, 64, 63, 17, 2, 1.
   a4  d512 H8, d_ffn 2432 (nb = 38), 1 layer, leaky-relu, 2 rows.  2432 is the largest d_ffn the LDS carve admits:
       persist_lds_bytes = (16 (d_ffn + 4) + 1024 + 64) x 4 bytes <= 160 KB - 512 B = 163 328  <=>  d_ffn <= 2480, and
       d_ffn % 64 == 0 leaves 2432 (160 256 bytes); 2496 needs 164 352 bytes and falls back (part E).
B. Ancestry over a long search (native.beam_search, no CTC, no LM, length normalisation on, eos threshold off, min_steps 69,
   max_steps 72: every hypothesis has 70-72 tokens; topk = beam).  Hypotheses are not compared with a second search (near-ties
   over 70 steps): every returned sequence is RESCORED by the fp64 decoder, and the kernel's out_logp must be the fp64
   log-probs of that very sequence (0 behind it), out_score their sum / token count (sbk.h: out_logp; S2SBeamSearcher's
   length-normalised score).  A row that read another row's cache slot reports log-probs its own tokens do not have.
   The inputs make the beams diverge early and keep reordering; asserted on the returned lists: per utterance at least half of
   the hypotheses differ from the best one before position 16, no two are equal.  Scaling seq down alone does not get there
   (a flat source coalesces to one ancestor within ~beam steps; x 0.5 gave 0 of 3 for every seed tried): what keeps branches
   alive side by side is a PEAKED source whose branches cost about the same, so model seed, seq scale (x 4 at beam 4, x 2 at
   beam 16) and the seed of every utterance's memory were searched for it.  Achieved, the same on both backends and both
   paths: beam 16: 12 of 15 differ before position 16 (first position with two different tokens: 6); three utterances x
   beam 4: 2, 2, 2 of 3 (first positions 4, 9, 4).
C. Greedy, one row (native.greedy_search, 70 steps, eos suppressed by a seq bias of -30, vocabulary 9 < 16): the fp64 decoder
   teacher-forced on the kernel's own tokens; every chosen token is the fp64 arg-max or within the logit tolerance
   (K_RATIO x the largest fp32 logit error of the run) of the fp64 maximum; >= 90 % of the steps are decided by more than
   that (a condition on the inputs: the fp64 decoder alone).
D. Grid independence at length: a2 and the beam-16 search under persist_grid 1 / 5 / 128 x persist_tree 0 / 1 are bit-equal to
   the default run.
E. Fall-back at the limits: d_ffn 2496 (64 past the LDS edge), d_ffn 96 (no multiple of 64), 17 rows do NOT launch the
   persistent step and meet the bound through the plain launches.  enc_len 0 and enc_len > T: every cross-attention kernel
   attends to min(max(enc_len, 1), T) frames (include/sbk.h, sbk_decoder_prefix_f32); both paths meet the bound against the
   fp64 decoder at the clamped lengths.

CASE RATIOS (largest kernel error of a (row, position) or hypothesis / RMS fp32 error of the case; persistent step | plain launches):
                        emulator        MI355X
   a1                   1.14 | 1.39     0.93 | 1.09
   a2                   0.85 | 0.97     0.87 | 1.02
   a3                   0.84 | 0.97     1.17 | 1.31
   a4                   1.10 | 1.65     0.81 | 1.25
   B beam 16            0.55 | 0.71     0.70 | 0.86
   B 3 x beam 4         0.94 | 0.98     0.92 | 0.97
   C (log-prob, RMS)    0.24 | 0.24     0.24 | 0.24
   E d_ffn 2496         - | 1.63        - | 1.20
   E d_ffn 96           - | 1.00        - | 0.90
   E 17 rows            - | 1.06        - | 1.03
   E enc_len            0.75 | 0.77     0.66 | 0.70
(the fp32 yardstick itself moves with the host's BLAS: 1.2e-7 .. 2.8e-7 per row in part A.)  Part C: 100 % of the steps are
decided by more than the logit tolerance (2.8e-5), every token is the fp64 arg-max.

PLANTED MISTAKES (each on a scratch copy of csrc/decoder_persist.hip, emulator): the new cases that fail with the largest
kernel / fp32 ratio of each, and whether test_model_parity's persistent-step test still passes (the gap this file closes).
   attn_item<true>: the merge ignores wave 3           a2 3.0e5, B 1.2e5 / 6.7e4, C 118                       old test passes
   attn_item<true>: one pass only (keys >= 64 dropped) a2 1.4e5, B 3.7e4 / 6.4e3, C 25.6                      old test passes
   corr left out of acc (self-attention)               a2 1.6e5, B 2.9e3 / 4.8e4                              old test passes
     (in both forms: also a3 2.8e4; the old test's 300-frame search fails)
   slot[p] replaced by i                               B 2.0e5 / 2.5e5 (part A untouched: no reordering)      old test fails
   attn_item<false>: len -> min(len, 64)               a2 1.7e5, a3 3.2e5                                     old d128 fails (300 frames)
   attn_item<false>: u = i instead of i / beam         B (3 x beam 4) 4.0e5                                   old test fails
   tiles_gemm: wc = wn skipped, last partial block     a3 (nb 17) 6.4e5, a4 (nb 38) 1.5e6                     old test passes
   tiles_gemm: residual from col - 1 in the last tile  a1-a4 2.0e6 .. 5.4e6, B, C 3.7e3, D, enc_len            old test fails
   stage_rows<true>: variance / 1024                   a1-a4 3.1e6 .. 1.8e7, B, C 3.8e3, enc_len              old test fails
   act_of: gelu computed as swish                      a2 4.5e5 (the only gelu case)                          old test fails
Every mistake moves its most sensitive case by >= 1.4e5 x the fp32 error; the smallest figure of ANY failing case is 25.6:
K_RATIO = 5 is below half of it and above twice 1.65.
"""
import math

import pytest
import torch

import decoder_host_ref as R

BOS, EOS = 1, 2
K_RATIO = 5.0
LN_EPS = 1e-6
_CACHE = {}


# ------------------------------------------------------------------------------------------------------------ models
def make_model(d, H, dffn, nl, act, V, seed, seq_scale=4.0, eos_bias=0.0, max_len=80):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    lin = lambda o, i, scale=1.0: (scale * math.sqrt(2.0 / (o + i)) * rn(o, i), 0.1 * rn(o))
    ln = lambda: (1.0 + 0.3 * rn(d), 0.3 * rn(d))
    layers = [dict(ln1=ln(), sa_in=lin(3 * d, d), sa_out=lin(d, d), ln2=ln(), ca_in=lin(3 * d, d), ca_out=lin(d, d), ln3=ln(),
                   ff1=lin(dffn, d), ff2=lin(d, dffn)) for _ in range(nl)]
    pos = torch.arange(max_len, dtype=torch.float64)[:, None]
    den = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * -(math.log(10000.0) / d))
    pe = torch.zeros(max_len, d, dtype=torch.float64)
    pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * den), torch.cos(pos * den)
    seq = lin(V, d, seq_scale)
    seq[1][EOS] += eos_bias
    return dict(layers=layers, emb=math.sqrt(2.0 / (V + d)) * rn(V, d), pe=pe.float(), final_ln=ln(), seq=seq, nhead=H,
                ffn_act=act, ln_eps=LN_EPS, emb_scale=0.0)


def handle(nat, spec, dev):
    mv = lambda t: t.to(dev).contiguous()
    pair = lambda p: tuple(mv(t) for t in p)
    return nat.DecoderHandle.from_tensors([{k: pair(v) for k, v in L.items()} for L in spec["layers"]], mv(spec["emb"]),
                                          mv(spec["pe"]), pair(spec["final_ln"]), pair(spec["seq"]), spec["nhead"],
                                          spec["ffn_act"], spec["ln_eps"], spec["emb_scale"])


def profiled(nat, fn):
    nat.prof_reset()
    nat.prof_enable(True)
    try:
        out = fn()
    finally:
        nat.prof_enable(False)
    return out, {k: v["count"] for k, v in nat.prof_report().items()}


def attention_launches(rep):
    return sorted(k for k in rep if k.startswith("self_attn") or k.startswith("cross_attn"))


def assert_persistent(rep, steps, tag):
    assert rep.get("decoder_step_persist", 0) == steps and not attention_launches(rep), (tag, steps, rep)


def assert_plain(rep, tag):
    assert "decoder_step_persist" not in rep and attention_launches(rep), (tag, rep)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------------------ part A
A_CASES = {
    "a1": dict(d=128, H=2, dffn=64, nl=1, act=R.ACT_RELU, L=3, T=1, lens=[1], seed=101),
    "a2": dict(d=128, H=2, dffn=320, nl=3, act=R.ACT_GELU, L=70, T=70, lens=[70, 65, 64, 63, 1], seed=102),
    "a3": dict(d=256, H=4, dffn=1088, nl=2, act=R.ACT_SWISH, L=18, T=260,
               lens=[260, 257, 256, 255, 193, 192, 129, 128, 127, 66, 65, 64, 63, 17, 2, 1], seed=103),
    "a4": dict(d=512, H=8, dffn=2432, nl=1, act=R.ACT_LEAKY_RELU, L=4, T=20, lens=[20, 7], seed=104),
}
E_CASES = {
    "ffn_past_lds_edge": dict(d=512, H=8, dffn=2496, nl=1, act=R.ACT_LEAKY_RELU, L=4, T=20, lens=[20, 7], seed=105),
    "ffn_96": dict(d=128, H=2, dffn=96, nl=2, act=R.ACT_RELU, L=5, T=9, lens=[9, 4, 1], seed=106),
    "rows_17": dict(d=128, H=2, dffn=64, nl=1, act=R.ACT_GELU, L=3, T=5, lens=[5, 4, 3, 2, 1] * 3 + [5, 2], seed=107),
}
LEN_CASE = dict(d=128, H=2, dffn=128, nl=2, act=R.ACT_SWISH, L=4, T=6, lens=[0, 9, 4, 6], seed=108)
PERSIST_LDS_LIMIT = 160 * 1024 - 512


def persist_lds_bytes(d, dffn, Lmax):
    """The arithmetic of persist_lds_bytes (csrc/decoder_persist.hip), restated: 16 staged rows of max(d, d_ffn) + 4 floats
    (or the attention scratch, if larger), the 4 x 256 partial tiles, 64 floats of slack."""
    return (max(16 * (max(d, dffn) + 4), 8 + 256 + Lmax + 64) + 1024 + 64) * 4


def prefix_case(c, clamp=False):
    """(spec, tokens, enc, enc_len, h64, fp32 error per (row, position)) of a teacher-forced case; computed once."""
    key = ("prefix", c["seed"])
    if key not in _CACHE:
        V, n = 24, len(c["lens"])
        spec = make_model(c["d"], c["H"], c["dffn"], c["nl"], c["act"], V, c["seed"])
        g = torch.Generator().manual_seed(c["seed"] + 1000)
        tokens = torch.randint(0, V, (n, c["L"]), generator=g).int()
        enc = torch.randn(n, c["T"], c["d"], generator=g)
        lens = torch.tensor(c["lens"], dtype=torch.int32)
        ref_lens = lens.clamp(1, c["T"]) if clamp else lens
        assert clamp or (int(lens.min()) >= 1 and int(lens.max()) <= c["T"])
        h64 = R.Decoder(**spec).decode(tokens, enc, ref_lens)
        e32 = row_err(R.Decoder(**spec, fp32=True).decode(tokens, enc, ref_lens), h64)
        _CACHE[key] = (spec, tokens, enc, lens, h64, e32)
    return _CACHE[key]


def row_err(got, ref64):
    """[n,L,d] -> [n,L]: RMS over d of the difference, in units of the RMS of the fp64 row."""
    got = got.detach().cpu().double()
    return (got - ref64).pow(2).mean(-1).sqrt() / ref64.pow(2).mean(-1).sqrt()


def edge_of(c, row, pos):
    """What the kernel's loops do at this (row, position), so that a failure names the edge it sits on."""
    sl, cl = pos + 1, min(max(c["lens"][row], 1), c["T"])
    return (f"self-attention over {sl} keys (waves with keys: {min(4, -(-sl // 16))}, 64-key passes: {-(-sl // 64)}); "
            f"cross-attention over {cl} frames (waves with frames: {min(4, -(-cl // 64))}, 256-frame passes: {-(-cl // 256)})")


def check_rows(tag, c, got, h64, e32):
    assert bool(torch.isfinite(got).all()), tag
    e, base = row_err(got, h64), rms(e32)
    ratio = e / base
    row, pos = divmod(int(ratio.argmax()), ratio.shape[1])
    print(f"{tag}: fp32 restatement RMS {base:.3e}; kernel / fp32: RMS {rms(e) / base:.2f}, largest {float(ratio.max()):.2f} at "
          f"row {row} position {pos}")
    assert float(ratio.max()) <= K_RATIO, (tag, float(ratio.max()), f"row {row} position {pos}", edge_of(c, row, pos))
    return float(ratio.max())


def run_prefix(nat, dev, c, case, **knobs):
    spec, tokens, enc, lens = case[:4]
    h = handle(nat, spec, dev)
    with nat.knobs(**knobs):
        return profiled(nat, lambda: nat.decoder_prefix(h, tokens.to(dev), enc.to(dev), lens.to(dev)))


def test_lds_edge_arithmetic():
    """a4 sits on the LDS edge of the persistent step and the first fall-back case one 64-step behind it."""
    assert persist_lds_bytes(512, A_CASES["a4"]["dffn"], A_CASES["a4"]["L"]) <= PERSIST_LDS_LIMIT
    assert persist_lds_bytes(512, A_CASES["a4"]["dffn"] + 64, A_CASES["a4"]["L"]) > PERSIST_LDS_LIMIT
    assert E_CASES["ffn_past_lds_edge"]["dffn"] == A_CASES["a4"]["dffn"] + 64
    assert persist_lds_bytes(512, 2432, 4) == 160256 and persist_lds_bytes(512, 2496, 4) == 164352


@pytest.mark.parametrize("name", sorted(A_CASES))
def test_teacher_forced_step_vs_fp64(backend, name):
    """Part A: the persistent step at the edges of its attention passes and its operand ring, then the plain launches."""
    nat, dev = backend
    c = A_CASES[name]
    case = prefix_case(c)
    got, rep = run_prefix(nat, dev, c, case)
    assert_persistent(rep, c["L"], name)
    check_rows(f"{name} persistent step", c, got, *case[4:])
    got0, rep0 = run_prefix(nat, dev, c, case, persist=0)
    assert_plain(rep0, name)
    check_rows(f"{name} plain launches", c, got0, *case[4:])


# ------------------------------------------------------------------------------------------------------------ part B
B_CASES = {  # (model seed, seq scale and the seed of every utterance's memory: tuned for the divergence conditions, module docstring part B)
    "three_utterances_beam4": dict(nl=1, B=3, beam=4, V=16, lens=[33, 24, 17], seed=502, enc_seeds=[7001, 7003, 7010], seq_scale=4.0),
    "one_utterance_beam16": dict(nl=2, B=1, beam=16, V=23, lens=[24], seed=411, enc_seeds=[1411], seq_scale=2.0),
}
MIN_STEPS, MAX_STEPS = 69, 72  # eos is barred before step 69: every hypothesis has 70, 71 or 72 tokens


def search_case(c):
    key = ("search", c["seed"], c["beam"])
    if key not in _CACHE:
        spec = make_model(128, 2, 256, c["nl"], R.ACT_RELU, c["V"], c["seed"], seq_scale=c["seq_scale"])
        enc = torch.zeros(c["B"], max(c["lens"]), 128)  # (frames past enc_len are never read)
        for u, (n, seed) in enumerate(zip(c["lens"], c["enc_seeds"])):
            enc[u, :n] = torch.randn(n, 128, generator=torch.Generator().manual_seed(seed))
        _CACHE[key] = (spec, enc, torch.tensor(c["lens"], dtype=torch.int32))
    return _CACHE[key]


def run_search(nat, dev, c, **knobs):
    spec, enc, lens = search_case(c)
    h = handle(nat, spec, dev)
    cfg = nat.SearchConfig(bos=BOS, eos=EOS, blank=0, beam=c["beam"], min_steps=MIN_STEPS, max_steps=MAX_STEPS,
                           length_normalization=1, using_eos_threshold=0, check_every=8, overlap_ctc=0, ctc_weight=0.0,
                           temperature=1.0, eos_threshold=1.5, minus_inf=-1e20, lm_weight=0.0, lm_temperature=1.0,
                           topk=c["beam"], graph_mode=0)
    with nat.knobs(**knobs):
        (tok, ln, sc, lp, _, steps), rep = profiled(nat, lambda: nat.beam_search(h, cfg, enc.to(dev).contiguous(), lens.to(dev)))
    return tok.cpu(), ln.cpu(), sc.cpu(), lp.cpu(), steps, rep


def check_search(tag, c, tok, ln, sc, lp):
    """Rescore the returned sequences with the fp64 decoder and hold out_logp / out_score to it; the divergence conditions."""
    spec, enc, lens = search_case(c)
    B, beam = c["B"], c["beam"]
    ntok = (ln + 1).long()
    assert int(ntok.min()) >= MIN_STEPS + 1 and int(ntok.max()) <= MAX_STEPS, (tag, ntok.tolist())
    valid = torch.arange(MAX_STEPS)[None, :] < ntok[:, None]
    assert bool((tok[~valid] == 0).all()) and bool((lp[~valid] == 0).all()), tag
    # the inputs made the beams diverge early (checked AFTER the rescoring: a kernel that reads the wrong slot also searches differently)
    early, equal = [], []
    for u in range(B):
        rows = [tuple(tok[u * beam + j, :ntok[u * beam + j]].tolist()) for j in range(beam)]
        equal.append(beam - len(set(rows)))
        early.append(sum(rows[j][:16] != rows[0][:16] for j in range(1, beam)))
    first = [min([t for t in range(MAX_STEPS) if len({int(tok[u * beam + j, t]) for j in range(beam)}) > 1], default=-1) for u in range(B)]
    enc_rows, len_rows = enc.repeat_interleave(beam, 0), lens.repeat_interleave(beam, 0)
    ref = R.Decoder(**spec).rescore(tok, enc_rows, len_rows, BOS) * valid
    ref32 = R.Decoder(**spec, fp32=True).rescore(tok, enc_rows, len_rows, BOS) * valid
    per_row = lambda x: ((x.double() - ref).pow(2).sum(1) / ntok).sqrt()  # RMS over the hypothesis' own tokens
    base = float((per_row(ref32).pow(2).mean()).sqrt())
    e = per_row(lp)
    # out_score: the running sum is multiplied back and divided once per step (internal.h: score_cand, beam_update): three
    # roundings of the partial sum S_t per step, so |score - sum / n| <= 3 x 2^-24 x sum_t |S_t| / n on top of the log-prob errors
    score_ref = ref.sum(1) / ntok
    rounding = 3.0 * 2.0 ** -24 * (ref.cumsum(1).abs() * valid).sum(1) / ntok
    es = (sc.double() - score_ref).abs()
    print(f"{tag}: hypotheses that differ from the best before position 16: {early} of {beam - 1}; first position with two "
          f"different tokens: {first}; fp32 restatement RMS log-prob error {base:.3e}; kernel / fp32: largest hypothesis "
          f"{float(e.max()) / base:.2f}; score error / (K x fp32 + rounding): {float((es / (K_RATIO * base + rounding)).max()):.3f}")
    worst = int(e.argmax())
    assert float(e.max()) <= K_RATIO * base, (tag, "out_logp", worst, float(e.max()) / base)
    assert bool((es <= K_RATIO * base + rounding).all()), (tag, "out_score", es.tolist())
    assert not any(equal), (tag, "equal hypotheses", equal)
    assert all(n >= beam // 2 for n in early), (tag, "hypotheses that leave the best one before position 16", early)
    return float(e.max()) / base


@pytest.mark.parametrize("name", sorted(B_CASES))
def test_long_search_ancestry_by_rescoring(backend, name):
    """Part B: after ~70 steps of diverging, reordering beams every returned hypothesis carries the log-probs of its own tokens."""
    nat, dev = backend
    c = B_CASES[name]
    tok, ln, sc, lp, steps, rep = run_search(nat, dev, c)
    assert MIN_STEPS + 1 <= steps <= MAX_STEPS
    assert_persistent(rep, steps, name)
    check_search(f"{name} persistent step", c, tok, ln, sc, lp)
    tok0, ln0, sc0, lp0, steps0, rep0 = run_search(nat, dev, c, persist=0)
    assert_plain(rep0, name)
    check_search(f"{name} plain launches", c, tok0, ln0, sc0, lp0)


# ------------------------------------------------------------------------------------------------------------ part C
GREEDY = dict(nl=2, V=9, T=30, steps=70, seed=301, eos_bias=-30.0)


def greedy_case():
    key = ("greedy",)
    if key not in _CACHE:
        c = GREEDY
        spec = make_model(128, 2, 256, c["nl"], R.ACT_SWISH, c["V"], c["seed"], eos_bias=c["eos_bias"])
        enc = torch.randn(1, c["T"], 128, generator=torch.Generator().manual_seed(c["seed"] + 1000))
        _CACHE[key] = (spec, enc, torch.tensor([c["T"]], dtype=torch.int32))
    return _CACHE[key]


def check_greedy(tag, tok, sc):
    spec, enc, lens = greedy_case()
    steps = GREEDY["steps"]
    assert EOS not in tok[0].tolist(), tag
    inp = torch.cat([torch.tensor([[BOS]]), tok[:, :-1].long()], dim=1)
    d64, d32 = R.Decoder(**spec), R.Decoder(**spec, fp32=True)
    z = d64.logits(d64.decode(inp, enc, lens))[0]  # [steps, V]
    z32 = d32.logits(d32.decode(inp, enc, lens))[0]
    tol = K_RATIO * float((z32.double() - z).abs().max())
    top2 = z.topk(2, dim=-1).values
    gap_chosen = top2[:, 0] - z.gather(1, tok[0].long()[:, None])[:, 0]
    decided = float(((top2[:, 0] - top2[:, 1]) > tol).double().mean())
    lp = (z - z.logsumexp(-1, keepdim=True)).gather(1, tok[0].long()[:, None])[:, 0]
    lp32 = (z32 - z32.logsumexp(-1, keepdim=True)).gather(1, tok[0].long()[:, None])[:, 0]
    base, e = rms(lp32.double() - lp), rms(sc[0].double() - lp)
    print(f"{tag}: logit tolerance {tol:.3e}; steps decided by more: {100 * decided:.1f} %; tokens that are not the fp64 arg-max: "
          f"{int((gap_chosen > 0).sum())} of {steps}; log-prob of the chosen token, kernel / fp32 RMS: {e / base:.2f}")
    assert decided >= 0.9, (tag, decided)
    assert float(gap_chosen.max()) <= tol, (tag, int(gap_chosen.argmax()), float(gap_chosen.max()), tol)
    assert e <= K_RATIO * base, (tag, e / base)
    return e / base


def test_greedy_one_row_vs_fp64(backend):
    """Part C: n = 1 (one workgroup has rows, the other fifteen tile rows are zero), 70 steps, vocabulary below one 16-column tile."""
    nat, dev = backend
    spec, enc, lens = greedy_case()
    steps = GREEDY["steps"]
    for knobs, tag in (({}, "persistent step"), (dict(persist=0), "plain launches")):
        h = handle(nat, spec, dev)
        with nat.knobs(**knobs):
            (tok, sc, ran), rep = profiled(nat, lambda: nat.greedy_search(h, enc.to(dev), lens.to(dev), 0, steps, BOS, EOS, check_every=0))
        assert ran == steps
        if knobs:
            assert_plain(rep, tag)
        else:
            assert_persistent(rep, steps, tag)
        check_greedy(f"greedy {tag}", tok.cpu(), sc.cpu())


# ------------------------------------------------------------------------------------------------------------ part D
GRIDS = [(grid, tree) for grid in (1, 5, 128) for tree in (0, 1)]


def test_grid_independence_teacher_forced_70_positions(backend):
    """Part D: a2 with one workgroup (a single sub-counter, every loop over tiles and items serial), five, and the default 128."""
    nat, dev = backend
    c = A_CASES["a2"]
    case = prefix_case(c)
    base, rep = run_prefix(nat, dev, c, case)
    assert_persistent(rep, c["L"], "a2")
    for grid, tree in GRIDS:
        got, rep = run_prefix(nat, dev, c, case, persist_grid=grid, persist_tree=tree)
        assert_persistent(rep, c["L"], ("a2", grid, tree))
        assert torch.equal(got, base), ("a2", grid, tree, float((got - base).abs().max()))


def test_grid_independence_beam16_search(backend):
    nat, dev = backend
    c = B_CASES["one_utterance_beam16"]
    base = run_search(nat, dev, c)
    assert_persistent(base[5], base[4], "beam 16")
    for grid, tree in GRIDS:
        got = run_search(nat, dev, c, persist_grid=grid, persist_tree=tree)
        assert_persistent(got[5], got[4], ("beam 16", grid, tree))
        assert got[4] == base[4] and all(torch.equal(a, b) for a, b in zip(got[:4], base[:4])), ("beam 16", grid, tree)


# ------------------------------------------------------------------------------------------------------------ part E
@pytest.mark.parametrize("name", sorted(E_CASES))
def test_fallback_at_the_limits(backend, name):
    """Part E: shapes past a documented limit of persist_eligible take the plain launches and meet the same bound."""
    nat, dev = backend
    c = E_CASES[name]
    case = prefix_case(c)
    got, rep = run_prefix(nat, dev, c, case)
    assert_plain(rep, name)
    check_rows(f"{name} (fall-back)", c, got, *case[4:])


def test_enc_len_outside_the_memory_is_clamped_on_both_paths(backend):
    """enc_len 0 and enc_len > T: min(max(enc_len, 1), T) frames on the persistent step and on the plain launches (sbk.h)."""
    nat, dev = backend
    c = LEN_CASE
    case = prefix_case(c, clamp=True)
    got, rep = run_prefix(nat, dev, c, case)
    assert_persistent(rep, c["L"], "enc_len")
    check_rows("enc_len [0, 9, 4, 6] of 6 frames, persistent step", c, got, *case[4:])
    got0, rep0 = run_prefix(nat, dev, c, case, persist=0)
    assert_plain(rep0, "enc_len")
    check_rows("enc_len [0, 9, 4, 6] of 6 frames, plain launches", c, got0, *case[4:])
