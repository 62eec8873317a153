"""csrc/search.hip -- the S2S attention beam search beyond the fixture shapes -- on the CPU emulator of the kernel sources
(not gpu) and on the MI355X (-m gpu).

FROZEN LOGITS (parts 1-2).  A tiny random decoder whose seq_lin weight is zero and whose seq_lin bias is a chosen vector b
gives the logits b to every hypothesis at every step.  The search is then a search over a memoryless source, and
tests/search_host_ref.py restates it in numpy float32 on the log-prob row that native.log_softmax (the step's own
log_softmax_row_kernel; tests/test_frontend_shapes.py holds it to fp64 within 1e-5) makes of b.  Both sides perform the same
rounded operations on the same inputs, so tokens, lengths, scores, per-token log-probs and the longest length must agree
BIT FOR BIT: the tolerance is zero, derived, not measured.  Such a source is full of exact ties ("a b" and "b a" score the
same because fp addition commutes); planted equal logits add ties inside a row.

RANDOM MODELS (parts 3-4).  Frozen logits cannot see a wrong parent gather in the KV ancestry or the CTC state, so random
models run against oracle.sb_oracle at the same vocabulary and beam edges: hypotheses equal, scores within 1e-4, lengths within
1e-6 (the bounds of tests/test_model_parity.py for this comparison).  A CPU test asserts that the oracle in fp64 and in fp32
returns the same hypotheses for every chosen seed, so that no decision hangs on fp32 noise."""
import contextlib

import numpy as np
import pytest
import torch

import search_host_ref as R
from oracle import sb_oracle as O

BOS, EOS = 1, 2
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- frozen-logit cases
def _ranked(V, seed, scale=2.0):
    """Random logits and the tokens in descending order of them (eos and bos kept out of the ranking)."""
    g = np.random.default_rng(seed)
    b = (g.standard_normal(V) * scale).astype(F32)
    order = [int(t) for t in np.argsort(-b, kind="stable") if t not in (BOS, EOS)]
    return b, order


def _place(b, order, tok, rank):
    """Give ``tok`` a logit halfway between those of the tokens at ``rank - 1`` and ``rank`` (rank 0: above all)."""
    b[tok] = b[order[0]] + F32(0.5) if rank == 0 else F32(0.5) * (b[order[rank - 1]] + b[order[rank]])


def plain(V, seed, eos_rank=1, scale=2.0):
    b, order = _ranked(V, seed, scale)
    _place(b, order, EOS, eos_rank)
    return b


def planted(V, seed, beam, eos_rank=1, eos_in_tie=False):
    """A pair of equal logits among the winners and a triple across the beam-th rank of step 0 (a pair for beam < 3).  The
    ranks count the non-eos tokens; eos enters at ``eos_rank`` or, ``eos_in_tie``, shares the triple's logit."""
    b, order = _ranked(V, seed)
    if beam < 4 and not eos_in_tie:
        eos_rank = 0  # (no room for eos between distinct logits above the tie group)
    k = beam - 1 if eos_rank < beam and not eos_in_tie else beam  # non-eos tokens among the step-0 winners
    lo = max(k - 2, 0)
    for r in range(lo, k + 1):
        b[order[r]] = b[order[lo]]  # ranks lo .. k share a logit: the beam-th rank falls inside
    if lo >= 3:
        b[order[2]] = b[order[1]]
    if eos_in_tie:
        b[EOS] = b[order[lo]]
    else:
        _place(b, order, EOS, eos_rank)
    return b


def sea_finite(V=2600, first=1000, count=1500, above=5):
    """``count`` tokens from ``first`` on share one logit, ``above`` tokens and eos lie over it, the rest far below: at a beam
    over ``above + 1`` the beam-th rank of step 0 falls inside the sea, whose first 1 024-candidate block holds only
    1 024 - first members."""
    b = np.full(V, -9.0, dtype=F32)
    b[first:first + count] = 0.0
    b[10:10 + above] = np.linspace(2.0, 1.0, above, dtype=F32)
    b[EOS] = 0.5
    return b


def eos_at_threshold(V, seed, thr, delta):
    """eos with log-prob thr * max(log-prob) + delta (fixed point in fp64: the normaliser moves with the eos logit)."""
    b, order = _ranked(V, seed, 3.0)
    x = b.astype(np.float64)
    x[order[0]] += 3.0  # a peaked row: thr * max(log-prob) is then the second best log-prob
    top = x[order[0]]
    for _ in range(60):
        lp_max = -np.log(np.exp(x - top).sum())
        x[EOS] = top + (thr - 1.0) * lp_max + delta
    return x.astype(F32)


def case(b, beam, steps, min_steps=0, T=12, B=1, norm=True, thr=None, temperature=1.0, eos=True, ties=False, fills=None):
    """``thr`` None: no eos threshold.  ``eos``: the case lets hypotheses end through eos.  ``ties``: some step must have a tie
    group across the beam-th rank.  ``fills``: True = the list must fill before max_steps, False = nothing may be harvested."""
    return dict(b=b, beam=beam, steps=steps, min_steps=min_steps, T=T, B=B, norm=norm, thr=thr, temperature=temperature, eos=eos,
                ties=ties, fills=fills)


CASES = {
    # vocabulary: one column per thread ends at 256; NPT 4 -> 20 at 1 024, 20 -> 32 at 5 120; no fused pass above 8 192
    "v255_b5": lambda: case(plain(255, 1), 5, 6, B=2, norm=False),
    "v256_b5": lambda: case(plain(256, 2), 5, 6),
    "v257_b3_ragged": lambda: case(planted(257, 3, 3), 3, 6, ties=True),  # 3 * 257 = 771: no multiple of the 16 stage-1 slices
    "v1024_b8": lambda: case(plain(1024, 4), 8, 5),
    "v1025_b8": lambda: case(planted(1025, 5, 8), 8, 5, ties=True, norm=False),
    "v5120_b4": lambda: case(plain(5120, 6), 4, 5),
    "v5121_b16": lambda: case(planted(5121, 7, 16), 16, 4, ties=True),
    "v8192_b4": lambda: case(plain(8192, 8), 4, 4),
    "v8193_b5": lambda: case(planted(8193, 9, 5), 5, 4, ties=True),
    # beam: the two-stage lists end at 16, the radix select at 128
    "v40_b1": lambda: case(plain(40, 10, eos_rank=3), 1, 8, eos=False, fills=False),  # (the only beam never holds eos)
    "v40_b2": lambda: case(planted(40, 11, 2), 2, 8, ties=True),
    "v300_b15": lambda: case(planted(300, 12, 15), 15, 6, ties=True),
    "v300_b16": lambda: case(planted(300, 13, 16), 16, 6, ties=True, B=3),
    "v300_b17": lambda: case(planted(300, 14, 17), 17, 6, ties=True, B=2),  # a handful of ties on the radix threshold
    "v300_b17_nonorm": lambda: case(planted(300, 15, 17, eos_rank=3), 17, 6, ties=True, norm=False),
    "v600_b64": lambda: case(plain(600, 16), 64, 5),
    "v600_b127": lambda: case(planted(600, 17, 127), 127, 4, ties=True, norm=False),
    "v600_b128": lambda: case(planted(600, 18, 128), 128, 4, ties=True),
    # seas of equal keys
    "v40_b66_dead_sea": lambda: case(plain(40, 19), 66, 6, ties=True),       # step 0: 2 600 dead candidates, 26 taken
    "v2600_b64_finite_sea": lambda: case(sea_finite(), 64, 3, ties=True),   # need_eq reached in the sweep's second block
    "v8_b16_sea": lambda: case(plain(8, 20, eos_rank=2), 16, 6, ties=True, norm=False),  # 8 alive candidates for 16 beams at step 0
    # eos rules
    "eos_unique_max_thr1": lambda: case(plain(40, 21, eos_rank=0), 4, 6, thr=1.0, eos=False, fills=False),
    "eos_inside_thr": lambda: case(eos_at_threshold(50, 22, 1.5, +1e-3), 4, 8, thr=1.5),
    "eos_outside_thr": lambda: case(eos_at_threshold(50, 22, 1.5, -1e-3), 4, 8, thr=1.5, eos=False, fills=False),
    "min_steps_1": lambda: case(plain(40, 23, eos_rank=0), 4, 8, min_steps=1, thr=1.5),
    "min_steps_3": lambda: case(plain(300, 24, eos_rank=0), 6, 8, min_steps=3),
    "min_equals_max": lambda: case(plain(40, 25, eos_rank=0), 4, 5, min_steps=5, eos=False, fills=False),
    "eos_in_tie": lambda: case(planted(40, 26, 4, eos_in_tie=True), 4, 8, ties=True),
    # step limits, early stop, temperature
    "max_steps_1": lambda: case(plain(40, 27), 4, 1, eos=False),   # (one step: one length only)
    "max_steps_2": lambda: case(plain(40, 28, eos_rank=0), 4, 2),
    "fills_early": lambda: case(plain(40, 29, eos_rank=0), 3, 20, T=24, fills=True, thr=1.5),
    "fills_none": lambda: case(plain(300, 30, eos_rank=200), 4, 6, eos=False, fills=False),
    "temperature": lambda: case(planted(300, 31, 6), 6, 6, ties=True, temperature=1.7, thr=1.5),
}
STEPPING = ["v257_b3_ragged", "v300_b17", "fills_early"]  # cases that also run on the device-side counter and from a graph
_BUILT, _MODELS, _REFS = {}, {}, {}


def built(name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name]()
    return _BUILT[name]


def host_row(c):
    """log_softmax(b / temperature) in fp64, rounded to fp32: the row of the tests that touch no kernel."""
    x = c["b"].astype(np.float64) / c["temperature"]
    return (x - x.max() - np.log(np.exp(x - x.max()).sum())).astype(F32)


def reference(c, row, topk, **mistake):
    return R.search(row, c["beam"], EOS, c["min_steps"], c["steps"], bos=BOS, length_normalization=c["norm"],
                    using_eos_threshold=c["thr"] is not None, eos_threshold=c["thr"] or 1.5, topk=topk, return_topk=topk > 1,
                    **mistake)


def frozen_model(V, dev):
    """A tiny decoder whose logits are its seq_lin bias.  One per vocabulary and device; only the bias changes afterwards."""
    from speechbrain_amd.inference.builders import build_modules

    key = (V, dev.type)
    if key not in _MODELS:
        m = build_modules(dict(d_model=32, nhead=2, d_ffn=64, n_enc=1, n_dec=1, n_fft=512, win_length=32), vocab=V, seed=5)
        mods = torch.nn.ModuleDict({k: m[k] for k in ("Transformer", "seq_lin")}).to(dev).eval()
        with torch.no_grad():
            mods["seq_lin"].w.weight.zero_()
        _MODELS[key] = mods
    return _MODELS[key]


def searcher(c, dev, topk=1, **attrs):
    from speechbrain_amd.decoders import S2STransformerBeamSearcher

    mods = frozen_model(c["b"].size, dev)
    with torch.no_grad():
        mods["seq_lin"].w.bias.copy_(torch.from_numpy(c["b"]))
    T = c["T"]
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=BOS, eos_index=EOS,
                                    min_decode_ratio=(c["min_steps"] + 0.5) / T if c["min_steps"] else 0.0,
                                    max_decode_ratio=(c["steps"] + 0.5) / T, beam_size=c["beam"],
                                    using_eos_threshold=c["thr"] is not None, eos_threshold=c["thr"] or 1.5,
                                    length_normalization=c["norm"], temperature=c["temperature"], return_topk=topk > 1, topk=topk)
    for k, v in attrs.items():
        setattr(bs, k, v)
    assert bs._steps(T) == (c["min_steps"], c["steps"])
    return bs


def encoder_states(c, dev):
    enc = torch.randn(c["B"], c["T"], 32, generator=torch.Generator().manual_seed(c["T"])).to(dev)
    return enc, torch.linspace(1.0, 0.7, c["B"]).to(dev)


def kernel_row(nat, dev, c):
    b = torch.from_numpy(c["b"]).to(dev)
    return nat.log_softmax(b[None].contiguous(), c["temperature"], 1.0)[0].cpu().numpy()


def refs_of(name, nat, dev):
    """The case's log-prob row from this backend's own log-softmax kernel and the host searches on it: computed once."""
    key = (name, dev.type)
    if key not in _REFS:
        c = built(name)
        row = kernel_row(nat, dev, c)
        _REFS[key] = (row, {k: reference(c, row, k) for k in sorted({1, c["beam"]})})
    return _REFS[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.int32)


def assert_same(what, got, ref, K):
    """Device outputs (tokens [B*K, L], lens, scores, log-probs, longest per utterance) against one host Result per utterance."""
    tok, ln, sc, lp, longest = (np.asarray(t.cpu()) if torch.is_tensor(t) else np.asarray(t) for t in got)
    for u, r in enumerate(ref):
        rows = slice(u * K, (u + 1) * K)
        assert tok.shape[1] == r.tokens.shape[1], (what, tok.shape, r.tokens.shape)
        assert np.array_equal(tok[rows], r.tokens), (what, u, tok[rows], r.tokens)
        assert np.array_equal(ln[rows], r.lens), (what, u, ln[rows], r.lens)
        assert np.array_equal(bits(sc[rows]), bits(r.scores)), (what, u, sc[rows], r.scores)
        assert np.array_equal(bits(lp[rows]), bits(r.logp)), (what, u, lp[rows], r.logp)
        assert int(longest[u]) == r.longest, (what, u, longest, r.longest)


def run_case(nat, dev, name, what="", **attrs):
    c = built(name)
    _, refs = refs_of(name, nat, dev)
    assert refs[c["beam"]].straddles or not c["ties"]  # (on this backend's row too, not only on the fp64 row of the CPU test)
    enc, wl = encoder_states(c, dev)
    for topk in refs:
        bs = searcher(c, dev, topk, **attrs)
        for fused in (1, 0):
            with nat.knobs(score_fused=fused):
                tok, ln, sc, lp, mxl = bs.search_device(enc, wl)
            assert_same(f"{name} topk={topk} fused={fused} {what}", (tok, ln, sc, lp, [int(mxl.cpu())] * c["B"]),
                        [refs[topk]] * c["B"], topk)


def test_the_logits_are_the_bias(backend):
    """The premise, before anything else: with a zero seq_lin weight the first token's returned log-prob is the entry of
    native.log_softmax(b) at that token, bitwise, on the fused and on the separate scoring path and on every register-list
    width (a projection route that left the logits different from b would fail here first)."""
    nat, dev = backend
    for name in ("v40_b2", "v257_b3_ragged", "v1025_b8", "v5121_b16", "v8193_b5"):
        c = built(name)
        row = kernel_row(nat, dev, c)
        assert float(np.abs(row.astype(np.float64) - host_row(c)).max()) <= 1e-5
        enc, wl = encoder_states(c, dev)
        for fused in (1, 0):
            with nat.knobs(score_fused=fused):
                tok, _, _, lp, _ = searcher(c, dev, c["beam"]).search_device(enc, wl)  # (topk > 1: rows keep their last token)
            tok, lp = tok.cpu().numpy(), lp.cpu().numpy()
            assert np.array_equal(bits(lp[:, 0]), bits(row[tok[:, 0]])), (name, fused, lp[:, 0], row[tok[:, 0]])


@pytest.mark.parametrize("name", list(CASES))
def test_frozen_logits_equal_the_host_search(backend, name):
    """Every output of the public searcher, bit for bit, for the best hypothesis and for the whole finished list
    (return_topk, topk = beam), with the fused scoring pass and with the separate launches."""
    nat, dev = backend
    run_case(nat, dev, name)


@pytest.mark.parametrize("name", STEPPING)
@pytest.mark.parametrize("graph_mode", [1, 2])
def test_frozen_logits_in_every_stepping_mode(backend, name, graph_mode):
    """The step number in device memory (2) and two steps replayed from a captured graph (1; the emulator falls back to 2), each
    with the stop rule polled every 8 steps, every step and never: polling past the stop point changes nothing."""
    nat, dev = backend
    side = torch.cuda.stream(torch.cuda.Stream(dev)) if dev.type == "cuda" else contextlib.nullcontext()
    for check_every in (8, 1, 0):
        with side:
            run_case(nat, dev, name, f"graph_mode={graph_mode} check_every={check_every}", graph_mode=graph_mode, overlap_ctc=0,
                     check_every=check_every)


@pytest.mark.parametrize("check_every", [1, 0])
def test_early_stop_changes_nothing(backend, check_every):
    """Host step argument: lists that fill well before max_steps, stop rule polled every step (the search ends early) and never
    (it runs all 20 steps past full lists)."""
    nat, dev = backend
    run_case(nat, dev, "fills_early", f"check_every={check_every}", check_every=check_every)


def test_beam_above_the_limit_is_refused(backend):
    nat, dev = backend
    c = dict(built("v600_b128"), beam=129)
    enc, wl = encoder_states(c, dev)
    with pytest.raises(nat.SbkError, match=r"beam 129 outside \[1,128\]"):
        searcher(c, dev).search_device(enc, wl)


GROUP_MIN, GROUP_MAX = [0, 2, 1], [1, 7, 4]  # per utterance: one step only next to one that runs to the end


@pytest.mark.parametrize("beam", [4, 16, 17])
def test_grouped_search_with_per_utterance_limits(backend, beam):
    """native.beam_search with utt_min_steps / utt_max_steps: an utterance whose own limit is reached is frozen while the others
    go on; every utterance equals its own host search, want_longest included."""
    nat, dev = backend
    c = case(planted(300, 40 + beam, beam, eos_rank=0), beam, max(GROUP_MAX), B=3)
    row = kernel_row(nat, dev, c)
    enc, wl = encoder_states(c, dev)
    enc_len = torch.round(c["T"] * wl).int()
    umin, umax = (torch.tensor(v, dtype=torch.int32).to(dev) for v in (GROUP_MIN, GROUP_MAX))
    for topk in (1, beam):
        ref = [R.search(row, beam, EOS, mn, mx, bos=BOS, topk=topk, return_topk=topk > 1, pitch=max(GROUP_MAX))
               for mn, mx in zip(GROUP_MIN, GROUP_MAX)]
        assert len({r.longest for r in ref}) > 1 and ref[0].longest == 1
        bs = searcher(c, dev, topk)
        for mode in (0, 2):
            for fused in (1, 0):
                cfg = bs.config(c["T"])
                cfg.min_steps, cfg.max_steps, cfg.graph_mode, cfg.overlap_ctc = min(GROUP_MIN), max(GROUP_MAX), mode, 0
                with nat.knobs(score_fused=fused):
                    tok, ln, sc, lp, mxl, _, longest = nat.beam_search(bs._handle(), cfg, enc.contiguous(), enc_len,
                                                                       utt_min_steps=umin, utt_max_steps=umax, want_longest=True)
                assert_same(f"grouped beam={beam} topk={topk} fused={fused} mode={mode}", (tok, ln, sc, lp, longest), ref, topk)
                assert int(mxl.cpu()) == max(r.longest for r in ref)


# ------------------------------------------------------------------------------------- conditions on the inputs (no kernel)
def test_cases_are_not_degenerate():
    """Properties of the host search alone (rows from fp64 log-softmax): every case that lets hypotheses end through eos
    harvests at least two of them at two different lengths; at least one case fills its list early and one harvests nothing;
    every tie case has a tie group across the beam-th rank on some step, and the radix kernel's tie branches are all reached."""
    full, none = [], []
    for name in CASES:
        c = built(name)
        r = reference(c, host_row(c), c["beam"])
        lengths = {n for n, _ in r.harvested}
        print(f"{name}: V={c['b'].size} beam={c['beam']} harvested {len(r.harvested)} at lengths {sorted(lengths)}, full after "
              f"{r.full_at} of {c['steps']} steps, {len(r.straddles)} steps with a tie group across the beam-th rank "
              f"(largest group {max([s[2] for s in r.straddles], default=0)})")
        if c["eos"]:
            assert len(r.harvested) >= 2 and len(lengths) >= 2, name
        if c["fills"] is True:
            assert 0 < r.full_at < c["steps"] - 3, name
            full.append(name)
        if c["fills"] is False:
            assert not r.harvested, name
            none.append(name)
        if c["ties"]:
            assert len(r.straddles) > 0, name
    assert full and none
    step0 = lambda name: [s for s in reference(built(name), host_row(built(name)), 1).straddles if s[0] == 0][0]  # noqa: E731
    _, value, size, taken, last = step0("v40_b66_dead_sea")  # the -inf form: the lowest indices of the dead candidates
    assert value == -np.inf and size == 65 * 40 and taken == 26 and last == 40 + 25
    _, value, size, taken, last = step0("v2600_b64_finite_sea")  # the finite form: past the sweep's first block
    assert np.isfinite(value) and size == 1500 > 1024 and taken == 64 - 6 and last >= 1024
    _, value, size, taken, last = step0("v300_b17")  # a few ties on the radix threshold
    assert np.isfinite(value) and 1 < size < 1024
    _, value, size, taken, last = step0("v8_b16_sea")
    assert value == -np.inf and size == 15 * 8 and taken == 16 - 8


@pytest.mark.parametrize("mistake", list(R.MUTATIONS))
def test_cases_tell_mistakes_apart(mistake):
    """CPU only: every planted mistake of the host search changes the expected output of at least one case, so a kernel that
    made it would fail that case."""
    seen = []
    for name in CASES:
        c = built(name)
        row = host_row(c)
        for topk in sorted({1, c["beam"]}):
            good, bad = reference(c, row, topk), reference(c, row, topk, **R.MUTATIONS[mistake])
            same = all(np.array_equal(getattr(good, f), getattr(bad, f)) for f in ("tokens", "lens", "logp")) and \
                np.array_equal(bits(good.scores), bits(bad.scores)) and good.longest == bad.longest
            if not same:
                seen.append(f"{name}/topk={topk}")
    print(f"'{mistake}' is seen by {len(seen)}: {' '.join(seen)}")
    assert seen


# ------------------------------------------------------------------------- history-dependent logits against the oracle
RANDOM_SEEDS = {257: 3, 1025: 4, 5121: 5, 8193: 6}
_RANDOM, _ORACLE = {}, {}


@contextlib.contextmanager
def default_dtype(dtype):
    """The oracle builds its constants in torch's default dtype: fp64 weights and states under an fp64 default run it in double."""
    keep = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        yield
    finally:
        torch.set_default_dtype(keep)


def _random_modules(V):
    from speechbrain_amd.inference.builders import build_modules

    m = build_modules(dict(d_model=32, nhead=2, d_ffn=64, n_enc=1, n_dec=2, n_fft=512, win_length=32), vocab=V,
                      seed=RANDOM_SEEDS[V])
    return torch.nn.ModuleDict({k: m[k] for k in ("Transformer", "seq_lin", "ctc_lin")}).eval()


def random_model(V, dev=None):
    """A random tiny model (CPU), its flat state dict, the oracle's configuration and two ragged utterances;
    with ``dev``: the same, its modules being a copy on that device."""
    if dev is not None and dev.type != "cpu":
        if (V, dev.type) not in _RANDOM:
            mods = _random_modules(V)
            mods.load_state_dict(random_model(V)[0].state_dict())
            _RANDOM[(V, dev.type)] = mods.to(dev)
        return (_RANDOM[(V, dev.type)],) + random_model(V)[1:]
    if V not in _RANDOM:
        mods = _random_modules(V)
        with torch.no_grad():
            mods["seq_lin"].w.weight.mul_(3.0)  # (flat enough for the lower ranks of the list to depend on the beam width)
            mods["ctc_lin"].w.weight.mul_(3.0)
            mods["seq_lin"].w.bias[EOS] += 4.0  # eos within reach: hypotheses end before the step limit
        sd = {f"{p}.{k}": v.detach().clone() for p in mods for k, v in mods[p].state_dict().items()}
        cfg = O.ModelCfg(d_model=32, nhead=2, num_encoder_layers=1, num_decoder_layers=2, d_ffn=64, vocab=V)
        enc = torch.randn(2, 14, 32, generator=torch.Generator().manual_seed(V)) * 1.5
        _RANDOM[V] = (mods, sd, cfg, enc, torch.tensor([1.0, 0.75]))
    return _RANDOM[V]


def oracle_search(V, beam, ctc_w, double=False):
    key = (V, beam, ctc_w, double)
    if key not in _ORACLE:
        _, sd, cfg, enc, wl = random_model(V)
        sc = O.SearchCfg(bos=BOS, eos=EOS, beam=beam, ctc_weight=ctc_w, using_eos_threshold=True, max_decode_ratio=0.5,
                         return_topk=True, topk=RANDOM_TOPK)
        if double:
            with default_dtype(torch.float64):
                _ORACLE[key] = O.beam_search(enc.double(), wl.double(), {k: v.double() for k, v in sd.items()}, cfg, sc)
        else:
            _ORACLE[key] = O.beam_search(enc, wl, sd, cfg, sc)
    return _ORACLE[key]


RANDOM_TOPK = 8  # the eight best of every list are compared: below the first, the entries depend on the beam width
RANDOM_CASES = [(V, beam, ctc_w) for V in (257, 1025, 5121) for beam in (16, 17, 33) for ctc_w in (0.0, 0.4)]


@pytest.mark.parametrize("V,beam,ctc_w", RANDOM_CASES)
def test_random_model_seeds_are_fair(V, beam, ctc_w):
    """CPU only: the oracle in fp64 and in fp32 returns the same eight hypotheses per utterance; their fp64 scores lie further
    apart than the 1e-4 the kernel's scores may be off, so no rank of the list hangs on rounding."""
    h32, l32, s32, _ = oracle_search(V, beam, ctc_w)
    h64, l64, s64, _ = oracle_search(V, beam, ctc_w, double=True)
    assert torch.equal(h32, h64) and float((l32.double() - l64).abs().max()) <= 1e-6
    assert float((s32.double() - s64).abs().max()) <= 2e-6
    assert float((s64[:, :-1] - s64[:, 1:]).min()) > 1e-4


def test_random_model_lists_depend_on_the_beam_and_end_through_eos():
    """CPU only: without the CTC scorer some listed hypotheses end through eos before the step limit, and the list of beam 33
    is not the list of beam 16 (the wide beam is not idle)."""
    for V in (257, 1025, 5121):
        narrow, wide = oracle_search(V, 16, 0.0), oracle_search(V, 33, 0.0)
        assert float(narrow[1].min()) < float(narrow[1].max())
        assert not torch.equal(narrow[0], wide[0]) or not torch.equal(narrow[2], wide[2])


@pytest.mark.parametrize("V,beam,ctc_w", RANDOM_CASES)
def test_random_model_beam_search_vs_oracle(backend, V, beam, ctc_w):
    """History-dependent logits at the vocabulary and beam edges (beams 17 and 33 cross the 16-beam CTC tiles): a wrong parent
    gather in the KV ancestry or in the CTC state shows here."""
    nat, dev = backend
    from speechbrain_amd.decoders import CTCScorer, S2STransformerBeamSearcher, ScorerBuilder

    mods, _, _, enc, wl = random_model(V, dev)
    scorer = None
    if ctc_w > 0:
        scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=EOS)],
                               weights={"ctc": ctc_w})
    bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=BOS, eos_index=EOS,
                                    min_decode_ratio=0.0, max_decode_ratio=0.5, beam_size=beam, using_eos_threshold=True,
                                    length_normalization=True, scorer=scorer, return_topk=True, topk=RANDOM_TOPK)
    hyps, lens, scores, _ = bs(enc.to(dev), wl.to(dev))
    hyps_ref, lens_ref, sc_ref, _ = oracle_search(V, beam, ctc_w)
    assert hyps.shape == hyps_ref.shape and torch.equal(hyps.cpu(), hyps_ref)
    assert float((scores.cpu() - sc_ref).abs().max()) <= 1e-4
    assert float((lens.cpu() - lens_ref).abs().max()) <= 1e-6


# ------------------------------------------------------------------------------------------- greedy pick at the vocabulary edges
@pytest.mark.parametrize("V", [257, 1025, 5121, 8193])
def test_greedy_search_vs_oracle(backend, V):
    nat, dev = backend
    mods, sd, cfg, enc, wl = random_model(V, dev)
    handle = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
    enc_len = torch.round(enc.shape[1] * wl).int().to(dev)
    tok, sc, _ = nat.greedy_search(handle, enc.to(dev).contiguous(), enc_len, 0, 7, BOS, EOS, check_every=0)
    hyps, _, sc_ref, _ = O.greedy_search(enc, wl, sd, cfg, O.SearchCfg(bos=BOS, eos=EOS, max_decode_ratio=0.5))
    tok, sc = tok.cpu(), sc.cpu()
    for u, h in enumerate(hyps):
        n = len(h)
        assert tok[u, :n].tolist() == h and (n == 7 or int(tok[u, n]) == EOS), (u, tok[u], h)
    L = sc_ref.shape[1]
    assert float((sc[:, :L] - sc_ref).abs().max()) <= 1e-4


@pytest.mark.parametrize("low,high", [(7, 200), (200, 263)])
def test_greedy_pick_of_tied_maxima(backend, low, high):
    """The contract of greedy_pick_kernel for equal maxima: the LOWER token index, as torch.argmax returns the first maximum on
    the reference's side.  Frozen logits with the maximum shared by two tokens: (7, 200) sit in the first and the last wave of
    one 256-column stripe; of (200, 263) the higher index belongs to the lower thread (263 = 256 + 7)."""
    nat, dev = backend
    b, order = _ranked(300, 50)
    b[low] = b[high] = b[order[0]] + F32(1.0)
    c = case(b, 1, 3)
    mods = frozen_model(300, dev)
    with torch.no_grad():
        mods["seq_lin"].w.bias.copy_(torch.from_numpy(b))
    enc, wl = encoder_states(c, dev)
    handle = nat.DecoderHandle(mods["Transformer"], mods["seq_lin"])
    tok, _, _ = nat.greedy_search(handle, enc.contiguous(), torch.round(c["T"] * wl).int(), 0, 3, BOS, EOS, check_every=0)
    print(f"greedy pick of maxima tied between tokens {low} and {high}: {tok.cpu().tolist()}")
    assert tok.cpu().tolist() == [[low] * 3]
