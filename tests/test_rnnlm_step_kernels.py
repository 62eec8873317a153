"""csrc/rnnlm_step.hip -- sbk_rnnlm_step_f32 through native.rnnlm_step -- against the host restatement (tests/rnnlm_host_ref.py) in
double, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_rnn_kernels.py): max(4 x the error of the fp32 host restatement against its fp64 run on the
same inputs, 1e-5), for the scores and for both halves (h, c) of the state.

Measured for NEW_CASES, the worst of scores, h and c against fp64 (the scores in every case; every bound is the 1e-5 floor), on the
emulator / on the MI355X:
  n 128 perm 1.12e-6 / 1.02e-6    n 129 perm 4.05e-7 / 5.44e-7     n 129 cross 4.29e-7 / 4.37e-7   n 129 no map 3.48e-7 / 3.35e-7
  n 161 cross 4.57e-7 / 5.26e-7   n 161 perm 2.82e-7 / 3.36e-7     n 161 first step 2.27e-7 / 2.32e-7   n 97 7.50e-7 / 8.46e-7
  H 5 3.57e-7 / 3.40e-7           H 33 6.18e-7 / 4.32e-7           no LSTM biases 7.84e-7 / 8.49e-7     no DNN bias 2.27e-7 / 2.15e-7
  no output bias 6.89e-7 / 7.38e-7   n_emb = V + 3 9.51e-7 / 9.40e-7   D 257 1.37e-6 / 1.52e-6          D 300 5.08e-7 / 5.27e-7
  V 257 9.06e-7 / 1.35e-6         V 1025 4.68e-7 / 6.39e-7         the chain across row 128 (steps 0 and 2) 3.72e-7 / 5.21e-7
No case failed when it was first run: the kernels had none of the planted mistakes."""
import pytest
import torch

import rnnlm_host_ref as R

# (H, n, layers, blocks, V, parent, first step, temperature, weight, activation).  H 8: one ownership group of eight units, 13: a
# partial second one, 130: past two MFMA K tiles of a wave's quarter with a remainder (and no multiple of 4: scalar loads); H 16 /
# 136 take the 16-byte loads.  n 1 / 33 / 65: below, just past one and just past two 32-row tiles (one, two and four tiles per
# workgroup).  parent "perm": a permutation, "rep": a map that repeats rows and drops others, None: NULL.
OLD_CASES = [
    (8, 1, 1, 1, 5, None, True, 1.0, 1.0, "leaky_relu"),      # the smallest of everything, the first step
    (8, 33, 2, 1, 70, "perm", False, 1.25, 0.5, "relu"),      # two tiles, a permutation, temperature and weight
    (13, 33, 1, 2, 5, "rep", False, 1.0, 1.0, "gelu"),        # a partial ownership group, rows repeated, two DNN blocks
    (13, 65, 2, 2, 70, "perm", False, 1.0, 0.5, "tanh"),      # four tiles with the last three nearly empty
    (130, 1, 2, 1, 70, None, False, 1.25, 1.0, "leaky_relu"),  # K with a remainder, a continued step without a map
    (130, 33, 1, 1, 5, "rep", False, 1.0, 1.0, "relu"),       # K with a remainder through a repeating map
    (130, 65, 2, 2, 70, "rep", False, 1.25, 0.5, "gelu"),     # everything at its largest
    (130, 65, 2, 1, 5, None, True, 1.0, 1.0, "tanh"),         # the first step of a wide, deep LM
    (16, 33, 2, 1, 70, "rep", False, 1.0, 1.0, "leaky_relu"),  # the 16-byte load path, two tiles
    (136, 65, 2, 2, 5, "perm", False, 1.25, 1.0, "relu"),     # the 16-byte load path, quarters that end inside a chunk group
    (8, 65, 1, 1, 5, "rep", True, 1.0, 0.5, "gelu"),          # a map given with the first step (nothing to read through it)
    (13, 1, 2, 2, 70, "perm", False, 1.0, 1.0, "tanh"),       # one row, its own parent
]
# Past the fixture shapes.  An eleventh entry holds options: "D=257" the DNN width (9 otherwise), "emb+3" an embedding table of
# V + 3 rows with every fourth token in [V, V + 3), "no_lstm_bias" / "no_dnn_bias" / "no_out_bias" that bias None.
# n 97: launch_lstm<4> whose fourth tile has one row; 128: four full tiles, one row group; 129 / 161: the second row group
# (blockIdx.y = 1) with one live row / with a full tile and one live row of the next.  parent "cross": every row >= 128 continues a
# row < 128 and sixteen rows < 128 continue rows >= 128.  H 5: fewer units than one ownership group, three of the four waves have an
# empty K quarter; H 33: wave 2's quarter holds a single k, wave 3's none.  D 257 / 300: the LayerNorm's 256-strided loops make a
# second trip.  V 257 / 1025: the output layer and its log-softmax past 256 and 1 024 columns.
NEW_CASES = [
    (13, 128, 2, 1, 70, "perm", False, 1.0, 1.0, "relu"),                   # four full tiles, one row group
    (13, 129, 2, 2, 70, "perm", False, 1.25, 0.5, "leaky_relu"),            # the second row group, one live row
    (16, 129, 1, 1, 5, "cross", False, 1.0, 1.0, "tanh"),                   # row 128 from below 128, rows below from row 128
    (13, 129, 2, 1, 5, None, False, 1.0, 1.0, "gelu"),                      # the second row group without a map
    (13, 161, 2, 1, 70, "cross", False, 1.0, 0.5, "gelu"),                  # the second group's second tile with one live row
    (16, 161, 2, 1, 5, "perm", False, 1.25, 1.0, "relu"),                   # the same through a permutation, 16-byte loads
    (13, 161, 1, 1, 5, None, True, 1.0, 1.0, "leaky_relu"),                 # the first step of two row groups
    (13, 97, 2, 1, 70, "perm", False, 1.0, 1.0, "tanh"),                    # four tiles, the fourth with one row
    (5, 33, 2, 1, 70, "perm", False, 1.0, 0.5, "relu"),                     # three waves with an empty K quarter
    (33, 65, 2, 1, 5, "rep", False, 1.25, 1.0, "gelu"),                     # a quarter of a single k, a quarter of none
    (13, 33, 2, 1, 70, "perm", False, 1.0, 1.0, "leaky_relu", ("no_lstm_bias",)),
    (16, 65, 1, 2, 5, "rep", False, 1.0, 0.5, "tanh", ("no_dnn_bias",)),
    (13, 33, 1, 1, 70, "perm", False, 1.25, 1.0, "relu", ("no_out_bias",)),
    (13, 33, 2, 1, 70, "rep", False, 1.0, 1.0, "gelu", ("emb+3",)),         # tokens past the output size, inside the table
    (13, 33, 1, 2, 70, "perm", False, 1.0, 1.0, "leaky_relu", ("D=257",)),  # one column in the LayerNorm's second trip
    (16, 65, 2, 2, 5, "rep", False, 1.25, 0.5, "gelu", ("D=300",)),
    (13, 33, 1, 1, 257, "perm", False, 1.0, 1.0, "relu"),                   # the output layer past 256 columns
    (16, 33, 2, 1, 1025, "rep", False, 1.25, 0.5, "tanh"),                  # ... and past 1 024
]
CASES = OLD_CASES + NEW_CASES
CHAIN = (13, 33, 2, 1, 70, "rep", False, 1.25, 0.5, "leaky_relu")  # 20 steps, a fresh map each step, the buffers swapped
CHAIN_STEPS = 20
CHAIN_128 = (13, 161, 2, 1, 70, "cross", False, 1.25, 0.5, "tanh")  # 3 steps across row 128, the buffers swapped
CHAIN_128_STEPS = 3
_CACHE = {}


def _ids(case):
    return "-".join("+".join(x) if isinstance(x, tuple) else str(x) for x in case)


def _opts(case):
    """(DNN width, rows of the embedding table past V, LSTM / DNN / output biases present)."""
    opts = case[10] if len(case) > 10 else ()
    D = [int(o[2:]) for o in opts if o.startswith("D=")]
    return D[0] if D else 9, 3 if "emb+3" in opts else 0, tuple(f"no_{k}_bias" not in opts for k in ("lstm", "dnn", "out"))


def _parent(kind, n, gen):
    if kind is None:
        return None
    if kind == "perm":
        return torch.randperm(n, generator=gen).int()
    if kind == "rep":
        return torch.randint(0, max(n // 2, 1), (n,), generator=gen, dtype=torch.int32)
    assert kind == "cross" and n > 128
    p = torch.randint(0, 128, (n,), generator=gen, dtype=torch.int32)
    below = torch.randperm(128, generator=gen)[:16]
    p[below] = torch.randint(128, n, (16,), generator=gen, dtype=torch.int32)
    return p


def _case(case, steps=1):
    """Inputs, the fp64 (out, state) of every step and the fp32 restatement's error per step: computed once, never modified."""
    key = (case, steps)
    if key not in _CACHE:
        H, n, layers, blocks, V, pk, first, temp, weight, act = case[:10]
        D, past, (lstm_bias, dnn_bias, out_bias) = _opts(case)
        gen = torch.Generator().manual_seed(1009 * H + 31 * n + 7 * layers + 3 * blocks + V + steps)
        lm = R.random_lm(gen, V, 6, H, layers, blocks, D, n_emb=V + past, lstm_bias=lstm_bias, dnn_bias=dnn_bias, out_bias=out_bias)
        tokens = [torch.randint(0, V, (n,), generator=gen, dtype=torch.int32) for _ in range(steps)]
        if past:
            for tok in tokens:
                tok[::4] = V + torch.arange(tok[::4].numel(), dtype=torch.int32) % past
        parents = [_parent(pk, n, gen) for _ in range(steps)]
        state0 = None if first else torch.randn(layers, 2, n, H, generator=gen) * 0.7
        x = dict(lm=lm, tokens=tokens, parents=parents, state0=state0)
        r32, r64 = _host(x, case, torch.float32), _host(x, case, torch.float64)
        err = [tuple(R.bound(a, b) for a, b in ((o32, o64), (s32[:, 0], s64[:, 0]), (s32[:, 1], s64[:, 1])))
               for (o32, s32), (o64, s64) in zip(r32, r64)]
        _CACHE[key] = (x, r64, err)
    return _CACHE[key]


def _host(x, case, dt, mistakes=()):
    lm, state = R.cast(x["lm"], dt), None if x["state0"] is None else x["state0"].to(dt)
    out = []
    for tok, par in zip(x["tokens"], x["parents"]):
        o, state = R.step(lm, case[9], tok, par, state, case[8], case[7], mistakes)
        out.append((o, state))
    return out


def _prepared(nat, dev, lm, act):
    d = lambda t: t.to(dev).contiguous() if torch.is_tensor(t) else t  # noqa: E731
    code = {"leaky_relu": nat.ACT_LEAKY_RELU, "relu": nat.ACT_RELU, "gelu": nat.ACT_GELU, "tanh": nat.ACT_TANH}[act]
    return nat.RNNLMPrepared(d(lm["emb"]), [tuple(d(t) for t in l) for l in lm["lstm"]], [tuple(d(t) for t in b) for b in lm["dnn"]],
                             d(lm["out_w"]), d(lm["out_b"]), code)


def _kernel(nat, dev, x, case):
    """Every step through native.rnnlm_step on two state buffers that swap roles."""
    prep = _prepared(nat, dev, x["lm"], case[9])
    n = x["tokens"][0].shape[0]
    bufs = [nat.rnnlm_state(prep, n), nat.rnnlm_state(prep, n)]
    state, out = None, []
    if x["state0"] is not None:
        bufs[1].copy_(x["state0"])
        state = bufs[1]
    for s, (tok, par) in enumerate(zip(x["tokens"], x["parents"])):
        o, state = nat.rnnlm_step(prep, tok.to(dev), None if par is None else par.to(dev), state, bufs[s & 1], case[8], case[7])
        out.append((o, state.clone()))
    return out


def _check(what, got, ref, err):
    for s, ((o, st), (o64, st64), (bo, bh, bc)) in enumerate(zip(got, ref, err)):
        o, st = o.cpu().double(), st.cpu().double()
        eo, eh, ec = (float((a - b).abs().max()) for a, b in ((o, o64), (st[:, 0], st64[:, 0]), (st[:, 1], st64[:, 1])))
        if s in (0, len(got) - 1):
            print(f"rnnlm_step {what} step {s}: out max|d| {eo:.3e} (bound {bo:.1e}), h {eh:.3e} ({bh:.1e}), c {ec:.3e} ({bc:.1e})")
        assert o.shape == o64.shape and st.shape == st64.shape
        assert eo <= bo and eh <= bh and ec <= bc, (what, s, eo, bo, eh, bh, ec, bc)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_step_vs_fp64(backend, case):
    nat, dev = backend
    x, ref, err = _case(case)
    _check(_ids(case), _kernel(nat, dev, x, case), ref, err)


def test_20_chained_steps(backend):
    """The state of step s is what step s - 1 wrote, read through a fresh map: the two buffers swap every step."""
    nat, dev = backend
    x, ref, err = _case(CHAIN, CHAIN_STEPS)
    _check("chain", _kernel(nat, dev, x, CHAIN), ref, err)


def test_3_chained_steps_across_row_128(backend):
    """Two row groups whose rows continue rows of the other group, three steps in a row: what the second group wrote at step s
    - 1 is what the first reads at step s."""
    nat, dev = backend
    x, ref, err = _case(CHAIN_128, CHAIN_128_STEPS)
    _check("chain across row 128", _kernel(nat, dev, x, CHAIN_128), ref, err)


def test_same_bits_twice_and_on_two_streams(backend):
    nat, dev = backend
    x, _, _ = _case(CHAIN, CHAIN_STEPS)
    few = dict(x, tokens=x["tokens"][:3], parents=x["parents"][:3])
    run = lambda: [t for pair in _kernel(nat, dev, few, CHAIN) for t in pair]  # noqa: E731
    a, b = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    if dev.type == "cuda":
        for _ in range(2):
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                o = run()
            s.synchronize()
            assert all(torch.equal(p, q) for p, q in zip(a, o))


def test_bad_arguments_are_named(backend):
    nat, dev = backend
    x, _, _ = _case(CASES[1])
    prep = _prepared(nat, dev, x["lm"], "relu")
    tok, state = x["tokens"][0].to(dev), x["state0"].to(dev)
    bad = lambda v: torch.cat([tok[:-1], torch.tensor([v], dtype=torch.int32, device=dev)])  # noqa: E731
    for kw, name in ((dict(tokens=bad(70)), "tokens"), (dict(tokens=bad(-1)), "tokens"), (dict(parent=bad(33)), "parent"),
                     (dict(parent=bad(-1)), "parent"), (dict(state_out=state), "alias"), (dict(temperature=0.0), "temperature")):
        with pytest.raises(nat.SbkError, match=name):
            nat.rnnlm_step(prep, **{**dict(tokens=tok, parent=None, state_in=state), **kw})


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_cases_tell_mistakes_apart(mistake):
    """Each planted mistake moves at least one committed case of this file by 1e3 x that case's bound or more."""
    worst = max(_moved(mistake, c, s) for c, s in [(c, 1) for c in CASES] + [(CHAIN, CHAIN_STEPS), (CHAIN_128, CHAIN_128_STEPS)])
    print(f"planted mistake '{mistake}': moves a committed case by {worst:.3e} x its bound")
    assert worst >= 1e3


def _moved(mistake, case, steps):
    """The largest distance, in units of the case's bounds, by which the planted mistake moves the case's fp64 outputs."""
    x, ref, err = _case(case, steps)
    worst = 0.0
    for (o, st), (o64, st64), (bo, bh, bc) in zip(_host(x, case, torch.float64, (mistake,)), ref, err):
        worst = max(worst, float((o - o64).abs().max()) / bo, float((st[:, 0] - st64[:, 0]).abs().max()) / bh,
                    float((st[:, 1] - st64[:, 1]).abs().max()) / bc)
    return worst


@pytest.mark.parametrize("mistake", ["parent_mod_128", "rows_past_128_from_zero", "ln_first_256", "token_clamped_to_vocab"])
def test_the_fixture_shapes_are_blind_to_it(mistake):
    """CPU only.  None of the cases this file had before NEW_CASES and CHAIN_128 (n <= 65, D = 9, an embedding table of V rows) is
    moved at all by these mistakes: the cases past those shapes are what sees them.  ('bias_once' is not listed: every one of
    those cases has both LSTM biases and is moved by it.)"""
    for case, steps in [(c, 1) for c in OLD_CASES] + [(CHAIN, CHAIN_STEPS)]:
        assert _moved(mistake, case, steps) == 0.0, (mistake, case)
