"""csrc/rnnlm_step.hip -- sbk_rnnlm_step_f32 through native.rnnlm_step -- against the host restatement (tests/rnnlm_host_ref.py) in
double, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_rnn_kernels.py): max(4 x the error of the fp32 host restatement against its fp64 run on the
same inputs, 1e-5), for the scores and for both halves (h, c) of the state."""
import pytest
import torch

import rnnlm_host_ref as R

# (H, n, layers, blocks, V, parent, first step, temperature, weight, activation).  H 8: one ownership group of eight units, 13: a
# partial second one, 130: past two MFMA K tiles of a wave's quarter with a remainder (and no multiple of 4: scalar loads); H 16 /
# 136 take the 16-byte loads.  n 1 / 33 / 65: below, just past one and just past two 32-row tiles (one, two and four tiles per
# workgroup).  parent "perm": a permutation, "rep": a map that repeats rows and drops others, None: NULL.
CASES = [
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
CHAIN = (13, 33, 2, 1, 70, "rep", False, 1.25, 0.5, "leaky_relu")  # 20 steps, a fresh map each step, the buffers swapped
CHAIN_STEPS = 20
_CACHE = {}


def _ids(case):
    return "-".join(str(x) for x in case)


def _case(case, steps=1):
    """Inputs, the fp64 (out, state) of every step and the fp32 restatement's error per step: computed once, never modified."""
    key = (case, steps)
    if key not in _CACHE:
        H, n, layers, blocks, V, pk, first, temp, weight, act = case
        gen = torch.Generator().manual_seed(1009 * H + 31 * n + 7 * layers + 3 * blocks + V + steps)
        lm = R.random_lm(gen, V, 6, H, layers, blocks, 9)
        tokens = [torch.randint(0, V, (n,), generator=gen, dtype=torch.int32) for _ in range(steps)]
        parents = [None if pk is None else torch.randperm(n, generator=gen).int() if pk == "perm" else
                   torch.randint(0, max(n // 2, 1), (n,), generator=gen, dtype=torch.int32) for _ in range(steps)]
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
    worst = 0.0
    for case, steps in [(c, 1) for c in CASES] + [(CHAIN, CHAIN_STEPS)]:
        x, ref, err = _case(case, steps)
        for (o, st), (o64, st64), (bo, bh, bc) in zip(_host(x, case, torch.float64, (mistake,)), ref, err):
            worst = max(worst, float((o - o64).abs().max()) / bo, float((st[:, 0] - st64[:, 0]).abs().max()) / bh,
                        float((st[:, 1] - st64[:, 1]).abs().max()) / bc)
    print(f"planted mistake '{mistake}': moves a committed case by {worst:.3e} x its bound")
    assert worst >= 1e3
