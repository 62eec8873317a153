"""csrc/sligru.hip -- sbk_sligru_layer_f32 (native.sligru_layer) -- against a plain torch loop of the cell in double on the CPU, on
the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound: max(4 x e32, 1e-5), e32 the error of the SAME loop run in fp32 against its fp64 run on the same inputs; the factor 4 covers
the split-K summation order and another reduction tree for the statistics (the margin of the CTC prefix scorer's bound), the floor
is the project's.  Inputs: the feed-forward term ~N(0,1), u orthogonal x 3 so the normalised term is not dominated by xp.  On these inputs
e32 is between 4e-9 and 2.6e-6: below 1e-5 / 4 for every tuple but H130-B33-D2-T7-affine-zeros-relu (2.58e-6, where 4 x e32 sets
the bound); the kernel's error is 0.46 to 2.07 x e32 on the emulator and 0.42 to 1.54 x on the MI355X."""
import pytest
import torch

ACTS = {"relu": torch.relu, "tanh": torch.tanh, "sin": torch.sin, "leaky_relu": torch.nn.functional.leaky_relu}
# (H, B, D, T, affine, h0, act): H one unit / below, at, across the 8-unit slice / K no multiple of 4 or of the waves' parts (at
# H 130 a wave's part is 48 k: one trip of the K loop, none for the last wave) / H 520 and 517: a part of 144 k is a second trip of
# 128 k, ragged in the last wave, with and without 16-byte rows, and a thread of the norm-and-cell pass holds units tid + 256 i for
# i up to 2; B the row-tile remainder and (33 x 2 directions) a third row tile; T first step only, the hand-off, a chain
CASES = [
    (1, 1, 1, 1, False, False, "relu"), (1, 3, 2, 2, True, True, "tanh"), (5, 1, 2, 7, True, False, "sin"),
    (5, 33, 1, 2, False, True, "leaky_relu"), (8, 3, 1, 7, True, True, "relu"), (8, 33, 2, 1, False, False, "tanh"),
    (13, 1, 1, 2, False, True, "sin"), (13, 3, 2, 7, True, False, "leaky_relu"), (13, 33, 2, 2, True, True, "relu"),
    (16, 1, 2, 1, True, True, "leaky_relu"), (16, 3, 1, 2, False, False, "sin"), (16, 33, 2, 7, False, True, "tanh"),
    (130, 1, 1, 7, True, True, "tanh"), (130, 3, 2, 2, False, True, "relu"), (130, 33, 1, 1, True, False, "sin"),
    (130, 33, 2, 7, True, False, "relu"), (130, 3, 2, 1, False, False, "leaky_relu"), (130, 1, 2, 2, True, False, "relu"),
    (8, 1, 2, 2, False, True, "sin"), (5, 3, 1, 1, True, True, "leaky_relu"),
    (520, 3, 2, 2, True, True, "relu"), (517, 3, 2, 2, False, False, "tanh"),
]
_CASES = {}


def _loop(xp, u, gamma, beta, h0, D, act):
    """The reference's cell (nnet/RNN.py:1743-1804): the time-flipped batch stacked under the batch, one loop over time."""
    B, T, G = xp.shape
    w = torch.cat([xp, xp.flip(1)], dim=0) if D == 2 else xp
    h = h0.reshape(D * B, -1) if h0 is not None else xp.new_zeros(D * B, G // 2)
    hs = []
    for k in range(T):
        gates = w[:, k] + torch.nn.functional.layer_norm(h @ u.t(), (G,), gamma, beta, 1e-5)
        a, z = gates.chunk(2, 1)
        z = torch.sigmoid(z)
        h = z * h + (1 - z) * ACTS[act](a)
        hs.append(h)
    o = torch.stack(hs, dim=1)
    out = torch.cat([o[:B], o[B:].flip(1)], dim=2) if D == 2 else o
    return out, h.reshape(D, B, -1)


def _case(case):
    """Inputs, the fp64 result and the error of the fp32 run of the same loop: computed once, never modified."""
    if case not in _CASES:
        H, B, D, T, affine, state, act = case
        gen = torch.Generator().manual_seed(H * 1000003 + B * 1009 + D * 101 + T * 7 + affine + 2 * state)
        xp = torch.randn(B, T, 2 * H, generator=gen)
        u = torch.nn.init.orthogonal_(torch.empty(2 * H, H), generator=gen) * 3.0
        gamma = 1.0 + 0.5 * torch.randn(2 * H, generator=gen) if affine else None
        beta = 0.5 * torch.randn(2 * H, generator=gen) if affine else None
        h0 = torch.randn(D, B, H, generator=gen) if state else None
        args = (xp, u, gamma, beta, h0)
        ref = _loop(*(None if t is None else t.double() for t in args), D, act)
        e32 = max(float((a.double() - b).abs().max()) for a, b in zip(_loop(*args, D, act), ref))
        _CASES[case] = (args, ref, e32)
    return _CASES[case]


def _run(nat, dev, case):
    args, _, _ = _case(case)
    return nat.sligru_layer(*(None if t is None else t.to(dev).contiguous() for t in args), act=case[6], D=case[2])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "H{}-B{}-D{}-T{}-{}-{}-{}".format(*c[:4], "affine" if c[4] else "plain",
                                                                                       "h0" if c[5] else "zeros", c[6]))
def test_vs_fp64_loop(backend, case):
    nat, dev = backend
    _, ref, e32 = _case(case)
    got = _run(nat, dev, case)
    errs = [float((g.cpu().double() - r).abs().max()) for g, r in zip(got, ref)]
    print(f"sligru_layer {case}: kernel max|d| out {errs[0]:.3e} hn {errs[1]:.3e}, torch fp32 {e32:.3e}, "
          f"ratio {max(errs) / max(e32, 1e-30):.2f}")
    assert all(g.shape == r.shape for g, r in zip(got, ref))
    assert max(errs) <= max(4.0 * e32, 1e-5)


def test_same_bits_twice(backend):
    nat, dev = backend
    a, b = _run(nat, dev, CASES[15]), _run(nat, dev, CASES[15])
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("kw,name", [(dict(H=0), "H=0"), (dict(H=2049), "H <= 2048"), (dict(D=3), "D=3"), (dict(B=0), "B=0"),
                                     (dict(T=0), "T=0"), (dict(act=4), "act=4"), (dict(alias=True), "h0 must not alias"),
                                     (dict(beta=False), "ln_beta"), (dict(short=1), "too small")])
def test_bad_arguments_are_named(backend, kw, name):
    nat, dev = backend
    lib = nat.load()
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731

    def rc(B=2, T=3, H=8, D=2, act=0, alias=False, beta=True, short=0):
        Hc, Bc, Tc = min(max(H, 1), 2048), max(B, 1), max(T, 1)
        xp, u, g, out, hn, ws = z(Bc, Tc, 2 * Hc), z(2 * Hc, Hc), z(2 * Hc), z(Bc, Tc, 2 * Hc), z(2, Bc, Hc), z(2 * Bc * 2 * Hc + 4)
        r = lib.sbk_sligru_layer_f32(nat._p(xp), nat._p(u), nat._p(g), nat._p(g) if beta else None, nat._p(hn) if alias else None,
                                     nat._p(out), nat._p(hn), nat._p(ws), 2 * Bc * 2 * Hc * 4 - short, B, T, H, D, act,
                                     nat._stream(xp))
        return r, lib.sbk_last_error().decode()

    assert rc()[0] == 0
    r, msg = rc(**kw)
    assert r == -22 and name in msg, (kw, r, msg)
    assert lib.sbk_sligru_layer_workspace_bytes(2, 8, 2) == 2 * 2 * 16 * 4 and lib.sbk_sligru_layer_workspace_bytes(2, 2049, 2) == 0
    assert lib.sbk_sligru_layer_workspace_bytes(1048560, 1, 2) > 0 and lib.sbk_sligru_layer_workspace_bytes(1048561, 1, 2) == 0
