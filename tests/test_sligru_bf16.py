"""csrc/sligru_bf16.hip -- sbk_sligru_layer_bf16 (native.sligru_layer under precision_scope("bf16")) -- against a plain fp64 loop of
the cell on the CPU, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's bf16 rule, tests/test_crdnn_bf16.py): 2 * e_model + 1e-3, e_model = the max error, against the fp64 loop, of
the same fp64 loop with the kernel's two roundings made explicit: u to bf16, and h_{t-1} to bf16 before the product only (the
sigmoid(z) h_{t-1} term keeps the unrounded state).  Inputs as tests/test_sligru_kernels.py: xp ~ N(0,1), u orthogonal x 3, the same
seed formula.  e_model is 8.2e-10 for H 1 and 3.2e-3 .. 1.9e-2 otherwise; reference values are O(1 .. 6), so a wrong lane order,
gate column or shadow index moves the result by O(0.1 .. 1).  Every case prints ratio = kernel error / e_model: 1.00 for every case with H >= 8,
on the MI355X and on the emulator (H 1: kernel error 2.4e-8)."""
import pytest
import torch

ACTS = {"relu": torch.relu, "tanh": torch.tanh, "sin": torch.sin, "leaky_relu": torch.nn.functional.leaky_relu}
# (H, B, D, T, affine, h0, act): H one unit / below, at, across an 8-unit slice / below one 32-k chunk, exactly one, 5 chunks (the
# last wave has none) / H 520 and 517: the cell's threads pass the first wave, 517 has no 16-byte rows; B the row-tile remainder
# and (33 x 2) a third row tile; T 1 with h0 (the entry kernel's shadow), 2 (the hand-off), 7 and 40 (the ping-pong chain)
CASES = [
    (1, 1, 1, 2, False, True, "relu"), (8, 1, 1, 2, False, True, "relu"), (8, 33, 2, 7, True, False, "tanh"),
    (13, 3, 2, 2, True, True, "sin"), (13, 33, 1, 7, False, False, "leaky_relu"), (32, 1, 2, 7, True, True, "relu"),
    (40, 33, 2, 2, False, True, "tanh"), (136, 1, 1, 7, True, False, "relu"), (136, 3, 2, 1, False, True, "sin"),
    (136, 33, 2, 7, True, True, "relu"), (136, 33, 2, 40, False, False, "leaky_relu"), (520, 3, 2, 2, True, True, "relu"),
    (517, 3, 2, 7, False, False, "tanh"),
]
_CASES = {}
_ID = lambda c: "H{}-B{}-D{}-T{}-{}-{}-{}".format(*c[:4], "affine" if c[4] else "plain", "h0" if c[5] else "zeros", c[6])  # noqa: E731


def _r(t):  # round to bf16 (nearest even) from fp32, as the kernel does; carried on in fp64
    return t.float().bfloat16().double()


def _loop(xp, u, gamma, beta, h0, D, act, rnd=lambda t: t):
    """The reference's cell (nnet/RNN.py:1743-1804): the time-flipped batch stacked under the batch, one loop over time; ``rnd`` is
    applied to u and to h_{t-1} as operands of their product, and to nothing else."""
    B, T, G = xp.shape
    w = torch.cat([xp, xp.flip(1)], dim=0) if D == 2 else xp
    h = h0.reshape(D * B, -1) if h0 is not None else xp.new_zeros(D * B, G // 2)
    hs = []
    for k in range(T):
        gates = w[:, k] + torch.nn.functional.layer_norm(rnd(h) @ rnd(u).t(), (G,), gamma, beta, 1e-5)
        a, z = gates.chunk(2, 1)
        z = torch.sigmoid(z)
        h = z * h + (1 - z) * ACTS[act](a)
        hs.append(h)
    o = torch.stack(hs, dim=1)
    out = torch.cat([o[:B], o[B:].flip(1)], dim=2) if D == 2 else o
    return out, h.reshape(D, B, -1)


def _case(case):
    """fp32 inputs, the fp64 result and e_model: computed once, never modified."""
    if case not in _CASES:
        H, B, D, T, affine, state, act = case
        gen = torch.Generator().manual_seed(H * 1000003 + B * 1009 + D * 101 + T * 7 + affine + 2 * state)
        xp = torch.randn(B, T, 2 * H, generator=gen)
        u = torch.nn.init.orthogonal_(torch.empty(2 * H, H), generator=gen) * 3.0
        gamma = 1.0 + 0.5 * torch.randn(2 * H, generator=gen) if affine else None
        beta = 0.5 * torch.randn(2 * H, generator=gen) if affine else None
        h0 = torch.randn(D, B, H, generator=gen) if state else None
        args = (xp, u, gamma, beta, h0)
        a64 = [None if t is None else t.double() for t in args]
        ref = _loop(*a64, D, act)
        e_model = max(float((m - r).abs().max()) for m, r in zip(_loop(*a64, D, act, rnd=_r), ref))
        _CASES[case] = (args, ref, e_model)
    return _CASES[case]


def _run(nat, dev, case, precision="bf16"):
    """(out, hn) on the host and the names the profiler saw"""
    args = [None if t is None else t.to(dev).contiguous() for t in _case(case)[0]]
    nat.prof_reset(), nat.prof_enable(True)
    with nat.precision_scope(precision):
        got = nat.sligru_layer(*args, act=case[6], D=case[2])
    nat.prof_enable(False)
    return [g.cpu() for g in got], set(nat.prof_report())


@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_vs_fp64_loop(backend, case):
    nat, dev = backend
    H, T, product = case[0], case[3], case[3] > 1 or case[5]
    _, ref, e_model = _case(case)
    got, names = _run(nat, dev, case)
    errs = [float((g.double() - r).abs().max()) for g, r in zip(got, ref)]
    print(f"sligru_layer bf16 {_ID(case)}: max|d| out {errs[0]:.3e} hn {errs[1]:.3e}, e_model {e_model:.3e}, "
          f"ratio {max(errs) / e_model:.2f}")
    assert all(g.shape == r.shape for g, r in zip(got, ref))
    assert max(errs) <= 2.0 * e_model + 1e-3
    assert bool((got[0].bfloat16().float() != got[0]).any())  # the state is kept in fp32
    # (u's image is made once per tensor object: its tag is there on a case's first call only)
    assert names - {"sligru_u_image"} == {"sligru_norm_cell_bf16"} | ({"sligru_product_bf16"} if product else set())
    for precision in ("fp32", "fp16", "fp8"):  # every other precision takes the fp32 entry
        other, names = _run(nat, dev, case, precision)
        assert names == {"sligru_norm_cell"} | ({"sligru_product"} if product else set())
        if precision == "fp32":
            f32 = other
        else:
            assert all(torch.equal(a, b) for a, b in zip(other, f32))
    if H >= 136 and product:  # the bf16 path is really taken
        assert not torch.equal(got[0], f32[0])


def test_same_bits_twice_and_on_two_streams(backend):
    nat, dev = backend
    a = _run(nat, dev, CASES[9])[0]
    assert all(torch.equal(p, q) for p, q in zip(a, _run(nat, dev, CASES[9])[0]))
    if dev.type == "cuda":
        for _ in range(2):
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                o = _run(nat, dev, CASES[9])[0]
            torch.cuda.synchronize()
            assert all(torch.equal(p, q) for p, q in zip(a, o))


@pytest.mark.parametrize("what,name", [("image", "was not made for H=136"), ("workspace", "too small"), ("H2049", "H <= 2048")])
def test_refusals_are_named(backend, what, name):
    nat, dev = backend
    lib, (B, T, D, H) = nat.load(), (2, 3, 2, 136)
    Hc = 2049 if what == "H2049" else H
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    img = nat.lp_weight(z(2 * 8, 8) if what == "image" else z(2 * H, H), "sligru_u")
    nbytes = lib.sbk_sligru_layer_bf16_workspace_bytes(B, H, D)
    assert nbytes > 0 and lib.sbk_sligru_layer_bf16_workspace_bytes(B, 2049, D) == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    xp, out, hn = z(B, T, 2 * H), z(B, T, D * H), z(D, B, H)
    rc = lib.sbk_sligru_layer_bf16(nat._p(xp), nat._p(img), img.numel() * 2, None, None, None, nat._p(out), nat._p(hn), nat._p(ws),
                                   nbytes - (1 if what == "workspace" else 0), B, T, Hc, D, 0, nat._stream(xp))
    assert rc == -22 and name in lib.sbk_last_error().decode(), lib.sbk_last_error().decode()
