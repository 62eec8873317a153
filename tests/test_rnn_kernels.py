"""csrc/rnn.hip -- sbk_rnn_layer_f32 (native.rnn_layer) -- against torch.nn.LSTM in double on the CPU, on the CPU emulator of the
kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_wav2vec2_kernels.py): max(4 x the error of torch.nn.LSTM in fp32 against fp64 on the same
inputs, 1e-5), for out, hn and cn each.  The input part xp comes from native.gemm_nt, as in the product."""
import pytest
import torch

import crdnn_host_ref as R
from speechbrain_amd import native

IN = 5
HS, BS, TS, DS = [8, 40, 130], [1, 3, 33], [1, 2, 9], [1, 2]  # slices of 8 units: one, no multiple, across; 33: past one 32-row tile
LONG = (2, 300, 16, 2)  # (B, T, H, D): many steps
_CASES = {}


def _bound(err32):
    return max(4.0 * err32, 1e-5)


def _case(B, T, H, D, state, layers=1):
    """Weights, inputs, the fp64 result of torch.nn.LSTM and the error of its fp32 run: computed once, never modified."""
    key = (B, T, H, D, state, layers)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(B * 1000003 + T * 1009 + H * 7 + D + (13 if state else 0) + layers)
        m = torch.nn.LSTM(IN, H, layers, batch_first=True, bidirectional=D == 2)
        with torch.no_grad():
            for p in m.parameters():  # order-1 gates, biases of both signs; b_ih and b_hh differ
                p.copy_(torch.randn(p.shape, generator=gen) * (0.5 if p.dim() == 1 else 1.0 / max(p.shape[1], 4) ** 0.5 * 1.5))
        x = torch.randn(B, T, IN, generator=gen)
        hx = (torch.randn(layers * D, B, H, generator=gen), torch.randn(layers * D, B, H, generator=gen)) if state else None
        with torch.no_grad():
            o32, (h32, c32) = m(x, hx)
            m64 = torch.nn.LSTM(IN, H, layers, batch_first=True, bidirectional=D == 2).double()
            m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
            o64, (h64, c64) = m64(x.double(), None if hx is None else (hx[0].double(), hx[1].double()))
        err32 = max(float((a.double() - b).abs().max()) for a, b in ((o32, o64), (h32, h64), (c32, c64)))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        _CASES[key] = (sd, x, hx, (o64, h64, c64), err32)
    return _CASES[key]


def _run(nat, dev, sd, x, hx, D, layers=1, route=0):
    """The layers of the stack through native.gemm_nt + native.rnn_layer -> (out, hn [L*D,B,H], cn)."""
    x = x.to(dev)
    hs, cs = [], []
    for l in range(layers):
        w_ih, w_hh, b_ih, b_hh = (t.to(dev).contiguous() for t in R.lstm_weights(sd, "", l, D))
        B, T, _ = x.shape
        H = w_hh.shape[2]
        xp = nat.gemm_nt(x.contiguous(), w_ih.reshape(D * 4 * H, -1).contiguous()).view(B, T, D, 4 * H)
        h0 = None if hx is None else hx[0][l * D:(l + 1) * D].to(dev).contiguous()
        c0 = None if hx is None else hx[1][l * D:(l + 1) * D].to(dev).contiguous()
        x, hn, cn = nat.rnn_layer(xp, w_hh, b_ih, b_hh, h0, c0, route=route)
        hs.append(hn), cs.append(cn)
    return x, torch.cat(hs), torch.cat(cs)


def _check(what, got, ref, err32):
    errs = [float((g.cpu().double() - r).abs().max()) for g, r in zip(got, ref)]
    print(f"rnn_layer {what}: kernel max|d| out {errs[0]:.3e} hn {errs[1]:.3e} cn {errs[2]:.3e}, torch fp32 {err32:.3e}, "
          f"ratio {max(errs) / max(err32, 1e-30):.2f}")
    for g, r in zip(got, ref):
        assert g.shape == r.shape
    assert max(errs) <= _bound(err32)


@pytest.mark.parametrize("state", [False, True], ids=["zeros", "h0c0"])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
def test_vs_fp64_lstm(backend, H, B, T, D, state):
    nat, dev = backend
    sd, x, hx, ref, err32 = _case(B, T, H, D, state)
    assert nat.rnn_layer_route(B, T, H, D) == 1
    _check(f"H={H} B={B} T={T} D={D} {'h0c0' if state else 'zeros'}", _run(nat, dev, sd, x, hx, D), ref, err32)


def test_long_scan(backend):
    """300 steps: the state is handed from launch to launch through `out` and `cn` the whole way."""
    nat, dev = backend
    B, T, H, D = LONG
    sd, x, hx, ref, err32 = _case(B, T, H, D, True)
    _check(f"long scan T={T}", _run(nat, dev, sd, x, hx, D), ref, err32)


def test_second_layer_reads_forward_then_backward(backend):
    nat, dev = backend
    sd, x, hx, ref, err32 = _case(3, 9, 40, 2, True, layers=2)
    _check("two layers", _run(nat, dev, sd, x, hx, 2, layers=2), ref, err32)


@pytest.mark.gpu
def test_recipe_width_on_the_gpu():
    """H 1024: the real distribution over workgroups (128 slices x 2 directions)."""
    native.load()
    dev = torch.device("cuda:0")
    sd, x, hx, ref, err32 = _case(2, 3, 1024, 2, True)
    assert native.rnn_layer_route(2, 3, 1024, 2) == 1
    _check("H=1024 B=2 T=3 D=2", _run(native, dev, sd, x, hx, 2), ref, err32)
    sd, x, hx, ref, err32 = _case(1, 2, 2048, 2, True)  # the widest layer accepted: 256 slices per direction
    assert native.rnn_layer_route(1, 2, 2048, 2) == 1
    _check("H=2048 B=1 T=2 D=2", _run(native, dev, sd, x, hx, 2), ref, err32)


def test_same_bits_twice_and_on_two_streams(backend):
    nat, dev = backend
    sd, x, hx, _, _ = _case(3, 9, 130, 2, True)
    a, b = _run(nat, dev, sd, x, hx, 2), _run(nat, dev, sd, x, hx, 2)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.equal(p, q) for p, q in zip(a, _run(nat, dev, sd, x, hx, 2, route=1)))  # route 0 IS route 1
    if dev.type == "cuda":
        outs = []
        for _ in range(2):
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                outs.append(_run(nat, dev, sd, x, hx, 2))
            s.synchronize()
        for o in outs:
            assert all(torch.equal(p, q) for p, q in zip(a, o))


def test_bad_arguments_are_named(backend):
    nat, dev = backend
    lib = nat.load()
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731

    def rc(B=2, T=3, H=8, D=2, cell=0, route=0, null_out=False, b_hh=True):
        xp, w, bi, bh = z(B if B > 0 else 1, max(T, 1), max(D, 1), 4 * max(H, 1)), z(max(D, 1), 4 * max(H, 1), max(H, 1)), z(2, 4 * max(H, 1)), z(2, 4 * max(H, 1))
        out, hn, cn = z(max(B, 1), max(T, 1), 2 * max(H, 1)), z(2, max(B, 1), max(H, 1)), z(2, max(B, 1), max(H, 1))
        r = lib.sbk_rnn_layer_f32(nat._p(xp), nat._p(w), nat._p(bi), nat._p(bh) if b_hh else None, None, None,
                                  None if null_out else nat._p(out), nat._p(hn), nat._p(cn), B, T, H, D, cell, route, nat._stream(xp))
        return r, lib.sbk_last_error().decode()

    assert rc()[0] == 0
    for kw, name in ((dict(H=0), "H=0"), (dict(H=nat.RNN_MAX_HIDDEN + 1), "H <= 2048"), (dict(D=3), "D=3"), (dict(B=0), "B=0"),
                     (dict(T=0), "T=0"), (dict(cell=1), "cell=1"), (dict(route=2), "route=2"), (dict(null_out=True), "out"),
                     (dict(b_hh=False), "b_hh")):
        r, msg = rc(**kw)
        assert r == -22 and name in msg, (kw, r, msg)
    assert nat.rnn_layer_route(2, 3, 4096, 2) == 0 and nat.rnn_layer_route(2, 3, 8, 3) == 0
    with pytest.raises(nat.SbkError, match="do not agree"):
        nat.rnn_layer(z(2, 3, 2, 32), z(2, 32, 9))
    with pytest.raises(nat.SbkError, match="h0"):
        nat.rnn_layer(z(2, 3, 2, 32), z(2, 32, 8), h0=z(2, 3, 8))


MUTATIONS = {
    "gate order i, f, o, g": dict(gate_order="ifog"),
    "backward direction written in scan order": dict(backward_in_scan_order=True),
    "b_hh dropped": dict(drop_b_hh=True),
    "the two directions' W_hh swapped": dict(swap_w_hh=True),
    "c not carried": dict(carry_c=False),
    "h0 ignored": dict(use_h0=False),
    "[bwd|fwd] concatenation": dict(backward_first=True),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_cases_tell_mistakes_apart(name):
    """CPU only, fp64, on the host restatement (which agrees with torch.nn.LSTM to 1e-12 on these cases): each planted mistake
    moves out, hn or cn of at least one committed case by more than 1e3 x that case's bound."""
    worst = 0.0
    cases = [(B, T, H, 2, True) for H in HS for B in BS for T in TS] + [LONG + (True,)]
    for B, T, H, D, state in cases:
        sd, x, hx, ref, err32 = _case(B, T, H, D, state)
        w = [t.double() for t in R.lstm_weights(sd, "", 0, D)]
        args = (x.double(), *w, hx[0].double(), hx[1].double())
        good = R.lstm_layer(*args)
        assert max(float((a - b).abs().max()) for a, b in zip(good, ref)) <= 1e-12
        moved = R.lstm_layer(*args, **MUTATIONS[name])
        worst = max(worst, max(float((a - b).abs().max()) for a, b in zip(moved, ref)) / _bound(err32))
    print(f"mutation '{name}': moves the result by {worst:.3e} x the bound")
    assert worst > 1e3
