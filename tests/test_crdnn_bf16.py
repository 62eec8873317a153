"""CRDNN under precision "bf16": sbk_rnn_layer_bf16 (csrc/rnn_bf16.hip, native.rnn_layer under precision_scope("bf16")) against a
plain fp64 LSTM layer, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu), and the model through
EncoderASR.from_hparams(..., run_opts={"precision": "bf16"}).

Bound (the project's bf16 rule, tests/test_ssl_bf16.py): 2 * e_model + 1e-3, e_model = the max error, against the fp64 layer, of
the same fp64 recurrence with the kernel's two roundings made explicit: W_hh to bf16, and h_{t-1} to bf16 before the product only.
Every case prints ratio = kernel error / e_model: 1.00 in every case with a product, on the MI355X and on the emulator (a single
step from a zero state has no product: e_model 0, kernel error 1e-7)."""
import os

import crdnn_host_ref as R
import pytest
import torch

CRDNN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrained_crdnn_ctc_tiny")
_CASES = {}


def _r(t):  # round to bf16 (nearest even) from fp32, as the kernel does; carried on in fp64
    return t.float().bfloat16().double()


def _lstm(xp, w_hh, b_ih, b_hh, h0, c0, rnd=lambda t: t):
    """torch.nn.LSTM semantics in fp64 on the input projection xp [B,T,D,4H]; ``rnd`` is applied to W_hh and to h_{t-1} as
    operands of their product, and to nothing else."""
    (B, T, D, G), H = xp.shape, xp.shape[3] // 4
    out, hn, cn = xp.new_zeros(B, T, D * H), [], []
    for d in range(D):
        h = h0[d] if h0 is not None else xp.new_zeros(B, H)
        c = c0[d] if c0 is not None else xp.new_zeros(B, H)
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            g = xp[:, t, d] + b_ih[d] + b_hh[d] + rnd(h) @ rnd(w_hh[d]).T
            i, f, gg, o = g.reshape(B, 4, H).unbind(1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[:, t, d * H:(d + 1) * H] = h
        hn.append(h), cn.append(c)
    return out, torch.stack(hn), torch.stack(cn)


def _case(H, B, D, T, state):
    """fp32 inputs, the fp64 reference and e_model: once per case, never modified."""
    key = (H, B, D, T, state)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(H * 10007 + B * 101 + D * 11 + T + (5 if state else 0))
        u = lambda *s: (2.0 * torch.rand(*s, generator=gen) - 1.0) / H ** 0.5  # noqa: E731  (torch's own init)
        args = [torch.randn(B, T, D, 4 * H, generator=gen), u(D, 4 * H, H), u(D, 4 * H), u(D, 4 * H)]
        args += [torch.randn(D, B, H, generator=gen), torch.randn(D, B, H, generator=gen)] if state else [None, None]
        a64 = [None if t is None else t.double() for t in args]
        ref = _lstm(*a64)
        e_model = max(float((m - r).abs().max()) for m, r in zip(_lstm(*a64, rnd=_r), ref))
        _CASES[key] = (args, ref, e_model)
    return _CASES[key]


def _run(nat, dev, args, precision="bf16"):
    nat.prof_reset(), nat.prof_enable(True)
    with nat.precision_scope(precision):
        got = nat.rnn_layer(*(None if t is None else t.to(dev) for t in args))
    nat.prof_enable(False)
    assert set(nat.prof_report()) == {"rnn_lstm_steps_bf16" if precision == "bf16" else "rnn_lstm_steps"}
    return got


@pytest.mark.parametrize("state", [False, True], ids=["zeros", "h0c0"])
@pytest.mark.parametrize("T", (1, 40))
@pytest.mark.parametrize("D", (1, 2))
@pytest.mark.parametrize("B", (1, 33))
@pytest.mark.parametrize("H", (8, 13, 136))
def test_rnn_layer_bf16_vs_fp64(backend, H, B, D, T, state):
    nat, dev = backend
    args, ref, e_model = _case(H, B, D, T, state)
    got = [g.cpu() for g in _run(nat, dev, args)]
    errs = [float((g.double() - r).abs().max()) for g, r in zip(got, ref)]
    print(f"rnn_layer_bf16 H={H} B={B} D={D} T={T} state={state}: max|d| out {errs[0]:.3e} hn {errs[1]:.3e} cn {errs[2]:.3e}, "
          f"e_model {e_model:.3e}, ratio {max(errs) / e_model if e_model else float('nan'):.2f}")
    assert all(g.shape == r.shape for g, r in zip(got, ref)) and max(errs) <= 2.0 * e_model + 1e-3
    out, _, cn = got
    assert bool((out.bfloat16().float() != out).any()) and bool((cn.bfloat16().float() != cn).any())  # the state is kept in fp32
    if H == 136 and (T > 1 or state):  # the path is really taken (one step from a zero state has no product to round)
        assert not torch.equal(out, _run(nat, dev, args, "fp32")[0].cpu())


def test_same_bits_twice_and_on_two_streams(backend):
    nat, dev = backend
    args = _case(136, 33, 2, 40, True)[0]
    a = _run(nat, dev, args)
    assert all(torch.equal(p, q) for p, q in zip(a, _run(nat, dev, args)))
    if dev.type == "cuda":
        for _ in range(2):
            with torch.cuda.stream(torch.cuda.Stream(dev)):
                o = _run(nat, dev, args)
            torch.cuda.synchronize()
            assert all(torch.equal(p, q) for p, q in zip(a, o))


@pytest.mark.parametrize("what,name", [("image", "was not made for H=136"), ("workspace", "too small"), ("H2049", "H <= 2048")])
def test_refusals_are_named(backend, what, name):
    nat, dev = backend
    lib, (B, T, D, H) = nat.load(), (2, 3, 2, 136)
    Hc = 2049 if what == "H2049" else H
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    img = nat.rnn_whh_bf16_image(z(D, 4 * 8, 8) if what == "image" else z(D, 4 * H, H))
    nbytes = lib.sbk_rnn_layer_bf16_workspace_bytes(B, H, D)
    assert nbytes > 0 and lib.sbk_rnn_layer_bf16_workspace_bytes(B, 2049, D) == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    xp, out, hn, cn = z(B, T, D, 4 * H), z(B, T, D * H), z(D, B, H), z(D, B, H)
    rc = lib.sbk_rnn_layer_bf16(nat._p(xp), nat._p(img), img.numel() * 2, None, None, None, None, nat._p(out), nat._p(hn), nat._p(cn),
                                nat._p(ws), nbytes - (1 if what == "workspace" else 0), B, T, Hc, D, nat.RNN_LSTM, nat._stream(xp))
    assert rc == -22 and name in lib.sbk_last_error().decode(), lib.sbk_last_error().decode()


def test_encoder_asr_crdnn_under_precision_bf16(backend):
    """The tiny CRDNN + CTC directory through EncoderASR.from_hparams.  Relative RMS error of the CTC log-probabilities against
    the fp64 host restatement (tests/crdnn_host_ref.py on the interface's own fp32 features): under "bf16" at most 2 x that of the
    fp32 restatement under torch.autocast("cpu", bfloat16) -- the reference's own bf16; the factor leaves room for a different
    placement of the roundings.  Measured: bf16 1.889e-4 on the MI355X and 1.888e-4 on the emulator, autocast 6.975e-4.  The
    bf16 output differs from the fp32 one, and "fp32" through the same interface is run_opts={} bit for bit."""
    import numpy as np
    from speechbrain_amd.inference.ASR import EncoderASR

    nat, dev = backend
    exp = np.load(os.path.join(os.path.dirname(CRDNN_DIR), "pretrained_crdnn_ctc_tiny_expected.npz"))
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    logp = {}
    for prec in (None, "fp32", "bf16"):
        opts = {"device": str(dev)} if prec is None else {"device": str(dev), "precision": prec}
        asr = EncoderASR.from_hparams(source=CRDNN_DIR, run_opts=opts)
        nat.prof_reset(), nat.prof_enable(True)
        logp[prec] = asr.encode_batch(wav, lens).cpu()
        nat.prof_enable(False)
        assert ("rnn_lstm_steps_bf16" in nat.prof_report()) == (prec == "bf16")
    assert torch.equal(logp["fp32"], logp[None]) and not torch.equal(logp["bf16"], logp["fp32"])
    enc = asr.mods.encoder
    with torch.no_grad():
        feats = enc["normalize"](enc["compute_features"](wav.to(dev)), lengths=lens.to(dev)).cpu()
    sd = {k: v.detach().cpu() for k, v in enc["enc"].state_dict().items()}
    w, b = enc["ctc_lin"].w.weight.detach().cpu(), enc["ctc_lin"].w.bias.detach().cpu()

    def host(dtype):
        x, _ = R.crdnn(feats.to(dtype), R.cast_dict(sd, dtype), (2, 2), 4, 2, True, 2)
        return torch.log_softmax(x @ w.to(dtype).T + b.to(dtype), dim=-1).double()

    ref = host(torch.float64)
    rms = lambda y: float(((y.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())  # noqa: E731
    with torch.autocast("cpu", dtype=torch.bfloat16):
        e_autocast = rms(host(torch.float32))
    e_bf16 = rms(logp["bf16"])
    print(f"crdnn EncoderASR: relative RMS error vs fp64: bf16 {e_bf16:.3e}, fp32 restatement under autocast(bf16) {e_autocast:.3e}, "
          f"fp32 path {rms(logp['fp32']):.3e}")
    assert e_bf16 <= 2.0 * e_autocast
