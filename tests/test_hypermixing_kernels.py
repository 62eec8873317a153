"""csrc/hypermix.hip -- sbk_hypermix_f32 (native.hypermix) -- against the fp64 restatement of HyperMixing
(tests/hypermixing_host_ref.py), on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_wav2vec2_kernels.py): max(4 x the fp32 torch composition's own error against fp64 on the
same inputs, 1e-5).  The measured ratio kernel error / fp32-composition error is printed per case."""
import pytest
import torch

import hypermixing_host_ref as R
from speechbrain_amd import native

B = 3
SPLIT = native.HYPERMIX_SPLIT_FRAMES  # frames of one piece of the time reduction: T = SPLIT + 1 is the first T that splits
# (H, Dh, k): a small one, the two recipe shapes (8M, 22M), the limits
SHAPES = {"small": (2, 8, 16), "8M": (8, 18, 72), "22M": (8, 32, 128), "limits": (1, 64, 256)}
TS = [1, 2, 31, 32, 33, 97, 130, SPLIT, SPLIT + 1, SPLIT + 2]
# A second family of inputs on the 8M shape, "tail": the same kind of tensors with an offset (h of mean 1.5, generator biases
# centred at -3 / -2 and at +2 / -1), so that the pre-activations of both GELUs sit on the negative tail, x = -2 ... -4.  The
# erf and tanh forms of GELU differ by at most 4.7e-4 ANYWHERE, which on inputs centred at zero is lost next to results of order
# 1 (test_cases_tell_mistakes_apart); on the tail the results are small and the two forms differ by 10 ... 45 % of them, and
# the LayerNorm behind the mixer removes the scale.  The kernels are held to the same bound there.
TAIL_CASES = [("8M", 2), ("8M", 31), ("8M", SPLIT + 1)]
_CASES = {}


def _bound(err32):
    return max(4.0 * err32, 1e-5)


def _inputs(shape, T, seed=0, tail=False):
    """Inputs of order 1, generator biases of both signs, a non-trivial LayerNorm affine, a residual (fp32, CPU)."""
    H, Dh, k = SHAPES[shape]
    d = H * Dh
    gen = torch.Generator().manual_seed(1000 * T + d + seed + (7 if tail else 0))
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    if tail:
        h = 1.5 + 0.6 * rn(B, T, d)
        gens = tuple((rn(H, Dh, Dh) / Dh ** 0.5, b1 + 0.5 * rn(H, Dh), 0.2 * rn(H, k, Dh) / Dh ** 0.5, b2 + 0.2 * rn(H, k))
                     for b1, b2 in ((-3.0, -2.0), (2.0, -1.0)))
    else:
        h = rn(B, T, d)
        gens = tuple((rn(H, Dh, Dh) / Dh ** 0.5, 0.5 * rn(H, Dh), rn(H, k, Dh) / Dh ** 0.5, 0.5 * rn(H, k)) for _ in range(2))
    return dict(h=h, pe=R.sine_table(T, d, torch.float32), w1=gens[0], w2=gens[1], ln_w=1.0 + 0.3 * rn(d), ln_b=0.3 * rn(d),
                res=rn(B, T, d), H=H)


def _key_len(T, ragged):
    return torch.tensor([T, 1, max(1, 2 * T // 3)], dtype=torch.int32) if ragged else None


def _host(x, key_len, dtype, **kw):
    c = lambda t: R.cast(t, dtype)  # noqa: E731
    return R.hypermix(c(x["h"]), key_len, c(x["pe"]), c(x["w1"]), c(x["w2"]), c(x["ln_w"]), c(x["ln_b"]), 1e-5, x["H"],
                      residual=c(x["res"]), **kw)


def _case(shape, T, ragged, tail=False):
    """Inputs, the fp64 reference and the fp32 composition's error: computed once per case, never modified."""
    key = (shape, T, ragged, tail)
    if key not in _CASES:
        x, kl = _inputs(shape, T, tail=tail), _key_len(T, ragged)
        ref = _host(x, kl, torch.float64)
        err32 = float((_host(x, kl, torch.float32).double() - ref).abs().max())
        _CASES[key] = (x, kl, ref, err32)
    return _CASES[key]


def _run(nat, dev, x, key_len, h=None, residual="res", out=None):
    t = lambda v: None if v is None else v.to(dev)  # noqa: E731
    res = t(x["res"]) if isinstance(residual, str) else residual
    return nat.hypermix(t(x["h"] if h is None else h), t(key_len), t(x["pe"]), [t(v) for v in x["w1"]],
                        [t(v) for v in x["w2"]], t(x["ln_w"]), t(x["ln_b"]), 1e-5, x["H"], residual=res, out=out)


def test_split_constant_is_the_librarys(backend):
    nat, _ = backend
    assert nat.hypermix_split_frames() == SPLIT


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_vs_fp64_restatement(backend, shape, T, ragged):
    nat, dev = backend
    x, kl, ref, err32 = _case(shape, T, ragged)
    y = _run(nat, dev, x, kl)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"hypermix {shape} T={T} {'ragged' if ragged else 'full'}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}, "
          f"ratio {err / max(err32, 1e-30):.2f}")
    assert err <= _bound(err32)


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("shape,T", TAIL_CASES)
def test_vs_fp64_restatement_on_the_gelu_tail(backend, shape, T, ragged):
    nat, dev = backend
    x, kl, ref, err32 = _case(shape, T, ragged, tail=True)
    y = _run(nat, dev, x, kl)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"hypermix tail {shape} T={T} {'ragged' if ragged else 'full'}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}, "
          f"ratio {err / max(err32, 1e-30):.2f}")
    assert err <= _bound(err32)


@pytest.mark.parametrize("shape,T", [("8M", 33), ("22M", SPLIT + 1)])
def test_key_len_zero(backend, shape, T):
    """An utterance without a valid frame: A = GELU(0) = 0, y = 0, LayerNorm(0) = beta -- its rows are beta + residual to the
    last bit; the other utterances stay within the bound."""
    nat, dev = backend
    x = _inputs(shape, T, seed=1)
    kl = torch.tensor([T, 0, max(1, T // 2)], dtype=torch.int32)
    ref = _host(x, kl, torch.float64)
    err32 = float((_host(x, kl, torch.float32).double() - ref).abs().max())
    y = _run(nat, dev, x, kl).cpu()
    assert torch.equal(y[1], x["ln_b"][None, :] + x["res"][1])
    err = float((y.double() - ref).abs().max())
    print(f"hypermix key_len 0 {shape} T={T}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}")
    assert err <= _bound(err32)


@pytest.mark.parametrize("shape,T", [("small", 33), ("8M", 130), ("22M", SPLIT + 2)])
def test_padded_content_is_dead(backend, shape, T):
    nat, dev = backend
    x, kl, _, _ = _case(shape, T, True)
    y = _run(nat, dev, x, kl).cpu()
    h2 = x["h"].clone()
    for b in range(B):
        h2[b, int(kl[b]):] = 7.0 - 3.0 * torch.randn(T - int(kl[b]), h2.shape[-1], generator=torch.Generator().manual_seed(b))
    assert not torch.equal(h2, x["h"])
    assert torch.equal(_run(nat, dev, x, kl, h=h2).cpu(), y)


@pytest.mark.parametrize("shape,T", [("8M", 97), ("22M", SPLIT + 1)])
def test_determinism_and_aliasing(backend, shape, T):
    """Two runs are bit-identical; ``out`` may be the residual itself (each element is read, then written, by one thread) and
    gives the same bits; ``out`` that is ``h`` is refused."""
    nat, dev = backend
    x, kl, _, _ = _case(shape, T, True)
    y1, y2 = _run(nat, dev, x, kl), _run(nat, dev, x, kl)
    assert torch.equal(y1, y2)
    res = x["res"].to(dev).clone()
    y3 = _run(nat, dev, x, kl, residual=res, out=res)
    assert y3.data_ptr() == res.data_ptr() and torch.equal(y3, y1)
    out = torch.empty_like(y1)
    assert _run(nat, dev, x, kl, out=out).data_ptr() == out.data_ptr() and torch.equal(out, y1)
    h = x["h"].to(dev).clone()
    with pytest.raises(nat.SbkError, match="alias"):
        nat.hypermix(h, None, x["pe"].to(dev), [v.to(dev) for v in x["w1"]], [v.to(dev) for v in x["w2"]], x["ln_w"].to(dev),
                     x["ln_b"].to(dev), 1e-5, x["H"], out=h)


@pytest.mark.parametrize("shape", ["8M", "22M"])
def test_batch_invariance(backend, shape):
    """An utterance alone at T = key_len (two pieces of the time axis) and the same utterance padded inside a longer batch
    (three pieces): its valid rows agree within the bound.  They are in fact equal: the pieces are cut at fixed frame positions,
    so the utterance's own partial sums are the same in both calls and the pieces past its length add exact zeros."""
    nat, dev = backend
    T = 2 * SPLIT + 40
    x, kl, ref, err32 = _case(shape, T, True)
    n = int(kl[2])
    alone = {**x, "h": x["h"][2:3, :n].contiguous(), "res": x["res"][2:3, :n].contiguous(), "pe": x["pe"][:n].contiguous()}
    t = lambda v: v.to(dev)  # noqa: E731
    ya = nat.hypermix(t(alone["h"]), None, t(alone["pe"]), [t(v) for v in x["w1"]], [t(v) for v in x["w2"]], t(x["ln_w"]),
                      t(x["ln_b"]), 1e-5, x["H"], residual=t(alone["res"])).cpu()
    yb = _run(nat, dev, x, kl).cpu()
    bound = _bound(err32)
    da, db = float((ya[0].double() - ref[2, :n]).abs().max()), float((yb[2, :n].double() - ref[2, :n]).abs().max())
    print(f"hypermix batch invariance {shape}: alone {da:.3e}, in batch {db:.3e}, between {float((ya[0] - yb[2, :n]).abs().max()):.3e}")
    assert n > SPLIT and da <= bound and db <= bound and float((ya[0] - yb[2, :n]).abs().max()) <= bound
    assert torch.equal(ya[0], yb[2, :n])


MUTATIONS = {
    "no pe": dict(use_pe=False),
    "pe shifted by a frame": "shift",
    "generators swapped": dict(swap_generators=True),
    "W not zeroed on padding": dict(mask_weights=False),
    "heads as [Dh, H]": dict(heads_last=True),
    "tanh GELU": dict(act=R.gelu_tanh),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_cases_tell_mistakes_apart(name):
    """CPU only, fp64: each planted mistake moves the result by more than 1e3 x the bound on at least one committed case (the
    ragged cases of the two accuracy tests above).  On the zero-centred family alone tanh-GELU reaches 7.3e2 x at most; the
    "tail" family is what tells it apart (the figures are printed)."""
    worst = 0.0
    for shape, T, tail in [(s, t, False) for s in SHAPES for t in TS] + [(s, t, True) for s, t in TAIL_CASES]:
        x, kl, ref, err32 = _case(shape, T, True, tail)
        mut = MUTATIONS[name]
        if mut == "shift":
            moved = _host({**x, "pe": R.sine_table(T, x["h"].shape[-1], torch.float32, shift=1)}, kl, torch.float64)
        else:
            moved = _host(x, kl, torch.float64, **mut)
        worst = max(worst, float((moved - ref).abs().max()) / _bound(err32))
    print(f"mutation '{name}': moves the result by {worst:.3e} x the bound")
    assert worst > 1e3


def test_refusals_name_the_limit(backend):
    nat, dev = backend
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731

    def call(H, Dh, k, T=4, d=None):
        d = H * Dh if d is None else d
        g = [z(H, Dh, Dh), z(H, Dh), z(H, k, Dh), z(H, k)]
        return nat.hypermix(z(1, T, d), None, z(T, d), g, g, z(d), z(d), 1e-5, H)

    with pytest.raises(nat.SbkError, match="Dh <= 64"):
        call(1, 65, 16)
    with pytest.raises(nat.SbkError, match="k <= 256"):
        call(1, 16, 257)
    with pytest.raises(nat.SbkError, match="d % H"):
        call(3, 5, 16, d=16)
    with pytest.raises(nat.SbkError, match="T <= 3000"):
        call(2, 8, 16, T=3001)
