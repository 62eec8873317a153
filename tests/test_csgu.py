"""sbk_csgu_f32 (csrc/csgu.hip: the Convolutional Spatial Gating Unit of the Branchformer cgMLP branch) against the fp64 torch
composition of tests/branchformer_host_ref.py, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound: the fp32 torch composition's own max error against fp64 on the same inputs, times 4 (another, equally legitimate,
summation order in the LayerNorm statistics and over the taps), with a floor of 1e-5 (test_glu_dwconv's bound for the same
tap count).  The measured ratio kernel error / fp32-torch error is printed per shape (DESIGN.md section 5 records them)."""
import pytest
import torch
import torch.nn.functional as F

import branchformer_host_ref as R

# (B, T, C, ksize)
SHAPES = [
    (1, 16, 72, 31),     # T = halo + 1: the reflection spans the whole sequence; C is no multiple of the 64-channel tile
    (2, 50, 32, 31),     # B > 1: the reflection must not cross batch rows
    (1, 70, 200, 31),    # two 64-frame tiles with a ragged last one, four channel tiles with a ragged last one
    (1, 33, 144, 7),
    (1, 9, 16, 3),
    (1, 40, 1536, 31),   # the recipe's channel count (csgu_linear_units 3072)
]
_CASES = {}


def _case(shape):
    """Inputs, the fp64 reference and the fp32 torch composition's error -- computed once per shape, never modified."""
    if shape not in _CASES:
        B, T, C, k = shape
        gen = torch.Generator().manual_seed(1000 * T + C + k)
        h = torch.randn(B, T, 2 * C, generator=gen)
        gamma = 1.0 + 0.1 * torch.randn(C, generator=gen)
        beta = 0.1 * torch.randn(C, generator=gen)
        w = 0.3 * torch.randn(C, k, generator=gen)
        bias = 1.0 + 0.1 * torch.randn(C, generator=gen)
        ref = R.csgu(h.double(), gamma.double(), beta.double(), 1e-5, w.double(), bias.double())
        err32 = float((R.csgu(h, gamma, beta, 1e-5, w, bias).double() - ref).abs().max())
        _CASES[shape] = (h, gamma, beta, w, bias, ref, err32)
    return _CASES[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_csgu_vs_fp64_composition(backend, shape):
    nat, dev = backend
    h, gamma, beta, w, bias, ref, err32 = _case(shape)
    y = nat.csgu(h.to(dev), gamma.to(dev), beta.to(dev), 1e-5, w.to(dev), bias.to(dev), shape[3])
    assert y.shape == ref.shape
    err = float((y.cpu().double() - ref).abs().max())
    print(f"csgu {shape}: kernel max|d| {err:.3e}, fp32 torch composition {err32:.3e}, ratio {err / err32:.2f}")
    assert err <= max(4.0 * err32, 1e-5)


@pytest.mark.parametrize("act,fn", [(1, F.silu), (2, F.gelu), (3, F.relu)])
def test_csgu_gate_activations(backend, act, fn):
    """The gate activations the kernel applies on the way out (Identity is the recipes'; Swish, GELU and ReLU share the act
    codes of the GEMM epilogues), same bound."""
    nat, dev = backend
    h, gamma, beta, w, bias, _, _ = _case(SHAPES[3])
    ref = R.csgu(h.double(), gamma.double(), beta.double(), 1e-5, w.double(), bias.double(), fn)
    err32 = float((R.csgu(h, gamma, beta, 1e-5, w, bias, fn).double() - ref).abs().max())
    y = nat.csgu(h.to(dev), gamma.to(dev), beta.to(dev), 1e-5, w.to(dev), bias.to(dev), SHAPES[3][3], gate_act=act)
    assert float((y.cpu().double() - ref).abs().max()) <= max(4.0 * err32, 1e-5)


def test_csgu_out_argument_and_views(backend):
    """``out=`` writes into the caller's rows (the grouped encoder pass hands the kernel a slice of a larger buffer)."""
    nat, dev = backend
    h, gamma, beta, w, bias, ref, err32 = _case(SHAPES[1])
    B, T, C, k = SHAPES[1]
    big = torch.full((B * T + 7, C), 7.0, device=dev)
    hh = torch.cat([torch.zeros(5, 2 * C), h.reshape(B * T, 2 * C)]).to(dev)
    nat.csgu(hh[5:].view(B, T, 2 * C), gamma.to(dev), beta.to(dev), 1e-5, w.to(dev), bias.to(dev), k, out=big[3: 3 + B * T].view(B, T, C))
    assert float((big[3: 3 + B * T].cpu().double().view(B, T, C) - ref).abs().max()) <= max(4.0 * err32, 1e-5)
    assert bool((big[:3] == 7.0).all()) and bool((big[3 + B * T:] == 7.0).all())  # nothing outside the slice is touched


def test_csgu_delta_filter_is_normalise_times_gate(backend):
    """gamma = 1, beta = 0, w = a delta at the centre tap, bias = 0: the output is EXACTLY normalise(x2) * x1 -- an off-by-one
    in the tap orientation, or the two halves swapped, changes it."""
    nat, dev = backend
    B, T, C, k = 2, 37, 72, 7
    gen = torch.Generator().manual_seed(5)
    h = torch.randn(B, T, 2 * C, generator=gen)
    w = torch.zeros(C, k)
    w[:, (k - 1) // 2] = 1.0
    y = nat.csgu(h.to(dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), 1e-5, w.to(dev), torch.zeros(C, device=dev), k).cpu()
    x1, x2 = h.double().chunk(2, dim=-1)
    want = F.layer_norm(x2, (C,), None, None, 1e-5) * x1
    x1f, x2f = h.chunk(2, dim=-1)
    tol = max(4.0 * float(((F.layer_norm(x2f, (C,), None, None, 1e-5) * x1f).double() - want).abs().max()), 1e-5)
    assert float((y.double() - want).abs().max()) <= tol  # (fp32 statistics against fp64: rounding only)
    swapped = F.layer_norm(x1, (C,), None, None, 1e-5) * x2
    assert float((y.double() - swapped).abs().max()) > 0.1
    # exactness: the same statistics pass applied without a filter -- a delta filter adds nothing but zeros to it
    w3 = torch.zeros(C, 3)
    w3[:, 1] = 1.0
    y3 = nat.csgu(h.to(dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), 1e-5, w3.to(dev), torch.zeros(C, device=dev), 3).cpu()
    assert torch.equal(y, y3)
    # one tap to the right of the centre reads frame t + 1 (torch conv1d is a cross-correlation), mirrored at the end
    w[:] = 0.0
    w[:, (k - 1) // 2 + 1] = 1.0
    ys = nat.csgu(h.to(dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), 1e-5, w.to(dev), torch.zeros(C, device=dev), k).cpu()
    n = F.layer_norm(x2, (C,), None, None, 1e-5)
    shifted = torch.cat([n[:, 1:], n[:, T - 2: T - 1]], dim=1) * x1
    assert float((ys.double() - shifted).abs().max()) <= tol


def test_csgu_refuses_what_the_reference_refuses(backend):
    nat, dev = backend
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    # T = halo: F.pad(mode="reflect") raises in the reference; both numbers are in the message
    with pytest.raises(nat.SbkError, match=r"T=15\b.*\b15\b.*ksize=31"):
        nat.csgu(z(1, 15, 16), z(8), z(8), 1e-5, z(8, 31), z(8), 31)
    with pytest.raises(nat.SbkError, match=r"T=3\b.*\b3\b.*ksize=7"):
        nat.csgu(z(2, 3, 16), z(8), z(8), 1e-5, z(8, 7), z(8), 7)
    nat.csgu(z(1, 4, 16), z(8), z(8), 1e-5, z(8, 7), z(8), 7)  # T = halo + 1 is legal
    with pytest.raises(nat.SbkError, match=r"kernel size 9 .*3, 5, 7, 15, 31"):
        nat.csgu(z(1, 20, 16), z(8), z(8), 1e-5, z(8, 9), z(8), 9)
    # the C entry point itself (a caller that does not come through the binding): SBK_EINVAL and the same words
    lib = nat.load()
    h, v, w, y, st = z(1, 15, 16), z(8), z(8, 31), z(1, 15, 8), z(30)
    p = lambda t: t.data_ptr()  # noqa: E731
    import ctypes

    args = lambda T, k: (p(h), p(v), p(v), ctypes.c_float(1e-5), p(w), p(v), p(y), p(st), 1, T, 8, k, 0, None)  # noqa: E731
    assert lib.sbk_csgu_f32(*args(15, 31)) == -22
    msg = lib.sbk_last_error().decode()
    assert "T=15" in msg and "ksize=31" in msg
    assert lib.sbk_csgu_f32(*args(15, 9)) == -22
    assert "(3,5,7,15,31)" in lib.sbk_last_error().decode()
    assert lib.sbk_csgu_f32(p(h), p(v), p(v), ctypes.c_float(1e-5), p(w), p(v), p(y), p(st), 1, 15, 8, 7, 9, None) == -22
    assert "gate activation" in lib.sbk_last_error().decode()
