"""csrc/wavlm.hip -- sbk_wavlm_attention_f32, attention with WavLM's gated relative-position bias fused in -- against the fp64
torch composition that materialises the [B,H,T,T] bias (tests/wavlm_host_ref.py), on the CPU emulator of the kernel sources (not
gpu) and on the MI355X (-m gpu); and native.wavlm_relative_buckets / wavlm_bias_table against the buckets the reference recorded.

Bound (the project's rule, tests/test_wav2vec2_kernels.py): max(4 x the fp32 torch composition's own error against fp64 on the
same inputs, 1e-5).  The measured ratio kernel error / fp32-torch error is printed per case."""
import os

import numpy as np
import pytest
import torch

import wavlm_host_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B, H = 3, 3
HEAD_DIMS = (16, 32, 64)
FRAMES = (1, 31, 32, 33, 97, 130)  # 130: a second 128-query workgroup whose only wave holds two queries
_CASES = {}


def _bound(err32):
    return max(4.0 * err32, 1e-5)


def _ragged(T):
    """key_len with 1 and T in it (clamped to T)."""
    return torch.tensor([T, 1, max(1, (2 * T) // 3)], dtype=torch.int32)


def _case(Dh, T, ragged):
    """Inputs, the fp64 reference and the fp32 composition's error: computed once per case, never modified."""
    key = (Dh, T, ragged)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(1000 * Dh + 7 * T + ragged)
        d = H * Dh
        qkv = torch.randn(B, T, H, 3, Dh, generator=gen)
        x = torch.randn(B, T, d, generator=gen)
        gate_w = torch.randn(8, Dh, generator=gen) * (0.6 / Dh ** 0.5)
        gate_b = 0.3 * torch.randn(8, generator=gen)
        gate_const = torch.tensor([1.3, -0.8, 0.4])  # both signs
        # distinct at every offset and in every head, of the scores' size: a shifted or mirrored index moves the output by O(1)
        n = 2 * T - 1
        tab = torch.stack([2.0 * torch.sin(0.37 * torch.arange(n) + 1.1 * h) + 0.011 * torch.arange(n) * (-1.0) ** h
                           for h in range(H)])
        assert len(set(tab.flatten().tolist())) == tab.numel()
        kl = _ragged(T) if ragged else None
        i = torch.arange(T)
        bias = tab[:, (i[None, :] - i[:, None]) + T - 1]  # [H,T,T]: [h, query, key] = tab[h, key - query + T - 1]
        q, k, v = (qkv[:, :, :, j].transpose(1, 2) for j in range(3))
        kl64 = None if kl is None else kl.long()
        scale = Dh ** -0.5
        dd = lambda t: t.double()  # noqa: E731
        ref = R.gated_attention(dd(q), dd(k), dd(v), dd(x), dd(gate_w), dd(gate_b), dd(gate_const), dd(bias), kl64, scale)
        got32 = R.gated_attention(q, k, v, x, gate_w, gate_b, gate_const, bias, kl64, scale)
        err32 = float((got32.double() - ref).abs().max())
        gates = R.gate(x, gate_w, gate_b, gate_const, H)
        _CASES[key] = (qkv.reshape(B, T, 3 * d).contiguous(), x, gate_w, gate_b, gate_const, tab, kl, ref, err32, bias, gates)
    return _CASES[key]


def _run(nat, dev, case, Dh, gate_const=None, tab=None):
    qkv, x, gate_w, gate_b, gc, tb, kl = case[:7]
    gc = gc if gate_const is None else gate_const
    tb = tb if tab is None else tab
    to = lambda t: None if t is None else t.to(dev)  # noqa: E731
    return nat.wavlm_attention(to(qkv), to(x), to(gate_w), to(gate_b), to(gc), to(tb.contiguous()), to(kl), H, Dh ** -0.5).cpu()


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("Dh", HEAD_DIMS)
def test_wavlm_attention_vs_fp64_composition(backend, Dh, T, ragged):
    nat, dev = backend
    case = _case(Dh, T, ragged)
    ref, err32 = case[7], case[8]
    y = _run(nat, dev, case, Dh)
    assert y.shape == ref.shape
    err = float((y.double() - ref).abs().max())
    print(f"wavlm_attention Dh={Dh} T={T} ragged={ragged}: kernel max|d| {err:.3e}, fp32 torch composition {err32:.3e}, "
          f"ratio {err / max(err32, 1e-30):.2f}")
    assert err <= _bound(err32)


def test_the_cases_can_tell_a_wrong_table_and_a_constant_gate():
    """CPU only: what the parametrised test relies on.  Mirroring the table (r -> -r), shifting it by one offset, or replacing
    the gate by a constant each move the fp64 composition by far more than the bound."""
    Dh, T = 32, 33
    qkv, x, gate_w, gate_b, gate_const, tab, kl, ref, err32, bias, gates = _case(Dh, T, True)
    q, k, v = (qkv.view(B, T, H, 3, Dh)[:, :, :, j].transpose(1, 2).double() for j in range(3))
    run = lambda bs, gw, gb: R.gated_attention(q, k, v, x.double(), gw.double(), gb.double(), gate_const.double(),  # noqa: E731
                                               bs.double(), kl.long(), Dh ** -0.5)
    assert float((run(bias.transpose(1, 2), gate_w, gate_b) - ref).abs().max()) > 1e3 * _bound(err32)
    assert float((run(torch.roll(bias, 1, dims=2), gate_w, gate_b) - ref).abs().max()) > 1e3 * _bound(err32)
    assert float((run(bias, torch.zeros_like(gate_w), gate_b) - ref).abs().max()) > 1e3 * _bound(err32)
    assert float(gates.max() - gates.min()) > 0.2


def test_padded_query_rows_are_computed(backend):
    """Queries past key_len[b] attend to the valid keys like any other row (the reference computes them; output_norm averages
    over them): they equal the composition's rows, which are not zero."""
    nat, dev = backend
    Dh, T = 32, 33
    case = _case(Dh, T, True)
    ref = case[7]
    y = _run(nat, dev, case, Dh)
    assert float((y[1, 1:].double() - ref[1, 1:]).abs().max()) <= _bound(case[8])  # key_len[1] = 1: rows 1.. are padding
    assert float(ref[1, 1:].abs().max()) > 1e-2


def test_out_is_a_slice_of_a_poisoned_buffer(backend):
    nat, dev = backend
    Dh, T = 16, 130
    qkv, x, gate_w, gate_b, gate_const, tab, kl, ref, err32 = _case(Dh, T, True)[:9]
    d = H * Dh
    big = torch.full((B * T + 9, d), float("nan"), device=dev)
    out = big[4: 4 + B * T].view(B, T, d)
    to = lambda t: t.to(dev)  # noqa: E731
    nat.wavlm_attention(to(qkv), to(x), to(gate_w), to(gate_b), to(gate_const), to(tab), to(kl), H, Dh ** -0.5, out=out)
    assert float((out.cpu().double() - ref).abs().max()) <= _bound(err32)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())


@pytest.mark.parametrize("setting", ["default", "small"])
def test_bucket_function_equals_the_recorded_buckets(setting):
    """native.wavlm_relative_buckets on every r in [-2000, 2000] against transformers' _relative_positions_bucket as the fixture
    generator recorded it: num_buckets 320 / max distance 800 (the released models) and 32 / 12 (the group fixture)."""
    from speechbrain_amd import native

    g = np.load(os.path.join(GOLD, "wavlm_model.npz"))
    nb, md = (320, 800) if setting == "default" else (32, 12)
    want = torch.from_numpy(g[f"buckets_{nb}_{md}"])
    r = torch.arange(-2000, 2001)
    assert want.shape == r.shape
    assert torch.equal(native.wavlm_relative_buckets(r, nb, md), want)
    assert torch.equal(R.relative_buckets(r, nb, md), want)
    assert int(want.min()) == 0 and int(want.max()) == nb - 1


def test_bias_table_is_the_toeplitz_form_of_compute_bias():
    """tab[h, j - i + T - 1] == compute_bias(T, T)[h, i, j] exactly, and the Derived cache is keyed on the parameter and T."""
    from speechbrain_amd import native

    gen = torch.Generator().manual_seed(5)
    T, nb, md, heads = 40, 32, 12, 3
    embed = torch.nn.Parameter(torch.randn(nb, heads, generator=gen))
    cache = native.Derived()
    tab = native.wavlm_bias_table(embed, T, nb, md, derived=cache)
    assert tab.shape == (heads, 2 * T - 1) and tab.dtype == torch.float32
    i = torch.arange(T)
    assert torch.equal(tab[:, (i[None, :] - i[:, None]) + T - 1], R.position_bias(embed.detach(), T, nb, md))
    assert native.wavlm_bias_table(embed, T, nb, md, derived=cache) is tab
    assert native.wavlm_bias_table(embed, T + 1, nb, md, derived=cache).shape == (heads, 2 * T + 1)
    with torch.no_grad():
        embed.mul_(2.0)
    assert torch.equal(native.wavlm_bias_table(embed, T, nb, md, derived=cache), 2.0 * tab)


def test_refuses_unsupported_shapes(backend):
    import ctypes

    nat, dev = backend
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(NotImplementedError, match=r"wavlm_attention: head dim 40/2"):
        nat.wavlm_attention(z(1, 4, 120), z(1, 4, 40), z(8, 20), z(8), z(2), z(2, 7), None, 2, 1.0)
    lib = nat.load()
    max_t = lib.sbk_wavlm_attention_max_frames()
    assert max_t >= 1499  # 30 s of audio at 20 ms a frame
    T = max_t + 1
    with pytest.raises(nat.SbkError, match=f"wavlm_attention: T={T} frames"):
        nat.wavlm_attention(z(1, T, 48), z(1, T, 16), z(8, 16), z(8), z(1), z(1, 2 * T - 1), None, 1, 1.0)
    # the C entry itself: EINVAL with the instantiated list / the bound, nothing launched
    a = z(1, 4, 120)
    rc = lib.sbk_wavlm_attention_f32(a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), None,
                                     a.data_ptr(), 1, 4, 2, 20, ctypes.c_float(1.0), None)
    assert rc == -22 and "(16,32,64)" in lib.sbk_last_error().decode()
    rc = lib.sbk_wavlm_attention_f32(a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), None,
                                     a.data_ptr(), 1, T, 1, 16, ctypes.c_float(1.0), None)
    assert rc == -22 and f"T <= {max_t}" in lib.sbk_last_error().decode()
