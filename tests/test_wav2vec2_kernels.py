"""csrc/wav2vec2.hip -- sbk_w2v_conv0_f32 with its statistics launch, and sbk_w2v_posconv_f32 -- against their fp64 torch
compositions (tests/wav2vec2_host_ref.py), on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_csgu.py): max(4 x the fp32 torch composition's own error against fp64 on the same inputs,
1e-5).  The measured ratio kernel error / fp32-torch error is printed per case."""
import pytest
import torch
import torch.nn.functional as F

import wav2vec2_host_ref as R

# name -> (B, N, C0, k, s)
CONV0 = {
    "t1": (1, 10, 32, 10, 5),            # T0 = 1
    "n14": (1, 14, 40, 10, 5),           # T0 = 1 with samples no window reads; C0 no multiple of 16
    "ragged": (1, 4005, 512, 10, 5),     # T0 = 800: 25 tiles of 32 frames; the real channel count (two channels per thread)
    "long": (1, 160000, 32, 10, 5),      # T0 = 31 999: the statistics length of a 10 s utterance, 14 chunks of partial sums
    "b2": (2, 1203, 48, 10, 5),          # B = 2: the statistics stay per utterance; T0 = 239, a ragged last tile
    "k3s2": (2, 777, 64, 3, 2),          # another kernel / stride (the four-tap instantiation)
}
_C0 = {}
_PC = {}


def _bound(err32):
    return max(4.0 * err32, 1e-5)


def _conv0_inputs(name, dc=0.0):
    B, N, C0, k, s = CONV0[name]
    gen = torch.Generator().manual_seed(N + C0 + k)
    wav = 0.5 * torch.randn(B, N, generator=gen) + dc
    if B > 1:  # a second utterance of another level and offset: statistics that leak between utterances show
        wav[1] = 3.0 * wav[1] + 0.7
        wav[1, int(0.6 * N):] = 0.0  # ... with the zero padding of a shorter utterance (the statistics run over it)
    w = 0.4 * torch.randn(C0, k, generator=gen)
    bias = 0.2 * torch.randn(C0, generator=gen)
    gamma = 1.0 + 0.1 * torch.randn(C0, generator=gen)
    beta = 0.1 * torch.randn(C0, generator=gen)
    return wav, w, bias, gamma, beta


def _conv0_case(name, mode, normalize, dc=0.0):
    """Inputs, the fp64 reference and the fp32 torch composition's error: computed once per case, never modified."""
    key = (name, mode, normalize, dc)
    if key not in _C0:
        wav, w, bias, gamma, beta = _conv0_inputs(name, dc)
        s = CONV0[name][4]
        b = bias if mode == "layer" else None  # (the "group" variant of the model has no convolution bias)
        dd = lambda t: None if t is None else t.double()  # noqa: E731
        ref = R.conv0(wav.double(), w.double(), dd(b), gamma.double(), beta.double(), s, mode, 1e-5, normalize)
        err32 = float((R.conv0(wav, w, b, gamma, beta, s, mode, 1e-5, normalize).double() - ref).abs().max())
        _C0[key] = (wav, w, b, gamma, beta, ref, err32)
    return _C0[key]


def _run_conv0(nat, dev, case, name, mode, normalize):
    wav, w, b, gamma, beta, ref, err32 = case
    m = nat.W2V_GROUP_NORM if mode == "group" else nat.W2V_LAYER_NORM
    y = nat.w2v_conv0(wav.to(dev), w.to(dev), None if b is None else b.to(dev), gamma.to(dev), beta.to(dev), CONV0[name][4], m,
                      eps=1e-5, normalize=normalize)
    assert y.shape == ref.shape
    return float((y.cpu().double() - ref).abs().max())


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normwav"])
@pytest.mark.parametrize("mode", ["group", "layer"])
@pytest.mark.parametrize("name", list(CONV0))
def test_conv0_vs_fp64_composition(backend, name, mode, normalize):
    nat, dev = backend
    case = _conv0_case(name, mode, normalize)
    err, err32 = _run_conv0(nat, dev, case, name, mode, normalize), case[-1]
    print(f"w2v_conv0 {name} {mode} normalize={normalize}: kernel max|d| {err:.3e}, fp32 torch composition {err32:.3e}, "
          f"ratio {err / max(err32, 1e-30):.2f}")
    assert err <= _bound(err32)


def _naive_group_error(wav, w, gamma, beta, s, ref):
    """GroupNorm with the one-pass variance E[y^2] - E[y]^2 in fp32: what the statistics launch must NOT do."""
    y = F.conv1d(wav[:, None], w[:, None], None, stride=s)
    mean = y.mean(dim=2, keepdim=True)
    var = (y * y).mean(dim=2, keepdim=True) - mean * mean
    out = F.gelu((y - mean) * torch.rsqrt(var + 1e-5) * gamma[None, :, None] + beta[None, :, None]).transpose(1, 2)
    return float((out.double() - ref).abs().max())


def test_conv0_dc_offset_fp32_composition_holds_and_naive_variance_loses():
    """CPU only.  A +3.0 DC offset on the waveform, normalisation off, T0 = 31 999: torch's own fp32 GroupNorm stays within the
    bound's floor-free part (its error does not blow up: below 1e-4, where a centred fp32 variance of O(1) values lands), while
    the one-pass variance loses digits to the offset and misses the bound the kernel is held to."""
    wav, w, b, gamma, beta, ref, err32 = _conv0_case("long", "group", False, dc=3.0)
    naive = _naive_group_error(wav, w, gamma, beta, CONV0["long"][4], ref)
    print(f"dc offset: fp32 torch composition {err32:.3e}, naive E[y^2]-E[y]^2 {naive:.3e}, bound {_bound(err32):.3e}")
    assert err32 <= _bound(err32) and err32 < 1e-4
    assert naive > _bound(err32)


def test_conv0_dc_offset_statistics(backend):
    """The same case through the kernel: the window covariance is centred before it is accumulated, so the offset costs nothing."""
    nat, dev = backend
    case = _conv0_case("long", "group", False, dc=3.0)
    err, err32 = _run_conv0(nat, dev, case, "long", "group", False), case[-1]
    print(f"w2v_conv0 dc offset: kernel max|d| {err:.3e}, fp32 torch composition {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    assert err <= _bound(err32)


def test_conv0_refuses_unsupported_shapes(backend):
    nat, dev = backend
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(nat.SbkError, match="kernel 17"):
        nat.w2v_conv0(z(1, 100), z(8, 17), None, z(8), z(8), 5, nat.W2V_LAYER_NORM)
    with pytest.raises(nat.SbkError, match="stride 4"):
        nat.w2v_conv0(z(1, 100), z(8, 3), None, z(8), z(8), 4, nat.W2V_LAYER_NORM)
    with pytest.raises(nat.SbkError, match="N=9 samples"):
        nat.w2v_conv0(z(1, 9), z(8, 10), None, z(8), z(8), 5, nat.W2V_GROUP_NORM)
    with pytest.raises(nat.SbkError, match="C0=1025"):
        nat.w2v_conv0(z(1, 100), z(1025, 10), None, z(1025), z(1025), 5, nat.W2V_LAYER_NORM)


# ---------------------------------------------------------------------------------------------- positional convolution
# name -> (d, G, k, B, T, key_len)
POSCONV = {
    "base_t1": (768, 16, 128, 1, 1, None),        # T <= k/2: every output reads padding on both sides
    "base_t64": (768, 16, 128, 1, 64, None),      # exactly one 64-frame tile
    "base_t65": (768, 16, 128, 1, 65, None),      # a second tile with one live frame
    "base_t70": (768, 16, 128, 1, 70, None),
    "large_lens": (1024, 16, 128, 3, 70, (70, 33, 1)),  # cg 64; masked frames, the halo of one utterance next to another's
    "cg48_k32": (96, 2, 32, 2, 40, (40, 25)),     # the group-norm fixture model's shape
    "cg64_k16": (128, 2, 16, 2, 19, (19, 7)),     # the layer-norm fixture model's shape
    "cg16_k15": (32, 2, 15, 2, 23, None),         # odd k: no frame is dropped; the narrowest group
}


def _posconv_case(name, ln):
    key = (name, ln)
    if key not in _PC:
        d, G, k, B, T, lens = POSCONV[name]
        cg = d // G
        gen = torch.Generator().manual_seed(d + k + T)
        x = torch.randn(B, T, d, generator=gen)
        w = torch.randn(d, cg, k, generator=gen) * (2.0 / (cg * k) ** 0.5)
        bias = 0.2 * torch.randn(d, generator=gen)
        gamma = 1.0 + 0.1 * torch.randn(d, generator=gen)
        beta = 0.1 * torch.randn(d, generator=gen)
        kl = None if lens is None else torch.tensor(lens, dtype=torch.int32)
        ln64 = (gamma.double(), beta.double(), 1e-5) if ln else None
        ln32 = (gamma, beta, 1e-5) if ln else None
        kl64 = None if kl is None else kl.long()
        ref = R.posconv(x.double(), kl64, w.double(), bias.double(), G, ln64)
        err32 = float((R.posconv(x, kl64, w, bias, G, ln32).double() - ref).abs().max())
        _PC[key] = (x, kl, w, bias, gamma, beta, ref, err32)
    return _PC[key]


def _tap_major(w):
    """[d, cg, k] -> [d, k * cg]: what the kernel reads (the wrapper derives it once per weight)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("name", list(POSCONV))
def test_posconv_vs_fp64_composition(backend, name, ln):
    nat, dev = backend
    x, kl, w, bias, gamma, beta, ref, err32 = _posconv_case(name, ln)
    d, G, k = POSCONV[name][:3]
    xd = x.to(dev)
    y = nat.w2v_posconv(xd, None if kl is None else kl.to(dev), _tap_major(w).to(dev), bias.to(dev), G, k,
                        ln=(gamma.to(dev), beta.to(dev), 1e-5) if ln else None)
    assert y.shape == ref.shape
    err = float((y.cpu().double() - ref).abs().max())
    print(f"w2v_posconv {name} ln={ln}: kernel max|d| {err:.3e}, fp32 torch composition {err32:.3e}, ratio {err / err32:.2f}")
    assert err <= _bound(err32)
    assert torch.equal(xd.cpu(), x)  # the mask is applied on read: the caller's x is as it was


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
def test_posconv_out_is_a_slice_of_a_poisoned_buffer(backend, ln):
    nat, dev = backend
    name = "cg48_k32"
    x, kl, w, bias, gamma, beta, ref, err32 = _posconv_case(name, ln)
    d, G, k, B, T, _ = POSCONV[name]
    big = torch.full((B * T + 9, d), float("nan"), device=dev)
    out = big[4: 4 + B * T].view(B, T, d)
    nat.w2v_posconv(x.to(dev), kl.to(dev), _tap_major(w).to(dev), bias.to(dev), G, k,
                    ln=(gamma.to(dev), beta.to(dev), 1e-5) if ln else None, out=out)
    assert float((out.cpu().double() - ref).abs().max()) <= _bound(err32)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())  # nothing outside the slice is touched


def test_posconv_padded_rows_are_computed_not_skipped(backend):
    """Frames past key_len come out as GELU(conv + bias) of the masked input -- not zero, not x: the reference computes them and
    output_norm averages over them."""
    nat, dev = backend
    x, kl, w, bias, _, _, ref, err32 = _posconv_case("cg64_k16", False)
    d, G, k = POSCONV["cg64_k16"][:3]
    y = nat.w2v_posconv(x.to(dev), kl.to(dev), _tap_major(w).to(dev), bias.to(dev), G, k).cpu()
    far = F.gelu(bias.double())  # frame 18 of utterance 1 (length 7, k/2 = 8) reads padding only
    assert float((y[1, 18].double() - far).abs().max()) <= 1e-6
    assert float((y[1, 8].double() - ref[1, 8]).abs().max()) <= _bound(err32) and float((ref[1, 8] - far).abs().max()) > 1e-3


def test_posconv_refuses_unsupported_shapes(backend):
    nat, dev = backend
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(nat.SbkError, match=r"group width 80/2|group width 40"):
        nat.w2v_posconv(z(1, 8, 80), None, z(80, 40 * 4), z(80), 2, 4)
    with pytest.raises(nat.SbkError, match="129 taps"):
        nat.w2v_posconv(z(1, 8, 32), None, z(32, 129 * 16), z(32), 2, 129)
    lib = nat.load()
    import ctypes

    x, w, b, y = z(1, 8, 80), z(80, 160), z(80), z(1, 8, 80)
    rc = lib.sbk_w2v_posconv_f32(x.data_ptr(), None, w.data_ptr(), b.data_ptr(), None, None, ctypes.c_float(0.0), y.data_ptr(),
                                 1, 8, 80, 2, 4, None)
    assert rc == -22 and "(16,32,48,64)" in lib.sbk_last_error().decode()
