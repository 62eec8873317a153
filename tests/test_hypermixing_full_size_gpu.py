"""HyperMixing at the recipes' widths on the MI355X, random weights: the hypermix call alone at the 8M (d 144, 8 heads, d_ffn 576)
and 22M (d 256, 8 heads, d_ffn 1024) shapes, and a 2-layer full-width ConformerEncoder with attention_type="hypermixing",
against the fp64 restatement (tests/hypermixing_host_ref.py, whose convolution is tests/encoder_host_ref.py's).

Bounds: the call alone max(4 x the fp32 restatement's own error, 1e-5) (tests/test_hypermixing_kernels.py); the encoder
max(4 x the fp32 restatement's error, 5e-5).  Measured distances are printed."""
import pytest
import torch

import hypermixing_host_ref as R

pytestmark = pytest.mark.gpu
B, T = 4, 74
KEY_LEN = [74, 51, 1, 33]


@pytest.fixture(scope="module")
def dev():
    from speechbrain_amd import native

    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    import emu_utils

    emu_utils.detach()
    native.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("d,H,d_ffn", [(144, 8, 576), (256, 8, 1024)], ids=["8M", "22M"])
def test_hypermix_at_recipe_width(dev, d, H, d_ffn):
    from speechbrain_amd import native

    Dh, k = d // H, d_ffn // H
    gen = torch.Generator().manual_seed(d)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    h, res = rn(B, T, d), rn(B, T, d)
    gens = tuple((rn(H, Dh, Dh) / Dh ** 0.5, 0.5 * rn(H, Dh), rn(H, k, Dh) / Dh ** 0.5, 0.5 * rn(H, k)) for _ in range(2))
    ln_w, ln_b, pe = 1.0 + 0.3 * rn(d), 0.3 * rn(d), R.sine_table(T, d, torch.float32)
    kl = torch.tensor(KEY_LEN, dtype=torch.int32)
    c = lambda t: R.cast(t, torch.float64)  # noqa: E731
    ref = R.hypermix(c(h), kl, c(pe), c(gens[0]), c(gens[1]), c(ln_w), c(ln_b), 1e-5, H, residual=c(res))
    err32 = float((R.hypermix(h, kl, pe, gens[0], gens[1], ln_w, ln_b, 1e-5, H, residual=res).double() - ref).abs().max())
    t = lambda v: v.to(dev)  # noqa: E731
    y = native.hypermix(t(h), t(kl), t(pe), [t(v) for v in gens[0]], [t(v) for v in gens[1]], t(ln_w), t(ln_b), 1e-5, H,
                        residual=t(res))
    err = float((y.cpu().double() - ref).abs().max())
    print(f"hypermix d={d} H={H} d_ffn={d_ffn} B={B} T'={T}: kernel max|d| {err:.3e}, fp32 restatement {err32:.3e}, "
          f"ratio {err / max(err32, 1e-30):.2f}")
    assert err <= max(4.0 * err32, 1e-5)


def test_full_width_hyperconformer_encoder(dev):
    from speechbrain_amd.lobes.models.transformer.Conformer import ConformerEncoder

    d, H, d_ffn, ksize, n_layers = 256, 8, 1024, 31, 2
    torch.manual_seed(256)
    enc = ConformerEncoder(num_layers=n_layers, d_model=d, d_ffn=d_ffn, nhead=H, kernel_size=ksize, attention_type="hypermixing")
    gen = torch.Generator().manual_seed(257)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if p.dim() > 1 and "hyper." not in n:
                torch.nn.init.xavier_normal_(p)
            elif p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    sd = {k_: v.detach().clone() for k_, v in enc.state_dict().items()}
    x = torch.randn(B, T, d, generator=gen)
    kl = torch.tensor(KEY_LEN, dtype=torch.int32)
    with torch.no_grad():
        ref = R.conformer_encoder(x.double(), {k_: R.cast(v, torch.float64) for k_, v in sd.items()}, "", H, n_layers, kl, ksize)
        err32 = float((R.conformer_encoder(x, sd, "", H, n_layers, kl, ksize).double() - ref).abs().max())
        enc = enc.to(dev).eval()
        pad = torch.arange(T)[None, :] >= kl[:, None]
        y = enc(x.to(dev), src_key_padding_mask=pad.to(dev))[0]
    err = float((y.cpu().double() - ref).abs().max())
    print(f"2-layer HyperConformer encoder d={d}: max|d| {err:.3e}, fp32 restatement {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    assert err <= max(4.0 * err32, 5e-5)
