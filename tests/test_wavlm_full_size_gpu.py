"""WavLM at its real widths on the MI355X (gpu only): conv_dim 512, {d 768, 12 heads, group norm, post-norm} (base-plus) and
{d 1024, 16 heads, layer norm, stable} (large), head dim 64, 320 / 800 buckets, 2 layers, seeded random weights built in the
test, B = 2 with N = (24 000, 16 400) -- so T' = 74 frames: three key tiles, the last one ragged, relative positions past the 80
exact buckets' half.  The relative-position embedding is drawn at unit scale and the gate parameters are perturbed, so that the
bias is of the scores' size.

Yardstick: the fp64 host restatement (tests/wavlm_host_ref.py, which materialises the [B,H,T',T'] bias) on the CPU; bound:
max(4 x the fp32 restatement's own error against it, 5e-5), on every frame, padded frames included -- the layout and the bound of
tests/test_wav2vec2_full_size_gpu.py."""
import pytest
import torch

import wavlm_host_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {
    "base_plus": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, feat_extract_norm="group", conv_bias=False,
                      do_stable_layer_norm=False),
    "large": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer", conv_bias=True,
                  do_stable_layer_norm=True),
}


def _config(name):
    return dict(model_type="wavlm", conv_dim=[512] * 7, conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_kernel=[10, 3, 3, 3, 3, 2, 2],
                num_hidden_layers=2, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5,
                hidden_act="gelu", feat_extract_activation="gelu", num_buckets=320, max_bucket_distance=800, **SHAPES[name])


@pytest.mark.parametrize("name", list(SHAPES))
def test_full_width_encoder_vs_fp64_host_restatement(name):
    from speechbrain_amd import native
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM

    import emu_utils

    emu_utils.detach()
    native.load()
    cfg = _config(name)
    normalize = name == "large"
    w = WavLM.from_config(cfg, normalize_wav=normalize, output_norm=True, seed=5)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in w.model.named_parameters():
            if "rel_attn_embed" in n:
                p.copy_(torch.randn(p.shape, generator=gen))
            elif "gru_rel_pos" in n:
                p.add_(0.3 * torch.randn(p.shape, generator=gen))
            elif p.dim() == 1 and "masked_spec" not in n:  # random norm affines / biases, so that they are exercised
                p.add_(0.1 * torch.randn(p.shape, generator=gen))
    N = 24000
    wav = 0.3 * torch.randn(2, N, generator=gen)
    lens = torch.tensor([1.0, 16400 / N])
    wav[1, 16400:] = 0
    sd = {k[len("model."):]: v.detach().clone() for k, v in w.state_dict().items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = R.forward(wav.double(), lens.double(), sd64, cfg, normalize, output_norm=True)
    err32 = float((R.forward(wav, lens, sd, cfg, normalize, output_norm=True).double() - ref).abs().max())
    assert ref.shape[1] == 74
    flat = {**sd64, "encoder.layers.0.attention.rel_attn_embed.weight": torch.zeros_like(
        sd64["encoder.layers.0.attention.rel_attn_embed.weight"])}
    moved = float((R.forward(wav.double(), lens.double(), flat, cfg, normalize, output_norm=True) - ref).abs().max())
    assert moved > 1e-2  # (the bias matters on these weights: a wrong table cannot pass)
    got = w.to("cuda:0")(wav.to("cuda:0"), lens.to("cuda:0")).cpu()
    err = float((got.double() - ref).abs().max())
    print(f"WavLM {name} full width: max|d| {err:.3e}, fp32 host restatement {err32:.3e}, ratio {err / err32:.2f}, "
          f"zeroed table moves the output by {moved:.2e}")
    assert err <= max(4.0 * err32, 5e-5)
