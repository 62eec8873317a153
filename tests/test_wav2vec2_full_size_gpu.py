"""wav2vec 2.0 at its real widths on the MI355X (gpu only): conv_dim 512, {d 768, 12 heads, group norm, post-norm} and
{d 1024, 16 heads, layer norm, stable}, 2 layers, seeded random weights built in the test, B = 2 with N = (24 000, 16 400) -- so
T' = 74 frames, more than half the 128-tap positional kernel.

Yardstick: the fp64 host restatement (tests/wav2vec2_host_ref.py) on the CPU; bound: max(4 x the fp32 restatement's own error
against it, 5e-5), on every frame, padded frames included."""
import pytest
import torch

import wav2vec2_host_ref as R

pytestmark = pytest.mark.gpu

SHAPES = {
    "base": dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, feat_extract_norm="group", conv_bias=False,
                 do_stable_layer_norm=False),
    "large": dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, feat_extract_norm="layer", conv_bias=True,
                  do_stable_layer_norm=True),
}


def _config(name):
    return dict(conv_dim=[512] * 7, conv_stride=[5, 2, 2, 2, 2, 2, 2], conv_kernel=[10, 3, 3, 3, 3, 2, 2], num_hidden_layers=2,
                num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, layer_norm_eps=1e-5, hidden_act="gelu",
                feat_extract_activation="gelu", **SHAPES[name])


@pytest.mark.parametrize("name", list(SHAPES))
def test_full_width_encoder_vs_fp64_host_restatement(name):
    from speechbrain_amd import native
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2

    import emu_utils

    emu_utils.detach()
    native.load()
    cfg = _config(name)
    normalize = name == "large"
    w = Wav2Vec2.from_config(cfg, normalize_wav=normalize, output_norm=True, seed=5)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for n, p in w.model.named_parameters():  # random norm affines / biases, so that they are exercised
            if p.dim() == 1 and "masked_spec" not in n:
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
    got = w.to("cuda:0")(wav.to("cuda:0"), lens.to("cuda:0")).cpu()
    err = float((got.double() - ref).abs().max())
    print(f"wav2vec2 {name} full width: max|d| {err:.3e}, fp32 host restatement {err32:.3e}, ratio {err / err32:.2f}")
    assert err <= max(4.0 * err32, 5e-5)
