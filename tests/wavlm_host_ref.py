"""Plain-torch restatement of the WavLM and HuBERT wrappers' forward (reference integrations/huggingface/wavlm.py and hubert.py:
the wav2vec 2.0 wrapper around HuggingFace's WavLMModel / HubertModel), dtype-generic: the tests run it in fp64 as the yardstick
and in fp32 for the reference's own rounding.  ``sd`` holds the HuggingFace parameter names WITHOUT the wrapper's ``model.``
prefix.  Neither ``transformers`` nor the reference is imported; the feature encoder and the positional convolution are those of
tests/wav2vec2_host_ref.py.

WavLM's attention (transformers WavLMAttention) MATERIALISES the gated bias here, [B,H,T,T], as HuggingFace does: it is what
the fused kernel is compared with.  tests/test_wavlm_model.py pins this file to the goldens written by the reference itself
(tools/make_wavlm_golden.py)."""
import math

import torch
import torch.nn.functional as F

import wav2vec2_host_ref as W


def relative_buckets(rel, num_buckets, max_distance):
    """WavLMAttention._relative_positions_bucket on an int64 tensor of key - query."""
    nb = num_buckets // 2
    out = (rel > 0).to(torch.long) * nb
    rel = rel.abs()
    max_exact = nb // 2
    large = torch.log(rel.float() / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact)
    large = torch.min((max_exact + large).to(torch.long), torch.full_like(rel, nb - 1))
    return out + torch.where(rel < max_exact, rel, large)


def position_bias(embed, T, num_buckets, max_distance):
    """compute_bias(T, T): rel_attn_embed.weight [num_buckets, H] -> [H, T, T], entry [h, i, j] for query i and key j."""
    pos = torch.arange(T)
    return embed[relative_buckets(pos[None, :] - pos[:, None], num_buckets, max_distance)].permute(2, 0, 1)


def gate(x, gate_w, gate_b, gate_const, heads):
    """x [B,T,d] -> the gate of every (batch, head, query) [B,H,T]; gate_const holds H values."""
    B, T, d = x.shape
    p = F.linear(x.view(B, T, heads, d // heads).permute(0, 2, 1, 3), gate_w, gate_b)
    ga, gb = torch.sigmoid(p.view(B, heads, T, 2, 4).sum(-1)).chunk(2, dim=-1)
    return (ga * (gb * gate_const.reshape(1, heads, 1, 1) - 1.0) + 2.0).squeeze(-1)


def gated_attention(q, k, v, x, gate_w, gate_b, gate_const, bias, key_len, scale):
    """q, k, v [B,H,T,Dh], x [B,T,H*Dh], bias [H,T,T] -> context [B,T,H*Dh]: softmax(scale q k^T + gate * bias, keys < key_len) v
    with the [B,H,T,T] bias formed -- the composition F.multi_head_attention_forward runs with a float attention mask."""
    B, H, T, Dh = q.shape
    s = (q * scale) @ k.transpose(-1, -2) + gate(x, gate_w, gate_b, gate_const, H)[..., None] * bias[None]
    if key_len is not None:
        dead = torch.arange(T)[None, :] >= key_len[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, H * Dh)


def _attention(h, sd, pre, heads, key_len, bias):
    """One attention module with its output projection.  bias None: plain attention (HuBERT / wav2vec 2.0)."""
    B, T, d = h.shape
    dh = d // heads
    q, k, v = (F.linear(h, sd[pre + f"{n}_proj.weight"], sd[pre + f"{n}_proj.bias"]).view(B, T, heads, dh).transpose(1, 2)
               for n in "qkv")
    if bias is None:
        ctx = gated_attention(q, k, v, h, h.new_zeros(8, dh), h.new_zeros(8), h.new_zeros(heads), h.new_zeros(heads, T, T),
                              key_len, dh ** -0.5)
    else:
        ctx = gated_attention(q, k, v, h, sd[pre + "gru_rel_pos_linear.weight"], sd[pre + "gru_rel_pos_linear.bias"],
                              sd[pre + "gru_rel_pos_const"], bias, key_len, dh ** -0.5)
    return F.linear(ctx, sd[pre + "out_proj.weight"], sd[pre + "out_proj.bias"])


def forward(wav, wav_lens, sd, cfg, normalize_wav, output_norm=False, output_all_hiddens=False):
    """The wrapper's ``extract_features``: wav [B,N], wav_lens relative [B] or None.  ``cfg["model_type"]``: "wavlm" (the gated
    relative-position bias; the table of layer 0 serves every layer) or "hubert" (plain attention; ``feat_proj_layer_norm``)."""
    eps = cfg.get("layer_norm_eps", 1e-5)
    wavlm = cfg["model_type"] == "wavlm"
    B, N = wav.shape
    key_len = None
    if wav_lens is not None:
        valid = torch.round(wav_lens.to(wav.dtype) * N).long()
    if normalize_wav:
        wav = F.layer_norm(wav, wav.shape[1:])
    h = W.feature_encoder(wav, sd, cfg)
    T = h.shape[1]
    if wav_lens is not None:
        key_len = W.feat_lengths(valid, cfg)
        key_len = torch.where(key_len <= 0, torch.full_like(key_len, T), key_len).clamp(max=T)
    ln = lambda x, name: F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)  # noqa: E731
    if wavlm or cfg.get("feat_proj_layer_norm", True):
        h = ln(h, "feature_projection.layer_norm")
    h = F.linear(h, sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"])
    stable = bool(cfg.get("do_stable_layer_norm", False))
    h = W.posconv(h, key_len, W.pos_weight(sd), sd["encoder.pos_conv_embed.conv.bias"], cfg["num_conv_pos_embedding_groups"])
    if not stable:
        h = ln(h, "encoder.layer_norm")
    bias = None
    if wavlm:
        bias = position_bias(sd["encoder.layers.0.attention.rel_attn_embed.weight"], T, cfg.get("num_buckets", 320),
                             cfg.get("max_bucket_distance", 800))
    heads = cfg["num_attention_heads"]
    hidden = []
    for i in range(cfg["num_hidden_layers"]):
        hidden.append(h)
        pre = f"encoder.layers.{i}."
        if stable:
            h = h + _attention(ln(h, pre + "layer_norm"), sd, pre + "attention.", heads, key_len, bias)
            f = ln(h, pre + "final_layer_norm")
        else:
            h = ln(h + _attention(h, sd, pre + "attention.", heads, key_len, bias), pre + "layer_norm")
            f = h
        f = F.gelu(F.linear(f, sd[pre + "feed_forward.intermediate_dense.weight"], sd[pre + "feed_forward.intermediate_dense.bias"]))
        f = F.linear(f, sd[pre + "feed_forward.output_dense.weight"], sd[pre + "feed_forward.output_dense.bias"])
        h = h + f
        if not stable:
            h = ln(h, pre + "final_layer_norm")
    if stable:
        h = ln(h, "encoder.layer_norm")
    hidden.append(h)
    out = torch.stack(hidden) if output_all_hiddens else h
    if output_norm:
        out = F.layer_norm(out, out.shape[-2:])
    return out
