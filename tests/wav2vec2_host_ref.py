"""Plain-torch restatement of the wav2vec 2.0 wrapper's forward (reference integrations/huggingface/wav2vec2.py:160-199 around
HuggingFace's Wav2Vec2Model), dtype-generic: the tests run it in fp64 as the yardstick and in fp32 for the reference's own
rounding.  ``sd`` holds the HuggingFace parameter names WITHOUT the wrapper's ``model.`` prefix; the positional filter is taken
from ``encoder.pos_conv_embed.conv.parametrizations.weight.original0/1`` (or the older ``weight_g`` / ``weight_v``).

tests/test_wav2vec2_model.py pins it to the goldens written by the reference itself (tools/make_wav2vec2_golden.py)."""
import torch
import torch.nn.functional as F


def feat_lengths(n, cfg):
    """Wav2Vec2Model._get_feat_extract_output_lengths on a sample count (tensor or int)."""
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        n = torch.div(n - k, s, rounding_mode="floor") + 1 if torch.is_tensor(n) else (n - k) // s + 1
    return n


def pos_weight(sd):
    """The effective filter of the weight-normalised positional convolution (weight_norm over dim 2): g * v / ||v||."""
    pre = "encoder.pos_conv_embed.conv."
    if pre + "parametrizations.weight.original0" in sd:
        g, v = sd[pre + "parametrizations.weight.original0"], sd[pre + "parametrizations.weight.original1"]
    else:
        g, v = sd[pre + "weight_g"], sd[pre + "weight_v"]
    return v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())


def channel_norm(h, gamma, beta, eps):
    """GroupNorm(C, C) of h [B,C,T]: every (utterance, channel) over time, biased variance, eps inside the root.  (Written out:
    F.group_norm refuses a single value per channel, which one frame of one utterance is.)"""
    mean = h.mean(dim=2, keepdim=True)
    var = (h - mean).pow(2).mean(dim=2, keepdim=True)
    return (h - mean) * torch.rsqrt(var + eps) * gamma[None, :, None] + beta[None, :, None]


def conv0(wav, w, bias, gamma, beta, stride, mode, eps=1e-5, normalize=False):
    """Layer 0 of the feature encoder as the kernel tests compose it: [B,N] -> [B,T0,C0].  mode "group" | "layer"."""
    if normalize:
        wav = F.layer_norm(wav, wav.shape[1:])
    h = F.conv1d(wav[:, None], w[:, None], bias, stride=stride)
    if mode == "group":
        h = channel_norm(h, gamma, beta, eps)
    else:
        h = F.layer_norm(h.transpose(1, 2), (w.shape[0],), gamma, beta, eps).transpose(1, 2)
    return F.gelu(h).transpose(1, 2)


def posconv(x, key_len, weight, bias, groups, ln=None):
    """mask(x) + GELU(conv(mask(x))): weight [d, d/groups, k] (effective); ln = (gamma, beta, eps) or None."""
    k = weight.shape[-1]
    if key_len is not None:
        keep = torch.arange(x.shape[1])[None, :] < key_len[:, None]
        x = x * keep[:, :, None].to(x.dtype)
    p = F.conv1d(x.transpose(1, 2), weight, bias, padding=k // 2, groups=groups)
    if k % 2 == 0:
        p = p[:, :, :-1]
    y = x + F.gelu(p).transpose(1, 2)
    if ln is not None:
        y = F.layer_norm(y, (x.shape[-1],), ln[0], ln[1], ln[2])
    return y


def feature_encoder(wav, sd, cfg):
    h = wav[:, None]
    group = cfg.get("feat_extract_norm", "group") == "group"
    for i, s in enumerate(cfg["conv_stride"]):
        pre = f"feature_extractor.conv_layers.{i}."
        h = F.conv1d(h, sd[pre + "conv.weight"], sd.get(pre + "conv.bias"), stride=s)
        if group and i == 0:
            h = channel_norm(h, sd[pre + "layer_norm.weight"], sd[pre + "layer_norm.bias"], 1e-5)
        elif not group:
            h = F.layer_norm(h.transpose(1, 2), (h.shape[1],), sd[pre + "layer_norm.weight"], sd[pre + "layer_norm.bias"],
                             1e-5).transpose(1, 2)
        h = F.gelu(h)
    return h.transpose(1, 2)


def _attention(h, sd, pre, heads, key_len):
    B, T, d = h.shape
    dh = d // heads
    q = F.linear(h, sd[pre + "q_proj.weight"], sd[pre + "q_proj.bias"]) * dh ** -0.5
    k = F.linear(h, sd[pre + "k_proj.weight"], sd[pre + "k_proj.bias"])
    v = F.linear(h, sd[pre + "v_proj.weight"], sd[pre + "v_proj.bias"])
    q, k, v = (t.view(B, T, heads, dh).transpose(1, 2) for t in (q, k, v))
    s = q @ k.transpose(-1, -2)
    if key_len is not None:  # keys only: the query rows past the length are computed like any other
        dead = torch.arange(T)[None, :] >= key_len[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    ctx = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, d)
    return F.linear(ctx, sd[pre + "out_proj.weight"], sd[pre + "out_proj.bias"])


def forward(wav, wav_lens, sd, cfg, normalize_wav, output_norm=False, output_all_hiddens=False):
    """The wrapper's ``extract_features``: wav [B,N], wav_lens relative [B] or None."""
    eps = cfg.get("layer_norm_eps", 1e-5)
    B, N = wav.shape
    key_len = None
    if wav_lens is not None:
        valid = torch.round(wav_lens.to(wav.dtype) * N).long()
    if normalize_wav:
        wav = F.layer_norm(wav, wav.shape[1:])
    feats = feature_encoder(wav, sd, cfg)
    T = feats.shape[1]
    if wav_lens is not None:
        key_len = feat_lengths(valid, cfg)
        key_len = torch.where(key_len <= 0, torch.full_like(key_len, T), key_len).clamp(max=T)  # (HF: index -1 marks every frame)
    h = F.layer_norm(feats, (feats.shape[-1],), sd["feature_projection.layer_norm.weight"],
                     sd["feature_projection.layer_norm.bias"], eps)
    h = F.linear(h, sd["feature_projection.projection.weight"], sd["feature_projection.projection.bias"])
    ln = lambda x, name: F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"], eps)  # noqa: E731
    stable = bool(cfg.get("do_stable_layer_norm", False))
    h = posconv(h, key_len, pos_weight(sd), sd["encoder.pos_conv_embed.conv.bias"], cfg["num_conv_pos_embedding_groups"])
    if not stable:
        h = ln(h, "encoder.layer_norm")
    hidden = []
    for i in range(cfg["num_hidden_layers"]):
        hidden.append(h)
        pre = f"encoder.layers.{i}."
        if stable:
            h = h + _attention(ln(h, pre + "layer_norm"), sd, pre + "attention.", cfg["num_attention_heads"], key_len)
            f = ln(h, pre + "final_layer_norm")
        else:
            h = ln(h + _attention(h, sd, pre + "attention.", cfg["num_attention_heads"], key_len), pre + "layer_norm")
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
        out = F.layer_norm(out, out.shape[-3:][1:])  # (wav2vec2.py:188-197: (T', d) of each utterance, with or without the stack)
    return out
