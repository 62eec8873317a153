"""Plain-torch restatement of the Branchformer encoder (lobes/models/transformer/Branchformer.py:188-234, :335-409) and of
its Convolutional Spatial Gating Unit (lobes/models/convolution.py:92-113): F.layer_norm, F.pad(mode="reflect"),
F.conv1d(groups=C) and the oracle's RelPosMHAXL pieces.  Every function computes in the dtype of its inputs, so the same
code is the fp32 composition and -- on .double() inputs -- the fp64 reference of the GPU tests (the GPU machine has no
reference checkout).  test_branchformer_model.py pins it to the reference's own outputs (tests/golden/model_branchformer.npz).
"""
import math

import torch
import torch.nn.functional as F

from oracle import sb_oracle as O


def csgu(h, gamma, beta, eps, w, bias, act=None):
    """h [B,T,2C]; gamma / beta [C]; w [C,1,k] (or [C,k]); bias [C] -> act(conv_reflect(LayerNorm(h[..., C:]))) * h[..., :C]."""
    x1, x2 = h.chunk(2, dim=-1)
    C = x2.shape[-1]
    w = w.reshape(C, 1, -1)
    halo = (w.shape[-1] - 1) // 2
    n = F.layer_norm(x2, (C,), gamma, beta, eps).transpose(1, 2)
    n = F.pad(n, (halo, halo), mode="reflect")  # nnet/CNN.py Conv1d, padding="same", padding_mode="reflect"
    c = F.conv1d(n, w, bias, groups=C).transpose(1, 2)
    if act is not None:
        c = act(c)
    return c * x1


def relpos_mha(x, pos, sd, pfx, H, key_pad):
    """oracle.relpos_mha in the dtype of x (the oracle's softmax is pinned to fp32)."""
    B, T, E = x.shape
    Dh = E // H
    q, k, v = F.linear(x, sd[pfx + "in_proj_weight"]).view(B, T, H, 3 * Dh).chunk(3, dim=-1)
    u = sd[pfx + "pos_bias_u"].view(1, 1, H, Dh)
    vb = sd[pfx + "pos_bias_v"].view(1, 1, H, Dh)
    p = F.linear(pos, sd[pfx + "linear_pos.weight"]).view(1, -1, H, Dh)
    s = 1.0 / math.sqrt(E)
    ac = torch.matmul(((q + u) * s).transpose(1, 2), k.permute(0, 2, 3, 1))
    bd = O.rel_shift(torch.matmul(((q + vb) * s).transpose(1, 2), p.permute(0, 2, 3, 1)))
    score = ac + bd
    if key_pad is not None:
        score = score.masked_fill(key_pad.view(B, 1, 1, T), float("-inf"))
    att = F.softmax(score, dim=-1)
    if key_pad is not None:
        att = att.masked_fill(key_pad.view(B, 1, 1, T), 0.0)
    o = torch.matmul(att, v.transpose(1, 2)).transpose(1, 2).reshape(B, T, E)
    return F.linear(o, sd[pfx + "out_proj.weight"], sd[pfx + "out_proj.bias"])


def layer(x, pos, sd, pfx, H, key_pad, act=F.gelu, gate_act=None):
    """BranchformerEncoderLayer.forward: x + merge_proj(cat[MHA(norm_mhsa(x)), cgMLP(norm_conv(x))]); the cgMLP branch is unmasked."""
    x1 = relpos_mha(O._ln(x, sd, pfx + "norm_mhsa.norm.", 1e-5), pos, sd, pfx + "mha_layer.", H, key_pad)
    cb = pfx + "convolution_branch."
    h = act(F.linear(O._ln(x, sd, pfx + "norm_conv.norm.", 1e-5), sd[cb + "pre_channel_proj.weight"], sd[cb + "pre_channel_proj.bias"]))
    g = csgu(h, sd[cb + "csgu.norm.norm.weight"], sd[cb + "csgu.norm.norm.bias"], 1e-5, sd[cb + "csgu.conv.conv.weight"],
             sd[cb + "csgu.conv.conv.bias"], gate_act)
    x2 = F.linear(g, sd[cb + "post_channel_proj.weight"], sd[cb + "post_channel_proj.bias"])
    return x + F.linear(torch.cat([x1, x2], dim=-1), sd[pfx + "merge_proj.weight"], sd[pfx + "merge_proj.bias"])


def encode(src, wav_lens, sd, d_model, nhead, num_layers, pfx="", return_layers=False):
    """TransformerASR.encode with encoder_module="branchformer": [B,T',F(,C)] -> [B,T',d] (+ the layers' outputs)."""
    if src.dim() == 4:
        src = src.reshape(src.shape[0], src.shape[1], -1)
    B, T, _ = src.shape
    key_pad = None
    if wav_lens is not None:
        key_pad = ~O.length_to_mask(torch.round(wav_lens.float() * T), T)
    x = F.linear(src, sd[pfx + "custom_src_module.layers.0.w.weight"], sd[pfx + "custom_src_module.layers.0.w.bias"])
    pos = O.relpos_table(T, d_model).to(x.dtype)  # (the fp32 table is an input of the model, in every precision)
    layers = []
    for l in range(num_layers):
        x = layer(x, pos, sd, f"{pfx}encoder.layers.{l}.", nhead, key_pad)
        layers.append(x)
    out = O._ln(x, sd, pfx + "encoder.norm.norm.", 1e-6)
    return (out, layers) if return_layers else out
