"""Plain-torch restatement of the Transformer-encoder ASR model (the transformer.yaml recipe): the three-block convolution front
end, plain multi-head attention, the encoder layer in both norm orders and TransformerASR.encode.  Nothing is imported from the
reference; every function runs in the dtype of its inputs (fp32 or fp64), so it serves as the fp64 reference of the kernel tests
and, in fp32, as the measure of what another summation order costs.

State-dict keys are the reference's (``sd`` maps key -> tensor, ``pfx`` is the prefix of the module)."""
import math

import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------ convolution front end
def conv2d_same(x, w, b, stride):
    """nnet/CNN.py Conv2d, padding "same", reflect: x [B,T,F,Cin], w [Cout,Cin,kF,kT] -> [B,T',F',Cout].  get_padding_elem:
    stride > 1 pads kernel // 2 on each side; stride 1 pads (L_in - L_out) // 2 (0 for a 1x1 kernel)."""
    kf, kt = w.shape[2], w.shape[3]
    h = x.permute(0, 3, 2, 1)  # [B,Cin,F,T]
    pf, pt = (kf // 2, kt // 2) if stride > 1 else ((kf - 1) // 2, (kt - 1) // 2)
    if pf or pt:
        h = F.pad(h, (pt, pt, pf, pf), mode="reflect")
    h = F.conv2d(h, w, b, stride=stride)
    return h.permute(0, 3, 2, 1)


def layer_norm_fc(x, g, b, eps=1e-5):
    """LayerNorm over the (F, C) dimensions of [B,T,F,C]; g / b [F,C]."""
    return F.layer_norm(x, tuple(x.shape[2:]), g.reshape(x.shape[2:]), b.reshape(x.shape[2:]), eps)


def conv_block(x, sd, pfx, stride, slope=0.01):
    """ConvBlock of one layer: conv -> LayerNorm(F',C') -> LeakyReLU; with reduce_conv keys present, + LayerNorm(reduce_conv(x))."""
    if x.dim() == 3:
        x = x.unsqueeze(-1)
    h = conv2d_same(x, sd[pfx + "convs.conv_0.conv.weight"], sd[pfx + "convs.conv_0.conv.bias"], stride)
    h = F.leaky_relu(layer_norm_fc(h, sd[pfx + "convs.norm_0.norm.weight"], sd[pfx + "convs.norm_0.norm.bias"]), slope)
    if pfx + "reduce_conv.conv.conv.weight" in sd:
        r = conv2d_same(x, sd[pfx + "reduce_conv.conv.conv.weight"], sd[pfx + "reduce_conv.conv.conv.bias"], stride)
        h = h + layer_norm_fc(r, sd[pfx + "reduce_conv.norm.norm.weight"], sd[pfx + "reduce_conv.norm.norm.bias"])
    return h


def conv_frontend(x, sd, pfx, strides=(2, 2, 1), return_blocks=False):
    """ConvolutionFrontEnd: [B,T,F] -> [B,T',F',C]; blocks convblock_{i}."""
    outs = []
    for i, s in enumerate(strides):
        x = conv_block(x, sd, f"{pfx}convblock_{i}.", s)
        outs.append(x)
    return (x, outs) if return_blocks else x


# ------------------------------------------------------------------------------------------ encoder
def abs_pos_encoding(L, d, dtype):
    """PositionalEncoding (Transformer.py): sin on the even, cos on the odd channels; computed in fp32 as the module's buffer is."""
    pos = torch.arange(0, L).unsqueeze(1).float()
    den = torch.exp(torch.arange(0, d, 2).float() * -(math.log(10000.0) / d))
    pe = torch.zeros(L, d)
    pe[:, 0::2] = torch.sin(pos * den)
    pe[:, 1::2] = torch.cos(pos * den)
    return pe.to(dtype)


def mha(x, sd, pfx, H, key_pad=None):
    """torch.nn.MultiheadAttention self-attention as nnet/attention.py MultiheadAttention wraps it: in_proj rows [q | k | v], scale
    1 / sqrt(head_dim), boolean key padding mask [B,T] (True = padded)."""
    B, T, E = x.shape
    Dh = E // H
    W, bias = sd[pfx + "att.in_proj_weight"], sd[pfx + "att.in_proj_bias"]
    q, k, v = [F.linear(x, W[i * E:(i + 1) * E], bias[i * E:(i + 1) * E]).view(B, T, H, Dh).transpose(1, 2) for i in range(3)]
    sc = torch.matmul(q * (1.0 / math.sqrt(Dh)), k.transpose(-1, -2))
    if key_pad is not None:
        sc = sc.masked_fill(key_pad.view(B, 1, 1, T), float("-inf"))
    o = torch.matmul(torch.softmax(sc, dim=-1), v).transpose(1, 2).reshape(B, T, E)
    return F.linear(o, sd[pfx + "att.out_proj.weight"], sd[pfx + "att.out_proj.bias"])


def _ln(x, sd, pfx, eps=1e-6):
    return F.layer_norm(x, (x.shape[-1],), sd[pfx + "weight"], sd[pfx + "bias"], eps)


def _ffn(x, sd, pfx, act):
    return F.linear(act(F.linear(x, sd[pfx + "ffn.0.weight"], sd[pfx + "ffn.0.bias"])), sd[pfx + "ffn.3.weight"], sd[pfx + "ffn.3.bias"])


def encoder_layer(x, sd, pfx, H, key_pad, normalize_before=True, act=F.gelu):
    """TransformerEncoderLayer (Transformer.py): pre-norm x + MHA(norm1(x)), x + ffn(norm2(x)); post-norm norm1(x + MHA(x)),
    norm2(x + ffn(x))."""
    h = _ln(x, sd, pfx + "norm1.norm.") if normalize_before else x
    x = x + mha(h, sd, pfx + "self_att.", H, key_pad)
    if not normalize_before:
        x = _ln(x, sd, pfx + "norm1.norm.")
    h = _ln(x, sd, pfx + "norm2.norm.") if normalize_before else x
    x = x + _ffn(h, sd, pfx + "pos_ffn.", act)
    if not normalize_before:
        x = _ln(x, sd, pfx + "norm2.norm.")
    return x


def length_to_pad_mask(wav_lens, T):
    """TransformerASR.make_masks: abs length = round(wav_len * T); True = padded."""
    n = torch.round(wav_lens.double() * T).long()
    return torch.arange(T)[None, :] >= n[:, None]


def encode(src, wav_lens, sd, pfx, H, num_layers, normalize_before=True, act=F.gelu, return_layers=False):
    """TransformerASR.encode with encoder_module="transformer", fixed_abs_sine positions: src [B,T,F] or [B,T,F,C] -> custom_src_module
    (Linear + Dropout) -> + positional encoding -> the layers -> LayerNorm(eps 1e-6)."""
    if src.dim() == 4:
        src = src.reshape(src.shape[0], src.shape[1], -1)
    B, T, _ = src.shape
    key_pad = None if wav_lens is None else length_to_pad_mask(wav_lens, T)
    x = F.linear(src, sd[pfx + "custom_src_module.layers.0.w.weight"], sd[pfx + "custom_src_module.layers.0.w.bias"])
    x = x + abs_pos_encoding(T, x.shape[-1], x.dtype)[None]
    layers = []
    for l in range(num_layers):
        x = encoder_layer(x, sd, f"{pfx}encoder.layers.{l}.", H, key_pad, normalize_before, act)
        layers.append(x)
    x = _ln(x, sd, pfx + "encoder.norm.norm.")
    return (x, layers) if return_layers else x


# ------------------------------------------------------------------------------------------ seeded weights
def seeded_state_dict(shapes, seed, sharpen=6.0):
    """Parameters drawn from a seed by a fixed rule (torch's CPU generator), for fixtures whose state dict is too large to commit:
    the golden generator loads them into the reference model, the tests rebuild the same tensors.  ``shapes``: name -> shape.
    Matrices N(0, 1 / fan_in), LayerNorm weights 1 + 0.1 N, every other vector 0.1 N; the output heads (seq_lin / ctc_lin) are
    multiplied by ``sharpen`` so that the searches are decided by clear margins."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name in sorted(shapes):
        shape = tuple(int(n) for n in shapes[name])
        if len(shape) >= 2:
            w = torch.randn(shape, generator=g) / math.sqrt(shape[-1])
            if name.startswith(("seq_lin.", "ctc_lin.")):
                w = w * sharpen
        elif name.endswith("norm.weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            w = 0.1 * torch.randn(shape, generator=g)
        sd[name] = w
    return sd
