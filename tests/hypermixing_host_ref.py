"""HyperMixing in plain torch, dtype-generic: the fp64 reference of tests/test_hypermixing_*.py and, run in fp32, the
"composition" whose own error sets their bound.  It forms the generated weights W_1 / W_2 [B,H,T,k] explicitly (what the fused
kernels never do), so that tests can also perturb them.  Our own restatement of the formulas of include/sbk.h (HyperMixing).

A generator is the tuple (fc1_weights [H,Dh,Dh], fc1_biases [H,Dh], fc2_weights [H,k,Dh], fc2_biases [H,k])."""
import math

import torch
import torch.nn.functional as F


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def sine_table(T, d, dtype=torch.float64, shift=0):
    """Rows shift .. shift+T-1 of the absolute sinusoid table: pe[t, 2i] = sin(t w_i), pe[t, 2i+1] = cos(t w_i),
    w_i = 10000^(-2i/d)."""
    pos = torch.arange(shift, shift + T, dtype=torch.float64).unsqueeze(1)
    w = torch.exp(torch.arange(0, d, 2, dtype=torch.float64) * -(math.log(10000.0) / d))
    pe = torch.zeros(T, d, dtype=torch.float64)
    pe[:, 0::2] = torch.sin(pos * w)
    pe[:, 1::2] = torch.cos(pos * w)
    return pe.to(dtype)


def valid_mask(key_len, B, T, dtype):
    if key_len is None:
        return torch.ones(B, T, 1, dtype=dtype)
    return (torch.arange(T, device=key_len.device)[None, :] < key_len.to(torch.long)[:, None]).to(dtype).unsqueeze(-1)


def split_heads(x, H, heads_last=False):
    """[B,T,d] -> [B,H,T,Dh]; channel c belongs to head c // Dh (heads_last: the WRONG layout c % H, for the mutation test)."""
    B, T, d = x.shape
    if heads_last:
        return x.reshape(B, T, d // H, H).permute(0, 3, 1, 2)
    return x.reshape(B, T, H, d // H).permute(0, 2, 1, 3)


def generate(p, gen, H, act=gelu_erf, heads_last=False):
    """W [B,H,T,k] of one generator from the hypernetwork input p [B,T,d]."""
    fc1w, fc1b, fc2w, fc2b = gen
    ph = split_heads(p, H, heads_last)                                      # [B,H,T,Dh]
    z = act(torch.einsum("bhtf,hef->bhte", ph, fc1w) + fc1b[None, :, None, :])
    return torch.einsum("bhte,hje->bhtj", z, fc2w) + fc2b[None, :, None, :]


def generated_weights(h, key_len, pe, w1_gen, w2_gen, H, act=gelu_erf, use_pe=True, mask_weights=True, heads_last=False):
    """(u, W_1, W_2): the masked input and both generated weight tensors."""
    B, T, d = h.shape
    m = valid_mask(key_len, B, T, h.dtype)
    u = h * m
    p = u + pe[:T].to(h.dtype)[None] if use_pe else u
    W1, W2 = generate(p, w1_gen, H, act, heads_last), generate(p, w2_gen, H, act, heads_last)
    if mask_weights:
        W1, W2 = W1 * m[:, None], W2 * m[:, None]
    return u, W1, W2


def mix(u, W1, W2, H, act=gelu_erf, heads_last=False):
    """y [B,T,d] = per head A W_2^T with A = act(u_head^T W_1)."""
    B, T, d = u.shape
    uh = split_heads(u, H, heads_last)                                      # [B,H,T,Dh]
    A = act(torch.einsum("bhtf,bhtj->bhfj", uh, W1))                         # [B,H,Dh,k]
    y = torch.einsum("bhfj,bhtj->bhtf", A, W2)                               # [B,H,T,Dh]
    if heads_last:
        return y.permute(0, 2, 3, 1).reshape(B, T, d)
    return y.permute(0, 2, 1, 3).reshape(B, T, d)


def hypermix(h, key_len, pe, w1_gen, w2_gen, ln_w, ln_b, eps, H, residual=None, act=gelu_erf, use_pe=True,
             mask_weights=True, heads_last=False, swap_generators=False):
    """LayerNorm_d(mix(h)) + residual; the keyword switches are the mistakes the mutation test plants."""
    if swap_generators:
        w1_gen, w2_gen = w2_gen, w1_gen
    u, W1, W2 = generated_weights(h, key_len, pe, w1_gen, w2_gen, H, act, use_pe, mask_weights, heads_last)
    y = mix(u, W1, W2, H, act, heads_last)
    out = F.layer_norm(y, (h.shape[-1],), ln_w, ln_b, eps)
    return out if residual is None else out + residual


def cast(tensors, dtype):
    if tensors is None:
        return None
    if isinstance(tensors, torch.Tensor):
        return tensors.to(dtype) if tensors.is_floating_point() else tensors
    return type(tensors)(cast(t, dtype) for t in tensors)


# ---- the HyperConformer encoder around it (state-dict driven, dtype-generic; the convolution is encoder_host_ref's) ----------
def _ln(x, sd, pfx, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[pfx + "weight"], sd[pfx + "bias"], eps)


def _ffn_half(x, sd, pfx):
    h = F.silu(F.linear(_ln(x, sd, pfx + "0.", 1e-5), sd[pfx + "1.ffn.0.weight"], sd[pfx + "1.ffn.0.bias"]))
    return x + 0.5 * F.linear(h, sd[pfx + "1.ffn.3.weight"], sd[pfx + "1.ffn.3.bias"])


def _generator(sd, pfx):
    return tuple(sd[pfx + k] for k in ("fc1_weights", "fc1_biases", "fc2_weights", "fc2_biases"))


def conformer_layer(x, sd, pfx, H, key_len, ksize, pe=None):
    """ConformerEncoderLayer with attention_type="hypermixing": half FFN, x + LayerNorm(mix(norm1(x))), x + conv module (masked),
    half FFN, norm2.  ``pe``: the mixer's table (default: the sinusoid table in x's dtype, what the module's buffer holds)."""
    import encoder_host_ref as E

    B, T, d = x.shape
    x = _ffn_half(x, sd, pfx + "ffn_module1.")
    m = pfx + "mha_layer."
    pe = sine_table(T, d, torch.float32).to(x.dtype) if pe is None else pe  # (the fp32 buffer is an input in every precision)
    x = hypermix(_ln(x, sd, pfx + "norm1.norm.", 1e-5), key_len, pe, _generator(sd, m + "hyper.w1_gen."),
                 _generator(sd, m + "hyper.w2_gen."), sd[m + "layer_norm.weight"], sd[m + "layer_norm.bias"], 1e-5, H, residual=x)
    c = pfx + "convolution_module."
    h = F.linear(_ln(x, sd, c + "layer_norm.", 1e-5), sd[c + "bottleneck.0.weight"].reshape(2 * d, d), sd[c + "bottleneck.0.bias"])
    h = E.glu_dwconv(h, sd[c + "conv.weight"].reshape(d, ksize), sd[c + "conv.bias"], ksize, 0, x.dtype)
    h = F.linear(F.silu(_ln(h, sd, c + "after_conv.0.", 1e-5)), sd[c + "after_conv.2.weight"], sd[c + "after_conv.2.bias"])
    x = x + h * valid_mask(key_len, B, T, x.dtype)
    return _ln(_ffn_half(x, sd, pfx + "ffn_module2."), sd, pfx + "norm2.norm.", 1e-5)


def conformer_encoder(x, sd, pfx, H, num_layers, key_len, ksize, return_layers=False):
    """ConformerEncoder: the layers and the final LayerNorm (eps 1e-6)."""
    layers = []
    for l in range(num_layers):
        x = conformer_layer(x, sd, f"{pfx}layers.{l}.", H, key_len, ksize)
        layers.append(x)
    out = _ln(x, sd, pfx + "norm.norm.", 1e-6)
    return (out, layers) if return_layers else out


def encode(src, wav_lens, sd, nhead, num_layers, ksize, pfx="", return_layers=False):
    """TransformerASR.encode with encoder_module="conformer", attention_type="hypermixing": nothing is added to src."""
    if src.dim() == 4:
        src = src.reshape(src.shape[0], src.shape[1], -1)
    T = src.shape[1]
    key_len = None if wav_lens is None else torch.round(wav_lens.float() * T).to(torch.int32).clamp(max=T)
    x = F.linear(src, sd[pfx + "custom_src_module.layers.0.w.weight"], sd[pfx + "custom_src_module.layers.0.w.bias"])
    return conformer_encoder(x, sd, pfx + "encoder.", nhead, num_layers, key_len, ksize, return_layers)
