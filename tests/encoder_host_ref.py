"""Plain torch compositions of the encoder's attention (csrc/relpos_attn.hip) and GLU + depthwise convolution
(csrc/convmodule.hip) -- the references of tests/test_encoder_kernels.py.

Dtype-generic: the same code gives the fp64 reference and the fp32 composition whose own error sets the bound.  Nothing here
shares an indexing idea with the kernels: the relative-position term is gathered with an explicit index table (no pad-and-view
shift), the chunk mask is a boolean [B,T,T] table, the convolution is a loop over taps."""
import torch
import torch.nn.functional as F


def allowed_keys(B, T, lens, chunk, left):
    """[B,T,T] bool: may query i of utterance b see key j?  Keys [0, lens[b]); with ``chunk`` > 0 query i (chunk c = i // chunk)
    sees [max(0, (c - left) * chunk), (c + 1) * chunk), ``left`` < 0 = unlimited left context."""
    klen = torch.full((B,), T) if lens is None else torch.tensor(list(lens))
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    ok = (j[None] < klen[:, None, None]).expand(B, T, T).clone()
    if chunk > 0:
        c = i // chunk
        ok &= (j < (c + 1) * chunk)[None]
        if left >= 0:
            ok &= (j >= ((c - left) * chunk).clamp(min=0))[None]
    return ok


def rel_index(T):
    """[T,T] row of the position table that the pair (query i, key j) reads: T - 1 - i + j."""
    return (T - 1) - torch.arange(T)[:, None] + torch.arange(T)[None, :]


def bf16_round(x):
    return x.float().bfloat16().to(x.dtype)


def _attend(qkv, H, Dh, lens, chunk, left, scale, dtype, pos, bias_u, bias_v, rope, rnd, index, allowed):
    B, T, _ = qkv.shape
    q, k, v = [t.transpose(1, 2) for t in qkv.to(dtype).reshape(B, T, H, 3, Dh).unbind(3)]  # [B,H,T,Dh]
    if rope is not None:  # x'[c] = x[c] cos[t][c] + x[c ^ 1] sin[t][c] (signed sines)
        cos, sin = rope[0][:T].to(dtype), rope[1][:T].to(dtype)
        swap = torch.arange(Dh) ^ 1
        q, k = q * cos + q[..., swap] * sin, k * cos + k[..., swap] * sin
    if pos is not None:
        u, w = bias_u.to(dtype).reshape(1, H, 1, Dh), bias_v.to(dtype).reshape(1, H, 1, Dh)
        p = pos.to(dtype).reshape(2 * T - 1, H, Dh).permute(1, 2, 0)  # [H,Dh,2T-1]
        bd = torch.matmul((q + w) * scale, p)  # [B,H,T,2T-1]: every query against every position row
        idx = rel_index(T) if index is None else index
        sc = torch.matmul((q + u) * scale, k.transpose(-1, -2)) + bd.gather(-1, idx.expand(B, H, T, T))
    else:
        qs = q * scale
        if rnd is not None:
            qs, k = rnd(qs), rnd(k)
        sc = torch.matmul(qs, k.transpose(-1, -2))
    ok = (allowed_keys(B, T, lens, chunk, left) if allowed is None else allowed)[:, None]  # [B,1,T,T]
    seen = ok.any(-1, keepdim=True)
    sc = sc.masked_fill(~ok, float("-inf"))
    m = torch.where(seen, sc.amax(-1, keepdim=True), torch.zeros((), dtype=dtype))
    e = torch.exp(sc - m)  # (exp(-inf) = 0 on the keys that are not allowed)
    norm = e.sum(-1, keepdim=True)
    norm = torch.where(seen, norm, torch.ones((), dtype=dtype))  # a query without an allowed key: zero weights, zero context
    if rnd is not None:  # rounded operands of the second product, the normaliser from the unrounded probabilities
        ctx = torch.matmul(rnd(e), rnd(v)) / norm
    else:
        ctx = torch.matmul(e / norm, v)
    return ctx.transpose(1, 2).reshape(B, T, H * Dh), e / norm


def attention(qkv, H, Dh, lens, chunk, left, scale, dtype, pos=None, bias_u=None, bias_v=None, rope=None, *, index=None,
              allowed=None):
    """qkv [B,T,H,(q|k|v)] -> (context [B,T,H*Dh], probabilities [B,H,T,T]) in ``dtype``.

    ``pos`` [2T-1, H*Dh] (already projected) with ``bias_u`` / ``bias_v`` [H*Dh]: the score is
    ((q + u) . k + (q + v) . pos[T-1-i+j]) * scale.  ``rope`` = (cos, sin) [>= T, Dh]: q and k are rotated.  Neither: plain
    attention.  ``index`` / ``allowed`` replace rel_index() / allowed_keys() (the sensitivity test's perturbations)."""
    return _attend(qkv, H, Dh, lens, chunk, left, scale, dtype, pos, bias_u, bias_v, rope, None, index, allowed)


def attention_bf16_model(qkv, H, Dh, lens, chunk, left, scale, rope=None):
    """The same attention in fp64 arithmetic with the roundings of rope_flash_t_bf16_kernel made explicit: q * scale (after the
    rotation), k (after the rotation) and v are rounded to bf16, the unnormalised probabilities exp(s - max) are rounded to bf16
    before the product with v, the normaliser is the sum of the unrounded probabilities.  Context only."""
    return _attend(qkv, H, Dh, lens, chunk, left, scale, torch.float64, None, None, None, rope, bf16_round, None, None)[0]


def glu_dwconv(h, w, bias, ksize, chunk, dtype):
    """h [B,T,2d], w [d,ksize], bias [d] -> y [B,T,d]: g = GLU(h), y[t] = bias + sum_k w[:,k] g[t + k - halo] over the taps with
    0 <= t + k - halo < end(t); end(t) = T without chunks, else min(T, (t // chunk + 1) * chunk)."""
    B, T, d2 = h.shape
    halo = (ksize - 1) // 2
    g = F.glu(h.to(dtype), dim=-1)
    w, t = w.to(dtype), torch.arange(T)
    end = torch.full((T,), T) if chunk == 0 else ((t // chunk + 1) * chunk).clamp(max=T)
    y = bias.to(dtype).expand(B, T, d2 // 2).clone()
    for k in range(ksize):
        src = t + k - halo
        ok = (src >= 0) & (src < end)
        y[:, ok] += w[:, k] * g[:, src[ok]]
    return y
