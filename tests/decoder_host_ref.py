"""Plain-torch restatement of the pre-norm Transformer decoder of TransformerASR.decode -- tests only.

Written from the reference's TransformerDecoderLayer.forward (lobes/models/transformer/Transformer.py:751-834, normalize_before):

    x  = emb[token] * emb_scale + pe[position]                                  (NormalizedEmbedding, PositionalEncoding)
    x += out_proj(softmax(q k^T / sqrt(dh), causal) v),   q, k, v = in_proj(norm1(x))
    x += out_proj(softmax(q k^T / sqrt(dh), frames < enc_len) v),  q = in_proj[:d](norm2(x)),  k, v = in_proj[d:](memory)
    x += ffn.3(act(ffn.0(norm3(x))))
    h  = decoder.norm(x);   logits = seq(h)

It takes the plain tensors native.DecoderHandle.from_tensors takes and imports nothing from the kernels' code.  Every operation is
the textbook one (a LayerNorm is mean / biased variance / affine, a softmax subtracts the row maximum) in float64 -- the
reference the kernels are held to -- or, ``fp32=True``, the IDENTICAL composition in float32: what one more fp32 evaluation of
the same function costs, the yardstick the tests size their tolerances by."""
import math

import torch

ACT_NONE, ACT_SWISH, ACT_GELU, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2, 3, 4  # include/sbk.h: SBK_ACT_*


def _act(x, code):
    if code == ACT_SWISH:
        return x * torch.sigmoid(x)
    if code == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if code == ACT_RELU:
        return torch.clamp(x, min=0.0)
    if code == ACT_LEAKY_RELU:
        return torch.where(x > 0, x, 0.01 * x)
    assert code == ACT_NONE, code
    return x


def _layer_norm(x, gb, eps):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gb[0] + gb[1]


def _linear(x, wb):
    return x @ wb[0].transpose(0, 1) + wb[1]


def _attention(q, k, v, nhead, mask):
    """q [n,Lq,d], k / v [n,Lk,d], mask [n,Lq,Lk] bool (True = attend) -> [n,Lq,d]."""
    n, Lq, d = q.shape
    dh = d // nhead
    q, k, v = (t.reshape(n, t.shape[1], nhead, dh).permute(0, 2, 1, 3) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(~mask[:, None], float("-inf"))
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    return (p @ v).permute(0, 2, 1, 3).reshape(n, Lq, d)


class Decoder:
    def __init__(self, layers, emb, pe, final_ln, seq, nhead, ffn_act, ln_eps, emb_scale, fp32=False):
        self.dtype = torch.float32 if fp32 else torch.float64
        cast = lambda t: t.detach().cpu().to(self.dtype)
        self.layers = [{k: tuple(cast(t) for t in v) for k, v in L.items()} for L in layers]
        self.emb, self.pe = cast(emb), cast(pe)
        self.final_ln = tuple(cast(t) for t in final_ln)
        self.seq = tuple(cast(t) for t in seq) if seq is not None else None
        self.nhead, self.act, self.eps = nhead, ffn_act, ln_eps
        self.d = self.emb.shape[1]
        self.emb_scale = emb_scale if emb_scale > 0 else math.sqrt(self.d)  # (sbk.h: 0 = sqrt(d_model))

    def decode(self, tokens, enc, enc_len):
        """Teacher forced: tokens [n,L], enc [n,T,d], enc_len [n] (frames each row attends to) -> decoder.norm output [n,L,d]."""
        tokens, enc_len = torch.as_tensor(tokens).cpu().long(), torch.as_tensor(enc_len).cpu().long()
        enc = enc.detach().cpu().to(self.dtype)
        n, L = tokens.shape
        T, d = enc.shape[1], self.d
        x = self.emb[tokens] * self.emb_scale + self.pe[:L]
        causal = torch.ones(L, L, dtype=torch.bool).tril()[None].expand(n, L, L)
        frames = (torch.arange(T)[None, :] < enc_len[:, None])[:, None, :].expand(n, L, T)
        for P in self.layers:
            qkv = _linear(_layer_norm(x, P["ln1"], self.eps), P["sa_in"])
            x = x + _linear(_attention(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], self.nhead, causal), P["sa_out"])
            w, b = P["ca_in"]
            q = _linear(_layer_norm(x, P["ln2"], self.eps), (w[:d], b[:d]))
            kv = _linear(enc, (w[d:], b[d:]))
            x = x + _linear(_attention(q, kv[..., :d], kv[..., d:], self.nhead, frames), P["ca_out"])
            x = x + _linear(_act(_linear(_layer_norm(x, P["ln3"], self.eps), P["ff1"]), self.act), P["ff2"])
        return _layer_norm(x, self.final_ln, self.eps)

    def logits(self, h):
        return _linear(h, self.seq)

    def log_probs(self, tokens, enc, enc_len):
        """log_softmax(seq(decode(...))) [n,L,V]."""
        z = self.logits(self.decode(tokens, enc, enc_len))
        z = z - z.max(-1, keepdim=True).values
        return z - torch.log(torch.exp(z).sum(-1, keepdim=True))

    def rescore(self, tokens, enc, enc_len, bos=1):
        """tokens [n,L]: the sequences a search returned (without <bos>).  -> [n,L]: log-prob of tokens[:, t] given <bos>,
        tokens[:, :t] -- what the search accumulated for that hypothesis if every step read the hypothesis' own history."""
        tokens = torch.as_tensor(tokens).cpu().long()
        inp = torch.cat([torch.full_like(tokens[:, :1], bos), tokens[:, :-1]], dim=1)
        return self.log_probs(inp, enc, enc_len).gather(-1, tokens[..., None])[..., 0]
