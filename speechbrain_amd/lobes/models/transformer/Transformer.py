"""speechbrain.lobes.models.transformer.Transformer mirror: the pieces TransformerASR is built from
(Transformer.py:35-1068).  The decoder classes are parameter holders with the reference's names;
their arithmetic is the fused KV-cached decode step in csrc/decoder.hip."""
import math
from typing import Optional

import torch
import torch.nn as nn

from speechbrain_amd import native
from speechbrain_amd.nnet.activations import Swish
from speechbrain_amd.nnet.attention import MultiheadAttention, PositionalwiseFeedForward, RelPosEncXL
from speechbrain_amd.nnet.embedding import Embedding
from speechbrain_amd.nnet.normalization import LayerNorm


class PositionalEncoding(nn.Module):
    """Absolute sinusoidal table, buffer ``pe`` [1,max_len,d] (Transformer.py:252-303)."""

    def __init__(self, input_size, max_len=2500):
        super().__init__()
        if input_size % 2 != 0:
            raise ValueError(f"Cannot use sin/cos positional encoding with odd channels (got channels={input_size})")
        self.max_len = max_len
        pe = torch.zeros(self.max_len, input_size, requires_grad=False)
        positions = torch.arange(0, self.max_len).unsqueeze(1).float()
        denominator = torch.exp(torch.arange(0, input_size, 2).float() * -(math.log(10000.0) / input_size))
        pe[:, 0::2] = torch.sin(positions * denominator)
        pe[:, 1::2] = torch.cos(positions * denominator)
        self.register_buffer("pe", pe.unsqueeze(0))

    def forward(self, x):
        return self.pe[:, : x.size(1)].clone().detach()


class NormalizedEmbedding(nn.Module):
    """emb(x) * sqrt(d_model) (Transformer.py:966-995); the scaling is fused into the decode step."""

    def __init__(self, d_model, vocab):
        super().__init__()
        self.emb = Embedding(num_embeddings=vocab, embedding_dim=d_model, blank_id=0)
        self.d_model = d_model


class TransformerEncoderLayer(nn.Module):
    """Transformer.py:306-481 (regularMHA + regularFFN): self_att / pos_ffn / norm1-2 under the reference's names.

    Two users.  TransformerLM reads the parameters only: its arithmetic is the KV-cached step in csrc/search.hip (lm_step).  The
    Transformer ASR encoder (transformer.yaml) runs ``forward``: pre-norm  x + out_proj(MHA(norm1(x))), x + ffn(norm2(x));
    post-norm  norm1(x + out_proj(MHA(x))), norm2(x + ffn(x)) -- LayerNorm written as the next contraction's operand, every
    Linear one MFMA GEMM with bias / activation / residual in its epilogue, the attention one fused kernel
    (native.rope_attention without rotation tables: plain scaled-dot-product attention with key-length masking)."""

    def __init__(self, d_ffn, nhead, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU,
                 normalize_before=False, attention_type="regularMHA", ffn_type="regularFFN",
                 ffn_cnn_kernel_size_list=[3, 3], causal=False):
        super().__init__()
        if attention_type != "regularMHA":
            raise NotImplementedError(f"TransformerEncoderLayer attention_type={attention_type!r}: regularMHA is implemented")
        if ffn_type != "regularFFN":
            raise NotImplementedError(f"TransformerEncoderLayer ffn_type={ffn_type!r}: regularFFN is implemented")
        self.nhead = nhead
        self.self_att = MultiheadAttention(nhead=nhead, d_model=d_model, dropout=dropout, kdim=kdim, vdim=vdim)
        self.pos_ffn = PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout, activation=activation)
        self.norm1 = LayerNorm(d_model, eps=1e-6)
        self.norm2 = LayerNorm(d_model, eps=1e-6)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.normalize_before = normalize_before
        self.causal = causal
        self.collect_attention = False  # attention maps are opt-in (they are [B,H,T,T] of HBM traffic)
        self._in_proj_derived = native.Derived()

    def _in_proj(self):
        """torch's in_proj_weight / in_proj_bias are [q | k | v] by rows; the attention kernels read per-head (q|k|v): the rows
        permuted once to (head, q|k|v, channel)."""
        att = self.self_att.att
        w, b, H = att.in_proj_weight, att.in_proj_bias, self.nhead
        d = w.shape[1]
        return self._in_proj_derived.get((w, b), lambda: (
            w.detach().view(3, H, d // H, d).permute(1, 0, 2, 3).reshape(3 * d, d).contiguous(),
            b.detach().view(3, H, d // H).permute(1, 0, 2).reshape(3 * d).contiguous()))

    def _attend(self, qkv, key_len, out=None):
        """qkv [B,T,3d] per-head interleaved -> (context [B,T,d], head-averaged weights [B,T,T] | None)."""
        H, d = self.nhead, qkv.shape[-1] // 3
        Dh = d // H
        scale = 1.0 / math.sqrt(Dh)
        if not self.collect_attention:
            return native.rope_attention(qkv, None, None, key_len, H, scale, out=out)
        if Dh == 128:
            raise NotImplementedError("collect_attention with head_dim 128: the attention-weights output of the kernel is not "
                                      "instantiated at 128 (the context is)")
        # the weights come from the strip kernel, which takes rotation tables: the identity rotation
        T = qkv.shape[1]
        ones, zeros = torch.ones(T, Dh, device=qkv.device), torch.zeros(T, Dh, device=qkv.device)
        ctx, attn = native.rope_attention(qkv, ones, zeros, key_len, H, scale, want_attn=True, out=out)
        return ctx, attn.mean(1)  # (torch.nn.MultiheadAttention averages its weights over the heads)

    def _check(self, src_mask):
        if self.causal:
            raise NotImplementedError("causal=True (a look-ahead mask in the encoder) is not implemented")
        if src_mask is not None:
            raise NotImplementedError("src_mask (causal / chunked attention masks) is not supported by the Transformer encoder")

    def forward(self, src, src_mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos_embs: Optional[torch.Tensor] = None, key_len=None):
        self._check(src_mask)
        if key_len is None and src_key_padding_mask is not None:
            key_len = (~src_key_padding_mask).sum(-1, dtype=torch.int32)
        B, T, d = src.shape
        out, attn = self._layer(src.contiguous().view(B * T, d), [(0, B, T, key_len, 0)], want_attn=True)
        return out.view(B, T, d), attn

    def forward_group(self, x, segs):
        """``forward`` over several independently padded batches laid end to end (x [M,d], segs = [(row0, B, T, key_len,
        pos0)]): every row-wise launch covers all the batches at once, the attention runs per batch."""
        self._check(None)
        return self._layer(x, segs, want_attn=False)[0]

    def _layer(self, x, segs, want_attn):
        from speechbrain_amd.lobes.models.transformer.Conformer import _norm

        att = self.self_att.att
        w, b = self._in_proj()
        d = x.shape[-1]
        h = _norm(x, self.norm1.norm, w) if self.normalize_before else x
        qkv = native.gemm_nt(h, w, b)
        ctx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        attn = None
        for row0, B, T, key_len, _ in segs:
            _, a = self._attend(qkv[row0: row0 + B * T].view(B, T, 3 * d), key_len, out=ctx[row0: row0 + B * T].view(B, T, d))
            attn = a if want_attn else None
        x = native.gemm_nt(ctx, att.out_proj.weight, att.out_proj.bias, residual=x)
        if not self.normalize_before:
            x = self.norm1(x)
        h = _norm(x, self.norm2.norm, self.pos_ffn.ffn[0].weight) if self.normalize_before else x
        x = self.pos_ffn(h, residual=x)
        if not self.normalize_before:
            x = self.norm2(x)
        return x, attn


class TransformerEncoder(nn.Module):
    """Transformer.py:484-640: N encoder layers + final LayerNorm(eps 1e-6)."""

    def __init__(self, num_layers, nhead, d_ffn, input_shape=None, d_model=None, kdim=None, vdim=None, dropout=0.0,
                 activation=nn.ReLU, normalize_before=False, causal=False, layerdrop_prob=0.0,
                 attention_type="regularMHA", ffn_type="regularFFN", ffn_cnn_kernel_size_list=[3, 3],
                 output_hidden_states=False):
        super().__init__()
        self.layers = nn.ModuleList([
            TransformerEncoderLayer(d_ffn=d_ffn, nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout,
                                    activation=activation, normalize_before=normalize_before, causal=causal,
                                    attention_type=attention_type, ffn_type=ffn_type,
                                    ffn_cnn_kernel_size_list=ffn_cnn_kernel_size_list)
            for _ in range(num_layers)])
        self.norm = LayerNorm(d_model, eps=1e-6)
        self.layerdrop_prob = layerdrop_prob
        self.output_hidden_states = output_hidden_states

    def forward(self, src, src_mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos_embs: Optional[torch.Tensor] = None, dynchunktrain_config=None):
        if dynchunktrain_config is not None:  # (the reference asserts, :622)
            raise NotImplementedError("dynchunktrain_config: Dynamic Chunk Training unsupported for this encoder")
        key_len = None
        if src_key_padding_mask is not None:
            key_len = (~src_key_padding_mask).sum(-1, dtype=torch.int32)
        output = src
        attention_lst = []
        hidden = [output] if self.output_hidden_states else None
        for layer in self.layers:
            output, attention = layer(output, src_mask=src_mask, pos_embs=pos_embs, key_len=key_len)
            attention_lst.append(attention)
            if hidden is not None:
                hidden.append(output)
        output = self.norm(output)
        if hidden is not None:
            return output, attention_lst, hidden
        return output, attention_lst

    def forward_group(self, x, pos2d, segs, dynchunktrain_config=None):
        """The layers + final norm over several independently padded batches laid end to end (see
        TransformerEncoderLayer.forward_group); returns [M,d]."""
        if dynchunktrain_config is not None:
            raise NotImplementedError("dynchunktrain_config: Dynamic Chunk Training unsupported for this encoder")
        for layer in self.layers:
            x = layer.forward_group(x, segs)
        return self.norm(x)


class TransformerDecoderLayer(nn.Module):
    """Transformer.py:659-834 (regularMHA): holder of self_attn / multihead_attn / pos_ffn / norm1-3."""

    def __init__(self, d_ffn, nhead, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU,
                 normalize_before=False, attention_type="regularMHA", causal=None):
        super().__init__()
        if attention_type != "regularMHA":
            raise NotImplementedError("the ASR decoder always uses regularMHA (Transformer.py:232)")
        self.nhead = nhead
        self.self_attn = MultiheadAttention(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout)
        self.multihead_attn = MultiheadAttention(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout)
        self.pos_ffn = PositionalwiseFeedForward(d_ffn=d_ffn, input_size=d_model, dropout=dropout, activation=activation)
        self.norm1 = LayerNorm(d_model, eps=1e-6)
        self.norm2 = LayerNorm(d_model, eps=1e-6)
        self.norm3 = LayerNorm(d_model, eps=1e-6)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.dropout3 = nn.Dropout(dropout)
        self.normalize_before = normalize_before


class TransformerDecoder(nn.Module):
    """Transformer.py:843-963."""

    def __init__(self, num_layers, nhead, d_ffn, d_model, kdim=None, vdim=None, dropout=0.0, activation=nn.ReLU,
                 normalize_before=False, causal=False, attention_type="regularMHA"):
        super().__init__()
        self.layers = nn.ModuleList([
            TransformerDecoderLayer(d_ffn=d_ffn, nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout,
                                    activation=activation, normalize_before=normalize_before, causal=causal,
                                    attention_type=attention_type)
            for _ in range(num_layers)])
        self.norm = LayerNorm(d_model, eps=1e-6)


class TransformerInterface(nn.Module):
    """Transformer.py:35-250: encoder_module="conformer" + RelPosMHAXL | RoPEMHA | hypermixing, encoder_module="branchformer" +
    RelPosMHAXL or encoder_module="transformer" + regularMHA (TransformerASR: the transformer.yaml recipe; TransformerLM)."""

    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, num_decoder_layers=6, d_ffn=2048, dropout=0.1,
                 activation=nn.ReLU, custom_src_module=None, custom_tgt_module=None,
                 positional_encoding="fixed_abs_sine", normalize_before=True, kernel_size: int = 31, bias: bool = True,
                 encoder_module: str = "transformer", conformer_activation=Swish, branchformer_activation=nn.GELU,
                 attention_type: str = "regularMHA", max_length: int = 2500, causal: bool = False,
                 encoder_kdim: Optional[int] = None, encoder_vdim: Optional[int] = None,
                 decoder_kdim: Optional[int] = None, decoder_vdim: Optional[int] = None, csgu_linear_units: int = 3072,
                 gate_activation=nn.Identity, use_linear_after_conv: bool = False, output_hidden_states=False,
                 layerdrop_prob=0.0):
        super().__init__()
        from speechbrain_amd.lobes.models.transformer.Conformer import ConformerEncoder

        self.causal, self.attention_type = causal, attention_type
        self.positional_encoding_type = positional_encoding
        self.output_hidden_states, self.layerdrop_prob = output_hidden_states, layerdrop_prob
        assert positional_encoding in ["fixed_abs_sine", None]
        assert num_encoder_layers + num_decoder_layers > 0
        lm_like = encoder_module == "transformer" and attention_type == "regularMHA"
        branchformer = encoder_module == "branchformer"
        if branchformer:
            if attention_type != "RelPosMHAXL":
                raise NotImplementedError(f"encoder_module='branchformer' with attention_type='{attention_type}': RelPosMHAXL "
                                          "is implemented (regularMHA and hypermixing are not)")
            if use_linear_after_conv:
                raise NotImplementedError("encoder_module='branchformer' with use_linear_after_conv=True is not implemented")
            if causal:
                raise NotImplementedError("encoder_module='branchformer' with causal=True is not implemented")
        elif not lm_like and (encoder_module != "conformer" or attention_type not in ("RelPosMHAXL", "RoPEMHA", "hypermixing")
                              or causal):
            if attention_type == "hypermixing" and encoder_module == "transformer":
                raise NotImplementedError("encoder_module='transformer' with attention_type='hypermixing' is not implemented: "
                                          "hypermixing runs in encoder_module='conformer'")
            if attention_type == "hypermixing" and encoder_module == "conformer":
                raise NotImplementedError("attention_type='hypermixing' with causal=True is not implemented")
            raise NotImplementedError(
                "implemented: encoder_module='conformer' with attention_type='RelPosMHAXL' | 'RoPEMHA' | 'hypermixing', "
                "causal=False and encoder_module='branchformer' with attention_type='RelPosMHAXL' (ASR); "
                "encoder_module='transformer' with attention_type='regularMHA' (TransformerLM)")
        if positional_encoding == "fixed_abs_sine":
            self.positional_encoding = PositionalEncoding(d_model, max_length)
        if attention_type == "RelPosMHAXL":
            self.positional_encoding = RelPosEncXL(d_model)  # overrides, as in the reference (:165-170)
            self.positional_encoding_decoder = PositionalEncoding(d_model, max_length)
        if attention_type == "RoPEMHA":  # Transformer.py:171-174
            self.positional_encoding_decoder = PositionalEncoding(d_model, max_length)
        if lm_like and num_decoder_layers > 0 and not normalize_before:
            raise NotImplementedError("normalize_before=False with decoder layers: the KV-cached decode step implements the "
                                      "pre-norm decoder (a post-norm encoder alone, num_decoder_layers=0, is implemented)")
        if num_encoder_layers > 0 and lm_like:
            if custom_src_module is not None:
                self.custom_src_module = custom_src_module(d_model)
            self.encoder = TransformerEncoder(nhead=nhead, num_layers=num_encoder_layers, d_ffn=d_ffn, d_model=d_model,
                                              dropout=dropout, activation=activation,
                                              normalize_before=normalize_before, causal=causal,
                                              attention_type=attention_type, kdim=encoder_kdim, vdim=encoder_vdim,
                                              output_hidden_states=output_hidden_states,
                                              layerdrop_prob=layerdrop_prob)
        elif num_encoder_layers > 0 and branchformer:  # Transformer.py:213-227
            from speechbrain_amd.lobes.models.transformer.Branchformer import BranchformerEncoder

            self.encoder = BranchformerEncoder(nhead=nhead, num_layers=num_encoder_layers, d_model=d_model, dropout=dropout,
                                               activation=branchformer_activation, kernel_size=kernel_size,
                                               attention_type=attention_type, csgu_linear_units=csgu_linear_units,
                                               gate_activation=gate_activation,
                                               use_linear_after_conv=use_linear_after_conv,
                                               output_hidden_states=output_hidden_states, layerdrop_prob=layerdrop_prob)
        elif num_encoder_layers > 0:
            self.encoder = ConformerEncoder(nhead=nhead, num_layers=num_encoder_layers, d_ffn=d_ffn, d_model=d_model,
                                            dropout=dropout, activation=conformer_activation, kernel_size=kernel_size,
                                            bias=bias, causal=causal, attention_type=attention_type,
                                            output_hidden_states=output_hidden_states, layerdrop_prob=layerdrop_prob)
            assert normalize_before, "normalize_before must be True for Conformer"
        if num_decoder_layers > 0:
            self.decoder = TransformerDecoder(num_layers=num_decoder_layers, nhead=nhead, d_ffn=d_ffn, d_model=d_model,
                                              dropout=dropout, activation=activation,
                                              normalize_before=normalize_before, causal=True,
                                              attention_type="regularMHA")


def get_lookahead_mask(padded_input):
    """Transformer.py:1037-1068 (kept for API completeness; the decode kernels are causal by construction)."""
    seq_len = padded_input.shape[1]
    mask = (torch.triu(torch.ones((seq_len, seq_len), device=padded_input.device)) == 1).transpose(0, 1)
    return mask.float().masked_fill(mask == 0, float("-inf")).masked_fill(mask == 1, 0.0).detach()


def get_key_padding_mask(padded_input, pad_idx):
    """Transformer.py:998-1034."""
    if len(padded_input.shape) == 4:
        bz, time, ch1, ch2 = padded_input.shape
        padded_input = padded_input.reshape(bz, time, ch1 * ch2)
    key_padded_mask = padded_input.eq(pad_idx)
    if len(padded_input.shape) > 2:
        key_padded_mask = key_padded_mask.float().prod(dim=-1).bool()
    return key_padded_mask.detach()
