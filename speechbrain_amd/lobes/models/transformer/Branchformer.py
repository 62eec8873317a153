"""speechbrain.lobes.models.transformer.Branchformer mirror (Branchformer.py:23-409): offline encoder.

ConvolutionBranch / BranchformerEncoderLayer / BranchformerEncoder keep the reference's constructors, forward signatures
and state_dict keys.  A layer is  x + merge_proj(cat[MHA(norm_mhsa(x)), cgMLP(norm_conv(x))]):  both LayerNorms are one
row kernel each, every Linear one MFMA GEMM with bias + activation (+ residual) in the epilogue, attention one fused
kernel and the Convolutional Spatial Gating Unit one fused kernel after its statistics pass (csrc/csgu.hip).  The
concatenation is never materialised: merge_proj.weight is split by columns and the two halves accumulate into the
residual (x + A Wa^T + b, then + C Wb^T).
"""
from typing import Optional

import torch
import torch.nn as nn

from speechbrain_amd import native
from speechbrain_amd.lobes.models.convolution import ConvolutionalSpatialGatingUnit
from speechbrain_amd.lobes.models.transformer.Conformer import _norm
from speechbrain_amd.nnet.attention import RelPosMHAXL, _act_code
from speechbrain_amd.nnet.normalization import LayerNorm


class ConvolutionBranch(nn.Module):
    """Channel Proj -> GELU -> CSGU -> Channel Proj (Branchformer.py:23-89); the LayerNorm in front is the layer's."""

    def __init__(self, input_size, linear_units=3072, kernel_size=31, activation=nn.GELU, gate_activation=nn.Identity,
                 dropout=0.0, use_linear_after_conv=False):
        super().__init__()
        self.pre_channel_proj = nn.Linear(input_size, linear_units)
        self.post_channel_proj = nn.Linear(linear_units // 2, input_size)
        self.activation = activation()
        self.act_code = _act_code(self.activation)
        self.csgu = ConvolutionalSpatialGatingUnit(input_size=linear_units, kernel_size=kernel_size, dropout=dropout,
                                                   use_linear_after_conv=use_linear_after_conv, activation=gate_activation)

    def forward(self, x):
        """x [B,T,D] (fp32 rows or the panel image written by the LayerNorm in front) -> [B,T,D]."""
        h = native.gemm_nt(x, self.pre_channel_proj.weight, self.pre_channel_proj.bias, act=self.act_code)
        return native.gemm_nt(self.csgu(h), self.post_channel_proj.weight, self.post_channel_proj.bias)

    def forward_group(self, x, segs):
        """``forward`` over several independently padded batches laid end to end (x [M,D], segs = [(row0, B, T, key_len,
        pos0)]): the projections run once over all rows, the CSGU -- whose reflect padding is each batch's own -- per batch."""
        h = native.gemm_nt(x, self.pre_channel_proj.weight, self.pre_channel_proj.bias, act=self.act_code)
        C2 = h.shape[-1]
        g = torch.empty(h.shape[0], C2 // 2, dtype=torch.float32, device=h.device)
        for row0, B, T, _, _ in segs:
            self.csgu(h[row0: row0 + B * T].view(B, T, C2), out=g[row0: row0 + B * T].view(B, T, C2 // 2))
        return native.gemm_nt(g, self.post_channel_proj.weight, self.post_channel_proj.bias)


class BranchformerEncoderLayer(nn.Module):
    """Branchformer.py:92-234: x + merge_proj(cat[MHA(norm_mhsa(x)), ConvolutionBranch(norm_conv(x))])."""

    def __init__(self, d_model, nhead, kernel_size=31, kdim=None, vdim=None, activation=nn.GELU, dropout=0.0,
                 attention_type="RelPosMHAXL", csgu_linear_units=3072, gate_activation=nn.Identity,
                 use_linear_after_conv=False):
        super().__init__()
        if attention_type != "RelPosMHAXL":
            raise NotImplementedError(f"Branchformer with attention_type={attention_type}: RelPosMHAXL is implemented "
                                      "(regularMHA and hypermixing are not)")
        self.mha_layer = RelPosMHAXL(num_heads=nhead, embed_dim=d_model, dropout=dropout, mask_pos_future=False)
        self.convolution_branch = ConvolutionBranch(input_size=d_model, kernel_size=kernel_size,
                                                    linear_units=csgu_linear_units, activation=activation,
                                                    gate_activation=gate_activation, dropout=dropout,
                                                    use_linear_after_conv=use_linear_after_conv)
        self.merge_proj = nn.Linear(d_model * 2, d_model)
        self.norm_mhsa = LayerNorm(d_model)
        self.norm_conv = LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)
        self.collect_attention = False  # attention maps are opt-in (they are [B,H,T,T] of HBM traffic)
        self._merge_derived = native.Derived()

    def _merge_halves(self):
        """merge_proj.weight [d,2d] as its two column halves, contiguous: the contraction over cat[x1, x2] is x1 Wa^T + x2 Wb^T."""
        w, d = self.merge_proj.weight, self.merge_proj.weight.shape[0]
        return self._merge_derived.get((w,), lambda: (w.detach()[:, :d].contiguous(), w.detach()[:, d:].contiguous()))

    def _merge(self, x, x1, x2):
        wa, wb = self._merge_halves()
        return native.gemm_nt(x2, wb, None, residual=native.gemm_nt(x1, wa, self.merge_proj.bias, residual=x))

    def forward(self, x, src_mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos_embs: Optional[torch.Tensor] = None, key_len=None):
        if src_mask is not None:
            raise NotImplementedError("src_mask (causal / chunked attention masks) is not supported by the Branchformer")
        if key_len is None and src_key_padding_mask is not None:
            key_len = (~src_key_padding_mask).sum(-1, dtype=torch.int32)
        x = x.contiguous()
        h = _norm(x, self.norm_mhsa.norm, self.mha_layer.in_proj_weight)
        x1, attn = self.mha_layer.core(h, pos_embs.reshape(-1, x.shape[-1]), key_len, want_attn=self.collect_attention)
        # the cgMLP branch runs unmasked, as in the reference (Branchformer.py:224-228): padded frames reach real ones
        x2 = self.convolution_branch(_norm(x, self.norm_conv.norm, self.convolution_branch.pre_channel_proj.weight))
        return self._merge(x, x1, x2), attn

    def forward_group(self, x, pos2d, segs):
        """``forward`` over several independently padded batches laid end to end (x [M,d], pos2d the batches' position tables
        end to end, segs = [(row0, B, T, key_len, pos0)]): every row-wise launch covers all the batches at once, only the
        kernels that see the time axis (attention, CSGU) run per batch."""
        h = _norm(x, self.norm_mhsa.norm, self.mha_layer.in_proj_weight)
        x1 = self.mha_layer.core_group(h, pos2d, segs)
        x2 = self.convolution_branch.forward_group(
            _norm(x, self.norm_conv.norm, self.convolution_branch.pre_channel_proj.weight), segs)
        return self._merge(x, x1, x2)


class BranchformerEncoder(nn.Module):
    """Branchformer.py:237-409: N layers + final LayerNorm(eps 1e-6)."""

    def __init__(self, num_layers, d_model, nhead, kernel_size=31, kdim=None, vdim=None, activation=nn.GELU, dropout=0.0,
                 attention_type="RelPosMHAXL", csgu_linear_units=3072, gate_activation=nn.Identity,
                 use_linear_after_conv=False, output_hidden_states=False, layerdrop_prob=0.0):
        super().__init__()
        self.layers = nn.ModuleList([
            BranchformerEncoderLayer(nhead=nhead, d_model=d_model, kdim=kdim, vdim=vdim, dropout=dropout,
                                     activation=activation, kernel_size=kernel_size, attention_type=attention_type,
                                     csgu_linear_units=csgu_linear_units, gate_activation=gate_activation,
                                     use_linear_after_conv=use_linear_after_conv)
            for _ in range(num_layers)])
        self.norm = LayerNorm(d_model, eps=1e-6)
        self.layerdrop_prob = layerdrop_prob
        self.attention_type = attention_type
        self.output_hidden_states = output_hidden_states

    def forward(self, src, src_mask: Optional[torch.Tensor] = None, src_key_padding_mask: Optional[torch.Tensor] = None,
                pos_embs: Optional[torch.Tensor] = None, dynchunktrain_config=None):
        if dynchunktrain_config is not None:
            raise NotImplementedError("Dynamic Chunk Training unsupported for this encoder")  # (the reference asserts, :369)
        if pos_embs is None:
            raise ValueError("The chosen attention type for the Branchformer is RelPosMHAXL. For this attention type, the "
                             "positional embeddings are mandatory")
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
        BranchformerEncoderLayer.forward_group); returns [M,d]."""
        if dynchunktrain_config is not None:
            raise NotImplementedError("Dynamic Chunk Training unsupported for this encoder")
        if pos2d is None:
            raise ValueError("RelPosMHAXL needs positional embeddings")
        for layer in self.layers:
            x = layer.forward_group(x, pos2d, segs)
        return self.norm(x)
