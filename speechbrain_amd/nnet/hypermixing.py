"""speechbrain.nnet.hypermixing mirror: HyperMixing (the HyperConformer recipes' token mixer), HyperNetwork, ParallelMLPs.

Constructors, parameter names and shapes and the ``positional_encoding.pe`` buffer are the reference's, so its checkpoints load
with ``strict=True``.  The computation is one fused call (``native.hypermix``, csrc/hypermix.hip): the two generated weight
tensors [B,H,T,hypernet_size/H] of the reference's composition are never formed.  Only the untied multi-head form with a
per-head hidden width (``tied=False``, ``fix_tm_hidden_size=False``: what ConformerEncoderLayer constructs) is implemented.
"""
import math
from typing import Optional

import torch
import torch.nn as nn

from speechbrain_amd import native


class ParallelMLPs(nn.Module):
    """``num_mlps`` two-layer MLPs side by side, one per head: holder of fc1_weights [H, hidden/H, in/H], fc1_biases
    [H, hidden/H], fc2_weights [H, out(/H), hidden/H], fc2_biases [H, out(/H)].  The fused mixer reads the parameters; the
    module has no forward of its own (its output is the tensor the kernel exists not to write)."""

    def __init__(self, input_size, hidden_size, output_size=None, num_mlps=1, keep_output_size=True):
        super().__init__()
        if output_size is None:
            output_size = input_size
        self.original_in_size, self.original_out_size = input_size, output_size
        if input_size % num_mlps or output_size % num_mlps or hidden_size % num_mlps:
            raise ValueError(f"ParallelMLPs: sizes {input_size}, {hidden_size}, {output_size} must be divisible by "
                             f"num_mlps={num_mlps}")
        if keep_output_size:
            raise NotImplementedError("ParallelMLPs keep_output_size=True (HyperMixing fix_tm_hidden_size=True) is not "
                                      "implemented: no recipe uses it")
        self.input_size, self.output_size, self.num_mlps = input_size // num_mlps, output_size // num_mlps, num_mlps
        hidden = hidden_size // num_mlps
        self.fc1_weights = nn.Parameter(torch.empty(num_mlps, hidden, self.input_size))
        self.fc1_biases = nn.Parameter(torch.empty(num_mlps, hidden))
        self.fc2_weights = nn.Parameter(torch.empty(num_mlps, self.output_size, hidden))
        self.fc2_biases = nn.Parameter(torch.empty(num_mlps, self.output_size))
        for p in (self.fc1_weights, self.fc1_biases, self.fc2_weights, self.fc2_biases):
            nn.init.xavier_uniform_(p, gain=math.sqrt(2.0))
        self.activation = nn.GELU()

    def tensors(self):
        """The generator as native.hypermix takes it."""
        return self.fc1_weights, self.fc1_biases, self.fc2_weights, self.fc2_biases

    def forward(self, x):
        raise NotImplementedError("ParallelMLPs.forward: the generated weights are not materialised; HyperMixing.forward "
                                  "runs the fused kernel on this module's parameters")


class HyperNetwork(nn.Module):
    """The two weight generators ``w1_gen`` / ``w2_gen`` of a token-mixing MLP."""

    def __init__(self, input_output_dim, hypernet_size, tied=False, num_heads=1, keep_output_size=True):
        super().__init__()
        if tied:
            raise NotImplementedError("HyperNetwork tied=True is not implemented: no recipe uses it")
        self.tied = tied
        self.w1_gen = ParallelMLPs(input_output_dim, input_output_dim, output_size=hypernet_size, num_mlps=num_heads,
                                   keep_output_size=keep_output_size)
        self.w2_gen = ParallelMLPs(input_output_dim, input_output_dim, output_size=hypernet_size, num_mlps=num_heads,
                                   keep_output_size=keep_output_size)

    def forward(self, input_tensor):
        raise NotImplementedError("HyperNetwork.forward: the generated weights are not materialised; HyperMixing.forward "
                                  "runs the fused kernel on this module's parameters")


class HyperMixing(nn.Module):
    """Multi-head HyperMixing with the call surface of the attention modules: ``forward(query, ...)`` mixes ``query`` over
    time (key, value, attn_mask and pos_embs have no effect, as in the reference) and returns ``(LayerNorm(mix), None)`` --
    the reference's second value is an all-zero [B,T,T]; attention maps are opt-in here and this module has none."""

    def __init__(self, input_output_dim, hypernet_size, tied=False, num_heads=1, fix_tm_hidden_size=False, max_length=3000):
        super().__init__()
        if tied:
            raise NotImplementedError("HyperMixing tied=True is not implemented: no recipe uses it")
        if fix_tm_hidden_size:
            raise NotImplementedError("HyperMixing fix_tm_hidden_size=True is not implemented: no recipe uses it")
        from speechbrain_amd.lobes.models.transformer.Transformer import PositionalEncoding

        self.input_output_dim, self.num_heads, self.max_length = input_output_dim, num_heads, max_length
        self.hyper = HyperNetwork(input_output_dim, hypernet_size, tied=tied, num_heads=num_heads,
                                  keep_output_size=fix_tm_hidden_size)
        self.activation = nn.GELU()
        self.layer_norm = nn.LayerNorm(input_output_dim)
        self.positional_encoding = PositionalEncoding(input_output_dim, max_length)

    def core(self, h, key_len, residual=None, out=None):
        """LayerNorm(mix(h)) + residual for h [B,T,d] with key_len int32 [B] (or None) valid frames per utterance."""
        T = h.shape[1]
        if T > self.max_length:
            raise ValueError(f"HyperMixing: {T} frames exceed max_length={self.max_length} (the position table's rows)")
        ln = self.layer_norm
        return native.hypermix(h, key_len, self.positional_encoding.pe[0], self.hyper.w1_gen.tensors(),
                               self.hyper.w2_gen.tensors(), ln.weight, ln.bias, ln.eps, self.num_heads, residual=residual,
                               out=out)

    def forward(self, query, key=None, value=None, attn_mask: Optional[torch.Tensor] = None,
                key_padding_mask: Optional[torch.Tensor] = None, return_attn_weights: Optional[bool] = True,
                pos_embs: Optional[torch.Tensor] = None):
        key_len = None
        if key_padding_mask is not None:  # True = padded; lengths are what the kernels take (padding is a suffix)
            key_len = torch.logical_not(key_padding_mask.bool()).sum(-1, dtype=torch.int32)
        return self.core(query.contiguous(), key_len), None
