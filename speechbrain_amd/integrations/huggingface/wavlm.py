"""speechbrain.integrations.huggingface.wavlm mirror: the WavLM encoder of the CTC recipes
(recipes/LibriSpeech/ASR/CTC/hparams/downsampled/train_hf_wavlm_*.yaml) on the MI355X kernels.

The reference's ``WavLM`` is its ``Wav2Vec2`` wrapper around HuggingFace's ``WavLMModel`` (wavlm.py:21-88).  Here it is the
wav2vec 2.0 mirror (wav2vec2.py: feature encoder, projection, positional convolution, GEMM epilogues, loader) with WavLM's
parameter tree -- ``gru_rel_pos_const`` [1,H,1,1] and ``gru_rel_pos_linear`` in every layer's attention, ``rel_attn_embed``
[num_buckets,H] in layer 0 only -- and ONE different step: the self-attention adds the gated relative-position bias
gate(x)[b,h,i] * rel_attn_embed[bucket(j - i), h] to every score.  HuggingFace materialises that bias as [B*H,T',T'] per layer;
``native.wavlm_attention`` (csrc/wavlm.hip) takes the [H,2T'-1] table (``native.wavlm_bias_table``, built once per T' from layer
0's embedding and shared by every layer) and the hidden states, and forms nothing T' x T'.  ``transformers`` is not imported.
fp32 only."""
import torch
from torch import nn

from speechbrain_amd import native
from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2, Wav2Vec2Model, _Attention, _checked_config


class _GatedAttention(_Attention):
    """HuggingFace's WavLMAttention as a parameter holder (its parameters in its order)."""

    def __init__(self, d, heads, num_buckets, max_distance, has_relative_position_bias):
        super().__init__(d, heads)
        self.num_buckets, self.max_distance = num_buckets, max_distance
        self.gru_rel_pos_const = nn.Parameter(torch.ones(1, heads, 1, 1))
        self.gru_rel_pos_linear = nn.Linear(self.head_dim, 8)
        if has_relative_position_bias:
            self.rel_attn_embed = nn.Embedding(num_buckets, heads)
            self._table = native.Derived()

    def bias_table(self, T):
        """[H, 2T-1]: entry [h, r + T - 1] = rel_attn_embed[bucket(r), h] for r = key - query."""
        return native.wavlm_bias_table(self.rel_attn_embed.weight, T, self.num_buckets, self.max_distance, derived=self._table)


class WavLMModel(Wav2Vec2Model):
    """The parameter tree of HuggingFace's WavLMModel and its forward on the kernels: group-norm / post-norm (base, base-plus)
    and layer-norm / stable layer norm (large)."""

    def check_config(self, cfg):
        cfg = {"num_buckets": 320, "max_bucket_distance": 800, **cfg}
        if cfg["num_buckets"] < 4:  # (half per sign, half of those exact: below 4 the logarithmic range divides by zero)
            raise ValueError(f"WavLM num_buckets={cfg['num_buckets']}: at least 4")
        return _checked_config(cfg, "WavLM", native.WAVLM_HEAD_DIMS)

    def new_attention(self, cfg, layer):
        return _GatedAttention(cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_buckets"], cfg["max_bucket_distance"],
                               has_relative_position_bias=layer == 0)

    def attend(self, att, a, qkv, key_len):
        tab = self.encoder.layers[0].attention.bias_table(qkv.shape[1])  # (cached: one table per T' serves every layer)
        g = att.gru_rel_pos_linear
        return native.wavlm_attention(qkv, a, g.weight, g.bias, att.gru_rel_pos_const, tab, key_len, att.num_heads,
                                      att.head_dim ** -0.5)


class WavLM(Wav2Vec2):
    """speechbrain.integrations.huggingface.wavlm.WavLM on the MI355X kernels: the constructor, ``forward`` /
    ``extract_features``, ``output_norm`` and ``output_all_hiddens`` of the wav2vec 2.0 wrapper, for a LOCAL HuggingFace
    directory whose config.json says ``model_type: "wavlm"`` (checkpoint keys with or without the ``wavlm.`` prefix)."""
    MODEL, MODEL_TYPE = WavLMModel, "wavlm"
