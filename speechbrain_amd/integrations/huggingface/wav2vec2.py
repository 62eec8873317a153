"""speechbrain.integrations.huggingface.wav2vec2 mirror: the wav2vec 2.0 encoder of the CTC recipes
(recipes/LibriSpeech/ASR/CTC/hparams/train_hf_wav2vec.yaml) on the MI355X kernels.

The reference wraps HuggingFace's ``Wav2Vec2Model`` (wav2vec2.py:30-199).  Here the same parameters -- HuggingFace's names under
``self.model``, so HuggingFace directories and SpeechBrain ``wav2vec2.ckpt`` files load unchanged -- drive:
  * layer 0 of the feature encoder, over the raw waveform, with its GroupNorm / LayerNorm and GELU: csrc/wav2vec2.hip
    (``native.w2v_conv0``; the group-norm statistics come from the waveform's window moments, the activation is written once);
  * layers 1-6: ``native.gemm_nt_rows`` over the time-major activation (K = k*C, lda = s*C: no im2col copy), bias and GELU in the
    epilogue, or followed by ``native.layernorm(..., act=GELU)`` in the layer-norm variant;
  * the grouped, weight-normalised positional convolution with its mask, GELU, residual (and the post-norm encoder's
    LayerNorm): ``native.w2v_posconv`` on the matrix cores;
  * the Transformer layers: the fused GEMM epilogues, ``native.rope_attention`` without a rotation table (keys < frame length;
    every query row is computed, as in the reference), ``native.layernorm``.
``transformers`` is not imported.  fp32 only."""
import json
import os

import torch
from torch import nn

from speechbrain_amd import native
from speechbrain_amd.integrations.huggingface.whisper import _read_checkpoint

ATTENTION_HEAD_DIMS = (8, 16, 32, 36, 64, 128)  # the instantiations of csrc/relpos_attn.hip


class _ConvLayer(nn.Module):
    """conv (+ layer_norm): HuggingFace's Wav2Vec2{NoLayerNorm,LayerNorm,GroupNorm}ConvLayer as a parameter holder."""

    def __init__(self, cin, cout, k, stride, bias, norm):
        super().__init__()
        self.conv = nn.Conv1d(cin, cout, k, stride=stride, bias=bias)
        if norm == "group":
            self.layer_norm = nn.GroupNorm(cout, cout, affine=True)
        elif norm == "layer":
            self.layer_norm = nn.LayerNorm(cout)
        self.gemm_w = native.Derived()

    def tap_major(self):
        """[out, in, k] -> [out, k*in], the tap as the slow index: one row of the strided window over [T, in]."""
        w = self.conv.weight
        return self.gemm_w.get((w,), lambda: w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous())


class _FeatureEncoder(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        dims, norm = cfg["conv_dim"], cfg["feat_extract_norm"]
        self.conv_layers = nn.ModuleList([
            _ConvLayer(1 if i == 0 else dims[i - 1], dims[i], cfg["conv_kernel"][i], cfg["conv_stride"][i], cfg["conv_bias"],
                       norm if (norm == "layer" or i == 0) else None) for i in range(len(dims))])


class _FeatureProjection(nn.Module):
    def __init__(self, cfg, layer_norm=True):
        super().__init__()
        self.layer_norm = nn.LayerNorm(cfg["conv_dim"][-1], eps=cfg["layer_norm_eps"]) if layer_norm else None
        self.projection = nn.Linear(cfg["conv_dim"][-1], cfg["hidden_size"])


class _WeightNormParams(nn.Module):
    """``parametrizations.weight`` of torch's weight_norm: original0 = g [1,1,k], original1 = v [d, d/G, k]."""

    def __init__(self, d, cg, k):
        super().__init__()
        v = torch.empty(d, cg, k)
        nn.init.normal_(v, mean=0, std=2 * (4.0 / (k * d)) ** 0.5)
        self.original0 = nn.Parameter(v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
        self.original1 = nn.Parameter(v)


class _PosConv(nn.Module):
    def __init__(self, d, groups, k):
        super().__init__()
        self.kernel_size, self.groups = k, groups
        self.bias = nn.Parameter(torch.zeros(d))
        self.parametrizations = nn.Module()
        self.parametrizations.weight = _WeightNormParams(d, d // groups, k)
        self._derived = native.Derived()

    def effective(self):
        """g * v / ||v|| (weight_norm over dim 2), tap-major [d, k*cg] for the kernel."""
        g, v = self.parametrizations.weight.original0, self.parametrizations.weight.original1

        def build():
            w = v * (g / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt())
            return w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()

        return self._derived.get((g, v), build)


class _PosConvEmbedding(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.conv = _PosConv(cfg["hidden_size"], cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"])


class _Attention(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.embed_dim, self.num_heads, self.head_dim = d, heads, d // heads
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = (nn.Linear(d, d) for _ in range(4))
        self._stack_derived = native.Derived()

    def stacked(self):
        """(in_proj weight [3d,d], bias [3d]) with rows ordered [head][q|k|v][head_dim]: what the attention kernel reads."""
        def build():
            H, Dh, d = self.num_heads, self.head_dim, self.embed_dim
            w = torch.stack([self.q_proj.weight, self.k_proj.weight, self.v_proj.weight]).view(3, H, Dh, d).permute(1, 0, 2, 3)
            b = torch.stack([self.q_proj.bias, self.k_proj.bias, self.v_proj.bias]).view(3, H, Dh).permute(1, 0, 2)
            return w.reshape(3 * d, d).contiguous(), b.reshape(-1).contiguous()

        ps = tuple(p for m in (self.q_proj, self.k_proj, self.v_proj) for p in (m.weight, m.bias))
        return self._stack_derived.get(ps, build)


class _FeedForward(nn.Module):
    def __init__(self, d, ffn):
        super().__init__()
        self.intermediate_dense = nn.Linear(d, ffn)
        self.output_dense = nn.Linear(ffn, d)


class _EncoderLayer(nn.Module):
    def __init__(self, cfg, attention):
        super().__init__()
        d, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.attention = attention
        self.layer_norm = nn.LayerNorm(d, eps=eps)
        self.feed_forward = _FeedForward(d, cfg["intermediate_size"])
        self.final_layer_norm = nn.LayerNorm(d, eps=eps)


class _Encoder(nn.Module):
    def __init__(self, cfg, new_attention):
        """``new_attention(cfg, i)``: the attention module of layer i."""
        super().__init__()
        self.pos_conv_embed = _PosConvEmbedding(cfg)
        self.layer_norm = nn.LayerNorm(cfg["hidden_size"], eps=cfg["layer_norm_eps"])
        self.layers = nn.ModuleList([_EncoderLayer(cfg, new_attention(cfg, i)) for i in range(cfg["num_hidden_layers"])])


_DEFAULTS = dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                 layer_norm_eps=1e-5, feat_extract_norm="group", feat_extract_activation="gelu",
                 conv_dim=(512,) * 7, conv_stride=(5, 2, 2, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 3, 2, 2), conv_bias=False,
                 num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16, do_stable_layer_norm=False,
                 mask_time_prob=0.05, mask_feature_prob=0.0, add_adapter=False)


def _checked_config(cfg, family="wav2vec 2.0", head_dims=ATTENTION_HEAD_DIMS):
    """The config over the defaults, or NotImplementedError / ValueError naming what the kernels do not take.  ``family`` names
    the model in the messages; ``head_dims``: the instantiations of the family's attention kernel."""
    cfg = {**_DEFAULTS, **cfg}
    if cfg["add_adapter"]:
        raise NotImplementedError(f"{family} with add_adapter (the convolutional adapter after the encoder)")
    for key in ("hidden_act", "feat_extract_activation"):
        if cfg[key] != "gelu":
            raise NotImplementedError(f"{family} with {key}={cfg[key]!r}: activations other than GELU are not fused")
    if cfg["feat_extract_norm"] not in ("group", "layer"):
        raise ValueError(f"feat_extract_norm={cfg['feat_extract_norm']!r}: 'group' or 'layer'")
    d, G, H = cfg["hidden_size"], cfg["num_conv_pos_embedding_groups"], cfg["num_attention_heads"]
    if d % G or d // G not in native.W2V_POSCONV_GROUP_WIDTHS:
        raise NotImplementedError(f"positional-conv group width {d}/{G}: the kernel is instantiated for "
                                  f"{native.W2V_POSCONV_GROUP_WIDTHS}")
    if cfg["num_conv_pos_embeddings"] > native.W2V_POSCONV_MAX_KERNEL:
        raise NotImplementedError(f"positional-conv kernel size {cfg['num_conv_pos_embeddings']} > {native.W2V_POSCONV_MAX_KERNEL}")
    if d % H or d // H not in head_dims:
        raise NotImplementedError(f"attention head dim {d}/{H}: the attention kernel is instantiated for {head_dims}")
    k0, s0 = cfg["conv_kernel"][0], cfg["conv_stride"][0]
    if not (1 <= s0 <= k0 <= native.W2V_CONV0_MAX_KERNEL) or cfg["conv_dim"][0] > 1024:
        raise NotImplementedError(f"first convolution kernel {k0} / stride {s0} / {cfg['conv_dim'][0]} channels: the waveform "
                                  f"kernel takes stride <= kernel <= {native.W2V_CONV0_MAX_KERNEL} and <= 1024 channels")
    return cfg


class Wav2Vec2Model(nn.Module):
    """The parameter tree of HuggingFace's Wav2Vec2Model and its forward on the kernels.  The HuBERT and WavLM models
    (hubert.py, wavlm.py) are this class with ``check_config``, ``projection_layer_norm``, ``new_attention`` and ``attend``
    of their own."""

    def check_config(self, cfg):
        return _checked_config(cfg)

    def projection_layer_norm(self, cfg):
        """feature_projection.layer_norm exists (and runs)."""
        return True

    def new_attention(self, cfg, layer):
        return _Attention(cfg["hidden_size"], cfg["num_attention_heads"])

    def attend(self, att, a, qkv, key_len):
        """The attention step of one layer: ``a`` [B,T',d] the hidden states the attention module received, ``qkv`` their stacked
        projection -> context [B,T',d]."""
        return native.rope_attention(qkv, None, None, key_len, att.num_heads, att.head_dim ** -0.5)[0]

    def __init__(self, cfg):
        super().__init__()
        self.config = cfg = self.check_config(cfg)
        if cfg["mask_time_prob"] > 0.0 or cfg["mask_feature_prob"] > 0.0:  # (present in the state dict; SpecAugment is training)
            self.masked_spec_embed = nn.Parameter(torch.empty(cfg["hidden_size"]).uniform_())
        self.feature_extractor = _FeatureEncoder(cfg)
        self.feature_projection = _FeatureProjection(cfg, self.projection_layer_norm(cfg))
        self.encoder = _Encoder(cfg, self.new_attention)

    def feat_lengths(self, n):
        """_get_feat_extract_output_lengths."""
        for k, s in zip(self.config["conv_kernel"], self.config["conv_stride"]):
            n = torch.div(n - k, s, rounding_mode="floor") + 1 if torch.is_tensor(n) else (n - k) // s + 1
        return n

    def features(self, wav, normalize):
        """wav [B,N] -> the feature encoder's output [B,T',C], time-major throughout."""
        cfg, layers = self.config, self.feature_extractor.conv_layers
        layer_mode = cfg["feat_extract_norm"] == "layer"
        L0 = layers[0]
        h = native.w2v_conv0(wav, L0.conv.weight.reshape(L0.conv.out_channels, -1), L0.conv.bias, L0.layer_norm.weight,
                             L0.layer_norm.bias, cfg["conv_stride"][0],
                             native.W2V_LAYER_NORM if layer_mode else native.W2V_GROUP_NORM, eps=L0.layer_norm.eps,
                             normalize=normalize)
        B = wav.shape[0]
        for L in layers[1:]:
            k, s, cin, cout = L.conv.kernel_size[0], L.conv.stride[0], L.conv.in_channels, L.conv.out_channels
            T = (h.shape[1] - k) // s + 1
            if T < 1:
                raise ValueError(f"the waveform is too short for the feature encoder ({h.shape[1]} frames before a kernel of {k})")
            w = L.tap_major()
            y = torch.empty(B, T, cout, dtype=torch.float32, device=wav.device)
            for b in range(B):  # frame t reads frames s*t .. s*t + k - 1: k*cin contiguous floats every s*cin
                native.gemm_nt_rows(h[b].reshape(-1), T, k * cin, s * cin, w, L.conv.bias,
                                    act=native.ACT_NONE if layer_mode else native.ACT_GELU, out=y[b])
            h = native.layernorm(y, L.layer_norm.weight, L.layer_norm.bias, L.layer_norm.eps, act=native.ACT_GELU) if layer_mode else y
        return h

    def forward(self, wav, valid_samples=None, normalize=False, output_hidden_states=False):
        """wav [B,N] fp32, valid_samples int64 [B] on the host (None: no masking) -> last hidden state [B,T',d] (and the tuple
        of hidden states, HuggingFace's convention)."""
        cfg = self.config
        feats = self.features(wav.float().contiguous(), normalize)
        B, T, _ = feats.shape
        key_len = None
        if valid_samples is not None:
            n = self.feat_lengths(valid_samples)
            n = torch.where(n <= 0, torch.full_like(n, T), n).clamp(max=T)  # (HuggingFace marks frame n-1: index -1 is the last)
            key_len = n.to(device=wav.device, dtype=torch.int32)
        fp, enc = self.feature_projection, self.encoder
        h = feats
        if fp.layer_norm is not None:
            h = native.layernorm(feats, fp.layer_norm.weight, fp.layer_norm.bias, fp.layer_norm.eps)
        h = native.gemm_nt(h, fp.projection.weight, fp.projection.bias)
        stable = bool(cfg["do_stable_layer_norm"])
        pc = enc.pos_conv_embed.conv
        x = native.w2v_posconv(h, key_len, pc.effective(), pc.bias, pc.groups, pc.kernel_size,
                               ln=None if stable else (enc.layer_norm.weight, enc.layer_norm.bias, enc.layer_norm.eps))
        hidden = [] if output_hidden_states else None
        for layer in enc.layers:
            if hidden is not None:
                hidden.append(x)
            att, ff = layer.attention, layer.feed_forward
            w_in, b_in = att.stacked()
            ln1, ln2 = layer.layer_norm, layer.final_layer_norm
            a = native.layernorm(x, ln1.weight, ln1.bias, ln1.eps) if stable else x
            qkv = native.gemm_nt(a, w_in, b_in)
            ctx = self.attend(att, a, qkv, key_len)
            x = native.gemm_nt(ctx, att.out_proj.weight, att.out_proj.bias, residual=x)
            if stable:
                f = native.layernorm(x, ln2.weight, ln2.bias, ln2.eps)
            else:
                f = x = native.layernorm(x, ln1.weight, ln1.bias, ln1.eps)
            f = native.gemm_nt(f, ff.intermediate_dense.weight, ff.intermediate_dense.bias, act=native.ACT_GELU)
            x = native.gemm_nt(f, ff.output_dense.weight, ff.output_dense.bias, residual=x)
            if not stable:
                x = native.layernorm(x, ln2.weight, ln2.bias, ln2.eps)
        if stable:
            x = native.layernorm(x, enc.layer_norm.weight, enc.layer_norm.bias, enc.layer_norm.eps)
        if hidden is not None:
            hidden.append(x)
            return x, tuple(hidden)
        return x


_OLD_WEIGHT_NORM = {"weight_g": "parametrizations.weight.original0", "weight_v": "parametrizations.weight.original1"}


def _rename_weight_norm(state, prefix=""):
    """The spelling checkpoints written by older torch use for the weight-normalised positional filter -> the current one."""
    stem = prefix + "encoder.pos_conv_embed.conv."
    for old, new in _OLD_WEIGHT_NORM.items():
        if stem + old in state:
            state[stem + new] = state.pop(stem + old)
    return state


# HuggingFace model_type -> the wrapper that runs it
_WRAPPERS = {"wav2vec2": "wav2vec2.Wav2Vec2", "hubert": "hubert.HuBERT", "wavlm": "wavlm.WavLM"}


class Wav2Vec2(nn.Module):
    """speechbrain.integrations.huggingface.wav2vec2.Wav2Vec2 on the MI355X kernels.

    ``source`` is a LOCAL HuggingFace model directory (config.json, preprocessor_config.json, model.safetensors or
    pytorch_model.bin); nothing is downloaded.  ``forward(wav, wav_lens)`` / ``extract_features(wav, wav_lens)`` return what the
    reference returns: the last hidden state [B,T',d], or with ``output_all_hiddens`` the stack [layers+1,B,T',d]; with
    ``output_norm`` normalised over each utterance's [T',d] block (padded frames included, as the reference does)."""

    MODEL, MODEL_TYPE = Wav2Vec2Model, "wav2vec2"  # (the model class; config.json's model_type = the checkpoint's key prefix)

    def __init__(self, source, save_path=None, output_norm=False, freeze=False, freeze_feature_extractor=False,
                 apply_spec_augment=False, output_all_hiddens=False, **kwargs):
        super().__init__()
        if kwargs.get("output_attentions"):
            raise NotImplementedError("output_attentions: attention maps are not produced by the fused attention kernel")
        if apply_spec_augment:
            raise NotImplementedError("apply_spec_augment: SpecAugment inside the encoder is a training-time option")
        with open(os.path.join(source, "config.json")) as f:
            cfg = json.load(f)
        kind = cfg.get("model_type", self.MODEL_TYPE)
        if kind != self.MODEL_TYPE:  # (every wrapper runs its own model type only: the parameter trees differ)
            hint = f" — load it with speechbrain.integrations.huggingface.{_WRAPPERS[kind]}" if kind in _WRAPPERS else ""
            raise NotImplementedError(f"{type(self).__name__}: model_type {kind!r}{hint}")
        self.normalize_wav = False
        pp = os.path.join(source, "preprocessor_config.json")
        if os.path.exists(pp):
            with open(pp) as f:
                self.normalize_wav = bool(json.load(f).get("do_normalize", True))
        self._setup(cfg, output_norm, freeze, freeze_feature_extractor, output_all_hiddens)
        own = self.model.state_dict()
        pre = self.MODEL_TYPE + "."
        state = {(k[len(pre):] if k.startswith(pre) else k): v for k, v in _read_checkpoint(source).items()}
        state = {k: v.float() for k, v in _rename_weight_norm(state).items() if k in own}  # (heads of task models are not ours)
        missing = sorted(set(own) - set(state) - {"masked_spec_embed"})
        if missing:
            raise KeyError(f"{source}: the checkpoint lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        self.model.load_state_dict(state, strict=False)

    def _setup(self, cfg, output_norm, freeze, freeze_feature_extractor, output_all_hiddens):
        self.model = self.MODEL(cfg)
        self.output_norm, self.freeze, self.freeze_feature_extractor = output_norm, freeze, freeze_feature_extractor
        self.output_all_hiddens = output_all_hiddens
        for p in self.model.parameters():  # inference path: parameters are constants
            p.requires_grad_(False)
        self._register_load_state_dict_pre_hook(lambda state, prefix, *_: _rename_weight_norm(state, prefix + "model."))

    @classmethod
    def from_config(cls, cfg, normalize_wav=False, output_norm=False, output_all_hiddens=False, seed=0):
        """A randomly initialised model of the given HuggingFace config dict (benchmarks, tests: no checkpoint on disk)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.normalize_wav = normalize_wav
        torch.manual_seed(seed)
        self._setup(cfg, output_norm, True, False, output_all_hiddens)
        return self

    def forward(self, wav, wav_lens=None):
        return self.extract_features(wav, wav_lens)

    @torch.no_grad()
    def extract_features(self, wav, wav_lens=None):
        valid = None
        if wav_lens is not None:  # make_padding_masks (huggingface.py:433-455): round(wav_lens * N) valid samples
            valid = torch.round(wav_lens.detach().float().cpu() * wav.shape[1]).long()
        out = self.model(wav, valid, normalize=self.normalize_wav, output_hidden_states=self.output_all_hiddens)
        if self.output_all_hiddens:
            out = torch.stack(out[1])
        if self.output_norm:
            out = native.w2v_utt_norm(out.contiguous())
        return out


class Wav2Vec2Pretrain(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("Wav2Vec2Pretrain (the self-supervised pre-training wrapper) is a training-time class")
