"""speechbrain.integrations.huggingface.hubert mirror: HuBERT on the MI355X kernels.

The reference's ``HuBERT`` is its ``Wav2Vec2`` wrapper around HuggingFace's ``HubertModel`` (hubert.py:21-88).  HubertModel is the
wav2vec 2.0 forward (wav2vec2.py) under another ``model_type`` and checkpoint prefix, with two config switches:
``feat_proj_layer_norm`` (false: ``feature_projection.layer_norm`` is absent from the state dict and skipped) and
``conv_pos_batch_norm`` (a BatchNorm in place of the weight-normalised positional filter: not run here).  ``transformers`` is not
imported.  fp32 only."""
from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2, Wav2Vec2Model, _checked_config


class HubertModel(Wav2Vec2Model):
    """The parameter tree of HuggingFace's HubertModel on the wav2vec 2.0 forward."""

    def check_config(self, cfg):
        if cfg.get("conv_pos_batch_norm", False):
            raise NotImplementedError("HuBERT with conv_pos_batch_norm=True (a BatchNorm1d before the positional convolution "
                                      "instead of its weight normalisation)")
        return _checked_config({"feat_proj_layer_norm": True, **cfg}, "HuBERT")

    def projection_layer_norm(self, cfg):
        return bool(cfg["feat_proj_layer_norm"])


class HuBERT(Wav2Vec2):
    """speechbrain.integrations.huggingface.hubert.HuBERT on the MI355X kernels: the wav2vec 2.0 wrapper for a LOCAL HuggingFace
    directory whose config.json says ``model_type: "hubert"`` (checkpoint keys with or without the ``hubert.`` prefix).  Head
    dimensions outside the attention kernel's instantiations (hubert-xlarge: 80) raise NotImplementedError."""
    MODEL, MODEL_TYPE = HubertModel, "hubert"
