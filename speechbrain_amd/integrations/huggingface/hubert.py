"""speechbrain.integrations.huggingface.hubert: named, not implemented."""


class HuBERT:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("the HuBERT wrapper is not implemented (speechbrain_amd runs wav2vec 2.0 through "
                                  "integrations.huggingface.wav2vec2.Wav2Vec2)")
