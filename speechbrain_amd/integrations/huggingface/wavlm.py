"""speechbrain.integrations.huggingface.wavlm: named, not implemented."""


class WavLM:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("the WavLM wrapper is not implemented (speechbrain_amd runs wav2vec 2.0 through "
                                  "integrations.huggingface.wav2vec2.Wav2Vec2)")
