"""Transducer models through the public interfaces: EncoderDecoderASR.from_hparams and StreamingASR.from_hparams on
tests/golden/pretrained_transducer_tiny (the LibriSpeech transducer recipe's layout at tiny sizes; checkpoints written by the
reference's savers, tools/make_transducer_golden.py), against the reference's own interfaces on the same inputs, on the CPU
emulator and on the MI355X (the `backend` fixture)."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MODEL_DIR = os.path.join(GOLD, "pretrained_transducer_tiny")


def _expected():
    return np.load(os.path.join(GOLD, "pretrained_transducer_tiny_expected.npz"))


def test_model_fixture_margins_make_token_identity_fair():
    exp = _expected()
    assert float(exp["min_gap"][0]) >= 0.05  # vs fp32 encoder differences of ~1e-5 in the joint's inputs
    n_tok = [int((row >= 0).sum()) for row in exp["tokens"]]
    assert all(k > 0 for k in n_tok) and any(len(t) > 0 for t in exp["chunk_texts"])


def test_encoder_decoder_asr_transducer_from_hparams_matches_reference(backend):
    """hyperparams.yaml (transducer_beam_search: True): the encoder output -- the padded rows included, which the
    transducer decodes -- and the words and tokens of the reference's EncoderDecoderASR on a batch of unequal lengths."""
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderDecoderASR

    native, dev = backend
    exp = _expected()
    asr = EncoderDecoderASR.from_hparams(source=MODEL_DIR, run_opts={"device": str(dev)})
    assert asr.transducer_beam_search and isinstance(asr.mods.decoder, TransducerBeamSearcher)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    tn = asr.encode_batch(wav, lens).cpu()
    ref = torch.from_numpy(exp["tn"])
    assert tn.shape == ref.shape
    scale = max(1.0, float(ref.abs().max()))
    for b, rel in enumerate(exp["lens"]):
        n = int(round(float(rel) * ref.shape[1]))
        assert float((tn[b, :n] - ref[b, :n]).abs().max()) <= 1e-4 * scale, b
        if n < ref.shape[1]:  # the padded rows: the reference's encoder writes them too, and they are decoded
            assert float((tn[b, n:] - ref[b, n:]).abs().max()) <= 1e-4 * scale, (b, "padded rows")
    words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == [[int(t) for t in row if t >= 0] for row in exp["tokens"]]
    assert words == [str(w) for w in exp["words"]]


def test_streaming_asr_transducer_from_hparams_matches_reference(backend):
    """hyperparams_streaming.yaml: the decoding function is TransducerBeamSearcher.transducer_greedy_decode_streaming bound
    to the greedy searcher by `!name:` with a positional argument, the tokenizer decodes with
    spm_decode_preserve_leading_space; the chunk texts of the reference's StreamingASR.transcribe_chunk over a wav file."""
    import functools

    from speechbrain_amd.inference.ASR import StreamingASR
    from speechbrain_amd.utils.dynamic_chunk_training import DynChunkTrainConfig

    native, dev = backend
    exp = _expected()
    asr = StreamingASR.from_hparams(source=MODEL_DIR, hparams_file="hyperparams_streaming.yaml",
                                    run_opts={"device": str(dev)})
    assert isinstance(asr.hparams.decoding_function, functools.partial)
    cfg = DynChunkTrainConfig(chunk_size=int(exp["chunk_size"][0]), left_context_size=int(exp["left_context_size"][0]))
    assert asr.get_chunk_size_frames(cfg) == int(exp["chunk"][0])
    texts = list(asr.transcribe_file_streaming(os.path.join(GOLD, str(exp["file_name"])), cfg))
    assert texts == [str(t) for t in exp["chunk_texts"]]
    assert asr.transcribe_file(os.path.join(GOLD, str(exp["file_name"])), cfg) == "".join(texts)
