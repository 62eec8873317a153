"""Transducer beam search with RNNLM shallow fusion through the public interface: EncoderDecoderASR.from_hparams on
tests/golden/pretrained_transducer_lm_tiny (the LibriSpeech transducer recipe's layout at tiny sizes: `lm_model` an RNNLM, a
beam searcher with `lm_module` / `lm_weight` as `decoder`, `lm` among the pretrainer's loadables; written by
tools/make_transducer_lm_golden.py with the reference's savers) against the reference's own
EncoderDecoderASR.transcribe_batch on the same inputs, on the CPU emulator and on the MI355X."""
import os
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MODEL_DIR = os.path.join(GOLD, "pretrained_transducer_lm_tiny")


def _expected():
    return (np.load(os.path.join(GOLD, "pretrained_transducer_tiny_expected.npz")),  # the inputs (shared)
            np.load(os.path.join(GOLD, "pretrained_transducer_lm_tiny_expected.npz")))


def test_lm_model_fixture_margins_make_token_identity_fair():
    _, exp = _expected()
    assert float(exp["margin"][0]) >= 1e-3  # vs fp32 encoder differences of ~1e-5 in the joint's inputs
    assert 1 <= int(exp["expansions"].min()) and int(exp["expansions"].max()) < 16  # under the cap of beam_size 4
    assert int((exp["tokens"] >= 0).sum()) > 0


def test_encoder_decoder_asr_transducer_lm_from_hparams_matches_reference(backend):
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderDecoderASR
    from speechbrain_amd.lobes.models.RNNLM import RNNLM

    native, dev = backend
    inputs, exp = _expected()
    asr = EncoderDecoderASR.from_hparams(source=MODEL_DIR, run_opts={"device": str(dev)})
    searcher = asr.mods.decoder
    assert asr.transducer_beam_search and isinstance(searcher, TransducerBeamSearcher)
    assert searcher.beam_size == 4 and searcher.nbest == 3 and searcher.lm_weight == 0.5 and isinstance(searcher.lm, RNNLM)
    # lm.ckpt came through the pretrainer: the module holds the checkpoint's values, not its initialisation
    ckpt = torch.load(os.path.join(MODEL_DIR, "lm.ckpt"), map_location="cpu")
    assert sorted(ckpt) == sorted(searcher.lm.state_dict())
    for k, v in searcher.lm.state_dict().items():
        assert torch.equal(v.cpu(), ckpt[k]), k
    wav, lens = torch.from_numpy(inputs["wav"]), torch.from_numpy(inputs["lens"])
    tn = asr.encode_batch(wav, lens)
    assert tn.shape == exp["tn"].shape  # (the encoder's parity is tests/test_transducer_model.py's subject)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (a search that reaches the cap warns)
        words, tokens = asr.transcribe_batch(wav, lens)
    assert tokens == [[int(t) for t in row if t >= 0] for row in exp["tokens"]]
    assert words == [str(w) for w in exp["words"]]
    _, _, _, _, (status, expansions) = searcher.transducer_beam_search_decode(tn, return_status=True)
    assert status == [0, 0, 0] and expansions == exp["expansions"].sum(axis=1).tolist()
