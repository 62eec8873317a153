"""EncoderASR.from_hparams on tests/golden/pretrained_ctc_lm_tiny (tools/make_ctc_lm_golden.py): a CTC model directory whose
test_beam_search names an ARPA n-gram model decodes with the fused device search and returns the reference's words."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
LM_DIR = os.path.join(GOLD, "pretrained_ctc_lm_tiny")


def test_encoder_asr_with_ngram_model_matches_reference(backend):
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderASR

    native, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_ctc_tiny_expected.npz"))
    want = json.loads(str(np.load(os.path.join(GOLD, "ctc_decode_lm.npz"))["meta"]))["interface"]
    # the path is taken as given (relative to the working directory), as in the reference: name the file outright
    asr = EncoderASR.from_hparams(source=LM_DIR, overrides={"kenlm_model_path": os.path.join(LM_DIR, "lm.arpa")},
                                  run_opts={"device": str(dev)})
    fn = asr.decoding_function
    assert isinstance(fn, CTCBeamSearcher) and fn.lm is not None and fn.lm.order == 3 and fn.prune_history is True
    words, pred = asr.transcribe_batch(torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"]))
    assert words == want["words"]
    for h, s, ls in zip(pred, want["score"], want["lm_score"]):
        # (the encoder's own 1e-4 relative parity carries into the scores, as in tests/test_ctc_decode.py)
        assert abs(float(h[0].score) - s) <= 1e-4 * max(1.0, abs(s))
        assert abs(float(h[0].lm_score) - ls) <= 1e-4 * max(1.0, abs(ls))
        assert h[0].last_lm_state is None and float(h[0].lm_score) != float(h[0].score)
