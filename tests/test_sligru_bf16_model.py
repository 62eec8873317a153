"""A CRDNN encoder with rnn_class SLiGRU under precision "bf16": the model directory tests/golden/pretrained_crdnn_sligru_ctc_tiny
through EncoderASR.from_hparams(..., run_opts={"precision": ...}) and the 2-layer SLiGRU module of tests/golden/model_sligru.npz under
native.precision_scope, on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound: the bf16 CTC log-probabilities lie within 1e-2 relative RMS of the fp32 path's (the project's bound for an encoder under
bf16 against its own fp32 path, tests/test_relpos_bf16.py) and differ from them; "fp32" is run_opts={} bit for bit."""
import os

import numpy as np
import torch

from test_sligru_model import GOLD, _model


def test_encoder_asr_crdnn_sligru_under_precision_bf16(backend):
    from speechbrain_amd.inference.ASR import EncoderASR

    nat, dev = backend
    sig = np.load(os.path.join(GOLD, "pretrained_crdnn_ctc_tiny_expected.npz"))  # (the waveforms of the fixture)
    wav, lens = torch.from_numpy(sig["wav"]), torch.from_numpy(sig["lens"])
    logp = {}
    for prec in (None, "fp32", "bf16"):
        opts = {"device": str(dev)} if prec is None else {"device": str(dev), "precision": prec}
        asr = EncoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_crdnn_sligru_ctc_tiny"), run_opts=opts)
        nat.prof_reset(), nat.prof_enable(True)
        logp[prec] = asr.encode_batch(wav, lens).cpu()
        nat.prof_enable(False)
        rep = nat.prof_report()
        assert ("sligru_product_bf16" in rep) == (prec == "bf16") and ("sligru_product" in rep) == (prec != "bf16")
    assert torch.equal(logp["fp32"], logp[None]) and not torch.equal(logp["bf16"], logp["fp32"])
    ref = logp["fp32"].double()
    rel = float(((logp["bf16"].double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())
    print(f"crdnn(sligru) EncoderASR, bf16 vs fp32 log-probs: relative RMS {rel:.3e}")
    assert rel <= 1e-2


def test_u_image_is_made_once_per_layer(backend):
    nat, dev = backend
    m, g, L = _model()
    m, x = m.to(dev), torch.from_numpy(g["x"]).to(dev)
    nat.prof_reset(), nat.prof_enable(True)
    with nat.precision_scope("bf16"):
        a, b = m(x)[0], m(x)[0]
    nat.prof_enable(False)
    rep = nat.prof_report()
    assert L == 2 and rep["sligru_u_image"]["count"] == L and rep["sligru_product_bf16"]["count"] > 0
    assert torch.equal(a, b)
