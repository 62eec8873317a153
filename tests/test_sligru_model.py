"""nnet/RNN.py SLiGRU and lobes/models/CRDNN.py with rnn_class SLiGRU against the reference's own modules (tests/golden/
model_sligru.npz and the model directory tests/golden/pretrained_crdnn_sligru_ctc_tiny, written by tools/make_sligru_golden.py),
on the CPU emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bounds (the project's): recorded layers and hh 5e-5, CTC log-probabilities 1e-4, ids and text exact.  The generator checked that
the reference's own fp32-vs-fp64 distance is under a quarter of each bound and that its fp64 run decodes the same ids."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from speechbrain_amd.lobes.models.CRDNN import CRDNN
from speechbrain_amd.nnet.RNN import SLiGRU

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _model():
    g = np.load(os.path.join(GOLD, "model_sligru.npz"))
    H, IN, B, T, L = (int(v) for v in g["cfg"])
    m = SLiGRU(hidden_size=H, input_shape=[B, T, IN], num_layers=L, bidirectional=True, recurrent_elementwise_affine=True).eval()
    sd = {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd/")}
    assert {"rnn.0.w.weight", "rnn.1.u.weight", "rnn.0.layer_norm.bias", "rnn.1.norm.running_var", "rnn.0.norm.num_batches_tracked",
            "rnn.0.h_init", "rnn.1.drop_mask_te"} <= set(sd)
    m.load_state_dict(sd, strict=True)
    return m, g, L


def test_layers_and_hh_match_the_reference(backend):
    nat, dev = backend
    m, g, L = _model()
    out, hh, layers = m.to(dev)(torch.from_numpy(g["x"]).to(dev), return_layers=True)
    assert torch.equal(out, layers[-1])
    for name, got in [(f"layer{i}", layers[i]) for i in range(L)] + [("hh", hh)]:
        ref = torch.from_numpy(g[name])
        err = float((got.cpu() - ref).abs().max())
        print(f"sligru {name}: max|d| {err:.3e}")
        assert got.shape == ref.shape and err <= 5e-5, name


def test_encoder_asr_from_hparams_matches_reference(backend):
    from speechbrain_amd.inference.ASR import EncoderASR

    nat, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_crdnn_sligru_ctc_tiny_expected.npz"))
    sig = np.load(os.path.join(GOLD, "pretrained_crdnn_ctc_tiny_expected.npz"))  # (the same waveforms as the LSTM fixture)
    asr = EncoderASR.from_hparams(source=os.path.join(GOLD, "pretrained_crdnn_sligru_ctc_tiny"), run_opts={"device": str(dev)})
    enc = asr.mods.encoder["enc"]
    assert isinstance(enc, CRDNN) and isinstance(enc["RNN"], SLiGRU)
    wav, lens = torch.from_numpy(sig["wav"]), torch.from_numpy(sig["lens"])
    logp = asr.encode_batch(wav, lens).cpu()
    ref = torch.from_numpy(exp["logp"])
    err = float((logp - ref).abs().max())
    print(f"crdnn(sligru) EncoderASR log-probs: max|d| {err:.3e}")
    assert logp.shape == ref.shape and err <= 1e-4
    words, pred = asr.transcribe_batch(wav, lens)
    assert words == [str(w) for w in exp["greedy_words"]]
    assert pred == [[int(t) for t in row if t >= 0] for row in exp["greedy_tokens"]]
    feats = torch.randn(2, 16, 40, generator=torch.Generator().manual_seed(3)).to(dev)
    assert sorted(k for k in enc(feats, return_stages=True)[1] if "layer" in k) == ["rnn_layer0", "rnn_layer1"]


def test_shim_path_resolves():
    code = ("import speechbrain_amd.compat as c; c.install(); from speechbrain.nnet.RNN import SLiGRU, SLiGRU_Layer; "
            "assert SLiGRU.__module__ == 'speechbrain_amd.nnet.RNN'; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_hx_raises_by_name():
    m, g, _ = _model()
    with pytest.raises(NotImplementedError, match="SLiGRU: hx"):
        m(torch.from_numpy(g["x"]), hx=torch.zeros(4, 3, 12))
    with pytest.raises(NotImplementedError, match="SLiGRU: training mode"):
        m.train()(torch.from_numpy(g["x"]))
