"""lobes/models/CRDNN.py against the reference's own CRDNN (tests/golden/model_crdnn.npz and the model directory
tests/golden/pretrained_crdnn_ctc_tiny, both written by tools/make_crdnn_golden.py), on the CPU emulator of the kernel sources
(not gpu) and on the MI355X (-m gpu).

Bounds (the project's): recorded stages 5e-5, CTC log-probabilities 1e-4, ids and text exact.  The generator checked that the
reference's own fp32-vs-fp64 distance is under a quarter of each bound and that its fp64 run decodes the same ids."""
import functools
import os

import numpy as np
import pytest
import torch

import crdnn_host_ref as R
from speechbrain_amd.lobes.models.CRDNN import CRDNN, CNN_Block, DNN_Block
from speechbrain_amd.nnet.RNN import GRU, LSTM, RNN, LiGRU

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
CRDNN_DIR = os.path.join(GOLD, "pretrained_crdnn_ctc_tiny")
STAGE_BOUND, LOGP_BOUND = 5e-5, 1e-4


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(os.path.join(GOLD, "model_crdnn.npz"))
    return {k: z[k] for k in z.files}


def _build(**over):
    n_mels, c0, c1, p0, p1, tp, layers, neurons, dnn_blocks, dnn_neurons, _ = (int(v) for v in _golden()["cfg"])
    kw = dict(input_shape=[None, None, n_mels], activation=torch.nn.LeakyReLU, dropout=0.15, cnn_blocks=2, cnn_channels=[c0, c1],
              cnn_kernelsize=(3, 3), inter_layer_pooling_size=[p0, p1], time_pooling=True, using_2d_pooling=False,
              time_pooling_size=tp, rnn_class=LSTM, rnn_layers=layers, rnn_neurons=neurons, rnn_bidirectional=True,
              rnn_re_init=True, dnn_blocks=dnn_blocks, dnn_neurons=dnn_neurons, use_rnnp=False)
    kw.update(over)
    return CRDNN(**kw)


def _state_dict():
    return {k[3:]: torch.from_numpy(v) for k, v in _golden().items() if k.startswith("sd/")}


def test_constructor_keys_and_strict_loading():
    m = _build()
    sd = _state_dict()
    assert set(m.state_dict().keys()) == set(sd.keys())
    for k in ("CNN.block_0.conv_1.conv.weight", "CNN.block_0.norm_1.norm.weight", "RNN.rnn.weight_hh_l0_reverse",
              "DNN.block_0.linear.w.weight", "DNN.block_0.norm.norm.running_mean", "DNN.block_0.norm.norm.num_batches_tracked"):
        assert k in sd and m.state_dict()[k].shape == sd[k].shape
    m.load_state_dict(sd, strict=True)
    assert isinstance(m["CNN"]["block_0"], CNN_Block) and isinstance(m["DNN"]["block_1"], DNN_Block)
    assert isinstance(m["RNN"], LSTM) and m["RNN"].rnn.bidirectional
    dw = m["RNN"].direction_weights()
    assert len(dw) == 2 and len(dw[0]) == 2 and dw[1][1][1] is m["RNN"].rnn.weight_hh_l1_reverse
    with pytest.raises(NotImplementedError, match="bidirectional.*CRDNN"):
        m["RNN"](torch.zeros(1, 2, 80))
    # the reference's default input_size form
    assert set(CRDNN(input_size=40, rnn_class=LSTM, cnn_channels=[4, 8], rnn_neurons=8, dnn_neurons=8).state_dict()) >= {"CNN.block_1.conv_2.conv.bias"}


def test_every_recorded_stage(backend):
    nat, dev = backend
    g = _golden()
    m = _build().eval()
    m.load_state_dict(_state_dict(), strict=True)
    m = m.to(dev)
    feats = torch.from_numpy(g["feats"]).to(dev)
    with torch.no_grad():
        out, stages = m(feats, return_stages=True)
        plain = m(feats)
    names = ["cnn_block0", "cnn_block1", "time_pooling", "lstm_layer0", "lstm_layer1", "dnn_block0", "dnn_block1"]
    assert sorted(stages) == sorted(names)
    for k in names:
        ref = torch.from_numpy(g[k])
        assert stages[k].shape == ref.shape, k
        err = float((stages[k].cpu() - ref).abs().max())
        print(f"crdnn stage {k}: max|d| {err:.3e}")
        assert err <= STAGE_BOUND, k
    # the time pooling fused into the last block's pass gives the same bits as a max over 4 frames of the block's own output
    blk = stages["cnn_block1"].cpu()
    Tp = blk.shape[1] // 4
    assert torch.equal(stages["time_pooling"].cpu(), blk[:, :Tp * 4].reshape(blk.shape[0], Tp, 4, *blk.shape[2:]).amax(dim=2))
    assert torch.equal(plain, out)
    assert float((out.cpu() - torch.from_numpy(g["output"])).abs().max()) <= STAGE_BOUND
    w, b = torch.from_numpy(g["ctc_lin/w.weight"]).to(dev), torch.from_numpy(g["ctc_lin/w.bias"]).to(dev)
    logp = torch.log_softmax(nat.gemm_nt(out.contiguous(), w, b).cpu(), dim=-1)
    err = float((logp - torch.from_numpy(g["logp"])).abs().max())
    print(f"crdnn ctc log-probs: max|d| {err:.3e}")
    assert err <= LOGP_BOUND
    from speechbrain_amd.decoders.ctc import ctc_greedy_decode

    ids = ctc_greedy_decode(logp.to(dev), torch.from_numpy(g["wav_lens"]).to(dev), blank_id=0)
    assert [[int(t) for t in h] for h in ids] == [[int(t) for t in row if t >= 0] for row in g["greedy_ids"]]


def test_a_checkpoint_loaded_after_the_first_call_is_picked_up(backend):
    """The folded BatchNorm / re-laid-out weights are derived values: new parameters AND new running statistics replace them."""
    nat, dev = backend
    g = _golden()
    m = _build().eval().to(dev)
    feats = torch.from_numpy(g["feats"]).to(dev)
    with torch.no_grad():
        first = m(feats)
        m.load_state_dict({k: v.to(dev) for k, v in _state_dict().items()}, strict=True)
        second = m(feats)
    assert not torch.equal(first, second)
    assert float((second.cpu() - torch.from_numpy(g["output"])).abs().max()) <= STAGE_BOUND
    with torch.no_grad():
        m["DNN"]["block_1"]["norm"].norm.running_mean.add_(0.5)
        third = m(feats)
    sd = {k: v.double() for k, v in m.state_dict().items()}
    ref, _ = R.crdnn(feats.cpu().double(), {k: v.cpu() for k, v in sd.items()}, (2, 2), 4, 2, True, 2)
    assert float((third.cpu().double() - ref).abs().max()) <= STAGE_BOUND and not torch.equal(third, second)


@pytest.mark.parametrize("yaml,key", [("hyperparams.yaml", "greedy"), ("hyperparams_beam.yaml", "beam")])
def test_encoder_asr_from_hparams_matches_reference(backend, yaml, key):
    """EncoderASR.from_hparams on a CRDNN + CTC hyperparams directory written by the reference (train_BPE_1000.yaml's encoder and
    CTC head): log-probabilities within bound; greedy ids, beam text and the transcriptions of the wav fixtures exact."""
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderASR

    nat, dev = backend
    exp = np.load(os.path.join(GOLD, "pretrained_crdnn_ctc_tiny_expected.npz"))
    asr = EncoderASR.from_hparams(source=CRDNN_DIR, hparams_file=yaml, run_opts={"device": str(dev)})
    assert isinstance(asr.mods.encoder["enc"], CRDNN)
    wav, lens = torch.from_numpy(exp["wav"]), torch.from_numpy(exp["lens"])
    logp = asr.encode_batch(wav, lens).cpu()
    ref = torch.from_numpy(exp["logp"])
    err = float((logp - ref).abs().max())
    print(f"crdnn EncoderASR log-probs: max|d| {err:.3e}")
    assert logp.shape == ref.shape and err <= LOGP_BOUND
    words, pred = asr.transcribe_batch(wav, lens)
    assert words == [str(w) for w in exp[f"{key}_words"]]
    if key == "greedy":
        assert pred == [[int(t) for t in row if t >= 0] for row in exp["greedy_tokens"]]
    else:
        assert isinstance(asr.decoding_function, CTCBeamSearcher)
        for h, s in zip(pred, exp["beam_scores"]):
            assert abs(float(h[0].score) - float(s)) <= 1e-4 * max(1.0, abs(float(s)))
        # the searcher's hypotheses carry text, not ids: the ids of the reference's best hypotheses, exactly
        ids = [[asr.tokenizer.lab2ind[c] for c in h[0].text] for h in pred]
        assert ids == [[int(t) for t in row if t >= 0] for row in exp["beam_ids"]]
    for name, w in zip(exp["file_names"], exp[f"{key}_file_words"]):
        assert asr.transcribe_file(os.path.join(GOLD, str(name))) == str(w)


def test_crdnn_shim_paths_resolve():
    import subprocess
    import sys

    code = ("import speechbrain_amd.compat as c; c.install(); "
            "from speechbrain.lobes.models.CRDNN import CRDNN, CNN_Block, DNN_Block; from speechbrain.nnet.pooling import Pooling1d; "
            "from speechbrain.nnet.dropout import Dropout2d; from speechbrain.nnet.normalization import BatchNorm1d; "
            "from speechbrain.nnet.RNN import LSTM; "
            "assert CRDNN.__module__ == 'speechbrain_amd.lobes.models.CRDNN' and Pooling1d.__module__.startswith('speechbrain_amd.'); "
            "print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


@pytest.mark.parametrize("over,match", [
    (dict(rnn_class=GRU), "GRU"), (dict(rnn_class=LiGRU), "LiGRU"), (dict(rnn_class=RNN), "RNN"), (dict(rnn_class=None), "LiGRU"),
    (dict(use_rnnp=True), "use_rnnp"), (dict(projection_dim=64), "projection_dim"), (dict(using_2d_pooling=True), "using_2d_pooling"),
    (dict(activation=torch.nn.ReLU), "ReLU"), (dict(cnn_kernelsize=(5, 5)), "cnn_kernelsize"), (dict(cnn_blocks=0), "cnn_blocks"),
    (dict(rnn_layers=0), "rnn_layers"),
])
def test_out_of_scope_variants_raise_by_name_at_construction(over, match):
    with pytest.raises(NotImplementedError, match=match):
        _build(**over)


def test_too_short_inputs_raise_value_errors(backend):
    """One frame: the reference's reflect padding refuses it; three frames under a time pooling of four: an empty output."""
    nat, dev = backend
    m = _build().eval()
    m.load_state_dict(_state_dict(), strict=True)
    m = m.to(dev)
    with pytest.raises(ValueError, match="reflect"):
        m(torch.zeros(2, 1, 40, device=dev))
    with pytest.raises(ValueError, match="empty"):
        m(torch.zeros(2, 3, 40, device=dev))
