"""The CRDNN encoder at the recipe's width (train_BPE_1000.yaml: n_mels 40, 128 / 256 channels, LSTM 1024 bidirectional, DNN 512)
on the MI355X, with 2 LSTM layers, 2 utterances and 32 frames: every stage against the fp64 restatement
(tests/crdnn_host_ref.py) under the kernel bound, max(4 x the fp32 torch composition's own error on the same inputs, 1e-5)."""
import pytest
import torch

import crdnn_host_ref as R

pytestmark = pytest.mark.gpu


def test_recipe_width_encoder_against_fp64():
    from speechbrain_amd import native
    from speechbrain_amd.lobes.models.CRDNN import CRDNN
    from speechbrain_amd.nnet.RNN import LSTM

    native.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    m = CRDNN(input_shape=[None, None, 40], cnn_blocks=2, cnn_channels=[128, 256], inter_layer_pooling_size=[2, 2],
              time_pooling=True, time_pooling_size=4, rnn_class=LSTM, rnn_layers=2, rnn_neurons=1024, rnn_bidirectional=True,
              rnn_re_init=True, dnn_blocks=2, dnn_neurons=512).eval()
    gen = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1 or "norm" in n:
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
        for n, b in m.named_buffers():
            if n.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=gen))
            elif n.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=gen))
    feats = torch.randn(2, 32, 40, generator=gen)
    sd = {k: v.detach() for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}
    args = ((2, 2), 4, 2, True, 2)
    with torch.no_grad():
        ref, ref_st = R.crdnn(feats.double(), R.cast_dict(sd, torch.float64), *args)
        c32, c32_st = R.crdnn(feats, sd, *args)
    assert native.rnn_layer_route(2, 8, 1024, 2) == 1
    with torch.no_grad():
        out, st = m.to(dev)(feats.to(dev), return_stages=True)
    assert out.shape == (2, 8, 512)
    for k in ref_st:
        err32 = float((c32_st[k].double() - ref_st[k]).abs().max())
        err = float((st[k].cpu().double() - ref_st[k]).abs().max())
        print(f"crdnn full size {k}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
        assert err <= max(4.0 * err32, 1e-5), k
