"""speechbrain.nnet.RNN mirror: the LSTM of a transducer's prediction network (nnet/RNN.py:187-302).

The LSTM's parameters live in ``self.rnn`` (a ``torch.nn.LSTM`` used as a parameter holder), so checkpoints keep the
reference's state_dict keys (``rnn.weight_ih_l0``, ...).  ``forward`` runs on the device (sbk_lstm_f32) for unidirectional
layers; as a prediction network it runs inside sbk_transducer_greedy_f32 (decoders/transducer.py).  A bidirectional stack is
the recurrent part of a CRDNN encoder: there this class holds the parameters and lobes.models.CRDNN.CRDNN runs the layers
(sbk_rnn_layer_f32 through ``direction_weights``); called on its own it raises.  ``GRU``, ``RNN`` and ``LiGRU`` are not
implemented."""
import torch

from speechbrain_amd import native


class LSTM(torch.nn.Module):
    def __init__(self, hidden_size, input_shape=None, input_size=None, num_layers=1, bias=True, dropout=0.0, re_init=True,
                 bidirectional=False):
        super().__init__()
        self.reshape = False
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = int(torch.prod(torch.tensor(input_shape[2:])).item())
        self.rnn = torch.nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, dropout=dropout,
                                 bidirectional=bidirectional, bias=bias, batch_first=True)
        if re_init:
            _rnn_init(self.rnn)

    def layer_weights(self):
        """[(w_ih [4H, in], w_hh [4H, H], b_ih or None, b_hh or None)] per layer."""
        if self.rnn.bidirectional:
            raise NotImplementedError("a bidirectional LSTM is not implemented on its own: CRDNN drives it "
                                      "(lobes.models.CRDNN.CRDNN, through direction_weights())")
        out = []
        for l in range(self.rnn.num_layers):
            g = lambda n: getattr(self.rnn, f"{n}_l{l}", None)  # noqa: E731
            out.append((g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh")))
        return out

    def direction_weights(self):
        """[[(w_ih [4H, in], w_hh [4H, H], b_ih or None, b_hh or None) per direction (forward, then ``_reverse``)] per layer]."""
        out = []
        for l in range(self.rnn.num_layers):
            dirs = []
            for sfx in ("", "_reverse")[:2 if self.rnn.bidirectional else 1]:
                g = lambda n: getattr(self.rnn, f"{n}_l{l}{sfx}", None)  # noqa: E731
                dirs.append((g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh")))
            out.append(dirs)
        return out

    def forward(self, x, hx=None, lengths=None):
        """x [B,T,in] -> (output [B,T,H], (h [L,B,H], c [L,B,H]))."""
        if lengths is not None:
            raise NotImplementedError("packed LSTM sequences (lengths) are not implemented")
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        return native.lstm(x, self.layer_weights(), hx)


def _rnn_init(module):
    """nnet/RNN.py rnn_init: orthogonal recurrent weights (the values are overwritten by any checkpoint)."""
    for name, param in module.named_parameters():
        if "weight_hh" in name or ".u.weight" in name:
            torch.nn.init.orthogonal_(param)


class _NotImplementedRNN(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} is not implemented (transducer prediction networks use LSTM)")


class GRU(_NotImplementedRNN):
    pass


class RNN(_NotImplementedRNN):
    pass


class LiGRU(_NotImplementedRNN):
    pass
