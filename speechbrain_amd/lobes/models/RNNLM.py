"""speechbrain.lobes.models.RNNLM mirror: the recurrent language model of the transducer recipes' "BS + RNNLM" decoding
(lobes/models/RNNLM.py:17-124): Embedding -> dropout -> LSTM -> dnn_blocks x [Linear, LayerNorm, activation, dropout] -> out.

The module keeps the reference's constructor and state_dict keys (``embedding.Embedding.weight``, ``rnn.rnn.weight_ih_l0``,
``dnn.linear.w.weight``, ``dnn.norm.norm.weight``, ``dnn.linear_0...`` for further blocks, ``out.w.weight``), so an ``lm.ckpt``
written by the reference loads through the Pretrainer.  ``forward`` is composed from this package's modules (the LSTM on
sbk_lstm_f32, the Linears and LayerNorms on their kernels); as the ``lm_module`` of a TransducerBeamSearcher the whole model
runs inside sbk_transducer_beam_search_lm_f32 (decoders/transducer.py).  Inference only: dropout is the identity."""
import torch

from speechbrain_amd.nnet.containers import Sequential
from speechbrain_amd.nnet.embedding import Embedding
from speechbrain_amd.nnet.linear import Linear
from speechbrain_amd.nnet.normalization import LayerNorm
from speechbrain_amd.nnet.RNN import LSTM


class RNNLM(torch.nn.Module):
    def __init__(self, output_neurons, embedding_dim=128, activation=torch.nn.LeakyReLU, dropout=0.15, rnn_class=LSTM,
                 rnn_layers=2, rnn_neurons=1024, rnn_re_init=False, return_hidden=False, dnn_blocks=1, dnn_neurons=512):
        super().__init__()
        if not (isinstance(rnn_class, type) and issubclass(rnn_class, LSTM)):
            raise NotImplementedError(f"RNNLM with rnn_class {getattr(rnn_class, '__name__', rnn_class)} is not implemented "
                                      "(LSTM only)")
        self.embedding = Embedding(num_embeddings=output_neurons, embedding_dim=embedding_dim)
        self.dropout = torch.nn.Dropout(p=dropout)
        self.rnn = rnn_class(input_size=embedding_dim, hidden_size=rnn_neurons, num_layers=rnn_layers, dropout=dropout,
                             re_init=rnn_re_init)
        self.return_hidden = return_hidden
        self.reshape = False
        # (the reference appends classes and infers the shapes; this package's Sequential takes explicit modules, and names
        # duplicates as the reference's does: linear, norm, act, dropout, linear_0, norm_0, ...)
        self.dnn = Sequential(input_shape=[None, None, rnn_neurons])
        width = rnn_neurons
        for _ in range(dnn_blocks):
            self.dnn.append(Linear(n_neurons=dnn_neurons, input_size=width, bias=True), layer_name="linear")
            self.dnn.append(LayerNorm(input_size=dnn_neurons), layer_name="norm")
            self.dnn.append(activation(), layer_name="act")
            self.dnn.append(torch.nn.Dropout(p=dropout), layer_name="dropout")
            width = dnn_neurons
        self.out = Linear(input_size=dnn_neurons, n_neurons=output_neurons)

    def forward(self, x, hx=None):
        """x: token ids [B] or [B,T] -> logits [B,V] or [B,T,V] (and (h, c) [L,B,H] with return_hidden).  As in the
        reference, once a 1-d input has been seen the time axis is squeezed out of every later output."""
        x = torch.nn.functional.embedding(x.long(), self.embedding.Embedding.weight)
        if x.ndim == 2:
            x = x.unsqueeze(1)
            self.reshape = True
        x, hidden = self.rnn(x, hx)
        x = self.dnn(x)
        out = self.out(x)
        if self.reshape:
            out = out.squeeze(dim=1)
        return (out, hidden) if self.return_hidden else out

    def blocks(self):
        """[(Linear, LayerNorm, activation module)] per DNN block, in order."""
        layers = [m for m in self.dnn.values() if not isinstance(m, torch.nn.Dropout)]
        return [tuple(layers[i:i + 3]) for i in range(0, len(layers), 3)]
