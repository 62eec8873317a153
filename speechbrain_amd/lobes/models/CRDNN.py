"""speechbrain.lobes.models.CRDNN mirror: convolution blocks, a bidirectional LSTM stack and linear blocks (CRDNN.py:16-315),
the encoder of the seq2seq and CTC recipes (recipes/LibriSpeech/ASR/seq2seq/hparams/train_BPE_1000.yaml).

The reference builds the model by lazy shape inference; here the shapes are computed in the constructor.  The state_dict keys
are the reference's (``CNN.block_0.conv_1.conv.weight``, ``CNN.block_0.norm_1.norm.weight``, ``RNN.rnn.weight_hh_l0_reverse``,
``DNN.block_0.linear.w.weight``, ``DNN.block_0.norm.norm.running_mean``).  ``forward(x)`` takes no lengths: the reference's
CRDNN is a plain Sequential, so the padded frames take part in the reflect padding and in the recurrence.

On the device (csrc/crdnn.hip, csrc/rnn.hip):
  CNN_Block   conv_1 + norm_1 + act_1: one fused launch for one input channel (native.crdnn_conv1), otherwise a patch matrix per
              run of frames contracted on the matrix cores (native.crdnn_conv) and one LayerNorm + LeakyReLU pass;
              conv_2 the same contraction; norm_2 + act_2 + the frequency pooling (+ CRDNN's time pooling behind the last block)
              in ONE pass that writes only the pooled tensor (native.crdnn_norm_pool)
  RNN         per layer ONE contraction x . [W_ih | W_ih_reverse]^T for both directions, then native.rnn_layer
  DNN_Block   Linear with the BatchNorm1d running statistics folded in and LeakyReLU in the GEMM epilogue

Not implemented (NotImplementedError when the model is constructed): rnn_class GRU / LiGRU / RNN, use_rnnp, projection_dim,
using_2d_pooling, activations other than LeakyReLU, kernels other than 3 x 3."""
import torch

from speechbrain_amd import native
from speechbrain_amd.nnet.CNN import Conv2d
from speechbrain_amd.nnet.containers import Sequential
from speechbrain_amd.nnet.dropout import Dropout2d
from speechbrain_amd.nnet.linear import Linear
from speechbrain_amd.nnet.normalization import BatchNorm1d, LayerNorm
from speechbrain_amd.nnet.pooling import Pooling1d
from speechbrain_amd.nnet.RNN import LSTM


def _leaky_slope(activation):
    """The negative slope of the activation class (or ``!name:`` partial) -- LeakyReLU is what the kernels' epilogues hold."""
    act = activation()
    if type(act) is not torch.nn.LeakyReLU:
        raise NotImplementedError(f"CRDNN: activation {type(act).__name__} is not implemented (torch.nn.LeakyReLU is)")
    if abs(act.negative_slope - 0.01) > 0:
        raise NotImplementedError(f"CRDNN: LeakyReLU(negative_slope={act.negative_slope}) is not implemented (0.01 is)")
    return act


class CNN_Block(Sequential):
    """CRDNN.py:199-278: input [B,T,F,Cin] (or [B,T,F]) -> [B,T,F // pooling_size,channels].  ``time_pool``: CRDNN's time pooling,
    fused into the last block's final pass."""

    def __init__(self, input_shape, channels, kernel_size=[3, 3], activation=torch.nn.LeakyReLU, using_2d_pool=False,
                 pooling_size=2, dropout=0.15):
        super().__init__(input_shape=input_shape)
        if using_2d_pool:
            raise NotImplementedError("CRDNN: using_2d_pooling=True is not implemented")
        if tuple(kernel_size) != (3, 3):
            raise NotImplementedError(f"CRDNN: cnn_kernelsize {tuple(kernel_size)} is not implemented ((3, 3) is)")
        F = input_shape[2]
        cin = 1 if len(input_shape) == 3 else input_shape[3]
        if F * channels > native.CRDNN_MAX_FRAME:
            raise NotImplementedError(f"CRDNN: a frame of {F} x {channels} values exceeds the limit of {native.CRDNN_MAX_FRAME}")
        self.append(Conv2d(out_channels=channels, kernel_size=kernel_size, in_channels=cin), layer_name="conv_1")
        self.append(LayerNorm(input_size=[F, channels]), layer_name="norm_1")
        self.append(_leaky_slope(activation), layer_name="act_1")
        self.append(Conv2d(out_channels=channels, kernel_size=kernel_size, in_channels=channels), layer_name="conv_2")
        self.append(LayerNorm(input_size=[F, channels]), layer_name="norm_2")
        self.append(_leaky_slope(activation), layer_name="act_2")
        self.append(Pooling1d(pool_type="max", input_dims=4, kernel_size=pooling_size, pool_axis=2), layer_name="pooling")
        self.append(Dropout2d(drop_rate=dropout), layer_name="drop")
        self.in_channels, self.channels, self.n_freq = cin, channels, F
        self.output_shape = [None, None, F // pooling_size, channels]
        self._w1, self._w2 = native.Derived(), native.Derived()

    def _conv(self, x, conv, cache):
        w = conv.conv.weight
        # [Cout,Cin,kF,kT] -> [Cout, (kf,kt,ci)]: a patch row is nine runs of Cin contiguous input values
        wk = cache.get((w,), lambda: w.detach().float().permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous())
        return native.crdnn_conv(x, wk, conv.conv.bias.detach())

    def forward(self, x, time_pool=1):
        if x.dim() == 3:
            x = x.unsqueeze(-1)
        x = x.float().contiguous()
        n1, n2 = self["norm_1"], self["norm_2"]
        g = lambda n: (n.norm.weight.detach().reshape(-1), n.norm.bias.detach().reshape(-1))  # noqa: E731
        slope = self["act_1"].negative_slope
        c1 = self["conv_1"]
        if self.in_channels == 1:
            w = c1.conv.weight
            w9 = self._w1.get((w,), lambda: w.detach().float().reshape(w.shape[0], 9).t().contiguous())  # [kf*3+kt, C]
            x = native.crdnn_conv1(x.squeeze(-1), w9, c1.conv.bias.detach(), *g(n1), eps=n1.eps, slope=slope)
        else:
            x = self._conv(x, c1, self._w1)
            x = native.crdnn_norm_pool(x, *g(n1), eps=n1.eps, slope=slope)
        x = self._conv(x, self["conv_2"], self._w2)
        return native.crdnn_norm_pool(x, *g(n2), pool_f=self["pooling"].kernel_size, pool_t=time_pool, eps=n2.eps, slope=slope)


class DNN_Block(Sequential):
    """CRDNN.py:281-315: Linear -> BatchNorm1d -> LeakyReLU -> Dropout as ONE contraction (statistics folded, act in the epilogue)."""

    def __init__(self, input_shape, neurons, activation=torch.nn.LeakyReLU, dropout=0.15):
        super().__init__(input_shape=input_shape)
        self.append(Linear(n_neurons=neurons, input_size=input_shape[-1]), layer_name="linear")
        self.append(BatchNorm1d(input_size=neurons), layer_name="norm")
        self.append(_leaky_slope(activation), layer_name="act")
        self.append(torch.nn.Dropout(p=dropout), layer_name="dropout")
        self.output_shape = list(input_shape[:-1]) + [neurons]
        self._folded = native.Derived()

    def forward(self, x):
        lin, norm = self["linear"].w, self["norm"]
        wf, bf = self._folded.get([lin.weight, lin.bias] + norm.sources(), lambda: norm.fold(lin.weight, lin.bias),
                                  extra=(norm.norm.eps,))
        with native.precision_scope("fp32"):  # (as the convolutions and the input projections: CRDNN is an fp32 model here)
            return native.gemm_nt(x.contiguous(), wf, bf, act=native.ACT_LEAKY_RELU)


class CRDNN(Sequential):
    """CRDNN.py:16-196 with the reference's constructor arguments; [B,T,n_mels] -> [B,T // time_pooling_size,dnn_neurons]."""

    def __init__(self, input_size=None, input_shape=None, activation=torch.nn.LeakyReLU, dropout=0.15, cnn_blocks=2,
                 cnn_channels=[128, 256], cnn_kernelsize=(3, 3), time_pooling=False, time_pooling_size=2, freq_pooling_size=2,
                 rnn_class=None, inter_layer_pooling_size=[2, 2], using_2d_pooling=False, rnn_layers=4, rnn_neurons=512,
                 rnn_bidirectional=True, rnn_re_init=False, dnn_blocks=2, dnn_neurons=512, projection_dim=-1, use_rnnp=False):
        if input_size is None and input_shape is None:
            raise ValueError("Must specify one of input_size or input_shape")
        if input_shape is None:
            input_shape = [None, None, input_size]
        super().__init__(input_shape=input_shape)
        if using_2d_pooling:
            raise NotImplementedError("CRDNN: using_2d_pooling=True is not implemented")
        if cnn_blocks < 1:
            raise NotImplementedError("CRDNN: cnn_blocks=0 is not implemented")
        if rnn_layers < 1 and dnn_blocks > 0:
            raise NotImplementedError("CRDNN: rnn_layers=0 (DNN blocks directly behind the CNN) is not implemented")
        if projection_dim != -1:
            raise NotImplementedError("CRDNN: projection_dim != -1 is not implemented")
        if use_rnnp:
            raise NotImplementedError("CRDNN: use_rnnp=True is not implemented")
        if rnn_layers > 0 and rnn_class is not LSTM:
            name = getattr(rnn_class, "__name__", "LiGRU (the reference's default)" if rnn_class is None else repr(rnn_class))
            raise NotImplementedError(f"CRDNN: rnn_class {name} is not implemented (speechbrain.nnet.RNN.LSTM is)")
        if rnn_layers > 0 and rnn_neurons > native.RNN_MAX_HIDDEN:
            raise NotImplementedError(f"CRDNN: rnn_neurons={rnn_neurons} exceeds the limit of {native.RNN_MAX_HIDDEN}")
        shape = list(input_shape)
        if cnn_blocks > 0:
            self.append(Sequential(input_shape=shape), layer_name="CNN")
        for i in range(cnn_blocks):
            block = CNN_Block(shape, channels=cnn_channels[i], kernel_size=cnn_kernelsize, using_2d_pool=using_2d_pooling,
                              pooling_size=inter_layer_pooling_size[i], activation=activation, dropout=dropout)
            self["CNN"].append(block, layer_name=f"block_{i}")
            shape = block.output_shape
        self.time_pool = 1
        if time_pooling:
            self.append(Pooling1d(pool_type="max", input_dims=4, kernel_size=time_pooling_size, pool_axis=1),
                        layer_name="time_pooling")
            self.time_pool = int(time_pooling_size)
        if rnn_layers > 0:
            self.append(LSTM(hidden_size=rnn_neurons, input_shape=shape, num_layers=rnn_layers, dropout=dropout,
                             bidirectional=rnn_bidirectional, re_init=rnn_re_init), layer_name="RNN")
            shape = [None, None, rnn_neurons * (2 if rnn_bidirectional else 1)]
        if dnn_blocks > 0:
            self.append(Sequential(input_shape=shape), layer_name="DNN")
        for i in range(dnn_blocks):
            block = DNN_Block(shape, neurons=dnn_neurons, activation=activation, dropout=dropout)
            self["DNN"].append(block, layer_name=f"block_{i}")
            shape = block.output_shape
        self._rnn_derived = native.Derived()

    def cnn_forward(self, x, return_blocks=False):
        """The convolution blocks and the time pooling: [B,T,n_mels] -> [B,T',F',C]; with ``return_blocks`` also each block's own
        output (the last block then runs twice: once without the time pooling for the record, once as it runs otherwise)."""
        blocks = list(self["CNN"].values())
        outs = []
        for i, block in enumerate(blocks):
            if i == len(blocks) - 1:
                if return_blocks:
                    outs.append(block(x))
                x = block(x, time_pool=self.time_pool)
            else:
                x = block(x)
                outs.append(x)
        return (x, outs) if return_blocks else x

    def _rnn_weights(self):
        """Per layer: (W_ih of the directions stacked [D*4H, in], w_hh [D,4H,H], b_ih [D,4H] or None, b_hh)."""
        rnn = self["RNN"]
        dirs = rnn.direction_weights()
        flat = [t for layer in dirs for d in layer for t in d]

        def build():
            out = []
            for layer in dirs:
                f = lambda k: [d[k].detach().float() for d in layer]  # noqa: E731
                bias = layer[0][2] is not None
                out.append((torch.cat(f(0), dim=0).contiguous(), torch.stack(f(1)).contiguous(),
                            torch.stack(f(2)).contiguous() if bias else None, torch.stack(f(3)).contiguous() if bias else None))
            return out

        return self._rnn_derived.get(flat, build)

    def rnn_forward(self, x, return_layers=False):
        """The LSTM stack on [B,T',F',C] (flattened F major, as the reference's reshape) or [B,T',in] -> [B,T',D*H]."""
        if x.dim() == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        outs = []
        for w_ih, w_hh, b_ih, b_hh in self._rnn_weights():
            B, T, _ = x.shape
            D, H = w_hh.shape[0], w_hh.shape[2]
            with native.precision_scope("fp32"):
                xp = native.gemm_nt(x.contiguous(), w_ih)  # [B,T,D*4H]: both directions in one contraction
            x, _, _ = native.rnn_layer(xp.view(B, T, D, 4 * H), w_hh, b_ih, b_hh)
            outs.append(x)
        return (x, outs) if return_layers else x

    def forward(self, x, return_stages=False):
        stages = {}
        if return_stages:
            x, blocks = self.cnn_forward(x, return_blocks=True)
            stages.update({f"cnn_block{i}": b for i, b in enumerate(blocks)})
            stages["time_pooling"] = x
        else:
            x = self.cnn_forward(x)
        if "RNN" in self:
            x, layers = self.rnn_forward(x, return_layers=True)
            stages.update({f"lstm_layer{i}": y for i, y in enumerate(layers)})
        if "DNN" in self:
            for i, block in enumerate(self["DNN"].values()):
                x = block(x)
                stages[f"dnn_block{i}"] = x
        return (x, stages) if return_stages else x

