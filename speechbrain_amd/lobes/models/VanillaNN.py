"""speechbrain.lobes.models.VanillaNN mirror: ``dnn_blocks`` x (Linear + activation), the ``enc`` of the wav2vec 2.0 CTC recipes
(lobes/models/VanillaNN.py:12-51).  The layers are explicit modules under the reference's names (linear, act, linear_0, act_0,
...); each block runs as ONE GEMM with the activation in its epilogue."""
import torch

from speechbrain_amd import native
from speechbrain_amd.nnet.containers import Sequential
from speechbrain_amd.nnet.linear import Linear


def _epilogue_act(act):
    """The GEMM epilogue's code for an activation module (a missing one is an error, not an eager fall-back)."""
    if isinstance(act, torch.nn.LeakyReLU) and act.negative_slope == 0.01:
        return native.ACT_LEAKY_RELU
    if isinstance(act, torch.nn.ReLU):
        return native.ACT_RELU
    if isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none":
        return native.ACT_GELU
    if isinstance(act, torch.nn.SiLU):
        return native.ACT_SWISH
    if isinstance(act, torch.nn.Identity):
        return native.ACT_NONE
    raise NotImplementedError(f"VanillaNN activation {act!r}: LeakyReLU(0.01), ReLU, GELU, SiLU or Identity")


class VanillaNN(Sequential):
    def __init__(self, input_shape, activation=torch.nn.LeakyReLU, dnn_blocks=2, dnn_neurons=512):
        super().__init__(input_shape=input_shape)
        size = input_shape[-1]
        self._blocks = []
        for _ in range(dnn_blocks):
            n = len(self._blocks)
            names = ("linear", "act") if n == 0 else (f"linear_{n - 1}", f"act_{n - 1}")
            self.append(Linear(n_neurons=dnn_neurons, input_size=size, bias=True), layer_name="linear")
            self.append(activation(), layer_name="act")
            assert names[0] in self and names[1] in self
            _epilogue_act(self[names[1]])
            self._blocks.append(names)
            size = dnn_neurons

    def forward(self, x):
        for lin, act in self._blocks:
            x = native.gemm_nt(x.contiguous(), self[lin].w.weight, self[lin].w.bias, act=_epilogue_act(self[act]))
        return x
