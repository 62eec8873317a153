"""speechbrain.nnet.pooling mirror: the Pooling1d configurations a CRDNN instantiates (nnet/pooling.py:21-133).

Max pooling over the time (1) or the frequency (2) axis of a 4-D [B,T,F,C] activation, kernel = stride, floor.  Inside a CRDNN
the pooling runs fused behind the LayerNorm + LeakyReLU that precede it (csrc/crdnn.hip, driven by lobes.models.CRDNN); this
module carries the configuration and has no parameters."""
import torch


class Pooling1d(torch.nn.Module):
    def __init__(self, pool_type, kernel_size, input_dims=3, pool_axis=1, ceil_mode=False, padding=0, dilation=1, stride=None):
        super().__init__()
        if stride is None:
            stride = kernel_size
        if (pool_type != "max" or input_dims != 4 or pool_axis not in (1, 2) or ceil_mode or padding != 0 or dilation != 1
                or stride != kernel_size):
            raise NotImplementedError("Pooling1d: max pooling over axis 1 or 2 of a 4-D input with kernel = stride, floor, is "
                                      "implemented (the configurations of CRDNN)")
        self.pool_type, self.kernel_size, self.pool_axis, self.stride = pool_type, int(kernel_size), pool_axis, int(stride)

    def forward(self, x):
        raise RuntimeError("Pooling1d runs fused inside CRDNN (LayerNorm + LeakyReLU + pooling) on this path")

