"""speechbrain.nnet.normalization mirror (LayerNorm, and BatchNorm1d with its inference semantics)."""
import torch

from speechbrain_amd import native


class LayerNorm(torch.nn.Module):
    """nnet/normalization.py:185-242: normalises over input_size (or input_shape[2:])."""

    def __init__(self, input_size=None, input_shape=None, eps=1e-05, elementwise_affine=True):
        super().__init__()
        if not elementwise_affine:
            raise NotImplementedError("affine-free LayerNorm is not on the ASR path")
        self.eps = eps
        if input_shape is not None:
            input_size = input_shape[2:]
        self.norm = torch.nn.LayerNorm(input_size, eps=self.eps, elementwise_affine=True)

    def forward(self, x):
        return native.layernorm(x.contiguous(), self.norm.weight.reshape(-1), self.norm.bias.reshape(-1), self.eps)


class BatchNorm1d(torch.nn.Module):
    """nnet/normalization.py:13-108 at inference: y = (x - running_mean) / sqrt(running_var + eps) * weight + bias on the last
    dimension.  A parameter holder with the reference's names (``norm.weight``, ``norm.running_mean``, ...): the affine map is
    folded into the Linear in front of it (``fold``; lobes.models.CRDNN.DNN_Block keeps the folded weights in a derived-weights
    cache keyed on the parameters AND the running statistics, so a checkpoint loaded later is picked up)."""

    def __init__(self, input_shape=None, input_size=None, eps=1e-05, momentum=0.1, affine=True, track_running_stats=True,
                 combine_batch_time=False, skip_transpose=False):
        super().__init__()
        if not affine or not track_running_stats:
            raise NotImplementedError("BatchNorm1d without affine parameters or running statistics is not on the ASR path")
        if input_size is None:
            input_size = input_shape[1] if skip_transpose else input_shape[-1]
        self.combine_batch_time, self.skip_transpose = combine_batch_time, skip_transpose
        self.norm = torch.nn.BatchNorm1d(input_size, eps=eps, momentum=momentum, affine=True, track_running_stats=True)

    def sources(self):
        n = self.norm
        return [n.weight, n.bias, n.running_mean, n.running_var]

    def fold(self, w, b):
        """(W', b') with BatchNorm(x W^T + b) = x W'^T + b' (w [N,K], b [N] or None)."""
        n = self.norm
        scale = n.weight.detach().float() / torch.sqrt(n.running_var.float() + n.eps)
        b0 = b.detach().float() if b is not None else torch.zeros_like(scale)
        return (w.detach().float() * scale[:, None]).contiguous(), ((b0 - n.running_mean.float()) * scale + n.bias.detach().float()).contiguous()

    def forward(self, x):
        raise RuntimeError("BatchNorm1d runs folded into the preceding Linear inside DNN_Block on this path")
