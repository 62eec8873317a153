"""speechbrain.nnet.activations mirror: only what the Conformer path instantiates."""
import torch


class Swish(torch.nn.Module):
    """x * sigmoid(beta * x) (nnet/activations.py:133-171).  On the MI355X path the
    activation is fused into the producing kernel's epilogue; this module is the
    constructor-compatible marker the lobes inspect."""

    def __init__(self, beta: float = 1.0):
        super().__init__()
        self.beta = beta
        if beta != 1.0:
            raise NotImplementedError("Swish beta != 1 is not on the ASR path")

    def forward(self, x):
        raise RuntimeError("Swish is fused into the HIP epilogues; it is never called stand-alone on this path")


class NativeLogSoftmax(torch.nn.Module):
    """``torch.nn.LogSoftmax(dim=-1)`` on sbk_log_softmax_f32 (same empty state_dict).  EncoderASR puts it in place of
    every LogSoftmax child over the last dimension of its encoder, so the CTC head's normalisation runs on the project's
    kernel instead of ATen's."""

    def __init__(self, dim=-1):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        from speechbrain_amd import native

        if self.dim not in (-1, x.dim() - 1):
            raise NotImplementedError(f"NativeLogSoftmax over dim {self.dim} of a {x.dim()}-d tensor: last dimension only")
        return native.log_softmax(x.contiguous())

    @staticmethod
    def replace_in(module):
        """Swap the LogSoftmax children over the last dimension of ``module`` (recursively); returns how many."""
        n = 0
        for name, child in list(module.named_children()):
            if type(child) is torch.nn.LogSoftmax and child.dim in (-1, 2):
                setattr(module, name, NativeLogSoftmax(child.dim))
                n += 1
            else:
                n += NativeLogSoftmax.replace_in(child)
        return n
