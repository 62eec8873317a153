"""speechbrain.nnet.activations mirror: only what the ASR paths instantiate."""
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


class Softmax(torch.nn.Module):
    """nnet/activations.py:16-86 -- the ``log_softmax`` of the wav2vec 2.0 CTC recipes is ``Softmax(apply_log=True)``: over the
    last dimension, on sbk_log_softmax_f32.  (The reference's reshape of 3-d / 4-d inputs changes nothing for the last dim.)"""

    def __init__(self, apply_log=False, dim=-1, reshape=True, dtype=torch.float32):
        super().__init__()
        if not apply_log:
            raise NotImplementedError("Softmax(apply_log=False): only the log form has a kernel (the CTC heads use it)")
        if dtype != torch.float32:
            raise NotImplementedError(f"Softmax(dtype={dtype}): fp32 only")
        self.apply_log, self.dim, self.reshape, self.dtype = apply_log, dim, reshape, dtype

    def forward(self, x):
        from speechbrain_amd import native

        if self.dim not in (-1, x.dim() - 1):
            raise NotImplementedError(f"Softmax over dim {self.dim} of a {x.dim()}-d tensor: last dimension only")
        return native.log_softmax(x.contiguous())


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
