"""speechbrain.nnet.dropout mirror (nnet/dropout.py:16-58): channel dropout is the identity at inference."""
import torch


class Dropout2d(torch.nn.Module):
    def __init__(self, drop_rate, inplace=False):
        super().__init__()
        self.drop_rate, self.inplace = drop_rate, inplace

    def forward(self, x):
        return x
