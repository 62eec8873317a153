"""speechbrain.lobes.models.convolution mirror: ConvolutionFrontEnd / ConvBlock (convolution.py:116-320)."""
from typing import List

import torch

from speechbrain_amd import native
from speechbrain_amd.nnet.CNN import Conv2d
from speechbrain_amd.nnet.normalization import LayerNorm


class _NamedChildren(torch.nn.ModuleDict):
    pass


def _gate_act_code(m) -> int:
    """Act code of the CSGU gate: Identity (the recipes') and the activations csrc/csgu.hip applies on the way out."""
    if isinstance(m, torch.nn.Identity):
        return native.ACT_NONE
    from speechbrain_amd.nnet.attention import _act_code

    try:
        code = _act_code(m)
    except NotImplementedError:
        code = None
    if code not in native.CSGU_GATE_ACTS:
        raise NotImplementedError(f"gate_activation {type(m).__name__}: Identity, Swish / SiLU, GELU and ReLU are fused into the CSGU kernel")
    return code


class ConvolutionalSpatialGatingUnit(torch.nn.Module):
    """CSGU of the Branchformer cgMLP branch (convolution.py:22-113): x1, x2 = x.chunk(2, -1); act(conv(LayerNorm(x2))) * x1
    with a depthwise reflect-padded convolution over time -- one fused kernel (native.csgu) after a per-frame statistics pass.
    [B,T,D] -> [B,T,D/2]; state_dict: norm.norm.{weight,bias}, conv.conv.{weight [D/2,1,k], bias}."""

    def __init__(self, input_size: int, kernel_size: int = 31, dropout: float = 0.0, use_linear_after_conv: bool = False,
                 activation=torch.nn.Identity):
        super().__init__()
        from speechbrain_amd.nnet.CNN import Conv1d

        if use_linear_after_conv:
            raise NotImplementedError("use_linear_after_conv=True (a Linear between the CSGU convolution and its gate) is not implemented")
        self.input_size, self.use_linear_after_conv = input_size, use_linear_after_conv
        self.activation = activation()
        self.act_code = _gate_act_code(self.activation)
        if self.input_size % 2 != 0:
            raise ValueError("Input size must be divisible by 2!")
        n_channels = input_size // 2
        if kernel_size not in native.CSGU_KERNEL_SIZES:
            raise NotImplementedError(f"CSGU kernel_size {kernel_size}: the kernel is instantiated for {native.CSGU_KERNEL_SIZES}")
        self.kernel_size = kernel_size
        self.norm = LayerNorm(n_channels)
        self.conv = Conv1d(input_shape=(None, None, n_channels), out_channels=n_channels, kernel_size=kernel_size, stride=1,
                           padding="same", groups=n_channels, conv_init="normal", skip_transpose=False)
        torch.nn.init.ones_(self.conv.conv.bias)
        self.dropout = torch.nn.Dropout(dropout)

    def forward(self, x, out=None):
        C = self.input_size // 2
        halo = (self.kernel_size - 1) // 2
        if x.shape[-2] <= halo:  # (the reference's F.pad(mode="reflect") raises here too)
            raise ValueError(f"CSGU: a sequence of T={x.shape[-2]} frames cannot be reflect-padded by {halo} (kernel_size={self.kernel_size})")
        return native.csgu(x.contiguous(), self.norm.norm.weight, self.norm.norm.bias, self.norm.eps,
                           self.conv.conv.weight.reshape(C, self.kernel_size), self.conv.conv.bias, self.kernel_size,
                           self.act_code, out=out)


class ConvBlock(torch.nn.Module):
    """One fused HIP launch per block, for the block shapes of the ASR recipes (one layer per block):
      (kernel_size, stride, residual) = (3, 2, False) / (5, 2, False): conv (reflect 'same') -> LayerNorm(F',C') -> LeakyReLU
      (1, 1, True): LeakyReLU(LayerNorm(conv1x1(x))) + LayerNorm(reduce_conv1x1(x))       (transformer.yaml's third block)
    State-dict keys as in the reference: convs.conv_0 / convs.norm_0 and, for the residual block, reduce_conv.conv / reduce_conv.norm."""

    SHAPES = ((3, 2, False), (5, 2, False), (1, 1, True))

    def __init__(self, num_layers, out_channels, input_shape, kernel_size=3, stride=1, dilation=1, residual=False,
                 conv_module=Conv2d, activation=torch.nn.LeakyReLU, norm=LayerNorm, dropout=0.1, conv_bias=True,
                 padding="same", conv_init=None):
        super().__init__()
        if num_layers != 1:
            raise NotImplementedError(f"ConvBlock num_layers={num_layers}: one layer per block is implemented")
        if dilation != 1:
            raise NotImplementedError(f"ConvBlock dilation={dilation}: only dilation 1 is implemented")
        if padding != "same":
            raise NotImplementedError(f"ConvBlock padding={padding!r}: only 'same' (reflect) is implemented")
        if (kernel_size, stride, bool(residual)) not in self.SHAPES:
            raise NotImplementedError(f"ConvBlock (kernel_size, stride, residual) = ({kernel_size}, {stride}, {bool(residual)}): "
                                      f"the fused kernels cover {self.SHAPES}")
        if conv_module is not Conv2d or norm is not LayerNorm or activation is not torch.nn.LeakyReLU:
            raise NotImplementedError("ConvBlock is fused for Conv2d + LayerNorm + LeakyReLU")
        if not conv_bias:
            raise NotImplementedError("ConvBlock conv_bias=False is not implemented")
        B, T, F = input_shape[0], input_shape[1], input_shape[2]
        cin = 1 if len(input_shape) == 3 else input_shape[3]
        self.kernel_size, self.stride, self.residual = kernel_size, stride, bool(residual)
        if stride == 2:  # get_padding_elem (nnet/CNN.py): kernel_size // 2 on each side -> (n - 1) // 2 + 1 for 3 and 5
            self.out_shape = (B, None if T is None else (T - 1) // 2 + 1, (F - 1) // 2 + 1, out_channels)
        else:
            self.out_shape = (B, T, F, out_channels)
        if self.residual and 256 % out_channels != 0:
            raise NotImplementedError(f"residual ConvBlock out_channels={out_channels}: the fused kernel takes a divisor of 256")
        self.convs = _NamedChildren()
        self.convs["conv_0"] = Conv2d(out_channels, kernel_size, in_channels=cin, stride=stride, bias=conv_bias,
                                      conv_init=conv_init)
        self.convs["norm_0"] = LayerNorm(input_shape=self.out_shape)
        self.convs["act_0"] = activation()
        self.convs["dropout_0"] = torch.nn.Dropout(dropout)
        self.reduce_conv = self.drop = None
        if self.residual:
            self.reduce_conv = _NamedChildren()
            self.reduce_conv["conv"] = Conv2d(out_channels, 1, in_channels=cin, stride=stride)
            self.reduce_conv["norm"] = LayerNorm(input_shape=self.out_shape)
            self.drop = torch.nn.Dropout(dropout)
        self._wt_derived = native.Derived()

    def get_filter_properties(self):
        """convolution.py:283-320: the block's one layer."""
        from speechbrain_amd.utils.filter_analysis import FilterProperties

        return FilterProperties(window_size=self.kernel_size, stride=self.stride, dilation=1)

    def _wt(self):
        w = self.convs["conv_0"].conv.weight
        if self.residual:  # the two 1x1 weights [Cout,Cin,1,1] -> [Cin,Cout]
            w2 = self.reduce_conv["conv"].conv.weight
            return self._wt_derived.get((w, w2), lambda: (w.detach().reshape(w.shape[0], -1).t().contiguous(),
                                                          w2.detach().reshape(w2.shape[0], -1).t().contiguous()))
        if self.kernel_size == 3:
            # [Cout,Cin,kF,kT] -> [(ci,kf,kt), Cout]: coalesced across output channels in the kernel
            return self._wt_derived.get((w,), lambda: w.detach().permute(1, 2, 3, 0).reshape(-1, w.shape[0]).contiguous())
        return self._wt_derived.get((w,), lambda: native.conv_block_weight(w, self.kernel_size))

    def forward(self, x):
        if x.dim() == 3:
            x = x.unsqueeze(-1)
        conv, norm = self.convs["conv_0"], self.convs["norm_0"]
        slope = self.convs["act_0"].negative_slope
        if self.residual:
            w1t, w2t = self._wt()
            rconv, rnorm = self.reduce_conv["conv"], self.reduce_conv["norm"]
            return native.conv_block_res1x1(x.contiguous(), w1t, conv.conv.bias, norm.norm.weight.reshape(-1),
                                            norm.norm.bias.reshape(-1), norm.eps, w2t, rconv.conv.bias,
                                            rnorm.norm.weight.reshape(-1), rnorm.norm.bias.reshape(-1), rnorm.eps,
                                            conv.out_channels, slope=slope)
        if self.kernel_size == 3:
            return native.conv_block(x.contiguous(), self._wt(), conv.conv.bias, norm.norm.weight.reshape(-1),
                                     norm.norm.bias.reshape(-1), conv.out_channels, eps=norm.eps, slope=slope)
        return native.conv_block_k(x.contiguous(), self._wt(), conv.conv.bias, norm.norm.weight.reshape(-1),
                                   norm.norm.bias.reshape(-1), conv.out_channels, self.kernel_size, self.stride, eps=norm.eps,
                                   slope=slope)


class ConvolutionFrontEnd(torch.nn.ModuleDict):
    """Stack of ConvBlocks, [B,T,F] -> [B,T',F',C]; children are named convblock_{i} as in the reference."""

    def __init__(self, input_shape, num_blocks=3, num_layers_per_block=5, out_channels: List[int] = [128, 256, 512],
                 kernel_sizes: List[int] = [3, 3, 3], strides: List[int] = [1, 2, 2], dilations: List[int] = [1, 1, 1],
                 residuals: List[bool] = [True, True, True], conv_module=Conv2d, activation=torch.nn.LeakyReLU,
                 norm=LayerNorm, dropout=0.1, conv_bias=True, padding="same", conv_init=None):
        super().__init__()
        shape = tuple(input_shape)
        for i in range(num_blocks):
            block = ConvBlock(num_layers=num_layers_per_block, out_channels=out_channels[i], input_shape=shape,
                              kernel_size=kernel_sizes[i], stride=strides[i], dilation=dilations[i],
                              residual=residuals[i], conv_module=conv_module, activation=activation, norm=norm,
                              dropout=dropout, conv_bias=conv_bias, padding=padding, conv_init=conv_init)
            self[f"convblock_{i}"] = block
            shape = block.out_shape

    def forward(self, x):
        for block in self.values():
            x = block(x)
        return x

    def get_filter_properties(self):
        """convolution.py:200-203."""
        from speechbrain_amd.utils.filter_analysis import stack_filter_properties

        return stack_filter_properties(block.get_filter_properties() for block in self.values())
