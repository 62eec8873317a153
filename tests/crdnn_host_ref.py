"""Plain-torch restatement of the CRDNN encoder (lobes/models/CRDNN.py of the reference) in any dtype: what the kernel tests
compare against in fp64, and what tools/make_crdnn_golden.py checks stage by stage against the reference itself before it writes
a fixture.  Every keyword that defaults to the right behaviour is a planted mistake for ``test_cases_tell_mistakes_apart``."""
import torch
import torch.nn.functional as F


def cast(t, dtype):
    if t is None:
        return None
    if isinstance(t, (tuple, list)):
        return type(t)(cast(v, dtype) for v in t)
    return t.to(dtype) if t.is_floating_point() else t


def cast_dict(sd, dtype):
    return {k: cast(v, dtype) for k, v in sd.items()}


# ------------------------------------------------------------------ recurrent layer
def lstm_layer(x, w_ih, w_hh, b_ih=None, b_hh=None, h0=None, c0=None, gate_order="ifgo", backward_in_scan_order=False,
               drop_b_hh=False, swap_w_hh=False, carry_c=True, use_h0=True, backward_first=False):
    """torch.nn.LSTM(batch_first=True), one layer: x [B,T,in], w_ih [D,4H,in], w_hh [D,4H,H], b_* [D,4H] or None,
    h0 / c0 [D,B,H] or None -> (out [B,T,D*H] = [fwd|bwd], hn [D,B,H], cn [D,B,H])."""
    B, T, _ = x.shape
    D, H = w_hh.shape[0], w_hh.shape[2]
    pos = {g: gate_order.index(g) for g in "ifgo"}
    outs, hn, cn = [], [], []
    for d in range(D):
        whh = w_hh[(D - 1 - d) if swap_w_hh else d]
        h = h0[d] if (h0 is not None and use_h0) else x.new_zeros(B, H)
        c = c0[d] if c0 is not None else x.new_zeros(B, H)
        c_init = c
        ys = [None] * T
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            g = x[:, t] @ w_ih[d].T + h @ whh.T
            if b_ih is not None:
                g = g + b_ih[d] + (0 if drop_b_hh else b_hh[d])
            q = g.reshape(B, 4, H)
            i, f = torch.sigmoid(q[:, pos["i"]]), torch.sigmoid(q[:, pos["f"]])
            gg, o = torch.tanh(q[:, pos["g"]]), torch.sigmoid(q[:, pos["o"]])
            c = f * (c if carry_c else c_init) + i * gg
            h = o * torch.tanh(c)
            ys[s if (d == 1 and backward_in_scan_order) else t] = h
        outs.append(torch.stack(ys, dim=1))
        hn.append(h)
        cn.append(c)
    if backward_first:
        outs = outs[::-1]
    return torch.cat(outs, dim=-1), torch.stack(hn), torch.stack(cn)


def lstm_weights(sd, prefix, layer, D):
    """(w_ih [D,4H,in], w_hh [D,4H,H], b_ih [D,4H], b_hh [D,4H]) of layer ``layer`` from torch.nn.LSTM's keys."""
    sfx = ["", "_reverse"][:D]
    g = lambda n: torch.stack([sd[f"{prefix}{n}_l{layer}{s}"] for s in sfx])  # noqa: E731
    has_bias = f"{prefix}bias_ih_l{layer}" in sd
    return g("weight_ih"), g("weight_hh"), (g("bias_ih") if has_bias else None), (g("bias_hh") if has_bias else None)


# ------------------------------------------------------------------ convolution blocks
def conv3x3(x, w, bias, zero_pad=False, transpose_taps=False):
    """nnet/CNN.py Conv2d(3x3, stride 1, padding "same", reflect): x [B,T,F,Cin], w [Cout,Cin,kF,kT] -> [B,T,F,Cout]."""
    if x.shape[1] < 2 or x.shape[2] < 2:
        raise ValueError("reflect padding of 1 needs at least 2 frames and 2 bins")
    if transpose_taps:
        w = w.transpose(2, 3)
    xc = x.permute(0, 3, 2, 1)  # [B,Cin,F,T]
    xc = F.pad(xc, (1, 1, 1, 1), mode="constant" if zero_pad else "reflect")
    return F.conv2d(xc, w, bias).permute(0, 3, 2, 1)


def norm_act(x, gamma, beta, eps=1e-5, slope=0.01, over_c_only=False):
    """LayerNorm over (F,C) of x [B,T,F,C] (gamma / beta [F,C]) + LeakyReLU."""
    dims = (-1,) if over_c_only else (-2, -1)
    mean = x.mean(dim=dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=dims, keepdim=True)
    return F.leaky_relu((x - mean) / torch.sqrt(var + eps) * gamma + beta, slope)


def max_pool(x, axis, k):
    """nnet/pooling.py Pooling1d("max", kernel = stride = k, floor) over ``axis`` of x [B,T,F,C]."""
    n = x.shape[axis] // k
    if n < 1:
        raise ValueError(f"pooling {x.shape[axis]} by {k} leaves an empty output")
    x = x.narrow(axis, 0, n * k)
    shape = list(x.shape)
    shape[axis:axis + 1] = [n, k]
    return x.reshape(shape).amax(dim=axis + 1)


def cnn_block(x, sd, prefix, pool, eps=1e-5, slope=0.01, **mut):
    """CNN_Block (CRDNN.py:199-278): x [B,T,F,Cin] -> [B,T,F//pool,C]."""
    conv_mut = {k: v for k, v in mut.items() if k in ("zero_pad", "transpose_taps")}
    norm_mut = {k: v for k, v in mut.items() if k in ("over_c_only",)}
    for i in (1, 2):
        x = conv3x3(x, sd[f"{prefix}conv_{i}.conv.weight"], sd[f"{prefix}conv_{i}.conv.bias"], **conv_mut)
        x = norm_act(x, sd[f"{prefix}norm_{i}.norm.weight"], sd[f"{prefix}norm_{i}.norm.bias"], eps, slope, **norm_mut)
    return max_pool(x, 2, pool)


def dnn_block(x, sd, prefix, eps=1e-5, slope=0.01, batch_statistics=False):
    """DNN_Block (CRDNN.py:281-315): Linear -> BatchNorm1d (eval: running statistics) -> LeakyReLU."""
    y = x @ sd[f"{prefix}linear.w.weight"].T + sd[f"{prefix}linear.w.bias"]
    if batch_statistics:
        mean, var = y.mean(dim=(0, 1)), y.var(dim=(0, 1), unbiased=False)
    else:
        mean, var = sd[f"{prefix}norm.norm.running_mean"], sd[f"{prefix}norm.norm.running_var"]
    y = (y - mean) / torch.sqrt(var + eps) * sd[f"{prefix}norm.norm.weight"] + sd[f"{prefix}norm.norm.bias"]
    return F.leaky_relu(y, slope)


def crdnn(feats, sd, cnn_pools, time_pool, rnn_layers, bidirectional, dnn_blocks, prefix="", c_major=False, **mut):
    """CRDNN.forward on feats [B,T,n_mels] -> (output [B,T',dnn], stages: a dict of every intermediate the golden records)."""
    lstm_mut = {k: v for k, v in mut.items() if k in ("gate_order", "backward_in_scan_order", "drop_b_hh", "swap_w_hh",
                                                       "carry_c", "backward_first")}
    cnn_mut = {k: v for k, v in mut.items() if k in ("zero_pad", "transpose_taps", "over_c_only")}
    dnn_mut = {k: v for k, v in mut.items() if k in ("batch_statistics",)}
    stages = {}
    x = feats.unsqueeze(-1)
    for i, p in enumerate(cnn_pools):
        x = cnn_block(x, sd, f"{prefix}CNN.block_{i}.", p, **cnn_mut)
        stages[f"cnn_block{i}"] = x
    if time_pool > 1:
        x = max_pool(x, 1, time_pool)
    stages["time_pooling"] = x
    if c_major:
        x = x.transpose(2, 3)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    D = 2 if bidirectional else 1
    for l in range(rnn_layers):
        x, _, _ = lstm_layer(x, *lstm_weights(sd, f"{prefix}RNN.rnn.", l, D), **lstm_mut)
        stages[f"lstm_layer{l}"] = x
    for i in range(dnn_blocks):
        x = dnn_block(x, sd, f"{prefix}DNN.block_{i}.", **dnn_mut)
        stages[f"dnn_block{i}"] = x
    return x, stages
