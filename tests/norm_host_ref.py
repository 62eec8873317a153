"""Plain host restatements of the row kernels: csrc/norm.hip (LayerNorm, the fp8 row quantisation, InputNormalization), the
utterance norm of csrc/wav2vec2.hip and the element conversions of csrc/gemm_lp.hip -- the reference of tests/test_norm_edges.py.

Value functions follow the dtype of their inputs (float64 in: the reference; float32 in: the "fp32 torch composition" whose
own error sets the bound).  The byte functions mirror the kernels' fp32 arithmetic operation by operation with numpy float32
(IEEE division and multiplication) and leave the rounding to torch's own casts.  The keyword arguments that default to the
right behaviour are the planted mistakes of test_cases_tell_mistakes_apart."""
import math

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_SWISH, ACT_GELU, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2, 3, 4


def act(v, code, leaky_slope=0.01, tanh_gelu=False):
    if code == ACT_SWISH:
        return v * torch.sigmoid(v)
    if code == ACT_GELU:
        if tanh_gelu:
            return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
        return 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    if code == ACT_RELU:
        return torch.clamp(v, min=0.0)
    if code == ACT_LEAKY_RELU:
        return torch.where(v > 0, v, leaky_slope * v)
    return v


def layernorm(x, gamma, beta, eps, code=ACT_NONE, unbiased=False, eps_outside=False, **act_kw):
    """act((x - mean) / sqrt(var + eps) * gamma + beta) over the last dimension: two-pass, biased variance."""
    d = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    dev = x - mean
    var = dev.square().sum(-1, keepdim=True) / (d - 1 if unbiased else d)
    rstd = 1.0 / (var.sqrt() + eps) if eps_outside else 1.0 / (var + eps).sqrt()
    return act(dev * rstd * gamma + beta, code, **act_kw)


def input_norm_stats(x, n_valid, per_batch, std_norm, eps, avoid_padding_norm, include_padding=False, clamp_batch=True,
                     clamp_sentence=False):
    """InputNormalization with the statistics of the input itself, x [B,T,C], n_valid[b] frames of utterance b count:
    "sentence" (per_batch False) takes each utterance's own two-pass mean / variance and the root of the variance as it is,
    "batch" those of all valid frames of the batch with the variance clamped at eps before the root; every frame is then
    (x - mean) / max(std, eps), the padded ones with mean 0 and std 1 under avoid_padding_norm."""
    B, T, C = x.shape
    n = [T if include_padding else min(int(v), T) for v in n_valid]
    if per_batch:
        frames = torch.cat([x[b, :n[b]] for b in range(B)], 0)
        mean = frames.mean(0)
        var = (frames - mean).square().mean(0)
        stats = [(mean, torch.clamp(var, min=eps) if clamp_batch else var)] * B
    else:
        stats = []
        for b in range(B):
            mean = x[b, :n[b]].mean(0)
            var = (x[b, :n[b]] - mean).square().mean(0)
            stats.append((mean, torch.clamp(var, min=eps) if clamp_sentence else var))
    y = torch.empty_like(x)
    for b, (mean, var) in enumerate(stats):
        std = var.sqrt() if std_norm else torch.ones_like(var)
        y[b] = (x[b] - mean) / torch.clamp(std, min=eps)
        if avoid_padding_norm:
            y[b, min(int(n_valid[b]), T):] = x[b, min(int(n_valid[b]), T):]
    return y


def input_norm_global(x, mean, std, eps):
    return (x - mean) / torch.clamp(std, min=eps)


def utt_norm(x, eps):
    """F.layer_norm over all n values of each row, no affine."""
    return F.layer_norm(x, x.shape[-1:], None, None, eps)


# ---- bytes -----------------------------------------------------------------------------------------------------------
E4M3_MAX = 448.0


def e4m3_decode(q):
    """uint8 e4m3fn codes -> float32 (torch's own decoder)."""
    return q.contiguous().view(torch.float8_e4m3fn).float()


def e4m3_magnitudes():
    """The 127 finite non-negative e4m3fn values in code order (0x00 ... 0x7e)."""
    return e4m3_decode(torch.arange(0x7f, dtype=torch.uint8))


def e4m3_encode(v, truncate=False):
    """float32 -> e4m3fn codes, saturating at +-448 (+-inf included), round to nearest even (torch's cast); NaN -> 0x7f.
    truncate: towards zero instead (a planted mistake)."""
    v = v.float()
    sat = torch.where(torch.isnan(v), v, torch.clamp(v, -E4M3_MAX, E4M3_MAX))
    if not truncate:
        return sat.to(torch.float8_e4m3fn).view(torch.uint8)
    mags = e4m3_magnitudes().double()
    code = (torch.searchsorted(mags, sat.abs().double().nan_to_num(0.0), right=True) - 1).to(torch.uint8)
    code = code | (torch.signbit(sat).to(torch.uint8) << 7)
    return torch.where(torch.isnan(sat), torch.full_like(code, 0x7f), code)


def quant_rows(x, d=None, divisor=E4M3_MAX, truncate=False, scale_cols=None):
    """rows_fp8_kernel<.., LN = false> on x [rows, ldx] fp32 (the first d columns count): scale = m / 448 with m the row's
    largest finite magnitude (1 for an all-zero row), inv = 1 / scale, byte = e4m3(clip(v * inv)) -- every operation in fp32.
    Returns (bytes [rows, d] uint8, scale [rows] float32)."""
    xn = x.numpy().astype(np.float32)
    d = xn.shape[1] if d is None else d
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax.reduce(np.abs(xn[:, :(d if scale_cols is None else scale_cols)]), axis=1, initial=np.float32(0.0))
        sc = np.where(m > 0, m / np.float32(divisor), np.float32(1.0)).astype(np.float32)
        inv = (np.float32(1.0) / sc).astype(np.float32)
        v = (xn[:, :d] * inv[:, None]).astype(np.float32)
    return e4m3_encode(torch.from_numpy(v), truncate=truncate), torch.from_numpy(sc)


def bf16_bits(x, truncate=False):
    """float32 -> bf16 bit patterns (int16), round to nearest even (torch's cast)."""
    if truncate:
        return (x.contiguous().view(torch.int32) >> 16).to(torch.int16)
    return x.to(torch.bfloat16).view(torch.int16)


def f16_bits(x):
    return x.to(torch.float16).view(torch.int16)


def bits(x):
    """The bit patterns of a float32 tensor (for equality that tells -0 from 0 and compares NaNs)."""
    return x.contiguous().view(torch.int32)
