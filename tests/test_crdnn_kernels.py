"""csrc/crdnn.hip -- the convolution blocks of a CRDNN (native.crdnn_conv1 / crdnn_conv / crdnn_norm_pool, driven by
lobes.models.CRDNN.CNN_Block) and the folded DNN block -- against the fp64 restatement tests/crdnn_host_ref.py, on the CPU
emulator of the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_wav2vec2_kernels.py): max(4 x the fp32 torch composition's own error against fp64 on the
same inputs, 1e-5)."""
import functools
import os

import numpy as np
import pytest
import torch

import crdnn_host_ref as R
from speechbrain_amd import native
from speechbrain_amd.lobes.models.CRDNN import CNN_Block, DNN_Block

# (B, T, F, Cin, Cout, pool): odd F and odd T; the shortest T the reflect padding admits; more input channels
BLOCKS = [(2, 5, 7, 1, 4, 2), (1, 2, 4, 1, 8, 2), (2, 9, 10, 8, 16, 2)]
GPU_BLOCK = (1, 6, 40, 128, 128, 2)  # the recipe's second convolution width (K = 1152): on the GPU only
TIME_POOLS = [(2, 9, 4), (2, 7, 4), (2, 9, 3)]  # (block index, T, time pooling): T no multiple of the pooling
_CASES = {}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bound(err32):
    return max(4.0 * err32, 1e-5)


def _block_case(shape, T=None, time_pool=1):
    """A block's parameters (random affines), its input, the fp64 result and the fp32 composition's error; made once."""
    B, T0, F, Cin, Cout, pool = shape
    T = T or T0
    key = (shape, T, time_pool)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(sum(shape) * 31 + T * 7 + time_pool)
        rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        sd = {}
        for i, ci in ((1, Cin), (2, Cout)):
            sd[f"conv_{i}.conv.weight"] = rn(Cout, ci, 3, 3) / (3.0 * ci ** 0.5)
            sd[f"conv_{i}.conv.bias"] = 0.5 * rn(Cout)
            sd[f"norm_{i}.norm.weight"] = 1.0 + 0.3 * rn(F, Cout)
            sd[f"norm_{i}.norm.bias"] = 0.3 * rn(F, Cout)
        x = rn(B, T, F, Cin) + 0.5  # an offset: zero padding is then visibly not reflect padding
        host = lambda dt: R.max_pool(R.cnn_block(x.to(dt), R.cast_dict(sd, dt), "", pool), 1, time_pool)  # noqa: E731
        ref = host(torch.float64)
        err32 = float((host(torch.float32).double() - ref).abs().max())
        _CASES[key] = (sd, x, ref, err32)
    return _CASES[key]


def _run_block(dev, shape, sd, x, time_pool=1):
    B, T, F, Cin, Cout, pool = shape
    blk = CNN_Block([None, None, F] if Cin == 1 else [None, None, F, Cin], channels=Cout, pooling_size=pool).eval()
    blk.load_state_dict(sd, strict=True)
    blk = blk.to(dev)
    with torch.no_grad():
        return blk(x.squeeze(-1).to(dev) if Cin == 1 else x.to(dev), time_pool=time_pool)


@pytest.mark.parametrize("shape", BLOCKS, ids=lambda s: "x".join(map(str, s)))
def test_block_vs_fp64_restatement(backend, shape):
    nat, dev = backend
    sd, x, ref, err32 = _block_case(shape)
    y = _run_block(dev, shape, sd, x)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"crdnn block {shape}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    assert y.shape == ref.shape and err <= _bound(err32)


@pytest.mark.gpu
def test_recipe_width_block_on_the_gpu():
    native.load()
    sd, x, ref, err32 = _block_case(GPU_BLOCK)
    y = _run_block(torch.device("cuda:0"), GPU_BLOCK, sd, x)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"crdnn block {GPU_BLOCK}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}")
    assert y.shape == ref.shape and err <= _bound(err32)


@pytest.mark.parametrize("index,T,tp", TIME_POOLS)
def test_time_pooling_fused_behind_the_block(backend, index, T, tp):
    nat, dev = backend
    shape = BLOCKS[index]
    sd, x, ref, err32 = _block_case(shape, T, tp)
    y = _run_block(dev, shape, sd, x, time_pool=tp)
    err = float((y.cpu().double() - ref).abs().max())
    print(f"crdnn block {shape} T={T} time pooling {tp}: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}")
    assert y.shape == ref.shape == (shape[0], T // tp, shape[2] // shape[5], shape[4]) and err <= _bound(err32)


def test_patch_matrix_in_chunks_gives_the_same_bits(backend):
    """native.crdnn_conv forms the patch matrix for a bounded run of frames at a time: one frame per chunk, three, or all."""
    nat, dev = backend
    sd, x, _, _ = _block_case(BLOCKS[2])
    w = sd["conv_1.conv.weight"]
    wk = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(dev)
    b = sd["conv_1.conv.bias"].to(dev)
    row = x.shape[2] * wk.shape[1] * 4
    whole = nat.crdnn_conv(x.to(dev), wk, b)
    ref = R.conv3x3(x.double(), w.double(), sd["conv_1.conv.bias"].double())
    err32 = float((R.conv3x3(x, w, sd["conv_1.conv.bias"]).double() - ref).abs().max())
    assert float((whole.cpu().double() - ref).abs().max()) <= _bound(err32)
    for frames in (1, 3):
        assert torch.equal(nat.crdnn_conv(x.to(dev), wk, b, col_bytes=frames * row), whole)


def test_dnn_block_folds_the_running_statistics(backend):
    nat, dev = backend
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    sd = {"linear.w.weight": rn(16, 24) / 24 ** 0.5, "linear.w.bias": 0.5 * rn(16), "norm.norm.weight": 1.0 + 0.3 * rn(16),
          "norm.norm.bias": 0.3 * rn(16), "norm.norm.running_mean": 0.5 * rn(16), "norm.norm.running_var": 0.5 + torch.rand(16, generator=gen),
          "norm.norm.num_batches_tracked": torch.tensor(7)}
    x = rn(3, 9, 24)
    ref = R.dnn_block(x.double(), R.cast_dict(sd, torch.float64), "")
    err32 = float((R.dnn_block(x, sd, "").double() - ref).abs().max())
    blk = DNN_Block([None, None, 24], neurons=16).eval()
    blk.load_state_dict(sd, strict=True)
    with torch.no_grad():
        y = blk.to(dev)(x.to(dev))
    err = float((y.cpu().double() - ref).abs().max())
    print(f"crdnn dnn block: kernel max|d| {err:.3e}, fp32 composition {err32:.3e}")
    assert err <= _bound(err32)


def test_short_inputs_raise_value_errors(backend):
    nat, dev = backend
    shape = BLOCKS[0]
    sd, x, _, _ = _block_case(shape)
    with pytest.raises(ValueError, match="reflect"):  # T = 1: the reference's F.pad(mode="reflect") refuses it too
        _run_block(dev, shape, sd, x[:, :1])
    with pytest.raises(ValueError, match="reflect"):
        R.cnn_block(x[:, :1], sd, "", 2)
    with pytest.raises(ValueError, match="empty"):  # 3 frames pooled by 4
        _run_block(dev, shape, sd, x[:, :3], time_pool=4)
    with pytest.raises(ValueError, match="empty"):
        R.max_pool(x[:, :3], 1, 4)


def test_refusals_name_the_limit(backend):
    nat, dev = backend
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    with pytest.raises(nat.SbkError, match="F \\* C <= 16384"):
        nat.crdnn_norm_pool(z(1, 2, 129, 128), z(129 * 128), z(129 * 128))
    with pytest.raises(nat.SbkError, match="expected \\[Cout, 72\\]"):
        nat.crdnn_conv(z(1, 2, 4, 8), z(4, 9), z(4))
    lib = nat.load()
    assert lib.sbk_crdnn_im2col_f32(nat._p(z(1, 2, 4, 8)), nat._p(z(8, 72)), 1, 2, 4, 8, 1, 2, nat._stream(z(1))) == -22
    assert "frames" in lib.sbk_last_error().decode()


@functools.lru_cache(maxsize=None)
def _model():
    z = np.load(os.path.join(GOLD, "model_crdnn.npz"))
    sd = {k[3:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("sd/") and not k.endswith("num_batches_tracked")}
    return sd, torch.from_numpy(z["feats"]).double()


BLOCK_MUTATIONS = {
    "zero instead of reflect padding": dict(zero_pad=True),
    "kF / kT transposed in the conv weight": dict(transpose_taps=True),
    "LayerNorm over C only": dict(over_c_only=True),
}
MODEL_MUTATIONS = {
    "C-major instead of F-major flattening": dict(c_major=True),
    "BatchNorm with batch statistics": dict(batch_statistics=True),
}


@pytest.mark.parametrize("name", list(BLOCK_MUTATIONS) + list(MODEL_MUTATIONS))
def test_cases_tell_mistakes_apart(name):
    """CPU only, fp64, on the host restatement: each planted mistake moves the result of a committed case by more than 1e3 x
    its bound -- the block cases above for the convolution and LayerNorm mistakes; the committed tiny model
    (tests/golden/model_crdnn.npz, bound 5e-5 on its stages) for the flattening and the BatchNorm statistics."""
    worst = 0.0
    if name in BLOCK_MUTATIONS:
        for shape in BLOCKS:
            sd, x, ref, err32 = _block_case(shape)
            moved = R.cnn_block(x.double(), R.cast_dict(sd, torch.float64), "", shape[5], **BLOCK_MUTATIONS[name])
            worst = max(worst, float((moved - ref).abs().max()) / _bound(err32))
    else:
        sd, feats = _model()
        args = (feats, sd, (2, 2), 4, 2, True, 2)
        ref, _ = R.crdnn(*args)
        moved, _ = R.crdnn(*args, **MODEL_MUTATIONS[name])
        worst = float((moved - ref).abs().max()) / 5e-5
    print(f"mutation '{name}': moves the result by {worst:.3e} x the bound")
    assert worst > 1e3
