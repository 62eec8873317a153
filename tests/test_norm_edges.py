"""The row kernels at their width edges: csrc/norm.hip (sbk_layernorm_f32 / _bf16o / _fp8o, sbk_quant_rows_fp8 / _bf16_fp8,
sbk_input_norm_*), sbk_w2v_utt_norm_f32 of csrc/wav2vec2.hip and the element conversions of csrc/gemm_lp.hip (sbk_f32_to_bf16 /
_f16 / _fp8, sbk_absmax_f32) against the plain fp64 / exact-byte restatements of tests/norm_host_ref.py, on the CPU emulator of
the kernel sources (not gpu) and on the MI355X (-m gpu).

Bound for values (the project's rule, tests/test_wav2vec2_kernels.py): max(4 x the fp32 torch composition's own error against
fp64 on the same inputs, 1e-5); the kernel's error, that error and their ratio are printed per case.  Bytes and scales of the
plain quantisation and of the conversions are demanded exactly.  Every case builds its inputs once from a seeded generator and
never modifies them."""
import ctypes

import pytest
import torch

import norm_host_ref as R

EPS = 1e-5
_CASES = {}


def _bound(err32):
    return max(4.0 * err32, 1e-5)


def _report(what, err, err32):
    print(f"{what}: kernel max|d| {err:.3e}, fp32 torch composition {err32:.3e}, ratio {err / max(err32, 1e-30):.2f}, "
          f"of the bound {err / _bound(err32):.2f}")


def _cached(key, make):
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


def _ptr(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes)


# ---- 1. LayerNorm ----------------------------------------------------------------------------------------------------
# both sides of every MAXV limit of layernorm_kernel (256, 512, 1024, 1280), multiples of 4 past 1280 (the generic kernel) and
# widths that are no multiple of 4 (the generic kernel again)
LN_WIDTHS = [4, 252, 256, 260, 512, 516, 1020, 1024, 1028, 1276, 1280, 1284, 2048, 3, 5, 255, 1281]
LN_ACT_WIDTHS = [4, 260, 1028, 1280, 255]
LN_ROWS = [1, 4, 5]  # 5: three idle waves of the second workgroup shadow the last row
LN_CASES = [(d, R.ACT_NONE) for d in LN_WIDTHS] + [(d, a) for a in (R.ACT_SWISH, R.ACT_GELU, R.ACT_RELU, R.ACT_LEAKY_RELU)
                                                   for d in LN_ACT_WIDTHS]


def _ln_inputs(rows, d):
    """Rows of mean near 40 and spread near 3 (a one-pass variance loses five digits to the mean); from 4 rows on, row 1 is the
    constant 40.0 -- its sums are exact in any order, so its variance is 0 and the row must come out as act(beta)."""
    def make():
        gen = torch.Generator().manual_seed(7919 * rows + d)
        x = 40.0 + 2.0 * torch.randn(rows, 1, generator=gen) + 3.0 * torch.randn(rows, d, generator=gen)
        if rows >= 4:
            x[1] = 40.0
        return x, 1.0 + 0.3 * torch.randn(d, generator=gen), 0.5 * torch.randn(d, generator=gen)
    return _cached(("ln_in", rows, d), make)


def _ln_case(rows, d, code):
    def make():
        x, g, b = _ln_inputs(rows, d)
        ref = R.layernorm(x.double(), g.double(), b.double(), EPS, code)
        err32 = float((R.layernorm(x, g, b, EPS, code).double() - ref).abs().max())
        return x, g, b, ref, err32
    return _cached(("ln", rows, d, code), make)


@pytest.mark.parametrize("d,code", LN_CASES)
def test_layernorm_vs_fp64(backend, d, code):
    nat, dev = backend
    for rows in LN_ROWS:
        x, g, b, ref, err32 = _ln_case(rows, d, code)
        y = nat.layernorm(x.to(dev), g.to(dev), b.to(dev), EPS, act=code).cpu()
        err = float((y.double() - ref).abs().max())
        _report(f"layernorm_f32 rows={rows} d={d} act={code}", err, err32)
        assert err <= _bound(err32)


@pytest.mark.parametrize("d,code", LN_CASES)
def test_layernorm_bf16_output(backend, d, code):
    """|y - ref64| <= bound + 2^-8 |ref64| (half a bf16 step), and the bits are the round-to-nearest-even bf16 of
    sbk_layernorm_f32's output on the same backend."""
    nat, dev = backend
    for rows in LN_ROWS:
        x, g, b, ref, err32 = _ln_case(rows, d, code)
        yb = nat.layernorm_bf16(x.to(dev), g.to(dev), b.to(dev), EPS, act=code).cpu()
        y32 = nat.layernorm(x.to(dev), g.to(dev), b.to(dev), EPS, act=code).cpu()
        over = float(((yb.double() - ref).abs() - 2.0 ** -8 * ref.abs()).max())
        _report(f"layernorm_bf16o rows={rows} d={d} act={code} (beyond half a bf16 step)", max(over, 0.0), err32)
        assert over <= _bound(err32)
        assert torch.equal(yb.view(torch.int16), R.bf16_bits(y32))


@pytest.mark.parametrize("which", ["x", "gamma"])
def test_layernorm_unaligned_operand(backend, which):
    """x or gamma starts 4 bytes into a buffer at d = 256: no 16-byte loads may be issued on it (the generic kernel)."""
    nat, dev = backend
    rows, d = 5, 256
    x, g, b, ref, err32 = _ln_case(rows, d, R.ACT_NONE)
    xd, gd = x.to(dev), g.to(dev)
    if which == "x":
        buf = torch.zeros(rows * d + 8, device=dev)
        buf[1: 1 + rows * d] = xd.reshape(-1)
        xd = buf[1: 1 + rows * d].view(rows, d)
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
    else:
        buf = torch.zeros(d + 8, device=dev)
        buf[1: 1 + d] = gd
        gd = buf[1: 1 + d]
        assert gd.data_ptr() % 16 == 4
    for name, fn in (("f32", nat.layernorm), ("bf16o", nat.layernorm_bf16)):
        y = fn(xd, gd, b.to(dev), EPS).cpu().double()
        half_step = 2.0 ** -8 * ref.abs() if name == "bf16o" else 0.0
        over = float(((y - ref).abs() - half_step).max())
        _report(f"layernorm_{name} unaligned {which}", max(over, 0.0), err32)
        assert over <= _bound(err32)


def test_layernorm_out_is_a_slice_of_a_poisoned_buffer(backend):
    nat, dev = backend
    rows, d = 5, 260
    x, g, b, ref, err32 = _ln_case(rows, d, R.ACT_SWISH)
    big = torch.full((8 + rows * d + 8,), float("nan"), device=dev)
    out = big[8: 8 + rows * d].view(rows, d)
    nat.layernorm(x.to(dev), g.to(dev), b.to(dev), EPS, act=R.ACT_SWISH, out=out)
    assert float((out.cpu().double() - ref).abs().max()) <= _bound(err32)
    assert bool(torch.isnan(big[:8]).all()) and bool(torch.isnan(big[8 + rows * d:]).all())
    # bf16 output through the C entry, into a 0xAAAA-filled buffer
    fill = 0xAAAA - 0x10000
    bigb = torch.full((8 + rows * d + 8,), fill, dtype=torch.int16, device=dev)
    xd, gd, bd = x.to(dev), g.to(dev), b.to(dev)
    assert nat.load().sbk_layernorm_bf16o(_ptr(xd), _ptr(gd), _ptr(bd), _ptr(bigb, 16), rows, d, EPS, R.ACT_SWISH, nat._stream(xd)) == 0
    got = bigb.cpu()
    assert torch.equal(got[8: 8 + rows * d].view(rows, d), R.bf16_bits(out.cpu()))
    assert bool((got[:8] == fill).all()) and bool((got[8 + rows * d:] == fill).all())


# ---- 2. fp8 rows -----------------------------------------------------------------------------------------------------
# both sides of every MAXV limit of launch_rows_fp8 (256, 512, 1024, 1280, 2048) and the largest width; bf16 input up to 2048
# (its limits: 512, 1280 -- 1284 is the <8> form)
Q_WIDTHS = [4, 256, 260, 512, 516, 1024, 1028, 1280, 1284, 2048, 2052, 5120]
Q_ROWS = [1, 5]
LNQ_CASES = [(d, a) for d in (4, 260, 1028, 1284, 2052, 5120) for a in (R.ACT_NONE, R.ACT_SWISH)]


def _q_inputs(rows, d, ldx=None):
    """Row scales from 1e-3 to 1e3, row 1 all zero, zeros scattered over row 3 (one row: scale 0.37); the columns past d of a
    strided operand hold values far larger than the row's (a scale taken over them would show)."""
    def make():
        gen = torch.Generator().manual_seed(104729 * rows + d)
        w = d if ldx is None else ldx
        scales = torch.tensor([0.37]) if rows == 1 else torch.logspace(-3, 3, rows)
        x = torch.randn(rows, w, generator=gen) * scales[:, None]
        if rows > 3:
            x[1] = 0.0
            x[3, torch.rand(w, generator=gen) < 0.3] = 0.0
        if w > d:
            x[:, d:] *= 1e4
            x[1, d:] = 5.0
        return x
    return _cached(("q_in", rows, d, ldx), make)


@pytest.mark.parametrize("d", Q_WIDTHS)
def test_quant_rows_fp8_is_exact(backend, d):
    """Scale bit-equal and every byte equal to the numpy float32 restatement; bf16 rows the same against the widened values."""
    nat, dev = backend
    for rows in Q_ROWS:
        x = _q_inputs(rows, d)
        want_q, want_sc = _cached(("q", rows, d), lambda: R.quant_rows(x))
        got = nat.quant_rows_fp8(x.to(dev))
        assert torch.equal(R.bits(got.scale.cpu()), R.bits(want_sc)), (rows, d)
        assert torch.equal(got.q.cpu(), want_q), (rows, d, int((got.q.cpu() != want_q).sum()))
        if rows > 3:
            assert float(want_sc[1]) == 1.0 and not want_q[1].any()
        if d <= 2048:
            xb = x.to(torch.bfloat16)
            want_q, want_sc = _cached(("qb", rows, d), lambda: R.quant_rows(xb.float()))
            got = nat.quant_rows_fp8(xb.to(dev))
            assert torch.equal(R.bits(got.scale.cpu()), R.bits(want_sc)), (rows, d, "bf16")
            assert torch.equal(got.q.cpu(), want_q), (rows, d, "bf16", int((got.q.cpu() != want_q).sum()))


STRIDED = dict(rows=6, d=516, ldx=528)


@pytest.mark.parametrize("bf16", [False, True])
def test_quant_rows_fp8_strided_into_poisoned_buffers(backend, bf16):
    """ldx = d + 12 through the C entries; q and scale are slices of poisoned buffers: exact bytes and scales, nothing else
    written."""
    nat, dev = backend
    rows, d, ldx = STRIDED["rows"], STRIDED["d"], STRIDED["ldx"]
    x = _q_inputs(rows, d, ldx)
    if bf16:
        x = x.to(torch.bfloat16)
    want_q, want_sc = R.quant_rows(x.float(), d)
    xd = x.to(dev)
    qbig = torch.full((16 + rows * d + 16,), 0xAA, dtype=torch.uint8, device=dev)
    sbig = torch.full((2 + rows + 2,), float("nan"), device=dev)
    fn = nat.load().sbk_quant_rows_bf16_fp8 if bf16 else nat.load().sbk_quant_rows_fp8
    assert fn(_ptr(xd), ldx, _ptr(qbig, 16), _ptr(sbig, 8), rows, d, nat._stream(xd)) == 0
    qbig, sbig = qbig.cpu(), sbig.cpu()
    assert torch.equal(R.bits(sbig[2: 2 + rows]), R.bits(want_sc))
    assert torch.equal(qbig[16: 16 + rows * d].view(rows, d), want_q)
    assert bool((qbig[:16] == 0xAA).all()) and bool((qbig[16 + rows * d:] == 0xAA).all())
    assert bool(torch.isnan(sbig[:2]).all()) and bool(torch.isnan(sbig[2 + rows:]).all())


def _lnq_case(rows, d, code):
    def make():
        x = _q_inputs(rows, d) + 10.0 * (torch.tensor([0.37]) if rows == 1 else torch.logspace(-3, 3, rows))[:, None]
        if rows > 3:
            x[1] = 0.0
        gen = torch.Generator().manual_seed(d)
        g, b = 1.0 + 0.3 * torch.randn(d, generator=gen), 0.5 * torch.randn(d, generator=gen)
        ref = R.layernorm(x.double(), g.double(), b.double(), EPS, code)
        err32 = float((R.layernorm(x, g, b, EPS, code).double() - ref).abs().max())
        return x, g, b, ref, err32
    return _cached(("lnq", rows, d, code), make)


@pytest.mark.parametrize("d,code", LNQ_CASES)
def test_layernorm_fp8_vs_fp64_layernorm(backend, d, code):
    """sbk_layernorm_fp8o against the fp64 LayerNorm (not the library's): |q * scale - ref| <= bound + 2^-4 |ref| + 2^-10 scale
    (half an e4m3 step, the subnormal step), |448 * scale - max |ref row|| <= bound, the largest code of every row is +-448."""
    nat, dev = backend
    for rows in Q_ROWS:
        x, g, b, ref, err32 = _lnq_case(rows, d, code)
        got = nat.layernorm_fp8(x.to(dev), g.to(dev), b.to(dev), EPS, act=code)
        sc = got.scale.cpu().double()
        val = R.e4m3_decode(got.q.cpu()).view(rows, d)
        over = float(((val.double() * sc[:, None] - ref).abs() - (2.0 ** -4 * ref.abs() + 2.0 ** -10 * sc[:, None])).max())
        top = float((448.0 * sc - ref.abs().amax(1)).abs().max())
        _report(f"layernorm_fp8o rows={rows} d={d} act={code} (beyond the e4m3 step)", max(over, 0.0), err32)
        _report(f"layernorm_fp8o rows={rows} d={d} act={code} (448 * scale)", top, err32)
        assert over <= _bound(err32) and top <= _bound(err32)
        assert bool(ref.abs().amax(1).gt(0).all()) and bool((val.abs().amax(1) == 448.0).all())


# ---- 3. LayerNorm to panel -------------------------------------------------------------------------------------------
# ragged: lanes whose run lies past d / 8 -- u + 8 j in layernorm_x3p_rows8_kernel (rows >= 4096, d < 512 or 512 < d < 1024),
# lane + 64 i in layernorm_x3p_kernel (fewer rows); tests/test_kernels.py::test_layernorm_x3p reaches the first only with every
# run live
X3P_SHAPES = [(4097, 144, 0), (4100, 640, 1), (4096, 16, 0), (4099, 1008, 1), (5, 528, 1), (70, 1040, 0)]


@pytest.mark.parametrize("rows,d,act", X3P_SHAPES)
def test_layernorm_x3p_ragged(backend, rows, d, act):
    """The assertions of test_layernorm_x3p against the fp64 LayerNorm: the three pieces of the panel image add up to it (2e-6
    relative to the row's largest magnitude), the padding rows of the last 64-row block are zero."""
    nat, dev = backend
    code = R.ACT_SWISH if act else R.ACT_NONE

    def make():
        gen = torch.Generator().manual_seed(rows + d)
        x = torch.randn(rows, d, generator=gen) * 3.0 + torch.arange(rows)[:, None] * (0.05 if rows < 1000 else 0.002)  # (that test's inputs)
        g, b = torch.randn(d, generator=gen), torch.randn(d, generator=gen)
        ref = R.layernorm(x.double(), g.double(), b.double(), EPS, code)
        return x, g, b, ref, float((R.layernorm(x, g, b, EPS, code).double() - ref).abs().max())
    x, g, b, ref, err32 = _cached(("x3p", rows, d, act), make)
    pan = nat.layernorm_x3p(x.to(dev), g.to(dev), b.to(dev), EPS, act=code)
    RB, KB = (rows + 63) // 64, d // 16
    pieces = (pan.data.cpu().view(torch.int16).to(torch.int32) << 16).view(torch.float32).view(RB, KB, 3, 2, 64, 8)
    full = pieces.double().sum(2).permute(0, 3, 1, 2, 4).reshape(RB * 64, d)
    _report(f"layernorm_x3p rows={rows} d={d} act={act}", float((full[:rows] - ref).abs().max()), err32)
    assert not full[rows:].any()
    assert float(((full[:rows] - ref).abs() / (ref.abs().amax(1, keepdim=True) + 1.0)).max()) <= 2e-6
    assert pan.rows == rows and pan.K == d


# ---- 4. input normalisation ------------------------------------------------------------------------------------------
# (B, T, C, n_valid): T below the 8 time splits; C past one 64-lane pass and n_valid << T; T just past the splits; T at the
# 4-way apply grid and C past two passes; T either side of the 16-way grid; C at its limit
STATS_SHAPES = [(2, 2, 5, [2, 2]), (3, 7, 65, [7, 2, 3]), (2, 9, 64, [9, 8]), (2, 64, 130, [64, 33]), (1, 513, 40, [512]),
                (2, 512, 4096, [512, 100])]
STATS_EPS = 1e-4


def _stats_inputs(B, T, C):
    """Mean near 20, spread near 4; channel 0 is centred at 0 with a spread of 1e-3, so its variance (1e-6) lies below eps:
    the clamp of the "batch" variance (and its absence for "sentence") shows in the output."""
    def make():
        gen = torch.Generator().manual_seed(B * 1000003 + T * 4099 + C)
        x = 20.0 + 4.0 * torch.randn(B, T, C, generator=gen)
        x[..., 0] = 1e-3 * torch.randn(B, T, generator=gen)
        return x
    return _cached(("stats_in", B, T, C), make)


def _stats_case(shape, per_batch, std_norm, avoid):
    B, T, C, n_valid = shape

    def make():
        x = _stats_inputs(B, T, C)
        ref = R.input_norm_stats(x.double(), n_valid, per_batch, std_norm, STATS_EPS, avoid)
        err32 = float((R.input_norm_stats(x, n_valid, per_batch, std_norm, STATS_EPS, avoid).double() - ref).abs().max())
        return x, ref, err32
    return _cached(("stats", B, T, C, per_batch, std_norm, avoid), make)


@pytest.mark.parametrize("per_batch", [False, True])
@pytest.mark.parametrize("shape", STATS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_input_norm_stats_vs_fp64(backend, shape, per_batch):
    nat, dev = backend
    n_valid = torch.tensor(shape[3], dtype=torch.int32)
    for std_norm in (True, False):
        for avoid in (False, True):
            x, ref, err32 = _stats_case(shape, per_batch, std_norm, avoid)
            y = nat.input_norm_stats(x.to(dev), n_valid.to(dev), per_batch, std_norm, STATS_EPS, avoid).cpu()
            err = float((y.double() - ref).abs().max())
            _report(f"input_norm_stats {shape[:3]} per_batch={per_batch} std_norm={std_norm} avoid={avoid}", err, err32)
            assert err <= _bound(err32)


@pytest.mark.parametrize("avoid", [False, True])
def test_input_norm_stats_one_valid_frame(backend, avoid):
    """Sentence statistics of ONE frame: the frame is its own mean, the variance 0 -- it comes out exactly 0 (0 / eps), and with
    avoid_padding_norm the padded frames are the input bit for bit (without it they are divided by eps: not asserted)."""
    nat, dev = backend
    shape = (2, 7, 5, [7, 1])
    x, ref, err32 = _stats_case(shape, False, True, avoid)
    y = nat.input_norm_stats(x.to(dev), torch.tensor(shape[3], dtype=torch.int32).to(dev), False, True, STATS_EPS, avoid).cpu()
    err = float((y[0].double() - ref[0]).abs().max())
    _report(f"input_norm_stats one valid frame avoid={avoid} (utterance 0)", err, err32)
    assert err <= _bound(err32)
    assert not y[1, 0].any()
    if avoid:
        assert torch.equal(R.bits(y[1, 1:]), R.bits(x[1, 1:]))


GLOBAL_N = 4096 * 256 + 300  # past the 4096-block grid: every block of input_norm_kernel loops


def _global_inputs(n):
    def make():
        gen = torch.Generator().manual_seed(n)
        x = 20.0 + 4.0 * torch.randn(n, generator=gen)
        return x, torch.tensor([19.0, -3.0, 20.5, 0.0]), torch.tensor([0.0, 1e-12, 0.5, 2.0])
    return _cached(("global_in", n), make)


def test_input_norm_global_grid_stride(backend):
    """Bit-equal to (x - mean) / max(std, eps) in fp32 (one subtraction, one IEEE division); std holds 0 and 1e-12."""
    nat, dev = backend
    x, mean, std = _global_inputs(GLOBAL_N)
    x = x.view(-1, 4)
    y = nat.input_norm_global(x.to(dev), mean.to(dev), std.to(dev), 1e-10).cpu()
    want = R.input_norm_global(x, mean, std, 1e-10)
    assert bool(torch.isfinite(want).all()) and torch.equal(R.bits(y), R.bits(want))


def test_input_norm_global_masked_grid_stride(backend):
    nat, dev = backend
    B, T = 3, 87407  # 3 * T * 4 = 1 048 884 elements: past the 4096-block grid
    assert B * T * 4 > 4096 * 256
    x, mean, std = _global_inputs(B * T * 4)
    x = x.view(B, T, 4)
    lens = [0, T, 40001]
    y = nat.input_norm_global_masked(x.to(dev), mean.to(dev), std.to(dev), torch.tensor(lens, dtype=torch.int32).to(dev), 1e-10).cpu()
    want = R.input_norm_global(x, mean, std, 1e-10)
    for b, n in enumerate(lens):
        assert torch.equal(R.bits(y[b, :n]), R.bits(want[b, :n])), b
        assert torch.equal(R.bits(y[b, n:]), R.bits(x[b, n:])), b


# ---- 5. utterance norm -----------------------------------------------------------------------------------------------
UTT_SHAPES = [(1, 1), (2, 255), (3, 257), (1, 100003)]


def _utt_case(rows, n):
    def make():
        gen = torch.Generator().manual_seed(rows * 1000 + n)
        x = 30.0 + 2.0 * torch.randn(rows, 1, n, generator=gen)
        ref = R.utt_norm(x.double(), EPS)
        return x, ref, float((R.utt_norm(x, EPS).double() - ref).abs().max())
    return _cached(("utt", rows, n), make)


@pytest.mark.parametrize("rows,n", UTT_SHAPES)
def test_utt_norm_vs_fp64(backend, rows, n):
    nat, dev = backend
    x, ref, err32 = _utt_case(rows, n)
    y = nat.w2v_utt_norm(x.to(dev), EPS).cpu()
    err = float((y.double() - ref).abs().max())
    _report(f"w2v_utt_norm rows={rows} n={n}", err, err32)
    assert err <= _bound(err32)
    z = x.clone().to(dev)  # in place (y == x), as the kernel's comment promises: through the C entry
    assert nat.load().sbk_w2v_utt_norm_f32(_ptr(z), _ptr(z), rows, n, EPS, nat._stream(z)) == 0
    assert torch.equal(R.bits(z.cpu()), R.bits(y))


# ---- 6. conversions --------------------------------------------------------------------------------------------------
def _f32_to_fp8(nat, dev, v):
    vd = v.to(dev)
    out = torch.empty(v.numel(), dtype=torch.uint8, device=dev)
    assert nat.load().sbk_f32_to_fp8(_ptr(vd), _ptr(out), v.numel(), 1.0, nat._stream(vd)) == 0
    return out.cpu()


def _fp8_probes():
    """Every finite e4m3 value, every midpoint between neighbours and its two fp32 neighbours, in both signs, and the edges of
    the range."""
    def make():
        mags = R.e4m3_magnitudes()
        mid = ((mags[:-1].double() + mags[1:].double()) / 2).float()  # (exact: 5 significant bits)
        pos = torch.cat([mags, mid, torch.nextafter(mid, torch.tensor(0.0)), torch.nextafter(mid, torch.tensor(1e9))])
        edge = torch.tensor([448.0, 460.0, 464.0, 1e9, -1e9, 1e-9, -0.0, float("inf")])
        return torch.cat([pos, -pos, edge])
    return _cached("fp8_probes", make)


def test_f32_to_fp8_codes_and_midpoints(backend):
    nat, dev = backend
    v = _fp8_probes()
    assert v.numel() % 2 == 0
    got, want = _f32_to_fp8(nat, dev, v), R.e4m3_encode(v)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, [(float(v[i]), int(got[i]), int(want[i])) for i in bad[:8]]


FP8_LONG = 8192 * 512 + 2  # past the 8192-block grid at two values per thread


def test_f32_to_fp8_grid_stride(backend):
    nat, dev = backend
    v = _cached("fp8_long", lambda: torch.randn(FP8_LONG, generator=torch.Generator().manual_seed(5)) *
                torch.logspace(-4, 3, 1024).repeat(FP8_LONG // 1024 + 1)[:FP8_LONG])
    got = _f32_to_fp8(nat, dev, v)
    assert torch.equal(got, R.e4m3_encode(v))


def _half_probes():
    """65 536 random bit patterns, the 32 768 exact bf16 ties (low half 0x8000) and, for fp16, the ties of ITS 13 dropped bits
    over every non-negative high part."""
    def make():
        gen = torch.Generator().manual_seed(11)
        rnd = torch.randint(-2 ** 31, 2 ** 31, (65536,), generator=gen, dtype=torch.int64).to(torch.int32)
        hi = torch.arange(32768, dtype=torch.int32)
        ties = (hi << 16) | 0x8000
        ties16 = (torch.arange(2 ** 18, dtype=torch.int32) << 13) | 0x1000
        return torch.cat([rnd, ties, ties16]).view(torch.float32)
    return _cached("half_probes", make)


HALF_LONG = 8192 * 256 + 3  # past the 8192-block grid


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_f32_to_half_bits(backend, kind):
    """Bits equal torch's cast wherever that is not NaN; where it is, the kernel's is a NaN too."""
    nat, dev = backend
    long = _cached("half_long", lambda: torch.randn(HALF_LONG, generator=torch.Generator().manual_seed(6)) * 3.0)
    fn = getattr(nat.load(), "sbk_f32_to_" + kind)
    for v in (_half_probes(), long):
        vd = v.to(dev)
        out = torch.empty(v.numel(), dtype=torch.int16, device=dev)
        assert fn(_ptr(vd), _ptr(out), v.numel(), nat._stream(vd)) == 0
        got = out.cpu()
        want = R.bf16_bits(v) if kind == "bf16" else R.f16_bits(v)
        as_float = torch.bfloat16 if kind == "bf16" else torch.float16
        nan = torch.isnan(want.view(as_float))
        assert torch.equal(got[~nan], want[~nan]), int((got[~nan] != want[~nan]).sum())
        assert bool(torch.isnan(got.view(as_float)[nan]).all())


def _absmax(nat, dev, v):
    vd = v.to(dev)
    out = torch.full((1,), float("nan"), device=dev)
    assert nat.load().sbk_absmax_f32(_ptr(vd), v.numel(), _ptr(out), nat._stream(vd)) == 0
    return out.cpu()


def test_absmax(backend):
    nat, dev = backend
    n = 2048 * 256 + 77  # past the 2048-block grid; the maximum sits alone in the last element, negative
    v = torch.randn(n, generator=torch.Generator().manual_seed(8))
    v[-1] = -7.25 - float(v.abs().max())
    assert torch.equal(R.bits(_absmax(nat, dev, v)), R.bits(v[-1:].abs()))
    assert torch.equal(R.bits(_absmax(nat, dev, torch.tensor([-0.3]))), R.bits(torch.tensor([0.3])))
    assert torch.equal(R.bits(_absmax(nat, dev, torch.zeros(1000))), R.bits(torch.zeros(1)))


# ---- 7. NaN through the fp8 conversion -------------------------------------------------------------------------------
def test_nan_becomes_the_fp8_nan_code(backend):
    """A NaN activation must stay visible: the NaN code (0x7f or 0xff), not the code of -448 that a clamp written with fmaxf /
    fminf makes of it.  The other elements of the row are scaled by its finite maximum."""
    nat, dev = backend
    nan = float("nan")
    v = torch.tensor([nan, 1.0, -2.5, nan, 448.0, -nan, nan, nan, 0.0, 3.0])
    got, want = _f32_to_fp8(nat, dev, v), R.e4m3_encode(v)
    isn = torch.isnan(v)
    assert bool(((got[isn] & 0x7f) == 0x7f).all()), got[isn].tolist()
    assert torch.equal(got[~isn], want[~isn])
    x = _q_inputs(5, 260).clone()
    where = [(0, 0), (2, 7), (2, 8), (4, 259)]
    for r, c in where:
        x[r, c] = nan
    want_q, want_sc = R.quant_rows(x)
    res = nat.quant_rows_fp8(x.to(dev))
    q, isn = res.q.cpu(), torch.isnan(x)
    assert torch.equal(R.bits(res.scale.cpu()), R.bits(want_sc)) and bool(torch.isfinite(want_sc).all())
    assert bool(((q[isn] & 0x7f) == 0x7f).all()), q[isn].tolist()
    assert torch.equal(q[~isn], want_q[~isn])


# ---- 8. the cases can tell mistakes apart ----------------------------------------------------------------------------
def _ln_moves(**mistake):
    """The largest move of a committed LayerNorm case under a planted mistake, in units of the case's bound: the value cases of
    test_layernorm_vs_fp64, and the row maxima (448 * scale) of test_layernorm_fp8_vs_fp64_layernorm."""
    worst = 0.0
    for d, code in LN_CASES:
        for rows in LN_ROWS:
            x, g, b, ref, err32 = _ln_case(rows, d, code)
            moved = R.layernorm(x.double(), g.double(), b.double(), EPS, code, **mistake)
            worst = max(worst, float((moved - ref).abs().max()) / _bound(err32))
    for d, code in LNQ_CASES:
        for rows in Q_ROWS:
            x, g, b, ref, err32 = _lnq_case(rows, d, code)
            moved = R.layernorm(x.double(), g.double(), b.double(), EPS, code, **mistake)
            worst = max(worst, float((moved.abs().amax(1) - ref.abs().amax(1)).abs().max()) / _bound(err32))
    return worst


def _stats_moves(**mistake):
    worst = 0.0
    for shape in STATS_SHAPES[:-1] + [(2, 7, 5, [7, 1])]:  # (all but the 4 M-element one)
        for per_batch in ((False, True) if shape[3] != [7, 1] else (False,)):
            for std_norm in (True, False):
                x, ref, err32 = _stats_case(shape, per_batch, std_norm, True)
                moved = R.input_norm_stats(x.double(), shape[3], per_batch, std_norm, STATS_EPS, True, **mistake)
                worst = max(worst, float((moved - ref).abs().max()) / _bound(err32))
    return worst


def _quant_bytes_changed(**mistake):
    changed = 0
    for d in Q_WIDTHS:
        for rows in Q_ROWS:
            x = _q_inputs(rows, d)
            changed += int((R.quant_rows(x, **mistake)[0] != R.quant_rows(x)[0]).sum())
    return changed


def _strided_changed():
    rows, d, ldx = STRIDED["rows"], STRIDED["d"], STRIDED["ldx"]
    x = _q_inputs(rows, d, ldx)
    (q0, s0), (q1, s1) = R.quant_rows(x, d), R.quant_rows(x, d, scale_cols=ldx)
    return min(int((q0 != q1).sum()), int((R.bits(s0) != R.bits(s1)).sum()))  # (bytes and scales both)


def _truncation_changed():
    v = _fp8_probes()
    h = _half_probes()
    keep = ~torch.isnan(h)
    return min(int((R.e4m3_encode(v, truncate=True) != R.e4m3_encode(v)).sum()),
               int((R.bf16_bits(h, truncate=True)[keep] != R.bf16_bits(h)[keep]).sum()))  # (the fp8 and the bf16 probes both)


VALUE_MISTAKES = {
    "unbiased variance": lambda: _ln_moves(unbiased=True),
    "eps outside the root": lambda: _ln_moves(eps_outside=True),
    "LeakyReLU slope 0.1": lambda: _ln_moves(leaky_slope=0.1),
    "sentence statistics over the padded frames": lambda: _stats_moves(include_padding=True),
    "batch variance not clamped": lambda: _stats_moves(clamp_batch=False),
    "sentence variance clamped": lambda: _stats_moves(clamp_sentence=True),
}
BYTE_MISTAKES = {
    "scale = max / 240": lambda: _quant_bytes_changed(divisor=240.0),
    "truncation instead of round-to-nearest-even": _truncation_changed,
    "scale over ldx instead of d columns": _strided_changed,
}


@pytest.mark.parametrize("name", list(VALUE_MISTAKES))
def test_cases_tell_mistakes_apart(name):
    """CPU only, fp64, on the host restatement: each planted mistake moves at least one committed case by more than 1e3 x its
    bound."""
    worst = VALUE_MISTAKES[name]()
    print(f"mistake '{name}': moves a committed case by {worst:.3e} x its bound")
    assert worst > 1e3


@pytest.mark.parametrize("name", list(BYTE_MISTAKES))
def test_cases_tell_byte_mistakes_apart(name):
    """CPU only: each planted mistake changes bytes (and, for the scales, bits) of the committed exact cases."""
    changed = BYTE_MISTAKES[name]()
    print(f"mistake '{name}': changes {changed} bytes of the committed cases")
    assert changed > 0


def test_cases_tell_tanh_gelu_apart():
    """CPU only, fp64.  The erf and tanh forms of GELU differ by at most 4.8e-4 at ANY argument, and a value bound is never
    below its 1e-5 floor: no input can move a value case by 1e3 x its bound (1e-2).  What the committed GELU cases do: the
    move is over 30 x the bound (the value tests fail on it by that factor; measured 47), and the bf16 image of the result
    -- the bytes sbk_layernorm_bf16o must produce -- changes."""
    worst, changed = 0.0, 0
    for d in LN_ACT_WIDTHS:
        for rows in LN_ROWS:
            x, g, b, ref, err32 = _ln_case(rows, d, R.ACT_GELU)
            moved = R.layernorm(x.double(), g.double(), b.double(), EPS, R.ACT_GELU, tanh_gelu=True)
            worst = max(worst, float((moved - ref).abs().max()) / _bound(err32))
            changed += int((R.bf16_bits(moved.float()) != R.bf16_bits(ref.float())).sum())
    v = torch.linspace(-12, 12, 240001, dtype=torch.float64)
    ceiling = float((R.act(v, R.ACT_GELU, tanh_gelu=True) - R.act(v, R.ACT_GELU)).abs().max())
    print(f"mistake 'tanh-GELU': moves a committed case by {worst:.3e} x its bound, changes {changed} bf16 values; "
          f"the two forms differ by {ceiling:.3e} at most")
    assert ceiling < 4.8e-4 and worst > 30.0 and changed > 0
