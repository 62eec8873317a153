"""The dense contractions (csrc/gemm.hip, gemm_lp.hip, gemm_lp256.hip, gemm_x3p.hip, gemm_x3r.hip) beyond the operand recipe
of tests/test_kernels.py: exact probes, an error bound that scales per row and column, leading dimensions with
poisoned destinations through the raw C ABI, and a check that these cases tell a wrong kernel from a right one.
The fp64 restatement, the probes and the planted mistakes are tests/gemm_host_ref.py.

Why: tests/test_kernels.py holds every GEMM to max|out - ref| <= 2e-6 * scale + 1e-5 with ONE scale per matrix (the
largest sum of magnitudes), on operands whose rows differ by 1e3 and 300 x.  A host model of the six-product bf16 split
with BOTH lo products removed passes that bound on the test's own operands (error / bound: 0.41 at 130 x 132 x 256,
0.25 at 70 x 72 x 512, 0.84 at 65 x 40 x 64; test_cases_tell_mistakes_apart prints the figures again).

A. Exact probes (torch.equal, no tolerance): every output element has one non-zero product (two in the hi*lo probe) and
   every partial sum is an fp32 number, so the result is known bit for bit whatever the summation order or K cut.
   Measured: every probe of every launch form is bit-exact on the emulator and on the MI355X; none is relaxed.
B. RMS of e_ij / (|a_i| |w_j|) against the fp64 product -- over the matrix, over the quietest quarter of the rows, over
   the loudest quarter of the columns -- at most C_RATIO x the same statistic of torch's fp32 composition on the CPU.
   Measured kernel RMS / fp32-composition RMS ("all" statistic; the two partial ones lie within 15 % of it):

     entry                   emulator              MI355X
                          130x132x256 70x72x512  130x132x256 70x72x512
     gemm_nt (skinny route)     0.52       0.71         0.73       0.87
     gemm_nt tile kernels       1.00       1.38         1.40       1.69
     gemm_nt stream-K forced    1.00       1.39         1.40       1.70
     f32x3                      1.96       2.72         1.16       1.45
     x3p                        1.96       2.72         1.16       1.45
     x3r                        0.93       1.34         0.57       0.69
     gemm_ln_nt_x3r             0.90       1.30         0.63       0.71
     gemm_ln_nt                 0.60       0.76         0.76       0.87
     bf16                       1.00       1.44         1.10       1.39
     bf16a                      1.00       1.44         1.10       1.39
     f16                        1.00       1.46         0.55       0.64
     fp8a                       0.99       1.01       353        350

   The emulator rounds after every partial product, the matrix core after every MFMA, hence the emulator's wider
   figures for the split-operand kernels.  Host model with all six products: 0.02 x; a_lo*w_hi dropped 8.3-8.5 x,
   mid*mid dropped 9.4-9.5 x, both lo products dropped 11.6-12.0 x, truncated W pieces > 1e4 x.  C_RATIO = 5 for the fp32-class entries: every measured
   ratio is <= 5 / 1.5 = 3.33 and every planted mistake >= 7.5.  The bf16 / fp16 entries are fp32 contractions of
   their rounded operands and are held to the same 5.  The fp8 matrix instruction adds its 64 products and the
   accumulator at a common exponent with ~18 bits below the largest term (tests/test_kernels.py::test_gemm_fp8a): six
   bits fewer than fp32 keeps (2^6), cut by truncation -- one-sided, up to a whole unit instead of half of one, on each of
   the 65 addends -- for which a factor 10 is allowed: C_RATIO_FP8A = 640 (measured 353 <= 640 / 1.5; none of the
   planted mistakes, which are about the bf16 split, applies to this entry).
   K stays <= 512: at K = 1024 the emulator's x3p (4.09 x) leaves the 1.5 x margin.  The maximum of the normalised
   error is printed and never asserted: it does not separate (emulator x3p 2.7 x against 4.5-4.9 x for a_lo*w_hi
   dropped at these shapes, 6.4 x against 6.8 x at K = 1024).
C. Through the raw C ABI with lda = K + 4, ldw = K + 8, ldr = N + 12, ldc = N + 8 (the entries whose operand rows are
   narrower than fp32 take the next stride their 16-byte rule allows), NaN in every padding element of the operands,
   the result written into a slice of a buffer of M + 3 rows filled with a sentinel NaN: the project's bound inside,
   the sentinel bit for bit outside; a row mask; an in-place residual; and one refused call per documented limit.
D. CPU only: each planted mistake of gemm_host_ref fails a probe of A and moves B's statistic past 1.5 x its threshold.

Out of scope: operands near the fp32 / bf16 denormal range (the lo piece of a number below about 2^-110 is denormal).
"""
import functools
from ctypes import c_void_p

import pytest
import torch
import torch.nn.functional as F

import gemm_host_ref as R

SWISH = "swish"


def _d(t, dev):
    return None if t is None else t.to(dev)


def _unpanel(img, rows, cols):  # panel image -> the sum of its three pieces as fp32 [rows, cols] (as tests/test_kernels.py)
    RB, KB = (rows + 63) // 64, cols // 16
    pieces = (img.cpu().view(torch.int16).to(torch.int32) << 16).view(torch.float32).view(RB, KB, 3, 2, 64, 8)
    return pieces.double().sum(2).permute(0, 3, 1, 2, 4).reshape(RB * 64, cols).float()[:rows]


class _force_f32x3:
    """Route nat.gemm_nt to sbk_gemm_nt_f32x3 at any row count (as tests/test_kernels.py::test_gemm_f32x3 does)."""

    def __init__(self, nat):
        self.nat = nat

    def __enter__(self):
        n = self.nat
        self.old = n.F32X3, n.F32X3_MIN_ROWS, n.F32X3_MIN_TILES, n.X3P
        n.F32X3, n.F32X3_MIN_ROWS, n.F32X3_MIN_TILES, n.X3P = True, 1, 1, False

    def __exit__(self, *exc):
        n = self.nat
        n.F32X3, n.F32X3_MIN_ROWS, n.F32X3_MIN_TILES, n.X3P = self.old


# ------------------------------------------------------------------ launch forms (through the binding): parts A and B
def _f32(**kn):
    def run(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
        with nat.knobs(**kn):
            return nat.gemm_nt(a.to(dev), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha).cpu()
    return run


def _splitk(slices, **kn):
    def run(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
        with nat.knobs(**kn):
            return nat.gemm_nt_splitk(a.to(dev), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha, slices=slices).cpu()
    return run


def _f32x3(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
    with _force_f32x3(nat):
        assert nat.f32x3_ok(a.shape[0], a.shape[1], w) and not nat.x3p_ok(a.shape[0], a.shape[1], w)
        return nat.gemm_nt(a.to(dev), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha).cpu()


def _x3p(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
    return nat.gemm_nt_x3p(nat.split_x3p(a.to(dev)), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha).cpu()


def _x3p_panel(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
    pc = nat.gemm_nt_x3p(nat.split_x3p(a.to(dev)), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha, panel_out=True, fp32_out=False)
    return _unpanel(pc.data, a.shape[0], w.shape[0])


def _x3r(**kn):
    def run(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
        with nat.knobs(**kn):
            return nat.gemm_nt_x3r(a.to(dev), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha).cpu()
    return run


def _lp(kind):
    def run(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
        return nat.gemm_nt_bf16(a.to(dev), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha, kind=kind).cpu()
    return run


def _bf16a(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
    assert torch.equal(a.bfloat16().float(), a)
    return nat.gemm_nt_bf16a(a.bfloat16().to(dev), w.to(dev), _d(b, dev), _d(r, dev), act=act, alpha=alpha).cpu()


# The shapes: M in 1, 63, 65, 129, 257 and N in 4, 68, 132, 260 (the smallest with an interior and a ragged edge of the
# 32 / 64 / 128 / 256 tiles; 144 where a panel result needs N % 16 == 0); K per entry from its divisibility rule in
# include/sbk.h: the smallest legal K, then one that is no multiple of the next larger unit.  ``slices`` only sizes the
# workspace of sbk_gemm_nt_splitk_f32; how often the register-operand path really cuts K across workgroups follows from K
# (each slice stays deeper than 4 x 128): not at all below K = 1 024, 2-way at 1 024, 4-way at 2 048, 8-way from 4 096 on.
# So "slices=2" runs the 2-way split at both shapes, "slices=8" the 8-way split at (1, 260, 4096) and the 4-way one at
# (40, 260, 2048), and the tiled split-K kernel (knob tiled_splitk, always 4-way) is reached from K = 2 048 on.
# form: (runner, significand bits of the operand type, shapes)
FORMS = {
    "f32 tile kernels": (_f32(skinny_off=1), 24, [(1, 4, 34), (63, 68, 36), (65, 132, 34), (129, 260, 36), (257, 68, 256)]),
    "f32 skinny route": (_f32(), 24, [(1, 68, 256), (40, 132, 256), (33, 260, 256)]),
    "f32 stream-K forced": (_f32(sk_mode=2), 24, [(129, 132, 256), (257, 260, 256), (65, 68, 256)]),
    "splitk slices=2": (_splitk(2), 24, [(1, 68, 1024), (40, 132, 1024)]),
    "splitk slices=8": (_splitk(8), 24, [(1, 260, 4096), (40, 260, 2048)]),
    "splitk tiled_splitk=64": (_splitk(4, tiled_splitk=64), 24, [(65, 260, 2048)]),
    "f32x3": (_f32x3, 24, [(1, 4, 64), (63, 68, 96), (129, 132, 64), (257, 260, 96)]),
    "x3p fp32 result": (_x3p, 24, [(1, 4, 32), (63, 68, 48), (65, 260, 272), (257, 132, 48)]),
    "x3p panel result": (_x3p_panel, 24, [(1, 144, 32), (65, 144, 48), (129, 144, 272)]),
    "x3r x3r_xc=1": (_x3r(x3r_xc=1), 24, [(1, 4, 256), (65, 132, 512), (257, 260, 256)]),
    **{f"x3r x3r_xc={xc}": (_x3r(x3r_xc=xc), 24, [(257, 260, 256)]) for xc in (2, 4, 8)},
    **{f"x3r x3r_pair={p}": (_x3r(x3r_pair=p), 24, [(63, 68, 256), (129, 260, 512)]) for p in (0, 3)},
    "bf16": (_lp("bf16"), 8, [(1, 4, 8), (63, 68, 72), (129, 132, 8), (257, 260, 72)]),
    "f16": (_lp("fp16"), 11, [(1, 4, 8), (63, 68, 72), (129, 132, 8), (257, 260, 72)]),
    "bf16a": (_bf16a, 8, [(1, 4, 64), (63, 68, 192), (129, 132, 64), (257, 260, 192)]),
}
MAX_DRAWS = 8  # one-hot draws per shape; ceil(K / N) (ceil(K / M) for the mirror) of them select every k: every form has a
# shape whose one-hot W does, the mirror does wherever the rows allow it

# Exactness on the MI355X.  The bf16 matrix instruction adds its 16 products and the accumulator with truncation; the
# probes are built so that no bit can be truncated.  Measured: every probe of every form below is bit-exact on the
# MI355X as on the emulator, so no probe is relaxed on either backend.


def _check_exact(out, want, what):
    if not torch.equal(out, want):
        bad = (out != want) | out.isnan()
        i, j = [int(v) for v in bad.nonzero()[0]]
        ulp = float(((out.double() - want.double()).abs() / torch.exp2(torch.floor(torch.log2(want.double().abs())) - 23))[bad].max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first [{i},{j}] "
                             f"got {float(out[i, j])!r} want {float(want[i, j])!r}; worst {ulp:.1f} ulp")


@pytest.mark.parametrize("form", list(FORMS))
def test_exact_probes(backend, form):
    """Part A.  Full-mantissa A x one-hot W and its mirror (three positive pieces with disjoint bits, and general
    significands whose pieces have both signs), the cross-term probes, and the one-hot probe through the epilogue
    (alpha = 0.5, bias and residual in units of the product's last bit): bit for bit."""
    nat, dev = backend
    run, bits, shapes = FORMS[form]
    styles = ("pieces", "general") if bits == 24 else ("pieces",)
    covered_w = False
    for M, N, K in shapes:
        seed = M * 1000 + N * 10 + K
        nw, na = R.draws_to_cover(N, K), R.draws_to_cover(M, K)
        covered_w = covered_w or nw <= MAX_DRAWS
        for style in styles:
            for draw in range(min(nw, MAX_DRAWS)):
                a, w, want = R.probe_one_hot_w(M, N, K, draw, seed + draw, bits, style)
                _check_exact(run(nat, dev, a, w), want, f"{form} {M}x{N}x{K} one-hot W ({style}) draw {draw}")
            for draw in range(min(na, MAX_DRAWS // 2)):
                a, w, want = R.probe_one_hot_a(M, N, K, draw, seed + 50 + draw, bits, style)
                _check_exact(run(nat, dev, a, w), want, f"{form} {M}x{N}x{K} one-hot A ({style}) draw {draw}")
        a, w, want = R.probe_cross(M, N, K, seed, shift=9 if bits == 24 else 7)
        _check_exact(run(nat, dev, a, w), want, f"{form} {M}x{N}x{K} cross term")
        if bits == 24:
            a, w, want = R.probe_cross_lo(M, N, K, seed)
            _check_exact(run(nat, dev, a, w), want, f"{form} {M}x{N}x{K} hi*lo cross term")
        a, w, b, r, want = R.probe_epilogue(M, N, K, 0, seed, bits)
        _check_exact(run(nat, dev, a, w, b, r, alpha=0.5), want, f"{form} {M}x{N}x{K} epilogue")
    assert covered_w, "no shape of this form selects every k of the one-hot W"


# ------------------------------------------------------------------ part B
B_SHAPES = [(130, 132, 256), (70, 72, 512)]
C_RATIO = 5.0
C_RATIO_FP8A = 640.0


@functools.lru_cache(maxsize=None)
def _b_case(M, N, K, kind):
    """Operands, the fp64 product and the statistic of the fp32 composition, made once per (shape, operand kind)."""
    a, w, g = R.scaled_operands(M, N, K, seed=M + N + K, lo=0 if kind == "ln" else -10)
    extra = None
    if kind == "ln":  # LayerNorm is not scale-invariant below eps: rows keep 2^0 .. 2^10, plus a mean of a few deviations
        a = a + a.std(1, keepdim=True) * torch.randn(M, 1, generator=g) * 2.0
        gamma, beta, b = 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g), torch.randn(N, generator=g)
        b = b * w.norm(dim=1)  # a bias of the size of the products, so that it does not drown a quiet column
        ln = R.layernorm64(a, gamma, beta, 1e-5)
        exact = ln @ w.double().t() + b.double()
        comp = F.linear(F.layer_norm(a, (K,), gamma, beta, 1e-5), w, b)
        norm_a, extra = ln, (gamma, beta, b)
    else:
        if kind == "bf16":
            a, w = a.bfloat16().float(), w.bfloat16().float()
        elif kind == "f16":
            a, w = a.half().float(), w.half().float()
        exact = a.double() @ w.double().t()
        comp = a @ w.t()
        norm_a = a
    return a, w, extra, exact, norm_a, R.row_col_stat(comp, exact, norm_a, w)


def _ln_x3r(nat, dev, a, w, extra):
    wf, bf = nat._fold_ln(w, extra[2], extra[0], extra[1])
    return nat.gemm_ln_nt_x3r(a.to(dev), wf.to(dev), bf.to(dev), 1e-5).cpu()


def _ln_f32(nat, dev, a, w, extra):
    wf, bf = nat._fold_ln(w, extra[2], extra[0], extra[1])
    return nat.gemm_ln_nt(a.to(dev), wf.to(dev), bf.to(dev), 1e-5).cpu()


B_ENTRIES = {
    "gemm_nt": ("f32", lambda nat, dev, a, w, x: _f32()(nat, dev, a, w)),
    "gemm_nt tile kernels": ("f32", lambda nat, dev, a, w, x: _f32(skinny_off=1)(nat, dev, a, w)),
    "gemm_nt stream-K forced": ("f32", lambda nat, dev, a, w, x: _f32(sk_mode=2)(nat, dev, a, w)),
    "f32x3": ("f32", lambda nat, dev, a, w, x: _f32x3(nat, dev, a, w)),
    "x3p": ("f32", lambda nat, dev, a, w, x: _x3p(nat, dev, a, w)),
    "x3r": ("f32", lambda nat, dev, a, w, x: _x3r()(nat, dev, a, w)),
    "gemm_ln_nt_x3r": ("ln", _ln_x3r),
    "gemm_ln_nt": ("ln", _ln_f32),
    "bf16": ("bf16", lambda nat, dev, a, w, x: _lp("bf16")(nat, dev, a, w)),
    "bf16a": ("bf16", lambda nat, dev, a, w, x: _bf16a(nat, dev, a, w)),
    "f16": ("f16", lambda nat, dev, a, w, x: _lp("fp16")(nat, dev, a, w)),
}


def _assert_stat(name, shape, got, base, c):
    ratios = {k: got[k] / base[k] for k in ("all", "quiet_rows", "loud_cols", "max")}
    print(f"part B {name} {shape}: kernel / fp32 composition " + ", ".join(f"{k} {v:.2f}x" for k, v in ratios.items()))
    for k in ("all", "quiet_rows", "loud_cols"):
        assert got[k] <= c * base[k], (name, shape, k, ratios)


@pytest.mark.parametrize("M,N,K", B_SHAPES)
@pytest.mark.parametrize("name", list(B_ENTRIES))
def test_error_scales_per_row_and_column(backend, name, M, N, K):
    """Part B: the normalised error's RMS (whole matrix, quietest quarter of the rows, loudest quarter of the columns) is
    at most C_RATIO x that of the fp32 composition on the same operands."""
    nat, dev = backend
    kind, run = B_ENTRIES[name]
    a, w, extra, exact, norm_a, base = _b_case(M, N, K, kind)
    _assert_stat(name, (M, N, K), R.row_col_stat(run(nat, dev, a, w, extra), exact, norm_a, w), base, C_RATIO)


def _e4m3(q):
    return q.cpu().view(torch.float8_e4m3fn).float()


@pytest.mark.parametrize("M,N,K", B_SHAPES)
def test_error_scales_per_row_and_column_fp8a(backend, M, N, K):
    """Part B for sbk_gemm_nt_fp8a: against a_scale[m] w_scale[n] (A8 . W8^T) of the quantised operands in fp64, next to the
    same expression in fp32 on the CPU."""
    nat, dev = backend
    a, w, _ = R.scaled_operands(M, N, K, seed=M + N + K)
    aq = nat.quant_rows_fp8(a.to(dev))
    wq, ws = nat.lp_weight(w.to(dev), "fp8r")
    a8, w8, sa, sw = _e4m3(aq.q).view(M, K), _e4m3(wq).view(N, K), aq.scale.cpu(), ws.cpu()
    exact = (a8.double() @ w8.double().t()) * sa.double()[:, None] * sw.double()[None, :]
    comp = (a8 @ w8.t()) * sa[:, None] * sw[None, :]
    norm_a, norm_w = a8.double() * sa.double()[:, None], w8.double() * sw.double()[:, None]
    base = R.row_col_stat(comp, exact, norm_a, norm_w)
    got = R.row_col_stat(nat.gemm_nt_fp8a(aq, w.to(dev)).cpu(), exact, norm_a, norm_w)
    _assert_stat("fp8a", (M, N, K), got, base, C_RATIO_FP8A)


# ------------------------------------------------------------------ part C: the raw C ABI
SENT32 = 0x7FC5A5A5  # a NaN: a kernel that reads its destination, or a padding element, cannot hide it
SENT16 = 0x7FC5
# launch form -> (entry, knobs): 15 forms of the 12 entries
C_ENTRIES = {
    "f32": ("f32", {}), "f32 tile kernels": ("f32", dict(skinny_off=1)), "f32 stream-K forced": ("f32", dict(sk_mode=2)),
    "splitk": ("splitk", {}), "splitk K cut": ("splitk", {}), "splitk tiled_splitk=64": ("splitk", dict(tiled_splitk=64)),
    "f32x3": ("f32x3", {}), "x3p": ("x3p", {}), "x3r": ("x3r", {}), "ln_x3r": ("ln_x3r", {}),
    "ln_f32": ("ln_f32", {}), "bf16": ("bf16", {}), "f16": ("f16", {}), "fp8": ("fp8", {}), "bf16a": ("bf16a", {}),
    "fp8a": ("fp8a", {}),
}
C_SHAPES = [(1, 4, 256), (70, 132, 256), (129, 260, 512), (257, 68, 256)]
# sbk_gemm_nt_splitk_f32 cuts K across workgroups only from K = 1 024 on (see FORMS): at the shapes above it runs the
# same kernel as sbk_gemm_nt_f32 and ignores its workspace.  These forms reach the partial tiles in the workspace and the
# reduce kernel, the only code of the entry that then reads the residual through ldr and writes C through ldc: the
# register-operand path cut in two, and the tiled kernel (4-way) with its reduce.
C_SHAPES_OF = {"splitk K cut": [(40, 132, 1024), (1, 4, 1024)], "splitk tiled_splitk=64": [(70, 132, 2048)]}
MASKED = ("f32", "f32x3", "x3p", "bf16", "f16", "fp8")  # the entries that take seq_len / rows_per_seq
VECTOR_C = ("f32x3", "x3p", "x3r", "ln_x3r")  # the entries that move rows of C as 16-byte vectors
# a K the entry's divisibility rule refuses, and the words of the message that name the rule
BAD_K = {"f32x3": (48, "multiple of 32"), "x3p": (40, "multiple of 16"), "x3r": (128, "multiple of 256"),
         "ln_x3r": (128, "256, 512, 1024 or 1280"), "ln_f32": (64, "not eligible"), "bf16": (36, "multiple of 8"),
         "f16": (36, "multiple of 8"), "fp8": (40, "multiple of 16"), "bf16a": (96, "multiple of 64"),
         "fp8a": (192, "multiple of 128")}


def _strided(x, ld, fill):
    buf = torch.full((x.shape[0], ld), fill, dtype=x.dtype)
    buf[:, : x.shape[1]] = x
    return buf


def _bytes_strided(q, ld):  # uint8 rows with 0x7F (the e4m3 NaN) in the padding
    buf = torch.full((q.shape[0], ld), 0x7F, dtype=torch.uint8, device=q.device)
    buf[:, : q.shape[1]] = q
    return buf


class _AbiCase:
    """One contraction set up for a direct sbk_* call: strided operands with NaN padding, a sentinel-filled destination of
    M + 3 rows, the fp64 reference of what the slice must hold."""

    def __init__(self, nat, dev, kind, M, N, K, mask=False, inplace=False, ldc_pad=8):
        self.nat, self.dev, self.kind, self.M, self.N, self.K = nat, dev, kind, M, N, K
        self.lib = nat.load()
        g = torch.Generator().manual_seed(M * 3 + N * 5 + K + len(kind))
        nan = float("nan")
        a = torch.randn(M, K, generator=g) + torch.arange(M)[:, None] * 0.01
        w = torch.randn(N, K, generator=g) - torch.arange(N)[:, None] * 0.02
        b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        self.r, self.bound_kind, self.keep = r, "fp32", []
        self.lda, self.ldw, self.ldr, self.ldc, self.ldcb = K + 4, K + 8, N + 12, N + ldc_pad, N + 16
        self.eps = 1e-5
        self.seq = self.rps = None
        if mask:
            self.rps = 10
            self.seq = torch.tensor([(i * 7) % (self.rps + 1) for i in range(M // self.rps)], dtype=torch.int32)
            assert M % self.rps == 0
        a_eff, w_eff, bias = a.double(), w.double(), b
        wd = w.to(dev)
        if kind in ("ln_x3r", "ln_f32"):
            a = a * (0.5 + torch.rand(M, 1, generator=g) * 3.0) + torch.randn(M, 1, generator=g) * 4.0
            w = w / K ** 0.5
            gamma, beta = 1.0 + 0.3 * torch.randn(K, generator=g), 0.2 * torch.randn(K, generator=g)
            wf, bias = nat._fold_ln(w, b, gamma, beta)
            a_eff, w_eff, wd = R.layernorm64(a, gamma, beta, self.eps), w.double(), wf.to(dev)
            w = wf
        if kind in ("bf16", "bf16a"):
            w_eff = w.bfloat16().double()
            a_eff = a.bfloat16().double()
        elif kind == "f16":
            a_eff, w_eff = a.half().double(), w.half().double()
        # ---- the A operand
        if kind == "bf16a":
            self.lda = K + 8  # bf16 rows: 16 bytes are 8 elements
            self.A = _strided(a.bfloat16(), self.lda, nan).to(dev)
        elif kind == "fp8a":
            self.lda = self.ldw = K + 16  # byte rows
            aq = nat.quant_rows_fp8(a.to(dev))
            self.A, self.a_scale = _bytes_strided(aq.q.view(M, K), self.lda), aq.scale
            a_eff = _e4m3(aq.q).view(M, K).double() * aq.scale.cpu().double()[:, None]
        else:
            self.A = _strided(a, self.lda, nan).to(dev)
            if kind == "x3p":
                self.PA = nat.split_x3p(self.A.reshape(-1), rows=M, K=K, ldx=self.lda)
        # ---- the W operand
        if kind in ("f32", "splitk", "ln_f32"):
            self.W = _strided(w, self.ldw, nan).to(dev)
        elif kind == "f32x3":
            self.keep.append(wd)
            self.W = nat.lp_weight(wd, "x3")
        elif kind in ("x3p", "x3r", "ln_x3r"):
            self.keep.append(wd)
            self.W = nat.lp_weight(wd, "x3p")
        elif kind in ("bf16", "bf16a"):
            self.W = _strided(w.bfloat16(), self.ldw, nan).to(dev)
        elif kind == "f16":
            self.W = _strided(w.half(), self.ldw, nan).to(dev)
        elif kind == "fp8":  # per-tensor scales, as tests/test_kernels.py::test_gemm_fp16_and_fp8_operands
            self.ldw = K + 16
            sa, self.w_scale = float(a.abs().max()) / 448.0, float(w.abs().max()) / 448.0
            wq = (w / self.w_scale).to(torch.float8_e4m3fn)
            self.W = _bytes_strided(wq.view(torch.uint8), self.ldw).to(dev)
            self.amax = torch.tensor([float(a.abs().max())]).to(dev)
            a_eff, w_eff = (a / sa).to(torch.float8_e4m3fn).double() * sa, wq.double() * self.w_scale
            self.bound_kind = "fp8"
        elif kind == "fp8a":
            self.keep.append(wd)
            wq, ws = nat.lp_weight(wd, "fp8r")
            self.W, self.w_scale = _bytes_strided(wq.view(N, K), self.ldw), ws
            w_eff = _e4m3(wq).view(N, K).double() * ws.cpu().double()[:, None]
            self.bound_kind = "fp8a"
        self.bias = bias.to(dev)
        acc = a_eff @ w_eff.t()
        self.scale = float((a_eff.abs() @ w_eff.abs().t()).max())
        ref_bias = b if kind in ("ln_x3r", "ln_f32") else bias
        self.ref = lambda **kw: R.epilogue(acc, ref_bias, r, SWISH, 0.5, self.seq, self.rps or 0, **kw)
        # ---- the residual and the destinations
        self.inplace = inplace
        C = torch.full((M + 3, self.ldc), SENT32, dtype=torch.int32).view(torch.float32)
        if inplace:
            C[:M, :N] = r
            self.ldr = self.ldc
        self.C = C.to(dev)
        self.R = self.C if inplace else _strided(r, self.ldr, nan).to(dev)
        self.R0 = self.R.cpu().clone()
        self.Cb = torch.full((M + 3, self.ldcb), SENT16, dtype=torch.int16).to(dev) if kind in ("bf16a", "fp8a") else None
        self.seq_d = self.seq.to(dev) if mask else None
        self.ws = torch.empty(8 * M * N, dtype=torch.float32, device=dev) if kind == "splitk" else None

    def call(self, ldc=None, c_off=0, K=None, ldr=None):
        """The entry's return code and sbk_last_error(); ``ldc`` / ``c_off`` (floats) / ``K`` / ``ldr`` replace the good values."""
        nat, lib, p = self.nat, self.lib, self.nat._p
        M, N, kind = self.M, self.N, self.kind
        K = self.K if K is None else K
        ldc = self.ldc if ldc is None else ldc
        C = c_void_p(self.C.data_ptr() + 4 * c_off)
        act, alpha, st = nat.ACT_SWISH, 0.5, nat._stream(self.A)
        seq, rps = p(self.seq_d), int(self.rps or 0)
        tail = (p(self.bias), p(self.R), self.ldr if ldr is None else ldr, C, ldc)
        if kind == "f32":
            rc = lib.sbk_gemm_nt_f32(p(self.A), self.lda, p(self.W), self.ldw, *tail, M, N, K, act, alpha, seq, rps, st)
        elif kind == "splitk":
            rc = lib.sbk_gemm_nt_splitk_f32(p(self.A), self.lda, p(self.W), self.ldw, *tail, M, N, K, act, alpha, p(self.ws),
                                            self.ws.numel(), st)
        elif kind == "f32x3":
            rc = lib.sbk_gemm_nt_f32x3(p(self.A), self.lda, p(self.W), *tail, M, N, K, act, alpha, seq, rps, st)
        elif kind == "x3p":
            rc = lib.sbk_gemm_nt_x3p(p(self.PA.data), p(self.W), *tail, None, M, N, K, act, alpha, seq, rps, st)
        elif kind == "x3r":
            rc = lib.sbk_gemm_nt_x3r(p(self.A), self.lda, p(self.W), *tail, M, N, K, act, alpha, st)
        elif kind == "ln_x3r":
            rc = lib.sbk_gemm_ln_nt_x3r(p(self.A), self.lda, p(self.W), *tail, M, N, K, self.eps, act, alpha, st)
        elif kind == "ln_f32":
            rc = lib.sbk_gemm_ln_nt_f32(p(self.A), self.lda, p(self.W), self.ldw, *tail, M, N, K, self.eps, act, alpha, st)
        elif kind in ("bf16", "f16"):
            fn = lib.sbk_gemm_nt_bf16 if kind == "bf16" else lib.sbk_gemm_nt_f16
            rc = fn(p(self.A), self.lda, p(self.W), self.ldw, *tail, M, N, K, act, alpha, seq, rps, st)
        elif kind == "fp8":
            rc = lib.sbk_gemm_nt_fp8(p(self.A), self.lda, p(self.amax), p(self.W), self.ldw, self.w_scale, *tail, M, N, K, act,
                                     alpha, seq, rps, st)
        elif kind == "bf16a":
            rc = lib.sbk_gemm_nt_bf16a(p(self.A), self.lda, p(self.W), self.ldw, *tail, p(self.Cb), self.ldcb, M, N, K, act,
                                       alpha, st)
        else:
            rc = lib.sbk_gemm_nt_fp8a(p(self.A), self.lda, p(self.a_scale), p(self.W), self.ldw, p(self.w_scale), *tail,
                                      p(self.Cb), self.ldcb, None, 0, 1.0, M, N, K, act, alpha, st)
        return rc, lib.sbk_last_error().decode()

    def check(self, what):
        M, N = self.M, self.N
        out = self.C.cpu()
        outside = torch.ones(out.shape, dtype=torch.bool)
        outside[:M, :N] = False
        assert bool((out.view(torch.int32)[outside] == SENT32).all()), f"{what}: wrote outside its [M, N] slice"
        got, ref = out[:M, :N], self.ref()
        assert not got.isnan().any(), f"{what}: NaN inside the slice (a padding element or the destination was read)"
        err = float((got.double() - ref).abs().max())
        if self.bound_kind == "fp8":  # (the same roundings up to stray ties, as in tests/test_kernels.py)
            rel = float((got.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
            assert rel <= 1e-3, (what, rel)
        else:
            bound = (1e-4 if self.bound_kind == "fp8a" else 2e-6) * self.scale + 1e-5
            assert err <= bound, (what, err, bound)
        if not self.inplace:
            assert torch.equal(self.R.cpu().view(torch.int32), self.R0.view(torch.int32)), f"{what}: the residual was written"
        if self.Cb is not None:
            cb = self.Cb.cpu()
            out_b = torch.ones(cb.shape, dtype=torch.bool)
            out_b[:M, :N] = False
            assert bool((cb[out_b] == SENT16).all()), f"{what}: wrote outside the bf16 slice"
            assert torch.equal(cb[:M, :N].view(torch.bfloat16), got.bfloat16()), f"{what}: bf16 result != rounded fp32 result"
        return err


@pytest.mark.parametrize("entry", list(C_ENTRIES))
def test_strides_and_poisoned_destination(backend, entry):
    """Part C: lda / ldw / ldr / ldc wider than the rows, bias + SWISH + alpha = 0.5, the result inside a sentinel-filled
    buffer: the project's bound inside the slice, every other element untouched; then the row mask (where the entry has
    one) and the in-place residual (C == residual, ldc == ldr), both with the same strides."""
    nat, dev = backend
    kind, kn = C_ENTRIES[entry]
    shapes = C_SHAPES_OF.get(entry, C_SHAPES)
    again = shapes[0] if entry in C_SHAPES_OF else (70, 132, 256)
    cases = [(s, False, False, 8) for s in shapes] + [(again, False, True, 8)]
    if kind in MASKED:
        cases.append((again, True, False, 8))
    if kind not in VECTOR_C:  # scalar stores: an odd ldc (rows at every residue of 16 bytes), plain and in place
        cases += [(again, False, False, 7), (again, False, True, 7)]
    with nat.knobs(**kn):
        for (M, N, K), mask, inplace, pad in cases:
            c = _AbiCase(nat, dev, kind, M, N, K, mask=mask, inplace=inplace, ldc_pad=pad)
            rc, msg = c.call()
            assert rc == 0, (entry, M, N, K, rc, msg)
            c.check(f"{entry} {M}x{N}x{K} ldc=N+{pad}" + (" row mask" if mask else "") + (" in place" if inplace else ""))


@pytest.mark.parametrize("entry", sorted(set(k for k, _ in C_ENTRIES.values())))
def test_documented_limits_are_refused_by_name(backend, entry):
    """One refused call (SBK_EINVAL = -22, the limit named by sbk_last_error) per limit include/sbk.h documents: ldc < N
    (the message says ldc); ldr < N;
    ldc % 4 != 0 and a C pointer off by one float where rows of C move as 16-byte vectors (the other entries store
    scalars: an odd ldc is run and checked instead); a K that breaks the entry's divisibility rule."""
    nat, dev = backend
    M, N, K = 70, 132, 256
    c = _AbiCase(nat, dev, entry, M, N, K)
    assert c.call()[0] == 0
    rc, msg = c.call(ldc=N - 4)
    assert rc == -22 and "ldc" in msg, (rc, msg)
    rc, msg = c.call(ldr=N - 4)  # (every entry takes a residual)
    assert rc == -22 and ("residual" in msg or "ldr" in msg), (rc, msg)
    if entry in VECTOR_C:
        for kw in (dict(ldc=N + 6), dict(c_off=1)):
            rc, msg = c.call(**kw)
            assert rc == -22 and ("ldc" in msg or "16-byte" in msg), (kw, rc, msg)
    else:
        c2 = _AbiCase(nat, dev, entry, M, N, K, ldc_pad=7)  # an odd stride: scalar stores take it
        assert c2.call()[0] == 0
        c2.check(f"{entry} odd ldc")
    if entry in BAD_K:
        bad, words = BAD_K[entry]
        rc, msg = c.call(K=bad)
        assert rc == -22 and words in msg, (bad, rc, msg)


# ------------------------------------------------------------------ part D: the cases tell mistakes apart (host model, CPU only)
def _probes(M=70, N=64, K=256):
    for style in ("pieces", "general"):
        yield f"one-hot W ({style})", R.probe_one_hot_w(M, N, K, 0, 11, 24, style)
        yield f"one-hot A ({style})", R.probe_one_hot_a(M, N, K, 0, 12, 24, style)
    yield "cross term", R.probe_cross(M, N, K, 13)
    yield "hi*lo cross term", R.probe_cross_lo(M, N, K, 14)


def test_host_model_passes_every_case():
    """The six-product model itself: bit-exact on every probe, and far inside part B's threshold (0.02 x the fp32
    composition: its sums are fp64, what is left is the three dropped products)."""
    for name, (a, w, want) in _probes():
        assert torch.equal(R.x3_product(a, w).float(), want), name
    a, w, b, r, want = R.probe_epilogue(70, 64, 256, 0, 15)
    assert torch.equal(R.epilogue(R.x3_product(a, w), b, r, alpha=0.5).float(), want)
    for M, N, K in B_SHAPES:
        a, w, _, exact, norm_a, base = _b_case(M, N, K, "f32")
        ratio = R.row_col_stat(R.x3_product(a, w), exact, norm_a, w)["all"] / base["all"]
        print(f"host model, all six products {M}x{N}x{K}: {ratio:.3f} x the fp32 composition")
        assert ratio <= C_RATIO / 1.5


@pytest.mark.parametrize("name", list(R.X3_MISTAKES))
def test_cases_tell_mistakes_apart(name):
    """Each planted arithmetic mistake fails at least one exact probe of part A and moves part B's statistic to at least
    1.5 x its threshold in every part-B case.  Printed next to it: what the one-scale-per-matrix bound of
    tests/test_kernels.py makes of the same mistake on that file's own operand recipe (it passes the dropped-lo models)."""
    kw = R.X3_MISTAKES[name]
    failed = [p for p, (a, w, want) in _probes() if not torch.equal(R.x3_product(a, w, **kw).float(), want)]
    print(f"'{name}' fails the probes: {failed}")
    assert failed
    for M, N, K in B_SHAPES:
        a, w, _, exact, norm_a, base = _b_case(M, N, K, "f32")
        got = R.row_col_stat(R.x3_product(a, w, **kw), exact, norm_a, w)
        ratios = {k: got[k] / base[k] for k in got}
        print(f"'{name}' {M}x{N}x{K}: " + ", ".join(f"{k} {v:.1f}x" for k, v in ratios.items()) + " the fp32 composition")
        for k in ("all", "quiet_rows", "loud_cols"):
            assert ratios[k] >= 1.5 * C_RATIO, (name, k, ratios)
    for M, N, K in ((130, 132, 256), (70, 72, 512), (65, 40, 64)):  # the recipe of tests/test_kernels.py::test_gemm_x3r
        g = torch.Generator().manual_seed(M + N + K)
        a = torch.randn(M, K, generator=g) + torch.arange(M)[:, None] * 0.01
        w = torch.randn(N, K, generator=g) - torch.arange(N)[:, None] * 0.02
        a[::7] *= 1e-3
        w[::5] *= 300.0
        err = float((R.x3_product(a, w, **kw).float().double() - a.double() @ w.double().t()).abs().max())
        bound = 2e-6 * float((a.double().abs() @ w.double().abs().t()).max()) + 1e-5
        print(f"'{name}' {M}x{N}x{K}, operands of tests/test_kernels.py: error = {err / bound:.2f} x the one-scale bound")


def test_layout_mistake_fails_the_one_hot_probe():
    """The two 8-k halves of a 16-k panel group swapped in one operand only: every one-hot probe fails."""
    for name, (a, w, want) in _probes():
        if name.startswith("one-hot"):
            assert not torch.equal(R.x3_product(a, w, **R.LAYOUT_MISTAKE).float(), want), name


def test_mask_mistake_moves_the_masked_case():
    """The row mask applied after the residual instead of before it moves part C's row-mask case by more than 1e3 x its bound."""
    import emu_utils

    nat = emu_utils.attach()
    try:
        c = _AbiCase(nat, torch.device("cpu"), "f32", 70, 132, 256, mask=True)
    finally:
        emu_utils.detach()
    moved = float((c.ref(mask_after_residual=True) - c.ref()).abs().max())
    bound = 2e-6 * c.scale + 1e-5
    print(f"mask after the residual: moves the masked case by {moved / bound:.3e} x its bound")
    assert moved > 1e3 * bound
