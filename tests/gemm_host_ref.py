"""Host restatement of the dense contractions (include/sbk.h, "dense contraction") in fp64, written from the header's
description of the arithmetic alone -- the operands and expectations of tests/test_gemm_edges.py:

  * the epilogue  C = residual + alpha * act(acc + bias)  with the row mask applied BEFORE the residual;
  * the exact three-piece bf16 split of an fp32 number (hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid, round to
    nearest even) and the six-product contraction the x3 kernels run, with switches for planted mistakes;
  * the exact probes: operands whose product is known bit for bit whatever the summation order;
  * the per-row / per-column error statistic;
  * the activation probes of tests/test_activation_edges.py: one-hot operands whose pre-activation values are chosen,
    the error statistic in units of the fp32 spacing, and planted activation mistakes.

Everything is plain torch on the CPU.  Denormal operands are out of scope: the lo piece of a number below about 2^-110
is a bf16 denormal, and no probe here goes near it (|values| stay within 2^-30 .. 2^30).
"""
import torch
import torch.nn.functional as F

# the six partial products the x3 kernels form (relative size >= 2^-17); mid*lo, lo*mid and lo*lo are dropped by design
SIX = (("hi", "hi"), ("hi", "mid"), ("mid", "hi"), ("hi", "lo"), ("lo", "hi"), ("mid", "mid"))

ACTS = {"none": lambda v: v, "swish": F.silu, "gelu": F.gelu, "relu": F.relu, "leaky_relu": F.leaky_relu}
ACT_CODES = {"none": 0, "swish": 1, "gelu": 2, "relu": 3, "leaky_relu": 4}  # SBK_ACT_* of include/sbk.h


def _rn(x):  # fp32 -> nearest bf16 (ties to even), as fp32
    return x.bfloat16().float()


def _trunc(x):  # fp32 -> bf16 by dropping the low 16 bits, as fp32
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def split3(x, truncate=False):
    """The three bf16 pieces of fp32 ``x`` (each returned as fp32).  hi + mid + lo == x exactly.

    ``truncate`` (planted mistake): every piece is cut by truncation while the remainder chain is still the one that
    round-to-nearest pieces leave -- the remainder is not re-derived from the piece actually taken, so wherever the
    rounding went up the pieces no longer sum to x."""
    x = x.float()
    hi = _rn(x)
    r1 = x - hi  # exact: the remainder of a rounding to fewer bits is an fp32 number
    mid = _rn(r1)
    r2 = r1 - mid
    lo = _rn(r2)
    if truncate:
        hi, mid, lo = _trunc(x), _trunc(r1), _trunc(r2)
    return {"hi": hi, "mid": mid, "lo": lo}


def swap_k_halves(x):
    """(planted mistake) the two 8-k halves of every 16-k panel group exchanged."""
    rows, K = x.shape
    return x.view(rows, K // 16, 2, 8).flip(2).reshape(rows, K)


def x3_product(a, w, drop=(), truncate_w=False, swap_halves=False):
    """a [M,K] . w [N,K]^T through the six bf16 partial products, every product and sum in fp64.
    ``drop``: pairs of SIX to leave out; ``truncate_w``: split3(w, truncate=True); ``swap_halves``: A's k halves swapped."""
    if swap_halves:
        a = swap_k_halves(a)
    pa, pw = split3(a), split3(w, truncate=truncate_w)
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float64)
    for x, y in SIX:
        if (x, y) not in drop:
            acc += pa[x].double() @ pw[y].double().t()
    return acc


# the planted arithmetic / layout mistakes of the six-product model (keyword arguments of x3_product)
X3_MISTAKES = {
    "a_lo*w_hi dropped": dict(drop=(("lo", "hi"),)),
    "both lo products dropped": dict(drop=(("lo", "hi"), ("hi", "lo"))),
    "mid*mid dropped": dict(drop=(("mid", "mid"),)),
    "W pieces truncated, remainders not renormalised": dict(truncate_w=True),
}
LAYOUT_MISTAKE = dict(swap_halves=True)


def row_keep(M, seq_len, rows_per_seq):
    """[M, 1] bool: rows are [batch][rows_per_seq]; a row is kept while its index inside the sequence < seq_len[batch]."""
    if seq_len is None:
        return torch.ones(M, 1, dtype=torch.bool)
    r = torch.arange(M)
    return (r % rows_per_seq < seq_len.long()[r // rows_per_seq]).reshape(M, 1)


def epilogue(acc, bias=None, residual=None, act="none", alpha=1.0, seq_len=None, rows_per_seq=0, mask_after_residual=False):
    """fp64: v = act(acc + bias); masked rows v = 0; C = residual + alpha * v.
    ``mask_after_residual`` (planted mistake): the mask zeroes the finished element, residual included."""
    v = acc.double()
    if bias is not None:
        v = v + bias.double()
    v = ACTS[act](v)
    keep = row_keep(acc.shape[0], seq_len, rows_per_seq)
    zero = torch.zeros((), dtype=torch.float64)
    if not mask_after_residual:
        v = torch.where(keep, v, zero)
    out = alpha * v
    if residual is not None:
        out = residual.double() + out
    if mask_after_residual:
        out = torch.where(keep, out, zero)
    return out


def layernorm64(x, gamma, beta, eps):
    return F.layer_norm(x.double(), (x.shape[-1],), gamma.double(), beta.double(), eps)


# ------------------------------------------------------------------ the error statistic of part B
def _rms(e):
    return float(e.pow(2).mean().sqrt())


def row_col_stat(out, exact, a, w):
    """e_ij / (|a_i|_2 |w_j|_2) against the fp64 ``exact``: its RMS over the matrix, over the quietest quarter of the rows
    and over the loudest quarter of the columns, and its maximum (printed, never asserted)."""
    na, nw = a.double().norm(dim=1), w.double().norm(dim=1)
    e = (out.double() - exact.double()) / (na[:, None] * nw[None, :])
    quiet = na.argsort()[: max(1, a.shape[0] // 4)]
    loud = nw.argsort()[-max(1, w.shape[0] // 4):]
    return {"all": _rms(e), "quiet_rows": _rms(e[quiet]), "loud_cols": _rms(e[:, loud]), "max": float(e.abs().max())}


def scaled_operands(M, N, K, seed, lo=-10, hi=10):
    """Zero-mean randn, every row of A (and of W) times a random power of two in 2^lo .. 2^hi: fp32 arithmetic is invariant
    under such scalings, so quiet and loud rows are held to the same relative standard."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(lo, hi + 1, (M, 1), generator=g).float())
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-10, 11, (N, 1), generator=g).float())
    return a, w, g


# ------------------------------------------------------------------ the exact probes of part A
def _exact32(x64):
    """fp64 -> fp32, refusing a value that fp32 cannot hold: an expectation of an exact probe must be representable."""
    x32 = x64.float()
    assert torch.equal(x32.double(), x64), "probe expectation is not an fp32 number"
    return x32


def full_mantissa(rows, K, g, sig_bits=24, style="pieces", e_lo=-6, e_hi=2, headroom=False):
    """[rows, K] fp32 with every significand bit in use, one exponent E per row.

    sig_bits 24, style "pieces": (128+p) 2^E + q 2^(E-8) + r 2^(E-16), p < 128, q in 64..127, r in 1..63 -- three positive
    pieces with disjoint bit ranges, each below half an ulp of the one above, so the round-to-nearest split (and a
    truncating one) returns exactly these pieces and every partial sum of them is an fp32 number.
    sig_bits 24, style "general": a random 24-bit significand with its leading byte in 128..254 and a random sign: the
    split has pieces of both signs (rounding differs from truncation); the leading byte stops short of 255 so that hi
    never rounds into the next binade, which keeps every partial sum of the pieces within 24 bits.
    sig_bits 8 / 11: (2^(s-1) + p) 2^(E-s+8): numbers a bf16 / fp16 operand holds exactly.
    ``headroom``: leading byte < 192, for probes that add a few ulps in the epilogue."""
    E = torch.randint(e_lo, e_hi + 1, (rows, 1), generator=g).double()
    top = 64 if headroom else 128
    if sig_bits == 24 and style == "pieces":
        p = torch.randint(0, top, (rows, K), generator=g).double()
        q = torch.randint(64, 128, (rows, K), generator=g).double()
        r = torch.randint(1, 64, (rows, K), generator=g).double()
        x = ((128 + p) * 65536 + q * 256 + r) * torch.exp2(E - 16)
    elif sig_bits == 24:
        tb = torch.randint(128, 192 if headroom else 255, (rows, K), generator=g).double()
        low = torch.randint(0, 65536, (rows, K), generator=g).double()
        sign = torch.randint(0, 2, (rows, K), generator=g).double() * 2 - 1
        x = sign * (tb * 65536 + low) * torch.exp2(E - 16)
    else:
        half = 2 ** (sig_bits - 1)
        p = torch.randint(0, half // 2 if headroom else half, (rows, K), generator=g).double()
        x = (half + p) * torch.exp2(E - (sig_bits - 8))
    return _exact32(x)


def one_hot(rows, K, draw, g):
    """[rows, K] with one entry +-2^e (e in -6..6) per row, at k(row) = (row + draw * rows) % K: ceil(K / rows) draws
    select every k.  Returns (matrix, k of every row)."""
    k = (torch.arange(rows) + draw * rows) % K
    val = torch.exp2(torch.randint(-6, 7, (rows,), generator=g).float()) * (torch.randint(0, 2, (rows,), generator=g).float() * 2 - 1)
    x = torch.zeros(rows, K)
    x[torch.arange(rows), k] = val
    return x, k


def draws_to_cover(rows, K):
    return -(-K // rows)


def probe_one_hot_w(M, N, K, draw, seed, sig_bits=24, style="pieces"):
    """Full-mantissa A, one-hot W: out[i,j] = a[i,k(j)] * w[j,k(j)], one non-zero (power-of-two) product per element."""
    g = torch.Generator().manual_seed(seed)
    a = full_mantissa(M, K, g, sig_bits, style)
    w, k = one_hot(N, K, draw, g)
    return a, w, _exact32(a[:, k].double() * w[torch.arange(N), k].double()[None, :])


def probe_one_hot_a(M, N, K, draw, seed, sig_bits=24, style="pieces"):
    """The mirror: one-hot power-of-two A, full-mantissa W: out[i,j] = a[i,k(i)] * w[j,k(i)]."""
    g = torch.Generator().manual_seed(seed)
    w = full_mantissa(N, K, g, sig_bits, style)
    a, k = one_hot(M, K, draw, g)
    return a, w, _exact32(a[torch.arange(M), k].double()[:, None] * w[:, k].double().t())


def probe_cross(M, N, K, seed, shift=9):
    """a = (1 + 2^-shift) 2^ea(i) in a one-hot position, w = +-(1 + 2^-shift) 2^ew(j) everywhere: every element is
    +-(1 + 2^(1-shift) + 2^(-2 shift)) 2^(ea+ew).  With shift = 9 the value needs hi*hi, hi*mid + mid*hi and mid*mid
    (with shift = 7, for bf16 / fp16 operands, it needs every bit of the one product)."""
    g = torch.Generator().manual_seed(seed)
    x = 1.0 + 2.0 ** -shift
    sa = torch.exp2(torch.randint(-4, 5, (M,), generator=g).double())
    sw = torch.exp2(torch.randint(-4, 5, (N,), generator=g).double()) * (torch.randint(0, 2, (N,), generator=g).double() * 2 - 1)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[torch.arange(M), (torch.arange(M) * 7 + 3) % K] = x * sa
    w = (x * sw)[:, None].expand(N, K).contiguous()
    return _exact32(a), _exact32(w), _exact32((x * sa)[:, None] * (x * sw)[None, :])


def probe_cross_lo(M, N, K, seed):
    """The probe whose answer needs hi*lo and lo*hi.  y = 1 + 2^-9 + 2^-18 has the pieces (1, 2^-9, 2^-18).  Every row of A
    holds y at an even k and 1 at the next odd k; W holds 1 at every even k and y at every odd k.  An element is
    y*1 + 1*y = 2 + 2^-8 + 2^-17 (times powers of two): a_lo*w_hi supplies one 2^-18, a_hi*w_lo the other, and because no
    k has a mid or lo piece on BOTH sides, the three products the kernels drop (mid*lo, lo*mid, lo*lo) are exactly zero.
    Every partial sum is a multiple of 2^-18 below 4: an fp32 number."""
    g = torch.Generator().manual_seed(seed)
    y = 1.0 + 2.0 ** -9 + 2.0 ** -18
    sa = torch.exp2(torch.randint(-4, 5, (M,), generator=g).double())
    sw = torch.exp2(torch.randint(-4, 5, (N,), generator=g).double()) * (torch.randint(0, 2, (N,), generator=g).double() * 2 - 1)
    k0 = (torch.arange(M) * 6 + 2) % (K - 1) // 2 * 2  # even, k0 + 1 < K
    a = torch.zeros(M, K, dtype=torch.float64)
    a[torch.arange(M), k0] = y * sa
    a[torch.arange(M), k0 + 1] = sa
    w = torch.ones(N, K, dtype=torch.float64)
    w[:, 1::2] = y
    w = w * sw[:, None]
    return _exact32(a), _exact32(w), _exact32((2 * y) * sa[:, None] * sw[None, :])


def probe_epilogue(M, N, K, draw, seed, sig_bits=24):
    """probe_one_hot_w with alpha = 0.5, a bias and a residual that are small multiples of the product's ulp, so
    residual + 0.5 * (product + bias) is still an fp32 number: the row exponents span 4 values, bias[j] is -3..3 units
    of the loudest row's last bit, residual[i,j] is -4..4 half-units of the element's own.  Returns (a, w, bias, residual, out)."""
    g = torch.Generator().manual_seed(seed)
    a = full_mantissa(M, K, g, sig_bits, "pieces", e_lo=-1, e_hi=2, headroom=True)
    w, k = one_hot(N, K, draw, g)
    wj = w[torch.arange(N), k].double()
    low = sig_bits - 8  # the last significand bit of a row with exponent E is 2^(E - low)
    E = torch.floor(torch.log2(a[:, :1].abs().double())) - 7
    unit = torch.exp2(E - low) * wj.abs()[None, :]  # [M, N]: the ulp of the product
    bias = torch.randint(-3, 4, (N,), generator=g).double() * 2.0 ** (2 - low) * wj.abs()
    res = torch.randint(-4, 5, (M, N), generator=g).double() * unit * 0.5
    prod = a[:, k].double() * wj[None, :]
    _exact32(prod + bias[None, :])  # (the sum the epilogue forms first)
    return a, w, _exact32(bias), _exact32(res), _exact32(res + 0.5 * (prod + bias[None, :]))


# ------------------------------------------------------------------ the activation probes (tests/test_activation_edges.py)
# pre-activation values every probe holds: zero and its neighbourhood, the knee, the GELU / SWISH tails where 1 + erf
# cancels (-5, -9, -12), and where expf(-v) underflows (+12, +80)
ACT_TARGETS = (0.0, 2.0 ** -20, -(2.0 ** -20), 0.5, -0.5, 1.0, -1.0, 3.0, -3.0, -5.0, -9.0, -12.0, 12.0, 80.0)


def _fits(x, sig_bits):
    """x (fp64) is a number of ``sig_bits`` significand bits."""
    m, _ = torch.frexp(x)
    s = m * 2.0 ** sig_bits
    return s == s.round()


def probe_act(M, N, K, seed, sig_bits=24, by_row=False):
    """probe_one_hot_w (draw 0) with chosen products: W one-hot +-2^e (e in -1..1; +-1 for sig_bits <= 4), a bias of +-0.5
    in every fourth column, and a[i, k(j)] = (T - bias[j]) / w[j, k(j)] for a target T of ACT_TARGETS that moves with
    (i, j), so that a . w^T + bias is T bit for bit -- the next target whose operand fits ``sig_bits`` where T's does not;
    where columns share a k (N > K) the last column wins and the others hold another exact fp32 number.
    ``by_row``: one |target| per row and the bias left out of the operand (rows that survive a per-row quantisation).
    The residual is uniform in (-1, 1) with a third of its elements zero (there the result is the activation alone).
    Returns (a, w, bias, residual, pre): ``pre`` fp64 [M, N], an fp32 number in every element."""
    g = torch.Generator().manual_seed(seed)
    a = full_mantissa(M, K, g, sig_bits, "pieces") if sig_bits > 4 else torch.zeros(M, K)
    k = torch.arange(N) % K
    sign = torch.randint(0, 2, (N,), generator=g).double() * 2 - 1
    wval = sign * torch.exp2(torch.randint(-1, 2, (N,), generator=g).double() * (sig_bits > 4))
    w = torch.zeros(N, K)
    w[torch.arange(N), k] = wval.float()
    bias = torch.zeros(N, dtype=torch.float64)
    bias[3::8], bias[7::8] = 0.5, -0.5
    T = torch.tensor(ACT_TARGETS, dtype=torch.float64)
    i = torch.arange(M)
    for j in range(N):
        first = i % len(T) if by_row else (i * 5 + j * 3) % len(T)
        val, done = torch.zeros(M, dtype=torch.float64), torch.zeros(M, dtype=torch.bool)
        for s in range(len(T)):
            cand = (T[(first + s) % len(T)] - (0.0 if by_row else bias[j])) / wval[j]
            take = ~done & _fits(cand, sig_bits)
            val, done = torch.where(take, cand, val), done | take
        assert bool(done.all())
        a[:, k[j]] = val.float()
    r = torch.rand(M, N, generator=g) * 2 - 1
    r[(i[:, None] + torch.arange(N)[None, :]) % 3 == 0] = 0.0
    pre = a[:, k].double() * wval[None, :] + bias[None, :]
    _exact32(pre)
    return a, w, bias.float(), r, pre


def probe_act_ln(M, N, K, seed):
    """The LayerNorm-prologue entries: every row of A holds +-ACT_TARGETS and zeros (mean 0), rolled by 7 per row; W is
    one-hot +-sqrt(var + eps), gamma = 1, beta = 0, so LayerNorm(A) . W^T + bias lies within a few fp32 spacings of the
    targets and is known in fp64.  Returns (a, w, bias, residual, pre): pre fp64 [M, N]."""
    g = torch.Generator().manual_seed(seed)
    row = torch.zeros(K, dtype=torch.float64)
    t = torch.tensor(ACT_TARGETS, dtype=torch.float64)
    row[: 2 * len(t)] = torch.cat([t, -t])
    a = torch.stack([row.roll(7 * i) for i in range(M)]).float()
    k = torch.arange(N) % K
    sign = torch.randint(0, 2, (N,), generator=g).double() * 2 - 1
    w = torch.zeros(N, K)
    w[torch.arange(N), k] = (sign * float((row.var(unbiased=False) + 1e-5).sqrt())).float()
    bias = torch.zeros(N)
    bias[3::8], bias[7::8] = 0.5, -0.5
    r = torch.rand(M, N, generator=g) * 2 - 1
    r[(torch.arange(M)[:, None] + torch.arange(N)[None, :]) % 3 == 0] = 0.0
    ln = layernorm64(a, torch.ones(K), torch.zeros(K), 1e-5)
    return a, w, bias, r, ln[:, k] * w[torch.arange(N), k].double()[None, :] + bias.double()[None, :]


def spacing32(x):
    """The distance between fp32 numbers at |x| (fp64 tensor); that of the smallest denormal at 0."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def act_stat(out, ref, pre, alpha, row_floor=False):
    """max |out - ref| in units of the fp32 spacing at max(|alpha pre|, |ref|): the error against what the epilogue had in
    its registers, so that the cancellation of 1 + erf in the negative tail counts as the absolute error it is.
    ``row_floor`` (LayerNorm prologue: x - mean cancels at the size of the row's loudest element): the spacing at
    alpha * max_j |pre_ij| where that is larger."""
    size = torch.maximum((alpha * pre).abs(), ref.abs())
    if row_floor:
        size = torch.maximum(size, (alpha * pre).abs().amax(1, keepdim=True))
    unit = spacing32(size)
    return float(((out.double() - ref).abs() / unit).max())


# planted activation mistakes: name -> (the activation they are planted into, fp64 function of (pre, alpha) -> alpha-scaled value)
ACT_MISTAKES = {
    "tanh-GELU for erf-GELU": ("gelu", lambda v, al: al * F.gelu(v, approximate="tanh")),
    "slope 0.1 for 0.01": ("leaky_relu", lambda v, al: al * F.leaky_relu(v, 0.1)),
    "RELU for LEAKY_RELU": ("leaky_relu", lambda v, al: al * F.relu(v)),
    "SWISH after alpha": ("swish", lambda v, al: F.silu(al * v)),
    "GELU after alpha": ("gelu", lambda v, al: F.gelu(al * v)),
}
