"""Every activation through every epilogue that applies one: the contraction entries (csrc/gemm.hip, gemm_lp.hip,
gemm_lp256.hip, gemm_x3p.hip, gemm_x3r.hip) with SBK_ACT_NONE / SWISH / GELU / RELU / LEAKY_RELU, and the transducer joint
(csrc/transducer.hip) with GELU / LEAKY_RELU / RELU / TANH.  The formulas live in csrc/act.h; this file runs every
epilogue that calls them.  The probes, the statistic and the planted mistakes are tests/gemm_host_ref.py.

Why: tests/test_gemm_edges.py runs the contraction epilogues with SWISH only (and GELU in tests/test_kernels.py); RELU and
LEAKY_RELU reached only bf16a, the decode step and LayerNorm, and no test put a value into the tails of GELU / SWISH.

Contraction entries.  Operands: gemm_host_ref.probe_act -- A . W^T + bias is, bit for bit and whatever the K cut, one of
0, +-2^-20, +-0.5, +-1, +-3, -5, -9, -12, +12, +80 (or, where several columns share a k, another exact fp32 number);
alpha = 0.5 and a residual of which a third is zero.  The reference is residual + alpha * act(pre) in fp64.
  * RELU, LEAKY_RELU and NONE: torch.equal with torch's fp32 composition (one rounding of the sum; 0.01f * v rounds once).
  * SWISH and GELU: max |out - ref| in units of the fp32 spacing at max(|alpha pre|, |ref|) is at most
    C_RATIO x (the same statistic of torch's fp32 composition F.silu / F.gelu (pre) * alpha + residual, plus one unit).
  * GELU of the entries on sbk::gelu_erfc (bf16a, fp8a; both tile sizes): |gelu(pre) - fp64| <= 4.2e-7 (include/sbk.h),
    measured with alpha = 1 and no residual, i.e. before alpha.
  * fp8a: the per-row quantisation of A and W leaves no exactly known product, so ``pre`` is the entry's own fp32 result
    with SBK_ACT_NONE, alpha = 1 and no residual (itself held to the dequantised operands' fp64 product); rows hold one
    |target| each so that they survive the quantisation.  K = 256 on the 128-tile route: the entry refuses K = 192.
  * the LayerNorm-prologue entries: gemm_host_ref.probe_act_ln, pre known in fp64 only; every activation is held to the
    ratio (the composition is F.layer_norm, F.linear, the activation), in units of the spacing at the row's loudest
    element where that is larger: x - mean cancels at that size.
  * 256-tile route (knob lp256 = 2): NONE / SWISH / GELU run csrc/gemm_lp256.hip; RELU / LEAKY_RELU are not instantiated
    there and must fall back to the 128-tile kernels -- its launcher would otherwise run them as NONE, which these cases fail.
  * x3p: SWISH once more without a residual (the straight-line epilogues of gemm_x3p.hip are taken without one).

Measured with the library of the commit before csrc/act.h existed: kernel statistic / (composition statistic + 1), SWISH
and GELU (the x3p forms: with / without a residual), and max |gelu_erfc - fp64| before alpha:

     entry                         emulator                MI355X
                                SWISH       GELU        SWISH       GELU
     f32 tile kernels            0.57       0.31         0.57       0.31
     f32 skinny route            0.54       0.20         0.54       0.20
     f32 stream-K forced         0.54       0.20         0.54       0.20
     splitk slices=2             0.54       0.20         0.54       0.20
     f32x3                       0.54       0.20         0.54       0.20
     x3p fp32 result          0.57 / 0.44   0.20      0.57 / 0.44   0.27
     x3p panel result         0.57 / 0.45   0.25      0.57 / 0.45   0.27
     x3r                         0.54       0.20         0.54       0.20
     gemm_ln_nt                  0.46       0.39         0.46       0.39
     gemm_ln_nt_x3r              0.46       0.39         0.46       0.39
     bf16, f16                   0.54       0.20         0.54       0.20
     bf16a 128-tile              0.54     3.223e-7       0.54     3.223e-7
     fp8a 128-tile               0.57     3.252e-7       0.57     3.252e-7
     bf16a 256-tile              0.57     3.223e-7       0.57     3.223e-7
     fp8a 256-tile               0.57     3.252e-7       0.57     3.252e-7

The largest ratio is 0.57 on both; C_RATIO = 1.5 x 0.57, rounded up to
one digit = 0.9.  gelu_erfc stays inside the header's 4.2e-7.  RELU / LEAKY_RELU / NONE are bit-exact everywhere.

NaN: a NaN pre-activation through RELU gives 0 from the contraction kernels and LayerNorm (v > 0 ? v : 0) and NaN from
the transducer joint (x <= 0 ? 0 : x, torch.relu's rule: the search must see a NaN frame as one).
Planted mistakes (CPU only, host model): tanh-GELU for erf-GELU, slope 0.1, RELU for LEAKY_RELU, the activation applied
after alpha: each moves the statistic past 1.5 x its threshold.

Transducer joint: the first utterance and six frames of the smallest fixture of tests/test_transducer.py, every
activation, against tests/transducer_host_ref.py: equal tokens, scores within test_transducer's tolerance.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gemm_host_ref as R
import test_gemm_edges as G
import test_transducer as T
import transducer_host_ref

ALPHA = 0.5
C_RATIO = 0.9  # 1.5 x the largest measured ratio (0.57, emulator and MI355X), one digit, rounded up
GELU_ERFC_BOUND = 4.2e-7  # include/sbk.h, sbk_gemm_nt_bf16a


def _fp8a(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
    return nat.gemm_nt_fp8a(nat.quant_rows_fp8(a.to(dev)), w.to(dev), G._d(b, dev), G._d(r, dev), act=act, alpha=alpha).cpu()


def _bf16a(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):  # (G._bf16a, for operands that may hold NaN)
    assert torch.equal(a.bfloat16().float().nan_to_num(), a.nan_to_num())
    return nat.gemm_nt_bf16a(a.bfloat16().to(dev), w.to(dev), G._d(b, dev), G._d(r, dev), act=act, alpha=alpha).cpu()


def _ln(entry):
    def run(nat, dev, a, w, b=None, r=None, alpha=1.0, act=0):
        K = a.shape[1]
        wf, bf = nat._fold_ln(w, b, torch.ones(K), torch.zeros(K))
        return getattr(nat, entry)(a.to(dev), wf.to(dev), bf.to(dev), 1e-5, G._d(r, dev), act=act, alpha=alpha).cpu()
    return run


# form: (runner, operand kind, (M, N, K), knobs).  kind: significand bits of the operand type, "fp8a" or "ln"
FORMS = {
    "f32 tile kernels": (G._f32(skinny_off=1), 24, (65, 132, 34), {}),
    "f32 skinny route": (G._f32(), 24, (40, 132, 256), {}),
    "f32 stream-K forced": (G._f32(sk_mode=2), 24, (65, 68, 256), {}),
    "splitk slices=2": (G._splitk(2), 24, (40, 132, 1024), {}),
    "f32x3": (G._f32x3, 24, (63, 68, 96), {}),
    "x3p fp32 result": (G._x3p, 24, (63, 68, 48), {}),
    "x3p panel result": (G._x3p_panel, 24, (65, 144, 48), {}),
    "x3r": (G._x3r(), 24, (65, 132, 512), {}),
    "gemm_ln_nt": (_ln("gemm_ln_nt"), "ln", (40, 132, 256), {}),
    "gemm_ln_nt_x3r": (_ln("gemm_ln_nt_x3r"), "ln", (40, 132, 256), {}),
    "bf16": (G._lp("bf16"), 8, (63, 68, 72), {}),
    "f16": (G._lp("fp16"), 11, (63, 68, 72), {}),
    "bf16a 128-tile": (_bf16a, 8, (63, 68, 192), {}),
    "fp8a 128-tile": (_fp8a, "fp8a", (63, 68, 256), {}),
    "bf16a 256-tile": (_bf16a, 8, (257, 260, 256), dict(lp256=2)),
    "fp8a 256-tile": (_fp8a, "fp8a", (257, 260, 256), dict(lp256=2)),
}
ERFC_FORMS = ("bf16a 128-tile", "fp8a 128-tile", "bf16a 256-tile", "fp8a 256-tile")
ACTS = list(R.ACT_CODES)


@functools.lru_cache(maxsize=None)
def _operands(form):
    _, kind, (M, N, K), _ = FORMS[form]
    seed = M * 1000 + N * 10 + K
    if kind == "ln":
        return R.probe_act_ln(M, N, K, seed)
    if kind == "fp8a":
        return R.probe_act(M, N, K, seed, 4, by_row=True)
    return R.probe_act(M, N, K, seed, kind)


def _covered(pre, rtol=0.0):
    have = pre.reshape(-1)
    return all(bool(((have - t).abs() <= rtol * abs(t)).any()) for t in R.ACT_TARGETS)


def _pre_of(nat, dev, form):
    """The pre-activation values [M, N] in fp64 and whether they are the bits the epilogue holds."""
    run, kind, _, _ = FORMS[form]
    a, w, b, r, pre = _operands(form)
    if kind == "ln":
        assert _covered(pre, 1e-5)
        return pre, False
    if kind != "fp8a":
        assert _covered(pre)
        return pre, True
    mine = run(nat, dev, a, w, b).double()
    aq = nat.quant_rows_fp8(a.to(dev))
    wq, ws = nat.lp_weight(w.to(dev), "fp8r")
    a8 = G._e4m3(aq.q).view(a.shape).double() * aq.scale.cpu().double()[:, None]
    w8 = G._e4m3(wq).view(w.shape).double() * ws.cpu().double()[:, None]
    assert float((mine - (a8 @ w8.t() + b.double())).abs().max()) <= 1e-4 * float((a8.abs() @ w8.abs().t()).max()) + 1e-5
    assert _covered(mine, 1e-6), "the quantised rows lost a target"
    return mine, True


def _composition(pre, known, act, form, alpha, r):
    """torch's own fp32 ops on the CPU."""
    if known:
        v = pre.float()
    else:  # (LayerNorm prologue)
        a, w, b, _, _ = _operands(form)
        v = F.linear(F.layer_norm(a, (a.shape[1],), None, None, 1e-5), w, b)
    v = R.ACTS[act](v) * alpha
    return v if r is None else v + r


def _ratio(out, comp, ref, pre, alpha, row_floor):
    got, base = R.act_stat(out, ref, pre, alpha, row_floor), R.act_stat(comp, ref, pre, alpha, row_floor)
    return got / (base + 1.0), got, base


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("form", list(FORMS))
def test_epilogue_activation(backend, form, act):
    nat, dev = backend
    run, kind, shape, kn = FORMS[form]
    a, w, b, r, _ = _operands(form)
    with nat.knobs(**kn):
        pre, known = _pre_of(nat, dev, form)
        out = run(nat, dev, a, w, b, r, alpha=ALPHA, act=R.ACT_CODES[act])
        variants = [("", out, r)]
        if form.startswith("x3p") and act == "swish":
            variants.append((" no residual", run(nat, dev, a, w, b, None, alpha=ALPHA, act=R.ACT_CODES[act]), None))
        if form in ERFC_FORMS and act == "gelu":
            g = run(nat, dev, a, w, b, None, alpha=1.0, act=R.ACT_CODES[act])
            err = float((g.double() - F.gelu(pre)).abs().max())
            print(f"{form} {shape} gelu_erfc before alpha: max |error| {err:.3e} (bound {GELU_ERFC_BOUND:.1e})")
            assert err <= GELU_ERFC_BOUND
    for what, out, res in variants:
        ref = ALPHA * R.ACTS[act](pre) + (0.0 if res is None else res.double())
        comp = _composition(pre, known, act, form, ALPHA, res)
        ratio, got, base = _ratio(out, comp, ref, pre, ALPHA, kind == "ln")
        print(f"{form} {shape} {act}{what}: kernel {got:.2f} units, fp32 composition {base:.2f}, ratio {ratio:.2f}")
        assert not out.isnan().any()
        if known and act in ("none", "relu", "leaky_relu"):
            G._check_exact(out, comp, f"{form} {shape} {act}{what}")
        elif not (form in ERFC_FORMS and act == "gelu"):
            assert ratio <= C_RATIO, (form, act, what, got, base)


NAN_FORMS = [f for f, v in FORMS.items() if v[1] != "fp8a"]


@pytest.mark.parametrize("form", NAN_FORMS + ["layernorm"])
def test_relu_of_nan_is_zero(backend, form):
    """A row of NaN pre-activations through RELU: residual + alpha * 0 from every contraction entry, 0 from LayerNorm;
    the other rows are what they are without it."""
    nat, dev = backend
    if form == "layernorm":
        x = torch.randn(5, 132, generator=torch.Generator().manual_seed(3))
        x[2, 7] = float("nan")
        y = nat.layernorm(x.to(dev), torch.ones(132, device=dev), torch.zeros(132, device=dev), 1e-5, act=R.ACT_CODES["relu"]).cpu()
        assert torch.equal(y[2], torch.zeros(132)) and not y.isnan().any()
        return
    run, kind, shape, kn = FORMS[form]
    a, w, b, r, _ = _operands(form)
    bad = a.clone()
    bad[5] = float("nan")
    with nat.knobs(**kn):
        want = run(nat, dev, a, w, b, r, alpha=ALPHA, act=R.ACT_CODES["relu"])
        out = run(nat, dev, bad, w, b, r, alpha=ALPHA, act=R.ACT_CODES["relu"])
    want[5] = r[5]
    G._check_exact(out, want, f"{form} RELU of a NaN row")


@pytest.mark.parametrize("name", list(R.ACT_MISTAKES))
def test_cases_tell_activation_mistakes_apart(name):
    """The host model of the epilogue with one planted mistake, on the operands of the first form: the statistic moves
    past 1.5 x its threshold; the fp32 composition alone stays inside it."""
    act, wrong = R.ACT_MISTAKES[name]
    _, _, _, r, pre = _operands("f32 tile kernels")
    ref = ALPHA * R.ACTS[act](pre) + r.double()
    comp = _composition(pre, True, act, None, ALPHA, r)
    base = R.act_stat(comp, ref, pre, ALPHA)
    got = R.act_stat((wrong(pre, ALPHA) + r.double()).float(), ref, pre, ALPHA)
    print(f"'{name}': {got:.3g} units against a threshold of {C_RATIO * (base + 1.0):.3g}")
    assert base <= C_RATIO * (base + 1.0)
    assert got >= 1.5 * C_RATIO * (base + 1.0)


# ------------------------------------------------------------------ the transducer joint
TD_ACTS = ("gelu", "leaky_relu", "relu", "tanh")
TD_FRAMES = 6


def _td_case(dev, act, blank=0, nan_frame=None):
    from speechbrain_amd import native

    z, meta = T._golden()
    case, sd = meta[0], T._case(z, 0)
    cfg = case["cfg"]
    s = T._searcher(cfg, sd, dev)
    tn = np.ascontiguousarray(sd["tn"][:1, :TD_FRAMES]).copy()
    if nan_frame is not None:
        tn[0, nan_frame, 1] = np.nan
    B, _, J = tn.shape
    st = [torch.empty(B, J, device=dev), torch.empty(cfg["L"], B, cfg["H"], device=dev), torch.empty(cfg["L"], B, cfg["H"], device=dev)]
    code = {"gelu": native.ACT_GELU, "leaky_relu": native.ACT_LEAKY_RELU, "relu": native.ACT_RELU, "tanh": native.ACT_TANH}[act]
    tokens, count, score = native.transducer_greedy(s._prepare(torch.device(dev)), torch.from_numpy(tn).to(dev), st[0], st[1], st[2],
                                                    blank, cfg["S"], start_from_blank=True, act=code)
    net = transducer_host_ref.Network({k: v for k, v in sd.items()}, act)
    with np.errstate(invalid="ignore"):
        want = transducer_host_ref.greedy(net, tn, blank, cfg["S"])
    n = int(count.cpu()[0])
    return tokens.cpu()[0, :n].tolist(), float(score.cpu()[0]), [t.cpu().numpy() for t in st], want


@pytest.mark.parametrize("act", TD_ACTS)
def test_transducer_joint_activation(backend, act):
    _, dev = backend
    toks, score, (out_pn, h, c), (w_toks, w_score, w_out, w_h, w_c, gaps) = _td_case(dev, act)
    assert min(gaps[0]) >= T.MIN_GAP, "the host search decides a frame by less than the margin token identity needs"
    assert toks == w_toks[0]
    T._close(score, w_score[0], what=(act, "score"))
    T._close(out_pn, w_out, what=(act, "out_pn"))
    T._close(h, w_h, what=(act, "h"))
    T._close(c, w_c, what=(act, "c"))


def test_transducer_relu_keeps_nan(backend):
    """One NaN element in one frame, RELU, blank = 1: the joint hands the NaN on, every log-probability of the frame is
    NaN, the arg-max rule (NaN above everything, first index) emits token 0 and the score is NaN.  A ReLU that mapped
    NaN to 0 would decode the frame as if nothing had happened."""
    _, dev = backend
    toks, score, _, (w_toks, w_score, *_) = _td_case(dev, "relu", blank=1, nan_frame=2)
    assert np.isnan(score) and np.isnan(w_score[0])
    assert toks == w_toks[0]
