"""wav2vec 2.0 / HuBERT / WavLM under precision "bf16": sbk_wavlm_attention_bf16 (csrc/wavlm.hip) and sbk_w2v_posconv_bf16
(csrc/wav2vec2.hip) against the plain fp64 compositions of tests/wavlm_host_ref.py / wav2vec2_host_ref.py, on the CPU emulator of
the kernel sources (not gpu) and on the MI355X (-m gpu), and the wrappers through an EncoderASR under run_opts precision "bf16".

Bound for both kernels (the rule for bf16 attention of tests/test_encoder_kernels.py): 2 * e_model + 1e-3, e_model = the max
error, against the plain fp64 composition, of the fp64 composition with the kernel's roundings made explicit (attention:
q * scale, k, v and exp(s - max) to bf16, normaliser from the unrounded probabilities, bias unrounded; positional convolution:
masked x and the filter to bf16, residual unrounded).  Every case prints ratio = kernel error / e_model.
Largest ratios: wavlm_attention 1.04 on the MI355X and 1.04 on the emulator; w2v_posconv 1.00 on both.
Model test, relative RMS error against the fp64 host restatement: the kernels under bf16 5.13e-3 (WavLM) / 5.07e-3 (wav2vec 2.0),
the fp32 restatement under torch.autocast("cpu", bfloat16) 1.01e-2 / 1.01e-2 (the fp32 path: 8.3e-7)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import wav2vec2_host_ref as W
import wavlm_host_ref as R

B, H, DH = 2, 2, 64
_CASES = {}


def _r(t):  # round to bf16 (nearest even) from fp32, as the kernels do; carried on in fp64
    return t.float().bfloat16().double()


def _bound(e_model):
    return 2.0 * e_model + 1e-3


def _rel_rms(y, ref):
    return float(((y.double() - ref).pow(2).mean() / ref.pow(2).mean()).sqrt())


def _attention_model(q, k, v, gate, bias, kl, scale, bias_on=True):
    """The composition with the roundings of wavlm_flash_t_bf16_kernel: q, k, v [B,H,T,Dh] fp32, gate [B,H,T], bias [H,T,T] fp64."""
    s = _r(q * scale) @ _r(k).transpose(-1, -2)
    if bias_on:
        s = s + gate[..., None] * bias[None]
    if kl is not None:
        s = s.masked_fill((torch.arange(s.shape[-1])[None, :] >= kl[:, None])[:, None, None, :], float("-inf"))
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return ((_r(p) @ _r(v)) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(q.shape[0], q.shape[2], -1)


def _attention_case(Dh, T, ragged):
    """Inputs, the fp64 reference, e_model: once per case, never modified."""
    key = ("att", Dh, T, ragged)
    if key not in _CASES:
        gen = torch.Generator().manual_seed(100 * Dh + 7 * T + ragged)
        d, n = H * Dh, 2 * T - 1
        qkv = torch.randn(B, T, H, 3, Dh, generator=gen)
        x = torch.randn(B, T, d, generator=gen)
        gate_w = torch.randn(8, Dh, generator=gen) * (0.6 / Dh ** 0.5)
        gate_b, gate_const = 0.3 * torch.randn(8, generator=gen), torch.tensor([1.3, -0.8])
        tab = torch.stack([2.0 * torch.sin(0.37 * torch.arange(n) + 1.1 * h) + 0.011 * torch.arange(n) * (-1.0) ** h
                           for h in range(H)])  # distinct at every offset and in every head, of the scores' size
        kl = torch.tensor([1, max(1, (2 * T) // 3)], dtype=torch.int32) if ragged else None  # a one-key utterance
        i = torch.arange(T)
        bias = tab[:, (i[None, :] - i[:, None]) + T - 1].double()
        q, k, v = (qkv[:, :, :, j].transpose(1, 2) for j in range(3))
        kl64 = None if kl is None else kl.long()
        dd = lambda t: t.double()  # noqa: E731
        ref = R.gated_attention(dd(q), dd(k), dd(v), dd(x), dd(gate_w), dd(gate_b), dd(gate_const), bias, kl64, Dh ** -0.5)
        model = functools.partial(_attention_model, q, k, v, R.gate(dd(x), dd(gate_w), dd(gate_b), dd(gate_const), H), bias, kl64,
                                  Dh ** -0.5)
        _CASES[key] = ((qkv.reshape(B, T, 3 * d).contiguous(), x, gate_w, gate_b, gate_const, tab, kl), ref,
                       float((model() - ref).abs().max()), model)
    return _CASES[key]


def _attend(nat, dev, args, Dh, precision, out=None):
    with nat.precision_scope(precision):
        return nat.wavlm_attention(*(None if t is None else t.to(dev) for t in args), H, Dh ** -0.5, out=out)


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("T", (1, 31, 32, 33, 97, 130))
def test_wavlm_attention_bf16_vs_fp64_composition(backend, T, ragged):
    nat, dev = backend
    args, ref, e_model, _ = _attention_case(DH, T, ragged)
    nat.prof_reset()
    nat.prof_enable(True)
    big = torch.full((B * T + 9, H * DH), float("nan"), device=dev)  # out: a slice of a poisoned buffer
    _attend(nat, dev, args, DH, "bf16", out=big[4: 4 + B * T].view(B, T, H * DH))
    nat.prof_enable(False)
    assert "wavlm_attention_bf16" in nat.prof_report() and "wavlm_attention" not in nat.prof_report()
    err = float((big[4: 4 + B * T].view(B, T, -1).cpu().double() - ref).abs().max())
    print(f"wavlm_attention_bf16 T={T} ragged={ragged}: kernel max|d| {err:.3e}, e_model {e_model:.3e}, ratio {err / e_model:.2f}")
    assert err <= _bound(e_model)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())


def test_wavlm_attention_head_dim_32_keeps_the_fp32_kernel(backend):
    nat, dev = backend
    args = _attention_case(32, 33, True)[0]
    assert torch.equal(_attend(nat, dev, args, 32, "bf16"), _attend(nat, dev, args, 32, "fp32"))


def _posconv_model(x, kl, w, bias, G, ln, flip=False):
    """The composition with the roundings of w2v_posconv_bf16_kernel (x, w fp32; the rest fp64)."""
    xm = x.double() if kl is None else x.double() * (torch.arange(x.shape[1])[None, :] < kl[:, None])[:, :, None]
    w = w.flip(-1) if flip else w
    y = W.posconv(_r(xm), None, _r(w), bias, G) - _r(xm) + xm  # (the residual is the unrounded masked x)
    return y if ln is None else F.layer_norm(y, (x.shape[-1],), *ln)


def _posconv_case(cg, k, T, ragged, ln):
    key = ("pc", cg, k, T, ragged, ln)
    if key not in _CASES:
        G, Bp = 2, 3
        d = G * cg
        gen = torch.Generator().manual_seed(1000 * cg + 10 * k + T)
        x = torch.randn(Bp, T, d, generator=gen)
        w = torch.randn(d, cg, k, generator=gen) * (2.0 / (cg * k) ** 0.5)
        bias, gamma, beta = (0.2 * torch.randn(d, generator=gen) for _ in range(3))
        kl = torch.tensor([T, 1, max(1, (2 * T) // 3)], dtype=torch.int32) if ragged else None
        kl64 = None if kl is None else kl.long()
        ln64 = (1.0 + gamma.double(), beta.double(), 1e-5) if ln else None
        ref = W.posconv(x.double(), kl64, w.double(), bias.double(), G, ln64)
        model = functools.partial(_posconv_model, x, kl64, w, bias.double(), G, ln64)
        args = (x, kl, w.permute(0, 2, 1).reshape(d, -1).contiguous(), bias, G, k)
        _CASES[key] = (args, (1.0 + gamma, beta, 1e-5) if ln else None, ref, float((model() - ref).abs().max()), model)
    return _CASES[key]


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
@pytest.mark.parametrize("T", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("k", (1, 3, 128))
@pytest.mark.parametrize("cg", (16, 32, 48, 64))
def test_posconv_bf16_vs_fp64_composition(backend, cg, k, T, ragged, ln):
    nat, dev = backend
    args, lnp, ref, e_model, _ = _posconv_case(cg, k, T, ragged, ln)
    to = lambda t: t.to(dev) if torch.is_tensor(t) else t  # noqa: E731
    nat.prof_reset()
    nat.prof_enable(True)
    with nat.precision_scope("bf16"):
        y = nat.w2v_posconv(*(to(t) for t in args), ln=None if lnp is None else tuple(to(t) for t in lnp))
    nat.prof_enable(False)
    assert "w2v_posconv_bf16" in nat.prof_report() and "w2v_posconv" not in nat.prof_report()
    err = float((y.cpu().double() - ref).abs().max())
    print(f"w2v_posconv_bf16 {cg} {k} {T} ragged={ragged} ln={ln}: max|d| {err:.3e}, e_model {e_model:.3e}, ratio {err / e_model:.2f}")
    assert err <= _bound(e_model)


def test_the_cases_can_tell_a_dropped_bias_and_reversed_taps():
    """Host only: the bias rounded to zero, and the taps reversed, each move a committed case by >= 1e2 x its bound.  (The
    attention case is a full-length one: the one-key utterance of the ragged cases has a softmax of 1 whatever the bias is.)"""
    _, ref, e_model, model = _attention_case(DH, 97, False)
    assert float((model(bias_on=False) - ref).abs().max()) >= 1e2 * _bound(e_model)
    _, _, ref, e_model, model = _posconv_case(64, 128, 130, True, False)
    assert float((model(flip=True) - ref).abs().max()) >= 1e2 * _bound(e_model)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["wavlm", "wav2vec2"])
def test_wrappers_under_an_encoder_asr_with_precision_bf16(kind):
    """A 2-layer d 768 / 12 heads wrapper (random weights, B 4, T' = 74: every contraction has >= 256 rows) as the child of an
    EncoderASR's encoder container: under "bf16" the profiler shows the bf16 kernels and no fp32 form of them, and the output
    is no further from the fp64 host restatement than that restatement in fp32 under torch.autocast("cpu", bfloat16) -- what
    the reference does for precision bf16; under "fp32" the container's output is the direct call's, bit for bit."""
    from speechbrain_amd import native
    from speechbrain_amd.inference.ASR import EncoderASR
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM
    from speechbrain_amd.nnet.containers import LengthsCapableSequential

    cfg = dict(model_type=kind, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072)
    w = (WavLM if kind == "wavlm" else Wav2Vec2).from_config(cfg, seed=3)
    sd = {k[len("model."):]: v.detach().clone() for k, v in w.state_dict().items()}
    cfg, host = w.model.config, (R if kind == "wavlm" else W)
    wav = 0.3 * torch.randn(4, 73 * 320 + 400, generator=torch.Generator().manual_seed(5))
    ref = host.forward(wav.double(), None, {k: v.double() for k, v in sd.items()}, cfg, False)  # [4, 74, 768]
    with torch.autocast("cpu", dtype=torch.bfloat16):
        e_autocast = _rel_rms(host.forward(wav, None, sd, cfg, False), ref)
    hparams = {"tokenizer": None, "decoding_function": functools.partial(lambda p, lens: None)}
    out = {}
    for prec in ("fp32", "bf16"):
        asr = EncoderASR({"encoder": LengthsCapableSequential(w2v=w)}, hparams, run_opts={"device": "cuda:0", "precision": prec})
        native.prof_reset()
        native.prof_enable(True)
        out[prec] = asr.encode_batch(wav, torch.ones(4)).cpu()
        native.prof_enable(False)
        names = set(native.prof_report())
        attention = "wavlm_attention" if kind == "wavlm" else "rope_attention"
        lp, f32 = {attention + "_bf16", "w2v_posconv_bf16", "gemm_nt_bf16"}, {attention, "w2v_posconv"}
        assert (lp <= names and not f32 & names) if prec == "bf16" else (f32 <= names and not lp & names), sorted(names)
    assert torch.equal(out["fp32"], w(wav.cuda()).cpu())
    e_kernels = _rel_rms(out["bf16"], ref)
    print(f"{kind}: relative RMS error vs fp64: kernels under bf16 {e_kernels:.3e}, fp32 restatement under autocast(bf16) "
          f"{e_autocast:.3e}, fp32 path {_rel_rms(out['fp32'], ref):.3e}")
    assert e_kernels <= e_autocast
