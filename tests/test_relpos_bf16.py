"""RelPosMHAXL attention under precision "bf16": relpos_flash_t_bf16_kernel (csrc/relpos_attn.hip, sbk_relpos_attention_bf16)
against the plain fp64 composition of tests/encoder_host_ref.py, on the CPU emulator of the kernel sources and, marked gpu, on
the MI355X; its routing from native.relpos_attention; and a Conformer reached through eval_precision "bf16" alone.

Inputs, fp64 references and shapes are those of tests/test_encoder_kernels.py (its cached _inputs / _case: the tile, ring and
workgroup edges, with T 70 / key length 64 / chunk (16, 0) whose queries 64 .. 69 have no allowed key).  Bound, the project's
rule for every bf16 kernel: 2 * e_model + 1e-3 on the max abs context error, e_model = the error against the fp64 composition
of _model below -- the same composition in fp64 with exactly the kernel's roundings.  Every case prints kernel error / e_model.
Largest ratio: 1.035 on the MI355X and 1.035 on the emulator (B 3, T 130, chunk (40, 0): 9.5e-3 against e_model 9.2e-3)."""
import functools

import pytest
import torch

import encoder_host_ref as R
from test_encoder_kernels import _case, _cid, _inputs, _ratio, _sid

SHAPES = [(1, 1, 1, None), (2, 31, 2, (31, 1)), (2, 33, 2, (33, 5)), (1, 65, 2, (33,)), (1, 70, 1, (64,)), (3, 130, 2, (130, 97, 1))]
CHUNKS = [(0, -1), (16, 0), (5, 2), (40, 0)]
TINY = dict(d_model=128, nhead=2, d_ffn=256, n_enc=2, n_dec=1, n_fft=512, win_length=32)


@functools.lru_cache(maxsize=None)
def _model_err(B, T, H, lens, chunk, left):
    """The kernel's roundings in fp64 arithmetic, position rows gathered with rel_index (no shift): (q+u) s and (q+v) s formed in
    fp32 and rounded to bf16; k, the position rows, v rounded; the position term added unrounded; exp(s - max) rounded as the
    operand of the context product, the normaliser from the unrounded values."""
    kw, r = _inputs("relpos", 64, B, T, H), R.bf16_round
    q, k, v = [t.transpose(1, 2) for t in kw["qkv"].reshape(B, T, H, 3, 64).unbind(3)]  # [B,H,T,64] fp32
    qu = r((q + kw["bias_u"].reshape(1, H, 1, 64)) * 0.125).double()
    qv = r((q + kw["bias_v"].reshape(1, H, 1, 64)) * 0.125).double()
    p = r(kw["pos"]).double().reshape(2 * T - 1, H, 64).permute(1, 2, 0)
    sc = qu @ r(k).double().transpose(-1, -2) + (qv @ p).gather(-1, R.rel_index(T).expand(B, H, T, T))
    ok = R.allowed_keys(B, T, lens, chunk, left)[:, None]
    seen = ok.any(-1, keepdim=True)
    sc = sc.masked_fill(~ok, float("-inf"))
    e = torch.exp(sc - torch.where(seen, sc.amax(-1, keepdim=True), torch.zeros((), dtype=torch.float64)))
    ctx = (r(e) @ r(v).double()) / torch.where(seen, e.sum(-1, keepdim=True), torch.ones((), dtype=torch.float64))
    return float((ctx.transpose(1, 2).reshape(B, T, H * 64) - _case("relpos", 64, B, T, H, lens, chunk, left)[0]).abs().max())


def _call(nat, dev, precision, Dh, B, T, H, lens, chunk=0, left=-1, want_attn=False, out=None):
    """(context on the host, names the profiler saw)"""
    kw = _inputs("relpos", Dh, B, T, H)
    kl = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    nat.prof_reset()
    nat.prof_enable(True)
    with nat.precision_scope(precision):
        ctx, _ = nat.relpos_attention(kw["qkv"].to(dev), kw["pos"].to(dev), kw["bias_u"].to(dev), kw["bias_v"].to(dev), kl, H,
                                      Dh ** -0.5, want_attn, chunk, left, out=out)
    nat.prof_enable(False)
    return ctx.cpu(), set(nat.prof_report())


@pytest.mark.parametrize("chunk,left", CHUNKS, ids=[_cid(c) for c in CHUNKS])
@pytest.mark.parametrize("B,T,H,lens", SHAPES, ids=[_sid(s) for s in SHAPES])
def test_relpos_bf16_vs_fp64_composition(backend, B, T, H, lens, chunk, left):
    nat, dev = backend
    ref, _, _, seen = _case("relpos", 64, B, T, H, lens, chunk, left)
    e_model = _model_err(B, T, H, lens, chunk, left)
    ctx, names = _call(nat, dev, "bf16", 64, B, T, H, lens, chunk, left)
    err = float((ctx.double() - ref).abs().max())
    print(f"[relpos bf16] {_sid((B, T, H))} {_cid((chunk, left))}: err {err:.3e} e_model {e_model:.3e} ratio {_ratio(err, e_model):.3f}")
    assert names == {"relpos_attention_bf16"}
    assert not bool(torch.isnan(ctx).any())
    assert err <= 2.0 * e_model + 1e-3
    assert not ctx[~seen].any()  # no allowed key: exactly zero


def test_routing_by_precision_weights_output_and_head_dim(backend):
    nat, dev = backend
    shape = (2, 33, 2, (33, 5))
    c32, names = _call(nat, dev, "fp32", 64, *shape)
    assert names == {"relpos_attention"}
    cb, names = _call(nat, dev, "bf16", 64, *shape)
    assert names == {"relpos_attention_bf16"} and not torch.equal(cb, c32)
    for Dh, want_attn in ((64, True), (32, False)):  # the weights output and other head dims keep the fp32 kernels, bit for bit
        a, names = _call(nat, dev, "bf16", Dh, *shape, want_attn=want_attn)
        assert names == {"relpos_attention"} and torch.equal(a, _call(nat, dev, "fp32", Dh, *shape, want_attn=want_attn)[0])
    assert torch.equal(_call(nat, dev, "fp32", 64, *shape)[0], c32) and nat.precision() == "fp32"  # nothing leaks out of the scope


def test_out_is_a_slice_of_a_group_buffer(backend):
    nat, dev = backend
    B, T, H, lens = 3, 130, 2, (130, 97, 1)
    big = torch.full((B * T + 9, H * 64), float("nan")).to(dev)
    got, _ = _call(nat, dev, "bf16", 64, B, T, H, lens, 16, 0, out=big[4: 4 + B * T].view(B, T, H * 64))
    assert torch.equal(got, _call(nat, dev, "bf16", 64, B, T, H, lens, 16, 0)[0])
    assert torch.equal(big[4: 4 + B * T].cpu().view(B, T, -1), got)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())


def test_conformer_reaches_the_kernel_through_eval_precision(backend):
    """Head dim 64 Conformer, two batches (T' 129 and 138) of >= 256 encoder rows AND >= 256 position rows each: gemm_nt picks
    the bf16 kernel by row count, so only then does every contraction round alike in the single and the grouped pass (with a
    position table below 256 rows the grouped pass, which projects both tables at once, differs at the bf16 level).  One bf16
    relpos launch per layer, encode_group = encode_batch bit for bit, and the bf16 "GEMMs + attention" encoder within the 1e-2
    relative RMS of the fp32 path that tests/test_full_size_gpu.py holds the project's bf16 path to."""
    nat, dev = backend
    from speechbrain_amd.inference.builders import build_asr

    asr = build_asr(TINY, vocab=30, seed=2, beam_size=2, ctc_weight=0.3, device=str(dev))
    g = torch.Generator().manual_seed(8)
    batches = [(0.1 * torch.randn(2, 81920, generator=g), torch.tensor([1.0, 0.6])), (0.1 * torch.randn(2, 88000, generator=g), torch.ones(2))]
    e32 = [asr.encode_batch(w, l).cpu() for w, l in batches]
    asr.eval_precision = "bf16"
    nat.prof_reset()
    nat.prof_enable(True)
    e16 = [asr.encode_batch(w, l).cpu() for w, l in batches]
    nat.prof_enable(False)
    rep = nat.prof_report()
    assert rep["relpos_attention_bf16"]["count"] == 2 * TINY["n_enc"] and "relpos_attention" not in rep and "gemm_nt_bf16" in rep
    for a, b in zip(asr.encode_group(batches), e16):
        assert torch.equal(a.cpu(), b)
    for a, b in zip(e16, e32):
        rel = float(((a - b).double().pow(2).mean() / b.double().pow(2).mean()).sqrt())
        print(f"conformer d 128 / 2 heads, bf16 vs fp32 encoder: relative RMS {rel:.3e}")
        assert 0.0 < rel <= 1e-2
