"""Head dim 128 under precision "bf16": rope_flash_t128_bf16_kernel (csrc/relpos_attn.hip, through sbk_rope_attention_bf16) against
the plain fp64 composition of tests/test_attention_dh128.py, on the CPU emulator of the kernel sources and, marked gpu, on the
MI355X; its routing from native.rope_attention; and a Transformer encoder (d 256, 2 heads) reached through the precision scope.

Shapes: one key / a ragged query tile and a key length inside the first tile / one key past two 32-key stages / a key length on a
stage edge / a second workgroup with ONE live wave (three idle ones that still meet the barriers) / three utterances of lengths
130, 97, 1.  Chunk masks at T = 70 ((16, 0): queries 64 .. 69 have no allowed key) and at T = 130 ((40, 0) and (5, 2): the waves of a
workgroup walk different key-tile ranges).  Bound, the project's rule for every bf16 kernel: 2 * e_model + 1e-3 on the max abs
context error, e_model = the error of the same fp64 composition with exactly the kernel's four roundings (_case).  Every case
prints kernel error / e_model.  Largest ratio: 1.012 on the MI355X and on the emulator (B 3, T 130, chunk (5, 2), RoPE)."""
import functools
import math

import pytest
import torch

from encoder_host_ref import allowed_keys, bf16_round
from test_attention_dh128 import _compose, _tables

DH = 128
SHAPES = [(1, 1, 1, None), (2, 33, 2, (33, 5)), (1, 65, 1, None), (1, 70, 1, (64,)), (1, 129, 1, (128,)), (3, 130, 2, (130, 97, 1))]
EXTRA = {70: [(16, 0), (8, -1)], 130: [(40, 0), (5, 2)]}
CASES = [(*s, c, l) for s in SHAPES for c, l in [(0, -1)] + EXTRA.get(s[1], [])]


@functools.lru_cache(maxsize=None)
def _case(B, T, H, lens, rope, chunk, left):
    """(qkv, fp64 reference, e_model, [B,T] bool: the query has an allowed key).  The model: q and k rotated in fp32, q scaled in
    fp32, both rounded to bf16; v rounded; exp(s - max) rounded as the operand of the context product, the normaliser from the
    unrounded values; everything else fp64."""
    qkv = torch.randn(B, T, 3 * H * DH, generator=torch.Generator().manual_seed(1000 * T + 10 * H + rope))
    ref = _compose(qkv, H, None if lens is None else list(lens), rope, chunk, left, torch.float64)
    q, k, v = [t.transpose(1, 2) for t in qkv.reshape(B, T, H, 3, DH).unbind(3)]  # [B,H,T,Dh] fp32
    if rope:
        cos, sin = _tables(T, torch.float32)
        swap = torch.arange(DH) ^ 1
        q, k = q * cos + q[..., swap] * sin, k * cos + k[..., swap] * sin
    sc = bf16_round(q * (1.0 / math.sqrt(DH))).double() @ bf16_round(k).double().transpose(-1, -2)
    ok = allowed_keys(B, T, lens, chunk, left)[:, None]
    seen = ok.any(-1, keepdim=True)
    sc = sc.masked_fill(~ok, float("-inf"))
    e = torch.exp(sc - torch.where(seen, sc.amax(-1, keepdim=True), torch.zeros((), dtype=torch.float64)))
    ctx = (bf16_round(e) @ bf16_round(v).double()) / torch.where(seen, e.sum(-1, keepdim=True), torch.ones((), dtype=torch.float64))
    return qkv, ref, float((ctx.transpose(1, 2).reshape(B, T, H * DH) - ref).abs().max()), seen[:, 0, :, 0]


def _call(nat, dev, precision, qkv, H, lens, rope, chunk=0, left=-1, **kw):
    """(context on the host, names the profiler saw); precision None = outside any scope"""
    cos, sin = [t.contiguous().to(dev) for t in _tables(qkv.shape[1], torch.float32)] if rope else (None, None)
    kl = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    args = (qkv.to(dev), cos, sin, kl, H, 1.0 / math.sqrt(DH), kw.pop("want_attn", False), chunk, left)
    nat.prof_reset()
    nat.prof_enable(True)
    if precision is None:
        ctx, _ = nat.rope_attention(*args, **kw)
    else:
        with nat.precision_scope(precision):
            ctx, _ = nat.rope_attention(*args, **kw)
    nat.prof_enable(False)
    return ctx.cpu(), set(nat.prof_report())


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("B,T,H,lens,chunk,left", CASES, ids=[f"B{c[0]}-T{c[1]}-H{c[2]}-chunk{c[4]}_{c[5]}" for c in CASES])
def test_dh128_bf16_vs_fp64_composition(backend, B, T, H, lens, chunk, left, rope):
    nat, dev = backend
    qkv, ref, e_model, seen = _case(B, T, H, lens, rope, chunk, left)
    ctx, names = _call(nat, dev, "bf16", qkv, H, lens, rope, chunk, left)
    err = float((ctx.double() - ref).abs().max())
    print(f"[dh128 bf16] {'rope' if rope else 'plain'} B={B} T={T} H={H} chunk=({chunk},{left}): err {err:.3e} e_model {e_model:.3e} "
          f"ratio {err / e_model if e_model > 0.0 else float(err > 0.0):.3f}")
    assert names == {"rope_attention_bf16"}
    assert not bool(torch.isnan(ctx).any())
    assert err <= 2.0 * e_model + 1e-3
    assert not ref[~seen].any() and not ctx[~seen].any()  # no allowed key: exactly zero
    assert (T, chunk, left) != (70, 16, 0) or not bool(seen[:, 64:].any())


def test_routing_by_precision_out_slice_and_refusals(backend):
    nat, dev = backend
    B, T, H, lens = 3, 130, 2, (130, 97, 1)
    qkv = _case(B, T, H, lens, True, 16, 0)[0]
    bare, names = _call(nat, dev, None, qkv, H, lens, True, 16, 0)
    assert names == {"rope_attention"}
    c32, names = _call(nat, dev, "fp32", qkv, H, lens, True, 16, 0)
    assert names == {"rope_attention"} and torch.equal(c32, bare)  # "fp32" is the fp32 kernel, bit for bit
    cb, names = _call(nat, dev, "bf16", qkv, H, lens, True, 16, 0)
    assert names == {"rope_attention_bf16"} and not torch.equal(cb, c32)
    big = torch.full((B * T + 9, H * DH), float("nan")).to(dev)  # out = a slice of a group buffer: filled exactly, nothing else written
    got, _ = _call(nat, dev, "bf16", qkv, H, lens, True, 16, 0, out=big[4: 4 + B * T].view(B, T, H * DH))
    assert torch.equal(got, cb) and torch.equal(big[4: 4 + B * T].cpu().view(B, T, -1), cb)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())
    with pytest.raises(nat.SbkError, match="head_dim 64"):
        _call(nat, dev, "bf16", qkv, H, lens, True, out_dtype=torch.bfloat16)
    with pytest.raises(nat.SbkError, match="head_dim 128"):
        _call(nat, dev, "bf16", qkv, H, lens, True, want_attn=True)
    u = torch.zeros(H * DH).to(dev)
    with nat.precision_scope("bf16"), pytest.raises(nat.SbkError, match=r"head_dim 128 not instantiated \(8,16,32,36,64\)"):
        nat.relpos_attention(qkv.to(dev), torch.randn(2 * T - 1, H * DH).to(dev), u, u, None, H, 0.1)  # RelPosMHAXL at 128: as before
    assert nat.precision() == "fp32" and torch.equal(_call(nat, dev, None, qkv, H, lens, True, 16, 0)[0], bare)  # nothing leaks


def test_transformer_encoder_reaches_the_kernel(backend):
    """2-layer pre-norm TransformerEncoder, d 256 / 2 heads, two batches of >= 256 rows each (gemm_nt picks its bf16 kernel by row
    count: only then does every contraction round alike in the single and the grouped pass).  One bf16 attention launch per layer,
    forward_group = forward bit for bit, and the bf16 encoder within the 1e-2 relative RMS of the fp32 one that
    tests/test_full_size_gpu.py holds the project's bf16 path to."""
    nat, dev = backend
    from speechbrain_amd.lobes.models.transformer.Transformer import TransformerEncoder

    torch.manual_seed(3)
    enc = TransformerEncoder(num_layers=2, nhead=2, d_ffn=256, d_model=256, normalize_before=True).to(dev).eval()
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(2, 129, 256, generator=g).to(dev), torch.randn(2, 138, 256, generator=g).to(dev)]
    kls = [torch.tensor(l, dtype=torch.int32).to(dev) for l in ((129, 70), (138, 138))]
    pad = lambda x, kl: torch.arange(x.shape[1], device=dev)[None] >= kl[:, None]  # noqa: E731
    with torch.no_grad():
        e32 = [enc(x, src_key_padding_mask=pad(x, kl))[0].cpu() for x, kl in zip(xs, kls)]
        nat.prof_reset()
        nat.prof_enable(True)
        with nat.precision_scope("bf16"):
            e16 = [enc(x, src_key_padding_mask=pad(x, kl))[0].cpu() for x, kl in zip(xs, kls)]
        nat.prof_enable(False)
        rep = nat.prof_report()
        assert rep["rope_attention_bf16"]["count"] == 2 * 2 and "rope_attention" not in rep and "gemm_nt_bf16" in rep
        segs = [(0, 2, 129, kls[0], 0), (2 * 129, 2, 138, kls[1], 0)]
        with nat.precision_scope("bf16"):
            grouped = enc.forward_group(torch.cat([x.reshape(-1, 256) for x in xs]), None, segs).cpu()
    for (r0, B, T, _, _), a, b in zip(segs, e16, e32):
        assert torch.equal(grouped[r0: r0 + B * T].view(B, T, 256), a)
        rel = float(((a - b).double().pow(2).mean() / b.double().pow(2).mean()).sqrt())
        print(f"transformer encoder d 256 / 2 heads, bf16 vs fp32: relative RMS {rel:.3e}")
        assert 0.0 < rel <= 1e-2
