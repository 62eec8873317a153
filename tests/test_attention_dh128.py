"""Head dim 128 in the fp32 attention kernels (the transformer.yaml recipe: d_model 512, 4 heads).

Encoder: csrc/relpos_attn.hip rope_flash_t128_kernel through native.rope_attention, plain (no tables) and RoPE, against the fp64
torch composition of the same inputs.  Decoder: csrc/decoder.hip cross_attn_step_kernel<128, .> and self_attn_step_kernel<2>
through native.decoder_prefix and the beam search, against the oracle's decoder run in fp64.

Bound (test_csgu.py's rule): the fp32 torch composition's own max error against fp64 on the same inputs, times 4 (another, equally
legitimate, summation order), with a floor of 1e-5.  References are computed once per shape and never modified."""
import functools
import math

import pytest
import torch

from oracle import sb_oracle as O

DH = 128

# (B, T, H, lens): a single query and key / one full 32-query tile plus one row, a key length inside the first key tile / a key
# length exactly on a tile edge with a ragged last query tile / more than 128 queries (two workgroups on the x axis), a one-key
# utterance
SHAPES = [(1, 1, 1, None), (2, 33, 2, [33, 5]), (1, 70, 1, [64]), (3, 130, 2, [130, 97, 1])]
# Dynamic Chunk masks at the T = 70 shape: chunk 16 with NO left context (the first key tile of the later query tiles is skipped,
# and the queries 64 .. 69 -- chunk 4, keys [64, 80) cut to the key length 64 -- have no allowed key: zero context), chunk 8 with
# unlimited left context
CHUNKS = [(16, 0), (8, -1)]


def _tables(T, dtype):
    from speechbrain_amd.nnet.attention import PrecomputedRoPESinusoids

    tab = PrecomputedRoPESinusoids(max(T, 2), DH, torch.float32, "cpu")
    return tab.cosines[:T].to(dtype), tab.sines[:T].to(dtype)


def _compose(qkv, H, lens, rope, chunk, left, dtype):
    """softmax(q k^T / sqrt(Dh), allowed keys) v in `dtype`; qkv [B,T,H,(q|k|v)]; a query without an allowed key gets zeros."""
    B, T, _ = qkv.shape
    q, k, v = [t.transpose(1, 2) for t in qkv.to(dtype).reshape(B, T, H, 3, DH).unbind(3)]  # [B,H,T,Dh]
    if rope:
        cos, sin = _tables(T, dtype)  # x'[c] = x[c] cos[t][c] + x[c ^ 1] sin[t][c] (signed sines)
        swap = torch.arange(DH) ^ 1
        q, k = q * cos + q[..., swap] * sin, k * cos + k[..., swap] * sin
    sc = torch.matmul(q * (1.0 / math.sqrt(DH)), k.transpose(-1, -2))
    klen = torch.full((B,), T) if lens is None else torch.tensor(lens)
    key = torch.arange(T)
    allowed = (key[None, None, :] < klen[:, None, None]).expand(B, T, T).clone()
    if chunk > 0:
        c = torch.arange(T) // chunk
        allowed &= (key[None, :] < ((c + 1) * chunk)[:, None])[None]
        if left >= 0:
            allowed &= (key[None, :] >= ((c - left) * chunk).clamp(min=0)[:, None])[None]
    sc = sc.masked_fill(~allowed[:, None], float("-inf"))
    p = torch.softmax(sc, dim=-1)
    p = torch.where(allowed[:, None].any(-1, keepdim=True), p, torch.zeros((), dtype=dtype))
    return torch.matmul(p, v).transpose(1, 2).reshape(B, T, H * DH)


@functools.lru_cache(maxsize=None)
def _case(B, T, H, lens, rope, chunk, left):
    g = torch.Generator().manual_seed(1000 * T + 10 * H + rope)
    qkv = torch.randn(B, T, 3 * H * DH, generator=g)
    lens = None if lens is None else list(lens)
    ref = _compose(qkv, H, lens, rope, chunk, left, torch.float64)
    err32 = float((_compose(qkv, H, lens, rope, chunk, left, torch.float32).double() - ref).abs().max())
    return qkv, ref, max(4.0 * err32, 1e-5)


def _run(nat, dev, qkv, H, lens, rope, chunk=0, left=-1):
    B, T, _ = qkv.shape
    cos = sin = None
    if rope:
        cos, sin = [t.contiguous().to(dev) for t in _tables(T, torch.float32)]
    kl = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    out, none = nat.rope_attention(qkv.to(dev), cos, sin, kl, H, 1.0 / math.sqrt(DH), False, chunk, left)
    assert none is None
    return out.cpu().double()


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("B,T,H,lens", SHAPES)
def test_attention_dh128_vs_fp64_composition(backend, B, T, H, lens, rope):
    nat, dev = backend
    qkv, ref, tol = _case(B, T, H, None if lens is None else tuple(lens), rope, 0, -1)
    err = float((_run(nat, dev, qkv, H, lens, rope) - ref).abs().max())
    print(f"dh128 {'rope' if rope else 'plain'} B={B} T={T} H={H}: err {err:.3e} bound {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("chunk,left", CHUNKS)
def test_attention_dh128_chunk_masks(backend, chunk, left, rope):
    nat, dev = backend
    B, T, H, lens = SHAPES[2]
    qkv, ref, tol = _case(B, T, H, tuple(lens), rope, chunk, left)
    out = _run(nat, dev, qkv, H, lens, rope, chunk, left)
    err = float((out - ref).abs().max())
    print(f"dh128 chunk=({chunk},{left}) {'rope' if rope else 'plain'}: err {err:.3e} bound {tol:.3e}")
    assert err <= tol
    if (chunk, left) == (16, 0):  # no allowed key -> exactly zero context
        assert not ref[:, 64:].any() and not out[:, 64:].any()


def test_attention_dh128_refusals(backend):
    """The attention-weights output is not instantiated at 128 and says so; RelPosMHAXL at 128 keeps its refusal."""
    nat, dev = backend
    qkv = torch.randn(1, 5, 3 * DH).to(dev)
    cos, sin = [t.contiguous().to(dev) for t in _tables(5, torch.float32)]
    with pytest.raises(nat.SbkError, match="head_dim 128"):
        nat.rope_attention(qkv, cos, sin, None, 1, 0.1, want_attn=True)
    pos, u = torch.randn(9, DH).to(dev), torch.zeros(DH).to(dev)
    with pytest.raises(nat.SbkError, match=r"head_dim 128 not instantiated \(8,16,32,36,64\)"):
        nat.relpos_attention(qkv, pos, u, u, None, 1, 0.1)


# ---------------------------------------------------------------------------------------------- decoder
D_MODEL, NHEAD, VOCAB, T_MEM, BEAM = 256, 2, 40, 40, 4


@functools.lru_cache(maxsize=None)
def _decoder_case(B):
    """A 2-layer decoder at d 256 / 2 heads, a 40-frame memory, utterance 1 (if any) 3 frames long; teacher-forced references in
    fp64 and the fp32 composition's error."""
    from speechbrain_amd.inference.builders import build_modules

    mods = build_modules(dict(d_model=D_MODEL, nhead=NHEAD, d_ffn=128, n_enc=1, n_dec=2, n_fft=400, win_length=25), vocab=VOCAB, seed=5)
    tr, seq = mods["Transformer"].eval(), mods["seq_lin"].eval()
    with torch.no_grad():
        seq.w.weight.mul_(4.0)
    sd = {"Transformer." + k: v.detach().clone() for k, v in tr.state_dict().items()}
    sd["seq_lin.w.weight"], sd["seq_lin.w.bias"] = seq.w.weight.detach().clone(), seq.w.bias.detach().clone()
    cfg = O.ModelCfg(d_model=D_MODEL, nhead=NHEAD, num_encoder_layers=1, num_decoder_layers=2, d_ffn=128, vocab=VOCAB)
    gen = torch.Generator().manual_seed(40 + B)
    enc = torch.randn(B, T_MEM, D_MODEL, generator=gen) * 1.5
    enc_len = torch.tensor([T_MEM, 3, 29][:B], dtype=torch.int32)
    # decoder_prefix runs one hypothesis per memory: each utterance repeated for its BEAM hypotheses
    enc_r, len_r = enc.repeat_interleave(BEAM, 0), enc_len.repeat_interleave(BEAM, 0)
    tgt = torch.randint(0, VOCAB, (B * BEAM, 6), generator=gen)
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = O.decode(tgt, enc_r.double(), len_r, sd64, cfg, "Transformer.")
    err32 = float((O.decode(tgt, enc_r, len_r, sd, cfg, "Transformer.").double() - ref).abs().max())
    wl, ratio = enc_len.float() / T_MEM, 6.5 / T_MEM
    hyps, _, scores, _ = O.beam_search(enc, wl, sd, cfg, O.SearchCfg(beam=BEAM, ctc_weight=0.0, max_decode_ratio=ratio))
    return tr, seq, enc, enc_len, enc_r, len_r, tgt, ref, max(4.0 * err32, 1e-5), wl, ratio, hyps, scores


@pytest.mark.parametrize("B", [3, 1])
def test_decoder_dh128_prefix_and_beam_search(backend, B):
    """B = 3: 12 hypothesis rows teacher-forced (self_attn_step_kernel<2>, cross_attn_step_kernel<128, .>) against the fp64 oracle,
    then the beam-4 search against the oracle's.  B = 1: a single utterance's beam -- the head-dim-64 cooperative decoder
    (csrc/decoder_persist.hip) does not take the shape, the search falls back to the plain launches."""
    nat, dev = backend
    from speechbrain_amd.decoders import S2STransformerBeamSearcher

    tr, seq, enc, enc_len, enc_r, len_r, tgt, ref, tol, wl, ratio, hyps_ref, sc_ref = _decoder_case(B)
    tr, seq = tr.to(dev), seq.to(dev)
    try:
        h = nat.DecoderHandle(tr, seq)
        out = nat.decoder_prefix(h, tgt.int().to(dev), enc_r.to(dev), len_r.to(dev)).cpu().double()
        err = float((out - ref).abs().max())
        print(f"dh128 decoder prefix B={B}: err {err:.3e} bound {tol:.3e}")
        assert err <= tol
        bs = S2STransformerBeamSearcher(modules=[tr, seq], bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=ratio,
                                        beam_size=BEAM, using_eos_threshold=False, length_normalization=True)
        nat.prof_reset()
        nat.prof_enable(True)
        try:
            hyps, _, sc, _ = bs(enc.to(dev), wl.to(dev))
        finally:
            nat.prof_enable(False)
        rep = nat.prof_report()
        assert "cross_attn_step" in rep and "self_attn_step" in rep, sorted(rep)
        assert "decoder_step_persist" not in rep and "cross_attn_ring" not in rep, sorted(rep)
        assert hyps == hyps_ref
        assert float((sc.cpu() - sc_ref).abs().max()) <= 1e-4
    finally:
        tr.cpu(), seq.cpu()
