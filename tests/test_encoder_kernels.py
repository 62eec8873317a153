"""The encoder's attention kernels (csrc/relpos_attn.hip) and GLU + depthwise convolution (csrc/convmodule.hip) against plain
fp64 compositions of the same operation (tests/encoder_host_ref.py), at tile and chunk edges.

Every kernel test runs on the CPU emulator of the kernel sources and, marked gpu, on the MI355X.  References are computed once
per case, shared by both backends and never modified; all inputs come from seeded generators.

Bound (the rule of test_csgu.py and test_attention_dh128.py): the fp32 torch composition's own max error against fp64 on the same
inputs, times 4 (another, equally legitimate, summation order), with a floor of 1e-5.  Attention weights: 1e-5 absolute against
the fp64 probabilities.  bf16 attention: twice the error of encoder_host_ref.attention_bf16_model (the kernel's roundings in
fp64 arithmetic) against the fp64 composition, plus 1e-3.  Every case prints `ratio` = kernel error / reference-model error.

Largest ratio over all cases on the MI355X (the emulator's in brackets), for the next rewrite to see how much room it has; the
cases whose fp32 composition is exact (a query that sees one key) have no ratio and stay below 2.4e-7 absolute:
  fp32 flash  2.29 (2.68)   relpos Dh 64, T 70, no chunks: 1.2e-6 against a bound of 1e-5 -- the floor sets every fp32 bound here
  fp32 strip  2.98 (2.98)   the same case, 1.6e-6; weights within 3.7e-7 of the fp64 probabilities (bound 1e-5)
  bf16        1.05 (1.05)   rope T 64, chunk (40, 0); the bound allows 2: the matrix core's accumulation order costs nothing visible
  glu_dwconv  1.36 (1.36)   T 32, d 65, kernel size 31, chunk 4: 7.6e-7; the largest error is 1.3e-6"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

import encoder_host_ref as R

KINDS = ["relpos", "rope", "plain"]
HEAD_DIMS = [8, 16, 32, 36, 64]
# (B, T, H, lens): one query, one key / one row short of a 32-query tile, a one-key utterance / exactly one tile / one row into the
# second tile / exactly one 64-row ring of the flash kernels / one row past it, a key length one past a key tile / a key length on
# the 64 edge with queries beyond it / one row past the 128 queries of a flash workgroup / two workgroups, ragged, one key
SHAPES = [(1, 1, 1, None), (2, 31, 2, (31, 1)), (2, 32, 1, (32, 17)), (2, 33, 2, (33, 5)), (1, 64, 1, (64,)), (1, 65, 2, (33,)),
          (1, 70, 1, (64,)), (1, 129, 1, (128,)), (3, 130, 2, (130, 97, 1))]
# (chunk, left): no mask / no left context: the first key tile of later query tiles is skipped, and at T = 70 with key length 64
# the queries 64 .. 69 have no allowed key / unlimited left / one left chunk / a chunk that divides no tile / a chunk wider than a
# key tile / a query sees only itself / ... and three keys before it
CHUNKS = [(0, -1), (16, 0), (8, -1), (16, 1), (5, 2), (40, 0), (1, 0), (1, 3)]
_sid = lambda s: f"B{s[0]}T{s[1]}H{s[2]}"  # noqa: E731
_cid = lambda c: f"c{c[0]}l{c[1]}"  # noqa: E731


def _seed(*key):
    return zlib.crc32(repr(key).encode())


@functools.lru_cache(maxsize=None)
def _tables(T, Dh):
    from speechbrain_amd.nnet.attention import PrecomputedRoPESinusoids

    tab = PrecomputedRoPESinusoids(max(T, 2), Dh, torch.float32, "cpu")
    return tab.cosines.contiguous(), tab.sines.contiguous()


@functools.lru_cache(maxsize=None)
def _inputs(kind, Dh, B, T, H):
    """qkv = randn; relpos: the projected position rows = randn [2T-1, d] and u, v = 0.3 randn, handed straight to the kernel
    (no projection GEMM: a failure names the attention kernel)."""
    g = torch.Generator().manual_seed(_seed(kind, Dh, B, T, H))
    d = H * Dh
    kw = {"qkv": torch.randn(B, T, 3 * d, generator=g)}
    if kind == "relpos":
        kw.update(pos=torch.randn(2 * T - 1, d, generator=g), bias_u=0.3 * torch.randn(d, generator=g),
                  bias_v=0.3 * torch.randn(d, generator=g))
    elif kind == "rope":
        kw["rope"] = _tables(T, Dh)
    return kw


def _compose(kind, Dh, B, T, H, lens, chunk, left, dtype, **over):
    kw = dict(_inputs(kind, Dh, B, T, H))
    return R.attention(kw.pop("qkv"), H, Dh, lens, chunk, left, Dh ** -0.5, dtype, **kw, **over)


@functools.lru_cache(maxsize=None)
def _case(kind, Dh, B, T, H, lens, chunk, left):
    """(fp64 context, fp64 probabilities, the fp32 composition's error on the context, [B,T] queries with an allowed key)"""
    ref, probs = _compose(kind, Dh, B, T, H, lens, chunk, left, torch.float64)
    err32 = float((_compose(kind, Dh, B, T, H, lens, chunk, left, torch.float32)[0].double() - ref).abs().max())
    return ref, probs, err32, R.allowed_keys(B, T, lens, chunk, left).any(-1)


def _run(nat, dev, kind, Dh, B, T, H, lens, chunk, left, want_attn, out=None):
    kw = _inputs(kind, Dh, B, T, H)
    qkv = kw["qkv"].to(dev)
    kl = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    if kind == "relpos":
        ctx, attn = nat.relpos_attention(qkv, kw["pos"].to(dev), kw["bias_u"].to(dev), kw["bias_v"].to(dev), kl, H, Dh ** -0.5,
                                         want_attn, chunk, left, out=out)
    else:
        cos, sin = [t.to(dev) for t in kw["rope"]] if kind == "rope" else (None, None)
        ctx, attn = nat.rope_attention(qkv, cos, sin, kl, H, Dh ** -0.5, want_attn, chunk, left, out=out)
    assert torch.equal(qkv.cpu(), kw["qkv"])  # the caller's rows are read, never written
    assert (attn is not None) == want_attn
    return ctx.cpu().double(), None if attn is None else attn.cpu().double()


def _ratio(err, model_err):
    return err / model_err if model_err > 0.0 else (0.0 if err == 0.0 else float("inf"))


def _check(group, label, case, ctx, attn):
    ref, probs, err32, seen = case
    err, tol = float((ctx - ref).abs().max()), max(4.0 * err32, 1e-5)
    print(f"[{group}] {label}: err {err:.3e} fp32-composition {err32:.3e} bound {tol:.3e} ratio {_ratio(err, err32):.3f}")
    assert err <= tol
    if attn is not None:
        perr = float((attn - probs).abs().max())
        print(f"[{group}] {label}: weights err {perr:.3e}")
        assert perr <= 1e-5
    if not bool(seen.all()):  # a query without an allowed key: exactly zero context and weights, in reference and kernel
        assert not ref[~seen].any() and not ctx[~seen].any()
        none = ~seen[:, None, :].expand(probs.shape[:3])
        assert not probs[none].any()
        assert attn is None or not attn[none].any()


# ------------------------------------------------------------------------------ 1. attention against the fp64 composition
@pytest.mark.parametrize("chunk,left", CHUNKS, ids=[_cid(c) for c in CHUNKS])
@pytest.mark.parametrize("B,T,H,lens", SHAPES, ids=[_sid(s) for s in SHAPES])
@pytest.mark.parametrize("Dh", HEAD_DIMS)
@pytest.mark.parametrize("kind,want_attn", [(k, w) for k in KINDS for w in (False, True) if (k, w) != ("plain", True)],
                         ids=lambda v: {False: "flash", True: "strip"}.get(v, v))
def test_attention_vs_fp64_composition(backend, kind, want_attn, Dh, B, T, H, lens, chunk, left):
    """want_attn False: relpos_flash_t_kernel / rope_flash_t_kernel; True: relpos_attn_kernel (the score strip in LDS), which also
    returns the weights.  Plain attention has no weights output."""
    nat, dev = backend
    ctx, attn = _run(nat, dev, kind, Dh, B, T, H, lens, chunk, left, want_attn)
    _check("fp32 strip" if want_attn else "fp32 flash", f"{kind} Dh={Dh} {_sid((B, T, H))} {_cid((chunk, left))}",
           _case(kind, Dh, B, T, H, lens, chunk, left), ctx, attn)


def test_the_unseen_query_cases_exist():
    """The shape list holds what its comments say: rows without an allowed key at (T 70, key length 64, chunk 16, no left)."""
    seen = R.allowed_keys(1, 70, (64,), 16, 0).any(-1)
    assert bool(seen[0, :64].all()) and not bool(seen[0, 64:].any())
    assert sum(not bool(R.allowed_keys(B, T, lens, c, left).any(-1).all()) for B, T, _, lens in SHAPES for c, left in CHUNKS) >= 8


def test_plain_attention_refuses_the_weights_output(backend):
    nat, dev = backend
    out = torch.full((1, 5, 16), float("nan")).to(dev)
    with pytest.raises(nat.SbkError, match="does not return attention weights"):
        nat.rope_attention(torch.zeros(1, 5, 48).to(dev), None, None, None, 1, 0.25, want_attn=True, out=out)
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------ 2. the reference can tell (CPU only)
def test_reference_detects_index_bias_and_mask_changes():
    """relpos at (Dh 32, T 65, chunk 16, left 1) in fp64: each single change of the reference's indexing moves the context by more
    than 1e3 x the bound the kernels are held to -- a kernel with that change could not pass."""
    kind, Dh, B, T, H, lens, chunk, left = "relpos", 32, 2, 65, 2, (65, 33), 16, 1
    ref, _, err32, _ = _case(kind, Dh, B, T, H, lens, chunk, left)
    tol = max(4.0 * err32, 1e-5)
    kw = _inputs(kind, Dh, B, T, H)
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    klen = torch.tensor(lens)[:, None, None]
    c = i // chunk
    edge = ((j >= ((c - left) * chunk).clamp(min=0)) & (j < (c + 1) * chunk + 1))[None] & (j[None] < klen)
    changes = {
        "mirrored position index": dict(index=(T - 1) + i - j),
        "position index shifted by one row": dict(index=(R.rel_index(T) + 1).clamp(max=2 * T - 2)),
        "bias_u and bias_v swapped": dict(bias_u=kw["bias_v"], bias_v=kw["bias_u"]),
        "chunk's right edge one key further": dict(allowed=edge),
        "no left limit": dict(allowed=R.allowed_keys(B, T, lens, chunk, -1)),
    }
    # (the hand-made mask is the module's but for the edge)
    assert torch.equal(R.allowed_keys(B, T, lens, chunk, left), edge & (j < (c + 1) * chunk)[None])
    for name, over in changes.items():
        args = {k: v for k, v in kw.items() if k != "qkv"}
        args.update(over)
        moved = float((R.attention(kw["qkv"], H, Dh, lens, chunk, left, Dh ** -0.5, torch.float64, **args)[0] - ref).abs().max())
        print(f"{name}: context moves by {moved:.3e} = {moved / tol:.0f} x the bound {tol:.3e}")
        assert moved > 1e3 * tol, name


# ------------------------------------------------------------------------------ 3. strip kernel: 8 waves, the LDS cap
def _strip_lds_bytes(Dh, T):
    """launch_attn / launch_attn_pf of csrc/relpos_attn.hip: two 32 x (Dh + 1) query tiles, (waves - column tiles) partial
    contexts of 32 x 33, the 32 x SP score strip; 8 waves once the 4-wave layout passes 80 KiB."""
    sp, nc = (T + 31) // 32 * 32 + 1, (Dh + 31) // 32
    waves = 8 if (2 * 32 * (Dh + 1) + 3 * 32 * 33 + 32 * sp) * 4 > 80 * 1024 else 4
    return (2 * 32 * (Dh + 1) + (waves - nc) * 32 * 33 + 32 * sp) * 4, waves


def _largest_strip_T(Dh):
    T = 1
    while _strip_lds_bytes(Dh, T + 1)[0] <= 160 * 1024:
        T += 1
    return T


STRIP = [("relpos", 64, 450, (450, 413), 0, -1), ("rope", 64, 450, (450, 413), 0, -1), ("relpos", 64, 417, (417, 1), 64, 1),
         ("rope", 64, 417, (417, 1), 64, 1), ("relpos", 8, 600, (600, 3), 0, -1), ("rope", 36, 500, (500, 3), 0, -1)]


@pytest.mark.parametrize("kind,Dh,T,lens,chunk,left", STRIP, ids=[f"{s[0]}-Dh{s[1]}-T{s[2]}" for s in STRIP])
def test_strip_kernel_eight_waves(backend, kind, Dh, T, lens, chunk, left):
    """relpos_attn_kernel<., ., ., 8> (and the RoPE prefetch variant): LDS strips above 80 KiB."""
    nat, dev = backend
    nbytes, waves = _strip_lds_bytes(Dh, T)
    assert 80 * 1024 < nbytes <= 160 * 1024 and waves == 8
    ctx, attn = _run(nat, dev, kind, Dh, 2, T, 1, lens, chunk, left, True)
    _check("fp32 strip", f"{kind} Dh={Dh} T={T} {_cid((chunk, left))}", _case(kind, Dh, 2, T, 1, lens, chunk, left), ctx, attn)


@pytest.mark.parametrize("kind,Dh", [("relpos", 64), ("rope", 64), ("relpos", 8), ("rope", 36)])
def test_strip_kernel_at_the_lds_cap(backend, kind, Dh):
    """The largest T whose strip fits the 160 KiB opt-in is computed right; one frame more is refused before any launch."""
    nat, dev = backend
    T = _largest_strip_T(Dh)
    assert T % 32 == 0 and _strip_lds_bytes(Dh, T)[0] <= 160 * 1024 < _strip_lds_bytes(Dh, T + 1)[0]
    if Dh in (8, 64):
        assert T == {8: 1024, 64: 928}[Dh]
    ctx, attn = _run(nat, dev, kind, Dh, 1, T, 1, (T - 3,), 0, -1, True)
    _check("fp32 strip", f"{kind} Dh={Dh} T={T} (cap)", _case(kind, Dh, 1, T, 1, (T - 3,), 0, -1), ctx, attn)
    out = torch.full((1, T + 1, Dh), float("nan")).to(dev)
    with pytest.raises(nat.SbkError, match="of LDS"):
        _run(nat, dev, kind, Dh, 1, T + 1, 1, (T - 2,), 0, -1, True, out=out)
    assert bool(torch.isnan(out).all())  # a refusal launches nothing


# ------------------------------------------------------------------------------ 4. the expf instantiation
@pytest.mark.parametrize("Dh,T,lens", [(36, 65, (65, 33)), (64, 130, (130, 33))])
def test_relpos_flash_expf_variant(backend, Dh, T, lens):
    """attn_exp2 = 0: relpos_flash_t_kernel<DH, false> (libm expf in place of 2^x on v_exp_f32)."""
    nat, dev = backend
    with nat.knobs(attn_exp2=0):
        ctx, _ = _run(nat, dev, "relpos", Dh, 2, T, 2, lens, 16, 1, False)
    _check("fp32 flash", f"relpos expf Dh={Dh} T={T} c16l1", _case("relpos", Dh, 2, T, 2, lens, 16, 1), ctx, None)


# ------------------------------------------------------------------------------ 5. destination discipline
@pytest.mark.parametrize("want_attn", [False, True], ids=["flash", "strip"])
@pytest.mark.parametrize("kind,Dh,B,T,H,lens", [("relpos", 16, 3, 130, 2, (130, 97, 1)), ("rope", 36, 2, 33, 2, (33, 5))])
def test_attention_writes_only_its_destination(backend, kind, Dh, B, T, H, lens, want_attn):
    """out = a slice of a NaN-filled buffer: the context lands there, nothing around it is touched (and _run checks that the
    caller's qkv is bit-identical after the call)."""
    nat, dev = backend
    d = H * Dh
    big = torch.full((B * T + 9, d), float("nan")).to(dev)
    out = big[4: 4 + B * T].view(B, T, d)
    ctx, attn = _run(nat, dev, kind, Dh, B, T, H, lens, 0, -1, want_attn, out=out)
    assert torch.equal(ctx, out.cpu().double())
    _check("fp32 strip" if want_attn else "fp32 flash", f"{kind} Dh={Dh} T={T} out=slice", _case(kind, Dh, B, T, H, lens, 0, -1),
           ctx, attn)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())


# ------------------------------------------------------------------------------ 6. bf16 attention (head dim 64)
@functools.lru_cache(maxsize=None)
def _bf16_model_err(kind, B, T, H, lens, chunk, left):
    kw = _inputs(kind, 64, B, T, H)
    model = R.attention_bf16_model(kw["qkv"], H, 64, lens, chunk, left, 0.125, rope=kw.get("rope"))
    return float((model - _case(kind, 64, B, T, H, lens, chunk, left)[0]).abs().max())


@pytest.mark.parametrize("chunk,left", CHUNKS, ids=[_cid(c) for c in CHUNKS])
@pytest.mark.parametrize("B,T,H,lens", SHAPES, ids=[_sid(s) for s in SHAPES])
@pytest.mark.parametrize("kind", ["rope", "plain"])
def test_attention_bf16_vs_fp64_composition(backend, kind, B, T, H, lens, chunk, left):
    """rope_flash_t_bf16_kernel under precision_scope("bf16") against the fp64 composition; the bound comes from the fp64 model of
    the kernel's roundings (factor 2: the matrix core's own accumulation order)."""
    nat, dev = backend
    ref, _, _, seen = _case(kind, 64, B, T, H, lens, chunk, left)
    model_err = _bf16_model_err(kind, B, T, H, lens, chunk, left)
    with nat.precision_scope("bf16"):
        ctx, _ = _run(nat, dev, kind, 64, B, T, H, lens, chunk, left, False)
    err, tol = float((ctx - ref).abs().max()), 2.0 * model_err + 1e-3
    print(f"[bf16] {kind} {_sid((B, T, H))} {_cid((chunk, left))}: err {err:.3e} model {model_err:.3e} bound {tol:.3e} "
          f"ratio {_ratio(err, model_err):.3f}")
    assert not bool(torch.isnan(ctx).any())
    assert err <= tol
    assert not ctx[~seen].any()


def test_attention_bf16_output_is_the_fp32_output_rounded(backend):
    """out_dtype = torch.bfloat16 at a chunked, ragged shape: bit for bit the fp32-output result rounded to bf16."""
    nat, dev = backend
    B, T, H, lens, chunk, left = 3, 130, 2, (130, 97, 1), 16, 1
    kw = _inputs("rope", 64, B, T, H)
    qkv, (cos, sin) = kw["qkv"].to(dev), [t.to(dev) for t in kw["rope"]]
    kl = torch.tensor(lens, dtype=torch.int32).to(dev)
    with nat.precision_scope("bf16"):
        c32, _ = nat.rope_attention(qkv, cos, sin, kl, H, 0.125, False, chunk, left)
    cb, none = nat.rope_attention(qkv, cos, sin, kl, H, 0.125, False, chunk, left, out_dtype=torch.bfloat16)
    assert none is None and cb.dtype == torch.bfloat16 and torch.equal(cb.cpu(), c32.cpu().bfloat16())


# ------------------------------------------------------------------------------ 7. glu_dwconv against its fp64 composition
KSIZES = [3, 5, 7, 15, 31]
CONV_CHUNKS = [0, 1, 4, 16, 33]
# (B, T, d): T below every halo / ... / one full frame tile, one channel in a second channel tile / ... / ... / T below the halo of
# 15 and 31, four channel tiles with a ragged last one
CONV_SHAPES = [(1, 1, 8), (2, 31, 64), (1, 32, 65), (2, 33, 70), (1, 65, 144), (1, 7, 200)]


@functools.lru_cache(maxsize=None)
def _conv_inputs(B, T, d, ks):
    g = torch.Generator().manual_seed(_seed("glu_dwconv", B, T, d, ks))
    return torch.randn(B, T, 2 * d, generator=g), 0.2 * torch.randn(d, ks, generator=g), torch.randn(d, generator=g)


@functools.lru_cache(maxsize=None)
def _conv_case(B, T, d, ks, chunk):
    h, w, b = _conv_inputs(B, T, d, ks)
    ref = R.glu_dwconv(h, w, b, ks, chunk, torch.float64)
    return ref, float((R.glu_dwconv(h, w, b, ks, chunk, torch.float32).double() - ref).abs().max())


def _conv_check(label, case, y):
    ref, err32 = case
    err, tol = float((y.cpu().double() - ref).abs().max()), max(4.0 * err32, 1e-5)
    print(f"[glu_dwconv] {label}: err {err:.3e} fp32-composition {err32:.3e} bound {tol:.3e} ratio {_ratio(err, err32):.3f}")
    assert err <= tol


def test_glu_dwconv_reference_is_conv1d_without_chunks():
    for B, T, d in CONV_SHAPES:
        for ks in KSIZES:
            h, w, b = [t.double() for t in _conv_inputs(B, T, d, ks)]
            want = F.conv1d(F.glu(h.transpose(1, 2), dim=1), w.unsqueeze(1), b, padding=(ks - 1) // 2, groups=d).transpose(1, 2)
            assert float((R.glu_dwconv(h, w, b, ks, 0, torch.float64) - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("chunk", CONV_CHUNKS)
@pytest.mark.parametrize("ks", KSIZES)
@pytest.mark.parametrize("B,T,d", CONV_SHAPES)
def test_glu_dwconv_vs_fp64_composition(backend, B, T, d, ks, chunk):
    nat, dev = backend
    h, w, b = _conv_inputs(B, T, d, ks)
    hd = h.to(dev)
    y = nat.glu_dwconv(hd, w.to(dev), b.to(dev), ks, chunk)
    assert torch.equal(hd.cpu(), h)
    _conv_check(f"B={B} T={T} d={d} ks={ks} chunk={chunk}", _conv_case(B, T, d, ks, chunk), y)


def test_glu_dwconv_writes_only_its_destination(backend):
    nat, dev = backend
    B, T, d, ks, chunk = 2, 33, 70, 15, 16
    h, w, b = _conv_inputs(B, T, d, ks)
    big = torch.full((B * T + 9, d), float("nan")).to(dev)
    out = big[4: 4 + B * T].view(B, T, d)
    y = nat.glu_dwconv(h.to(dev), w.to(dev), b.to(dev), ks, chunk, out=out)
    assert y.data_ptr() == out.data_ptr()
    _conv_check(f"B={B} T={T} d={d} ks={ks} chunk={chunk} out=slice", _conv_case(B, T, d, ks, chunk), out)
    assert bool(torch.isnan(big[:4]).all()) and bool(torch.isnan(big[4 + B * T:]).all())


def test_glu_dwconv_does_not_mask_frames_past_a_length(backend):
    """The kernel takes no lengths: frames past an utterance's nominal length are convolved like any other (the module masks its
    output).  Two utterances that agree up to frame 20 and differ after it agree on the outputs whose taps end before 20 and
    differ beyond."""
    nat, dev = backend
    B, T, d, ks, n = 2, 33, 70, 7, 20
    h, w, b = _conv_inputs(B, T, d, ks)
    h = h.clone()
    h[1, :n] = h[0, :n]
    y = nat.glu_dwconv(h.to(dev), w.to(dev), b.to(dev), ks).cpu()
    halo = (ks - 1) // 2
    assert torch.equal(y[0, :n - halo], y[1, :n - halo])
    assert bool((y[0, n - halo:] != y[1, n - halo:]).any(-1).all())  # every later frame, the halo before the length included
    ref = R.glu_dwconv(h, w, b, ks, 0, torch.float64)
    assert float((y.double() - ref).abs().max()) <= max(4.0 * float((R.glu_dwconv(h, w, b, ks, 0, torch.float32) - ref).abs().max()), 1e-5)
