"""csrc/attn_rnn.hip -- sbk_attn_rnn_attend_f32, sbk_attn_rnn_attn_init_f32, sbk_gru_cell_f32 and the decode step strung from them
(sbk_attn_rnn_decode_f32) -- against the host restatement (tests/attn_rnn_host_ref.py) in double, on the CPU emulator of the
kernel sources (not gpu) and on the MI355X (-m gpu).

Bound (the project's rule, tests/test_rnn_kernels.py): max(4 x the error of the fp32 host restatement against its fp64 run on the
same inputs, 1e-5), for every output."""
import pytest
import torch

import attn_rnn_host_ref as R
from speechbrain_amd import native

# (T, A, E, C, k, scaling, n, rows): T 1, 2: below a tile; 63 / 64 / 65: around the 32-frame tiles and the 64-lane waves; 300: ten
# tiles, more than one 256-thread pass of the softmax.  A 8 / 24: below a wave, 130: past two.  E 5: one partial column block, 64:
# one whole.  k 100: 2k+1 > T for every T but 300.  n 33: more rows than utterances can share.  "rep": row_utt repeats utterances
# and leaves utterance 1 without a row.  The last case has A == E (what the planted mistake "ctx_from_enc_h" needs).
ATTEND_CASES = [
    (1, 8, 5, 0, 0, 1.0, 1, "id"), (1, 24, 64, 10, 100, 2.0, 3, "rep"), (2, 130, 5, 1, 1, 1.0, 3, "id"),
    (2, 8, 64, 10, 3, 2.0, 33, "rep"), (63, 24, 5, 10, 100, 1.0, 3, "id"), (63, 130, 64, 0, 0, 2.0, 1, "rep"),
    (64, 8, 64, 10, 3, 1.0, 3, "rep"), (64, 130, 5, 1, 1, 2.0, 33, "id"), (65, 24, 64, 10, 100, 2.0, 3, "rep"),
    (65, 8, 5, 0, 0, 1.0, 33, "id"), (300, 130, 64, 10, 100, 1.0, 3, "rep"), (300, 24, 5, 10, 3, 2.0, 1, "id"),
    (300, 8, 64, 1, 1, 1.0, 33, "rep"), (300, 24, 24, 10, 3, 2.0, 3, "id"),
]
CHAIN = (65, 24, 5, 10, 3, 2.0, 3, "rep")  # 40 steps, prev_attn handed from step to step
CHAIN_STEPS = 40
GRU_CASES = [(H, n, bias, mode) for H in (1, 8, 130) for n in (1, 33) for bias in (True, False) for mode in ("h", "null", "alias")]
DECODER = dict(inp=6, H=8, A=24, E=5, C=10, k=3, layers=2, B=3, T=37, L=6, scaling=2.0)  # a two-layer decoder, teacher forced
_CACHE = {}


def _ids(case):
    return "-".join(str(x) for x in case)


def _attend_case(case, steps=1):
    """Inputs of an attend case, the fp64 results of every step and the fp32 restatement's error: computed once, never modified."""
    key = (case, steps)
    if key not in _CACHE:
        T, A, E, C, k, scaling, n, rows = case
        gen = torch.Generator().manual_seed(hash((T, A, E, C, k, n, rows == "id", steps)) % (2 ** 31))
        rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        B = n if rows == "id" else 4
        row_utt = None if rows == "id" else torch.tensor([[0, 0, 2, 3][r % 4] for r in range(n)], dtype=torch.int32)
        enc_len = torch.tensor([[T, max(T - 1, 1), 1][b % 3] for b in range(B)], dtype=torch.int32)
        x = dict(enc=rn(B, T, E), enc_h=rn(B, T, A), enc_len=enc_len, v=rn(A) * (3.0 / A ** 0.5), row_utt=row_utt,
                 dec_h=[rn(n, A) for _ in range(steps)], prev=None, conv_w=None, loc_w=None, loc_b=None)
        if C:  # a peaked prev_attn that is nonzero on every frame, taps and mlp_loc of a size that makes the location term order 1
            x.update(prev=torch.softmax(3.0 * rn(n, T), dim=-1), conv_w=rn(C, 2 * k + 1) * 4.0, loc_w=rn(A, C) / C ** 0.5,
                     loc_b=rn(A) * 0.5)
        ref = {dt: _attend_host(x, scaling, dt) for dt in (torch.float32, torch.float64)}
        err = [(R.bound(a32, a64), R.bound(c32, c64)) for (a32, c32), (a64, c64) in zip(ref[torch.float32], ref[torch.float64])]
        _CACHE[key] = (x, ref[torch.float64], err)
    return _CACHE[key]


def _attend_host(x, scaling, dt, mistakes=()):
    """[(attn, ctx)] of every step on the host; prev_attn is handed on as the decoder does."""
    c = lambda t: None if t is None else t.to(dt)  # noqa: E731
    prev = c(x["prev"])
    out = []
    for dec_h in x["dec_h"]:
        attn, ctx = R.attend(c(x["enc"]), c(x["enc_h"]), x["enc_len"], c(dec_h), c(x["v"]), prev, c(x["conv_w"]), c(x["loc_w"]),
                             c(x["loc_b"]), scaling, x["row_utt"], mistakes)
        out.append((attn, ctx))
        if x["conv_w"] is not None and "prev_not_updated" not in mistakes:
            prev = attn
    return out


def _attend_kernel(nat, dev, x, scaling):
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    prev, out = d(x["prev"]), []
    for dec_h in x["dec_h"]:
        attn, ctx = nat.attn_rnn_attend(d(x["enc"]), d(x["enc_h"]), d(x["enc_len"]), d(dec_h), d(x["v"]), prev, d(x["conv_w"]),
                                        d(x["loc_w"]), d(x["loc_b"]), scaling, d(x["row_utt"]))
        out.append((attn, ctx))
        if x["conv_w"] is not None:
            prev = attn
    return out


def _check_attend(what, x, got, ref, err):
    lens = x["enc_len"] if x["row_utt"] is None else x["enc_len"][x["row_utt"].long()]
    T = x["enc"].shape[1]
    past = torch.arange(T)[None, :] >= lens[:, None]
    for s, ((attn, ctx), (attn64, ctx64), (ba, bc)) in enumerate(zip(got, ref, err)):
        attn, ctx = attn.cpu(), ctx.cpu()
        ea, ec = float((attn.double() - attn64).abs().max()), float((ctx.double() - ctx64).abs().max())
        dsum = float((attn.double().sum(-1) - 1.0).abs().max())
        if s in (0, len(got) - 1):
            print(f"attend {what} step {s}: attn max|d| {ea:.3e} (bound {ba:.1e}), ctx {ec:.3e} (bound {bc:.1e}), |sum-1| {dsum:.1e}")
        assert attn.shape == attn64.shape and ctx.shape == ctx64.shape
        assert ea <= ba and ec <= bc, (what, s, ea, ba, ec, bc)
        assert dsum <= 1e-6
        assert bool((attn[past] == 0).all())


@pytest.mark.parametrize("case", ATTEND_CASES, ids=_ids)
def test_attend_vs_fp64(backend, case):
    nat, dev = backend
    x, ref, err = _attend_case(case)
    _check_attend(_ids(case), x, _attend_kernel(nat, dev, x, case[5]), ref, err)


def test_attend_40_chained_steps(backend):
    """prev_attn of step s is the attention of step s - 1, from the first one on."""
    nat, dev = backend
    x, ref, err = _attend_case(CHAIN, CHAIN_STEPS)
    _check_attend("chain", x, _attend_kernel(nat, dev, x, CHAIN[5]), ref, err)


@pytest.mark.parametrize("T,rows", [(1, "id"), (65, "rep"), (300, "id"), (300, "rep")])
def test_attn_init(backend, T, rows):
    nat, dev = backend
    x, _, _ = _attend_case((T, 8, 5, 0, 0, 1.0, 5, rows))
    got = nat.attn_rnn_attn_init(x["enc_len"].to(dev), T, None if x["row_utt"] is None else x["row_utt"].to(dev)).cpu()
    want = R.attn_init(x["enc_len"], T, torch.float64, x["row_utt"])
    assert got.shape == want.shape
    assert float((got.double() - want).abs().max()) <= 1e-7  # (one fp32 division)
    assert bool((got[want == 0] == 0).all())


def _gru_case(H, n, bias, mode):
    key = ("gru", H, n, bias, mode)
    if key not in _CACHE:
        gen = torch.Generator().manual_seed(H * 1009 + n * 7 + bias + 3 * len(mode))
        rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        x = dict(gi=rn(n, 3 * H), gh=rn(n, 3 * H), b_ih=rn(3 * H) * 0.5 if bias else None, b_hh=rn(3 * H) * 0.5 if bias else None,
                 h=None if mode == "null" else rn(n, H))
        c = lambda t, dt: None if t is None else t.to(dt)  # noqa: E731
        r32, r64 = (R.gru_cell(c(x["gi"], dt), c(x["gh"], dt), c(x["b_ih"], dt), c(x["b_hh"], dt), c(x["h"], dt))
                    for dt in (torch.float32, torch.float64))
        _CACHE[key] = (x, r64, R.bound(r32, r64))
    return _CACHE[key]


@pytest.mark.parametrize("H,n,bias,mode", GRU_CASES)
def test_gru_cell_vs_fp64(backend, H, n, bias, mode):
    nat, dev = backend
    x, ref, bound = _gru_case(H, n, bias, mode)
    d = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    h = d(x["h"]).clone() if x["h"] is not None else None
    got = nat.gru_cell(d(x["gi"]), d(x["gh"]), d(x["b_ih"]), d(x["b_hh"]), h, out=h if mode == "alias" else None)
    if mode == "alias":
        assert got.data_ptr() == h.data_ptr()
    err = float((got.cpu().double() - ref).abs().max())
    print(f"gru_cell H={H} n={n} bias={bias} {mode}: max|d| {err:.3e} (bound {bound:.1e})")
    assert got.shape == ref.shape and err <= bound


def _decoder_case():
    """A small two-layer location-aware decoder with random weights, teacher forced: the fp64 records and the fp32 error."""
    if "decoder" not in _CACHE:
        c = DECODER
        gen = torch.Generator().manual_seed(29)
        rn = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
        H, A, E = c["H"], c["A"], c["E"]
        sd = {"proj.weight": rn(H, A + H) / (A + H) ** 0.5, "proj.bias": rn(H) * 0.3,
              "attn.mlp_enc.weight": rn(A, E) / E ** 0.5, "attn.mlp_enc.bias": rn(A) * 0.3,
              "attn.mlp_dec.weight": rn(A, H) / H ** 0.5, "attn.mlp_dec.bias": rn(A) * 0.3,
              "attn.mlp_attn.weight": rn(1, A) * (3.0 / A ** 0.5),
              "attn.conv_loc.weight": rn(c["C"], 1, 2 * c["k"] + 1) * 4.0,
              "attn.mlp_loc.weight": rn(A, c["C"]) / c["C"] ** 0.5, "attn.mlp_loc.bias": rn(A) * 0.5,
              "attn.mlp_out.weight": rn(A, E) / E ** 0.5, "attn.mlp_out.bias": rn(A) * 0.3}
        for l in range(c["layers"]):
            k_in = c["inp"] + A if l == 0 else H
            sd.update({f"rnn.rnn_cells.{l}.weight_ih": rn(3 * H, k_in) * (1.5 / k_in ** 0.5),
                       f"rnn.rnn_cells.{l}.weight_hh": rn(3 * H, H) * (1.5 / H ** 0.5),
                       f"rnn.rnn_cells.{l}.bias_ih": rn(3 * H) * 0.5, f"rnn.rnn_cells.{l}.bias_hh": rn(3 * H) * 0.5})
        enc, inp = rn(c["B"], c["T"], E), rn(c["B"], c["L"], c["inp"])
        enc_len = torch.tensor([c["T"], c["T"] // 3, 1], dtype=torch.int32)  # (a third: 1 / enc_len is far from 1 / T)
        r32 = R.HostDecoder(sd, c["scaling"], torch.float32).forward(inp, enc, enc_len)
        r64 = R.HostDecoder(sd, c["scaling"], torch.float64).forward(inp, enc, enc_len)
        _CACHE["decoder"] = (sd, enc, inp, enc_len, r64, [R.bound(a, b) for a, b in zip(r32, r64)])
    return _CACHE["decoder"]


def prepared_from(nat, sd, dev, scaling, emb=None, fc_w=None, fc_b=None):
    """native.AttnRNNPrepared of a decoder state dict under the reference's keys."""
    d = lambda t: None if t is None else t.detach().float().to(dev).contiguous()  # noqa: E731
    n_layers = len([k for k in sd if k.endswith("weight_ih")])
    layers = [tuple(d(sd.get(f"rnn.rnn_cells.{l}.{n}")) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
              for l in range(n_layers)]
    attn = dict(enc_w=d(sd["attn.mlp_enc.weight"]), enc_b=d(sd["attn.mlp_enc.bias"]), dec_w=d(sd["attn.mlp_dec.weight"]),
                dec_b=d(sd["attn.mlp_dec.bias"]), attn_v=d(sd["attn.mlp_attn.weight"].reshape(-1)),
                out_w=d(sd["attn.mlp_out.weight"]), out_b=d(sd["attn.mlp_out.bias"]))
    if "attn.conv_loc.weight" in sd:
        w = sd["attn.conv_loc.weight"]
        attn.update(conv_w=d(w.reshape(w.shape[0], w.shape[-1])), loc_w=d(sd["attn.mlp_loc.weight"]), loc_b=d(sd["attn.mlp_loc.bias"]))
    return nat.AttnRNNPrepared(layers, attn, d(sd["proj.weight"]), d(sd["proj.bias"]), scaling, emb=d(emb), fc_w=d(fc_w), fc_b=d(fc_b))


def test_decoder_steps_vs_fp64(backend):
    """sbk_attn_rnn_decode_f32: two GRU layers, the attention, mlp_out and proj over six teacher-forced steps; outputs, the attention
    of every step, and the final hs and c."""
    nat, dev = backend
    sd, enc, inp, enc_len, ref, bounds = _decoder_case()
    got = nat.attn_rnn_decode(prepared_from(nat, sd, dev, DECODER["scaling"]), inp.to(dev), enc.to(dev), enc_len.to(dev))
    for name, g, r, b in zip(("outputs", "attn", "hs", "c"), got, ref, bounds):
        err = float((g.cpu().double() - r).abs().max())
        print(f"decode {name}: max|d| {err:.3e} (bound {b:.1e})")
        assert g.shape == r.shape and err <= b, name


def test_same_bits_twice_and_on_two_streams(backend):
    nat, dev = backend
    x, _, _ = _attend_case(CHAIN, CHAIN_STEPS)
    few = dict(x, dec_h=x["dec_h"][:3])
    sd, enc, inp, enc_len, _, _ = _decoder_case()

    def run():
        out = [t for pair in _attend_kernel(nat, dev, few, CHAIN[5]) for t in pair]
        return out + list(nat.attn_rnn_decode(prepared_from(nat, sd, dev, DECODER["scaling"]), inp.to(dev), enc.to(dev), enc_len.to(dev)))

    a, b = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    if dev.type == "cuda":
        for _ in range(2):
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                o = run()
            s.synchronize()
            assert all(torch.equal(p, q) for p, q in zip(a, o))


def test_bad_arguments_are_named(backend):
    nat, dev = backend
    lib = nat.load()
    z = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731

    def attend(n=2, B=2, T=3, A=4, E=4, C=2, k=1, lens=(3, 2), rows=None, alias=False):
        a, e, c, kk, t = (max(v, 1) for v in (A, E, C, k, T))
        a, e, t = min(a, 8), min(e, 8), min(t, 8)  # (refused before anything is read: small buffers do)
        enc, enc_h, dec_h, prev = z(B, t, e), z(B, t, a), z(n, a), z(n, t)
        enc_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        row_utt = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev)
        attn, ctx = prev if alias else z(n, t), z(n, e)
        nbytes = 4 * (n * t + 4)
        ws, conv_w, loc_w, loc_b, v = z(n * t + 4), z(c, 2 * kk + 1), z(a, c), z(a), z(a)
        r = lib.sbk_attn_rnn_attend_f32(nat._p(enc), nat._p(enc_h), nat._p(enc_len), nat._p(row_utt), nat._p(dec_h), nat._p(prev),
                                        nat._p(conv_w), nat._p(loc_w), nat._p(loc_b), nat._p(v), 1.0, nat._p(attn),
                                        nat._p(ctx), nat._p(ws), nbytes, n, B, T, A, E, C, k, nat._stream(enc))
        return r, lib.sbk_last_error().decode()

    assert attend()[0] == 0
    assert attend(n=3, rows=(1, 0, 1))[0] == 0
    for kw, name in ((dict(A=2049), "A=2049"), (dict(E=2049), "E=2049"), (dict(T=4097), "T=4097"), (dict(C=33), "C=33"),
                     (dict(k=129), "k=129"), (dict(T=0), "T=0"), (dict(A=0), "A=0"), (dict(n=0), "n=0"), (dict(n=3), "row_utt"),
                     (dict(lens=(0, 2)), "enc_len"), (dict(lens=(3, 4)), "enc_len"), (dict(n=3, rows=(0, 2, 1)), "row_utt"),
                     (dict(n=3, rows=(0, -1, 1)), "row_utt"), (dict(alias=True), "alias")):
        r, msg = attend(**kw)
        assert r == -22 and name in msg, (kw, r, msg)

    def gru(n=2, H=4, b_hh=True, null_out=False):
        h = min(max(H, 1), 8)
        gi, gh, bi, bh, out = z(max(n, 1), 3 * h), z(max(n, 1), 3 * h), z(3 * h), z(3 * h), z(max(n, 1), h)
        r = lib.sbk_gru_cell_f32(nat._p(gi), nat._p(gh), nat._p(bi), nat._p(bh) if b_hh else None, None,
                                 None if null_out else nat._p(out), n, H, nat._stream(gi))
        return r, lib.sbk_last_error().decode()

    assert gru()[0] == 0
    for kw, name in ((dict(H=2049), "H=2049"), (dict(H=0), "H=0"), (dict(n=0), "n=0"), (dict(b_hh=False), "b_hh"),
                     (dict(null_out=True), "h_out")):
        r, msg = gru(**kw)
        assert r == -22 and name in msg, (kw, r, msg)
    with pytest.raises(nat.SbkError, match="prev_attn"):
        nat.attn_rnn_attend(z(2, 3, 4), z(2, 3, 4), torch.ones(2, dtype=torch.int32, device=dev), z(2, 4), z(4), None, z(2, 3), z(4, 2), z(4))
    with pytest.raises(nat.SbkError, match="b_hh"):
        nat.gru_cell(z(2, 12), z(2, 12), z(12), None)
    # the whole-search entries refuse a length outside [1, T] too
    sd, enc, inp, _, _, _ = _decoder_case()
    with pytest.raises(nat.SbkError, match="enc_len"):
        nat.attn_rnn_decode(prepared_from(nat, sd, dev, 1.0), inp.to(dev), enc.to(dev),
                            torch.tensor([DECODER["T"] + 1, 1, 1], dtype=torch.int32, device=dev))


@pytest.mark.gpu
def test_recipe_width_on_the_gpu():
    """The recipe's widths: A 1024, E 512, C 10, k 100, T 250, two rows, three chained steps; the GRU cell at H 1024."""
    native.load()
    dev = torch.device("cuda:0")
    case = (250, 1024, 512, 10, 100, 1.0, 2, "id")
    x, ref, err = _attend_case(case, 3)
    _check_attend("recipe width", x, _attend_kernel(native, dev, x, 1.0), ref, err)
    x, ref, bound = _gru_case(1024, 2, True, "h")
    got = native.gru_cell(*(None if t is None else t.to(dev) for t in (x["gi"], x["gh"], x["b_ih"], x["b_hh"], x["h"])))
    assert float((got.cpu().double() - ref).abs().max()) <= bound


# ------------------------------------------------------------------ planted mistakes (CPU only, on the host restatement)
def _moved_attend(mistake):
    worst = 0.0
    for case, steps in [(c, 1) for c in ATTEND_CASES] + [(CHAIN, CHAIN_STEPS)]:
        if mistake == "ctx_from_enc_h" and case[1] != case[2]:
            continue
        x, ref, err = _attend_case(case, steps)
        moved = _attend_host(x, case[5], torch.float64, (mistake,))
        for (a, c), (a64, c64), (ba, bc) in zip(moved, ref, err):
            worst = max(worst, float((a - a64).abs().max()) / ba, float((c - c64).abs().max()) / bc)
    return worst


def _moved_gru(mistake):
    worst = 0.0
    for case in GRU_CASES:
        x, ref, bound = _gru_case(*case)
        c = lambda t: None if t is None else t.double()  # noqa: E731
        moved = R.gru_cell(c(x["gi"]), c(x["gh"]), c(x["b_ih"]), c(x["b_hh"]), c(x["h"]), (mistake,))
        worst = max(worst, float((moved - ref).abs().max()) / bound)
    return worst


def _moved_decoder(mistake):
    sd, enc, inp, enc_len, ref, bounds = _decoder_case()
    moved = R.HostDecoder(sd, DECODER["scaling"], torch.float64, (mistake,)).forward(inp, enc, enc_len)
    return max(float((m - r).abs().max()) / b for m, r, b in zip(moved, ref, bounds))


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_cases_tell_mistakes_apart(mistake):
    """Each planted mistake moves at least one committed case of this file by 1e3 x that case's bound or more."""
    assert max(float((a - b).abs().max()) for a, b in zip(
        _attend_host(_attend_case(CHAIN, CHAIN_STEPS)[0], CHAIN[5], torch.float64)[-1], _attend_case(CHAIN, CHAIN_STEPS)[1][-1])) == 0.0
    if mistake in ("gate_order_zrn", "b_hn_outside"):
        worst = max(_moved_gru(mistake), _moved_decoder(mistake))
    elif mistake in ("cell_input_c_emb", "dec_out_cell_c"):
        worst = _moved_decoder(mistake)
    else:
        worst = max(_moved_attend(mistake), _moved_decoder(mistake) if mistake != "ctx_from_enc_h" else 0.0)
    print(f"planted mistake '{mistake}': moves a committed case by {worst:.3e} x its bound")
    assert worst >= 1e3
