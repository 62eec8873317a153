"""Transducer beam search with RNNLM shallow fusion (csrc/transducer.hip, speechbrain_amd/decoders/transducer.py,
speechbrain_amd/lobes/models/RNNLM.py) against fixtures the reference wrote (tools/make_transducer_lm_golden.py), on the CPU
emulator and on the MI355X (the `backend` fixture); the host restatement (tests/transducer_lm_host_ref.py) pinned to the same
fixtures and used as the yardstick at shapes beyond them; identities that hold whatever the weights are; the bound on the
expansions of a frame; and the refusals."""
import ctypes
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch

import transducer_lm_host_ref as host_ref
from test_transducer import ACTS, _close, _searcher
from test_transducer_beam import _random_case

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MIN_MARGIN = 1e-3  # as tests/test_transducer_beam.py: token identity is demanded of searches decided by this margin
_cache = {}


def _golden():
    if "golden" not in _cache:
        z = np.load(os.path.join(GOLD, "transducer_beam_lm.npz"))
        meta = json.loads(str(z["meta"]))
        cases = [{k[len(f"c{i}."):]: z[k] for k in z.files if k.startswith(f"c{i}.")} for i in range(len(meta))]
        _cache["golden"] = (meta, cases)
    return _cache["golden"]


def _lm(cfg, sd, dev, **kw):
    """The fixture's RNNLM from this package, through the import shim's name."""
    import speechbrain_amd.compat

    speechbrain_amd.compat.install()
    from speechbrain.lobes.models.RNNLM import RNNLM

    lm = RNNLM(output_neurons=cfg["lm_V"] or cfg["V"], embedding_dim=cfg["lm_E"], activation=ACTS[cfg["lm_act"]], dropout=0.0,
               rnn_layers=cfg["lm_L"], rnn_neurons=cfg["lm_H"], return_hidden=True, dnn_blocks=cfg["lm_dnn"],
               dnn_neurons=cfg["lm_D"], **kw)
    lm.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("lm.")})
    return lm.to(dev).eval()


def _lm_searcher(cfg, sd, dev, lm_weight=None, lm=None):
    s = _searcher(cfg, sd, dev, beam_size=cfg["beam"], state_beam=cfg["state_beam"], expand_beam=cfg["expand_beam"],
                  lm_module=_lm(cfg, sd, dev) if lm is None else lm, lm_weight=cfg["lm_weight"] if lm_weight is None else lm_weight)
    s.nbest = cfg["nbest"]
    return s


def _decode(native, s, tn, **kw):
    """The binding's raw results as host lists: (nbest tokens, nbest scores, status, expansions, LM steps)"""
    prep, lm = s._prepare(tn.device, beam=True), s._prepare_lm(tn.device)
    tok, ln, sc, cnt, st, ex, steps = native.transducer_beam_search(
        prep, tn, s.blank_id, s.beam_size, s.nbest, s.state_beam, s.expand_beam, act=s.tjoint.act_code, lm=lm,
        lm_weight=s.lm_weight, return_lm_steps=True, **kw)
    tok, ln, sc, cnt = tok.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
    nb = [[tok[b, k, :ln[b, k]].tolist() for k in range(cnt[b])] for b in range(len(cnt))]
    return nb, [sc[b, :cnt[b]].tolist() for b in range(len(cnt))], st.cpu().tolist(), ex.cpu().tolist(), steps.cpu().tolist()


def _host(cfg, sd, lm_weight=None):
    return host_ref.beam_search(host_ref.Network(sd, cfg["act"]), host_ref.LM(sd, cfg["lm_act"]),
                                cfg["lm_weight"] if lm_weight is None else lm_weight, sd["tn"], 0, cfg["beam"], cfg["nbest"],
                                cfg["state_beam"], cfg["expand_beam"])


# ------------------------------------------------------------------------------------------------ 1, 2: the yardstick
def test_lm_fixture_margins_make_token_identity_fair():
    meta, cases = _golden()
    names = {c["name"] for c in meta}
    assert {"w03_l1_leaky_relu", "w10_l2_relu", "dnn2_gelu", "odd_sizes_tanh", "wide_v70", "lm_vocab_larger",
            "beam10_whole_row", "padded_b3", "lm_decides"} <= names
    for case, sd in zip(meta, cases):
        assert case["path_agrees"] and case["margin"] >= MIN_MARGIN, case["name"]
        assert int(sd["expansions"].max()) < 4 * case["cfg"]["beam"], case["name"]  # under the cap of the default
        assert int(sd["expansions"].min()) >= 1
    by = {c["name"]: c for c in meta}
    assert {c["cfg"]["lm_weight"] for c in meta} >= {0.3, 1.0}
    assert {c["cfg"]["lm_act"] for c in meta} == {"leaky_relu", "relu", "gelu", "tanh"}
    assert {c["cfg"]["lm_L"] for c in meta} >= {1, 2} and {c["cfg"]["lm_dnn"] for c in meta} >= {1, 2}
    odd = by["odd_sizes_tanh"]["cfg"]
    assert odd["lm_H"] % 4 and odd["lm_D"] % 4
    assert by["wide_v70"]["cfg"]["V"] == 70 and by["lm_vocab_larger"]["cfg"]["lm_V"] > by["lm_vocab_larger"]["cfg"]["V"]
    assert by["beam10_whole_row"]["cfg"]["beam"] == by["beam10_whole_row"]["cfg"]["V"]
    decides = by["lm_decides"]
    assert decides["best_without_lm"] is not None and decides["best_without_lm"] != [n[0] for n in decides["nbest"]]


def test_lm_host_restatement_matches_reference():
    meta, cases = _golden()
    for case, sd in zip(meta, cases):
        got = _host(case["cfg"], sd)
        assert got["nbest"] == case["nbest"], case["name"]
        assert np.array_equal(got["expansions"], sd["expansions"]), case["name"]
        for x, y in zip(got["scores"], case["scores"]):
            _close(x, y, what=(case["name"], "scores"))
        _close(got["mean"], case["mean"], what=(case["name"], "mean"))
    # ... and without the LM term it is the restatement of the plain search, which finds the other hypothesis
    (case, sd), = [(c, sd) for c, sd in zip(meta, cases) if c["name"] == "lm_decides"]
    plain = _host(case["cfg"], sd, lm_weight=0.0)
    assert [n[0] for n in plain["nbest"]] == case["best_without_lm"] and int(plain["lm_steps"].sum()) == 0


# ------------------------------------------------------------------------------------------------ 3: the module
def test_rnnlm_module_matches_reference(backend):
    native, dev = backend
    meta, cases = _golden()
    for case, sd in zip(meta, cases):
        cfg = case["cfg"]
        lm = _lm(cfg, sd, dev)
        assert type(lm).__module__ == "speechbrain_amd.lobes.models.RNNLM"
        assert sorted(lm.state_dict()) == sorted(k[3:] for k in sd if k.startswith("lm.")), case["name"]
        toks = torch.from_numpy(sd["lm_tokens"]).to(dev)
        logits, (h, c) = lm(toks)
        assert logits.shape == sd["lm_logits"].shape and h.shape == (cfg["lm_L"], toks.shape[0], cfg["lm_H"])
        _close(logits.cpu().numpy(), sd["lm_logits"], what=(case["name"], "sequence"))
        hx, steps = None, []
        for t in range(toks.shape[1]):  # one token at a time with the state carried, as the search feeds it
            out, hx = lm(toks[:, t:t + 1].to(torch.int32), hx=hx)
            steps.append(out)
        _close(torch.cat(steps, dim=1).cpu().numpy(), sd["lm_logits"], what=(case["name"], "steps"))
        _close(hx[0].cpu().numpy(), h.cpu().numpy(), what=(case["name"], "h"))
        # the restatement's LM, too
        hl = host_ref.LM(sd, cfg["lm_act"])
        hh, hc = hl.zero()
        for t in range(toks.shape[1]):
            out, hh, hc = hl.logits(int(sd["lm_tokens"][0, t]), hh, hc)
            _close(out, sd["lm_logits"][0, t], what=(case["name"], "host LM", t))
    lm = _lm(meta[0]["cfg"], cases[0], dev)
    lm.return_hidden = False
    flat = lm(torch.from_numpy(cases[0]["lm_tokens"][:, 0]).to(dev))  # 1-d input: a time axis is added and squeezed again
    assert flat.shape == (2, cases[0]["lm_logits"].shape[2])
    _close(flat.cpu().numpy(), cases[0]["lm_logits"][:, 0], what="1-d input")


# ------------------------------------------------------------------------------------------------ 4: the fixture
def test_transducer_lm_kernel_matches_reference(backend):
    native, dev = backend
    meta, cases = _golden()
    for case, sd in zip(meta, cases):
        cfg = case["cfg"]
        s = _lm_searcher(cfg, sd, dev)
        tn = torch.from_numpy(sd["tn"]).to(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # (a search that reaches the cap warns)
            best, mean, nbest, scores, (status, expansions) = s.transducer_beam_search_decode(tn, return_status=True)
        assert nbest == case["nbest"], case["name"]
        assert best == [n[0] for n in case["nbest"]]
        for x, y in zip(scores, case["scores"]):
            _close(x, y, what=(case["name"], "scores"))
        _close(float(mean), case["mean"], what=(case["name"], "mean"))
        assert status == [0] * len(nbest), case["name"]
        assert expansions == sd["expansions"].sum(axis=1).tolist(), case["name"]


# ------------------------------------------------------------------------------------------------ 5: beyond the fixture
def _random_lm(seed, V, lm_V=None, E=6, H=12, L=1, n_dnn=1, D=8, act="leaky_relu", sharpen=3.0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape, k=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * k).numpy()  # noqa: E731
    lm_V = lm_V or V
    sd = {"lm.embedding.Embedding.weight": torch.randn(lm_V, E, generator=g).numpy()}
    k = 2.0 / np.sqrt(H)
    for l in range(L):
        sd[f"lm.rnn.rnn.weight_ih_l{l}"] = u(4 * H, E if l == 0 else H, k=k)
        sd[f"lm.rnn.rnn.weight_hh_l{l}"] = u(4 * H, H, k=k)
        sd[f"lm.rnn.rnn.bias_ih_l{l}"], sd[f"lm.rnn.rnn.bias_hh_l{l}"] = u(4 * H, k=k / 2), u(4 * H, k=k / 2)
    for i in range(n_dnn):
        name, K = ("" if i == 0 else f"_{i - 1}"), (H if i == 0 else D)
        sd[f"lm.dnn.linear{name}.w.weight"], sd[f"lm.dnn.linear{name}.w.bias"] = u(D, K, k=1.0 / np.sqrt(K)), u(D, k=0.5)
        sd[f"lm.dnn.norm{name}.norm.weight"], sd[f"lm.dnn.norm{name}.norm.bias"] = 1.0 + u(D, k=0.3), u(D, k=0.3)
    sd["lm.out.w.weight"], sd["lm.out.w.bias"] = u(lm_V, D, k=sharpen / np.sqrt(D)), u(lm_V, k=0.5)
    return dict(lm_V=lm_V, lm_E=E, lm_H=H, lm_L=L, lm_dnn=n_dnn, lm_D=D, lm_act=act), sd


# (the LM's term takes about lm_weight * log(V) off every non-blank candidate: the two wide-beam shapes shift the blank by 2
# and 3 instead of the default 5, so that three frames still give some hypothesis a token)
SHAPES = {"b1_t3_beam3": (dict(B=1, T=3, beam=3, V=10, L=1), dict(L=1)),
          "b5_t37_beam3_v64_lm2": (dict(B=5, T=37, beam=3, V=64, L=1, sharpen=8.0, shift=16.0), dict(L=2, H=16)),
          "b1_t3_beam16_v65_odd_lm": (dict(B=1, T=3, beam=16, V=65, L=1, shift=2.0), dict(H=15, n_dnn=2, D=13, act="tanh")),
          "b5_t3_beam16_v64_l2_lm4": (dict(B=5, T=3, beam=16, V=64, L=2, shift=3.0), dict(L=4, act="gelu", lm_V=70))}


def _draw(key):
    """As tests/test_transducer_beam.py: the first of at most 20 seeds whose search, by the host restatement, stays under
    the cap with every decision made by MIN_MARGIN; computed once per parameter set and shared by the backends."""
    if key not in _cache:
        tkw, lkw = SHAPES[key]
        for seed in range(20):
            base = 1000 * (11 + sorted(SHAPES).index(key)) + seed
            cfg, sd = _random_case(base, **tkw)
            lcfg, lsd = _random_lm(base + 500, tkw["V"], **lkw)
            cfg, sd = dict(cfg, lm_weight=0.5, **lcfg), dict(sd, **lsd)
            try:
                ref = _host(cfg, sd)
            except host_ref.ExpansionCap:
                continue
            some_tokens = any(len(h) > 0 for n in ref["nbest"] for h in n)
            if ref["margin"] >= MIN_MARGIN and int(ref["expansions"].max()) < 4 * cfg["beam"] and some_tokens:
                _cache[key] = (cfg, sd, ref)
                break
        else:
            pytest.fail(f"{key}: none of 20 seeds stays under the cap with margins above {MIN_MARGIN}")
    return _cache[key]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_transducer_lm_kernel_matches_host_restatement_beyond_the_fixture(backend, name):
    native, dev = backend
    cfg, sd, ref = _draw(name)
    s = _lm_searcher(cfg, sd, dev)
    nb, sc, status, expansions, steps = _decode(native, s, torch.from_numpy(sd["tn"]).to(dev))
    assert status == [0] * len(nb)
    assert nb == ref["nbest"]
    assert expansions == ref["expansions"].sum(axis=1).tolist()
    assert steps == ref["lm_steps"].tolist()  # a (token, state) pair expanded again reads what its first step left
    for x, y in zip(sc, ref["scores"]):
        _close(x, y, what=(name, "scores"))


# ------------------------------------------------------------------------------------------------ 6: identities
def test_transducer_lm_identities(backend):
    native, dev = backend
    meta, cases = _golden()
    (case, sd), = [(c, sd) for c, sd in zip(meta, cases) if c["name"] == "lm_vocab_larger"]
    cfg = case["cfg"]
    tn = torch.from_numpy(sd["tn"]).to(dev)
    plain = _searcher(cfg, sd, dev, beam_size=cfg["beam"], state_beam=cfg["state_beam"], expand_beam=cfg["expand_beam"])
    plain.nbest = cfg["nbest"]
    _, _, p_nbest, p_scores = plain(tn)
    # lm_weight = 0: the LM is never touched -- the same tokens and the same score bits
    _, _, nbest, scores = _lm_searcher(cfg, sd, dev, lm_weight=0.0)(tn)
    assert nbest == p_nbest and scores == p_scores
    # a uniform LM (out weights and bias zero) takes lm_weight * log(V_lm) off the score per emitted token, whatever it is.
    # The tokens are the plain search's only where that constant per token flips none of the search's decisions (it weighs
    # on every comparison of hypotheses of unequal lengths), so the inputs are drawn: the first of at most 20 seeds for
    # which the host restatement -- not the kernel -- takes the same path with and without the uniform LM, every decision of
    # both made by MIN_MARGIN.  lm_weight 0.05: 0.05 * log(12) = 0.12 per token, four orders above _close's tolerance.
    if "uniform" not in _cache:
        for seed in range(20):
            cfg2, sd2 = _random_case(31000 + seed, B=2, T=12, beam=4, V=10, L=1)
            lcfg, lsd = _random_lm(31500 + seed, 10, lm_V=12)
            lsd["lm.out.w.weight"], lsd["lm.out.w.bias"] = np.zeros_like(lsd["lm.out.w.weight"]), np.zeros_like(lsd["lm.out.w.bias"])
            cfg2, sd2 = dict(cfg2, lm_weight=0.05, **lcfg), dict(sd2, **lsd)
            try:
                h_plain, h_uni = _host(cfg2, sd2, lm_weight=0.0), _host(cfg2, sd2)
            except host_ref.ExpansionCap:
                continue
            if (h_uni["nbest"] == h_plain["nbest"] and min(h_uni["margin"], h_plain["margin"]) >= MIN_MARGIN
                    and any(len(h) > 1 for n in h_uni["nbest"] for h in n)):
                _cache["uniform"] = (cfg2, sd2)
                break
        else:
            pytest.fail("none of 20 seeds keeps its path under a uniform LM with margins above MIN_MARGIN")
    cfg2, sd2 = _cache["uniform"]
    tn2 = torch.from_numpy(sd2["tn"]).to(dev)
    plain2 = _searcher(cfg2, sd2, dev, beam_size=cfg2["beam"], state_beam=cfg2["state_beam"], expand_beam=cfg2["expand_beam"])
    plain2.nbest = cfg2["nbest"]
    _, _, p_nbest, p_scores = plain2(tn2)
    _, _, nbest, scores = _lm_searcher(cfg2, sd2, dev)(tn2)
    assert nbest == p_nbest
    for b in range(len(nbest)):
        for k, hyp in enumerate(nbest[b]):
            n = len(hyp) + 1
            _close(scores[b][k], p_scores[b][k] - cfg2["lm_weight"] * math.log(cfg2["lm_V"]) * (n - 1) / n, what=("uniform", b, k))
    # the same call twice: the same bits
    s = _lm_searcher(cfg, sd, dev)
    first, second = s(tn), s(tn)
    assert first[2] == second[2] and first[3] == second[3] and first[2] == case["nbest"]
    # the layouts are kept until a parameter changes
    prep = s._prepare_lm(dev)
    assert s._prepare_lm(dev) is prep
    with torch.no_grad():
        s.lm.out.w.bias.add_(0.25)
    assert s._prepare_lm(dev) is not prep


# ------------------------------------------------------------------------------------------------ 7: the cap
def test_transducer_lm_expansion_cap_ends_the_search(backend):
    """As test_transducer_beam_expansion_cap_ends_the_search, with the LM: blank pushed out of every top-k, and NaN frames.
    Both inputs are bounded by construction; the tokens are unspecified."""
    native, dev = backend
    meta, cases = _golden()
    case, sd = meta[0], dict(cases[0])
    cfg = dict(case["cfg"], beam=4, nbest=5)
    sd["transducer_lin.w.bias"] = sd["transducer_lin.w.bias"].copy()
    sd["transducer_lin.w.bias"][0] -= 200.0
    s = _lm_searcher(cfg, sd, dev)
    tn = torch.from_numpy(sd["tn"][:, :8].copy()).to(dev)
    T = tn.shape[1]
    nb, sc, status, expansions, steps = _decode(native, s, tn, max_expansions=8)
    assert all(st & native.TBEAM_CAPPED for st in status)
    assert expansions == [8 * T] * len(nb) and all(1 <= n <= 8 * T for n in steps)
    assert all(1 <= len(n) <= 5 and all(len(h) <= 8 * T for h in n) for n in nb)
    nb, sc, status, _, _ = _decode(native, s, tn, max_expansions=8, max_tokens=5)
    assert all(st & native.TBEAM_CAPPED and st & native.TBEAM_TRUNCATED for st in status)
    assert all(len(h) <= 5 for n in nb for h in n)
    with pytest.warns(UserWarning, match=r"utterances \[0, 1, 2\] reached the bound"):
        best, _, nbest, _ = s.transducer_beam_search_decode(tn, max_expansions=8)
    assert len(best) == tn.shape[0]
    # NaN frames
    s = _lm_searcher(cfg, dict(cases[0]), dev)
    bad = torch.from_numpy(cases[0]["tn"][:, :12].copy())
    bad[0, 3:9] = float("nan")
    bad[1, :, 2] = float("nan")
    nb, sc, status, expansions, _ = _decode(native, s, bad.to(dev), max_expansions=8)
    assert len(nb) == bad.shape[0] and all(len(n) >= 1 and all(len(h) <= 8 * 12 for h in n) for n in nb)
    assert all(e <= 8 * 12 for e in expansions) and status[2] == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (it may warn; it returns)
        best, _, _, _ = s.transducer_beam_search_decode(bad.to(dev), max_expansions=8)
    assert len(best) == bad.shape[0]
    empty = s.transducer_beam_search_decode(torch.zeros(0, 4, tn.shape[2], device=dev))
    assert empty[0] == [] and empty[2] == [] and empty[3] == []


# ------------------------------------------------------------------------------------------------ 8, 9: the refusals
def test_transducer_lm_bad_arguments_are_reported(backend):
    native, dev = backend
    lib = native.load()
    meta, cases = _golden()
    case, sd = meta[0], cases[0]
    s = _lm_searcher(case["cfg"], sd, dev)
    prep, lm = s._prepare(dev, beam=True), s._prepare_lm(dev)
    B, T, J, V = 2, 5, case["cfg"]["J"], case["cfg"]["V"]
    tn = torch.zeros(B, T, J, device=dev)
    cfg = native.TransducerBeamConfig(blank=0, beam_size=4, nbest=3, state_beam=2.3, expand_beam=2.3, max_expansions=16,
                                      max_tokens=T * 16, act=native.ACT_GELU)
    nbytes = lib.sbk_transducer_beam_lm_workspace_bytes(ctypes.byref(prep.W), ctypes.byref(lm.M), ctypes.byref(cfg), B, T)
    assert nbytes > lib.sbk_transducer_beam_workspace_bytes(ctypes.byref(prep.W), ctypes.byref(cfg), B, T) > 0
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 16
    tok = torch.zeros(B, 3, T * 16, dtype=torch.int32, device=dev)
    ln, cnt, st = (torch.zeros(B, 3, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                   torch.zeros(B, dtype=torch.int32, device=dev))
    sc = torch.zeros(B, 3, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def changed(**kw):
        M = native.RNNLMWeights()
        ctypes.memmove(ctypes.byref(M), ctypes.byref(lm.M), ctypes.sizeof(M))
        for k, v in kw.items():
            setattr(M, k, v)
        return ctypes.byref(M)

    def call(M=ctypes.byref(lm.M), w=0.5, ws_bytes=nbytes, B=B, tn_p=p(tn)):
        return lib.sbk_transducer_beam_search_lm_f32(ctypes.byref(prep.W), M, ctypes.c_float(w), ctypes.byref(cfg), tn_p,
                                                     ctypes.c_void_p(wp), ws_bytes, p(tok), p(ln), p(sc), p(cnt), p(st), B, T,
                                                     None)

    assert call() == 0
    assert call(M=None) == -22 and b"NULL" in lib.sbk_last_error()
    for w in (0.0, -0.5, float("nan"), float("inf")):
        assert call(w=w) == -22 and b"lm_weight" in lib.sbk_last_error(), w
    assert call(M=changed(vocab=V - 1)) == -22 and b"vocab" in lib.sbk_last_error()
    for n in (0, 5):
        assert call(M=changed(n_layers=n)) == -22 and b"LSTM layers" in lib.sbk_last_error(), n
    for n in (0, 3):
        assert call(M=changed(n_dnn=n)) == -22 and b"n_dnn" in lib.sbk_last_error(), n
    assert call(ws_bytes=nbytes - 1) == -22 and b"workspace" in lib.sbk_last_error()
    # (refused from the sizes alone, before any weight is read)
    assert call(M=changed(hidden=20000)) == -22 and b"LDS" in lib.sbk_last_error()
    assert lib.sbk_transducer_beam_lm_workspace_bytes(ctypes.byref(prep.W), changed(hidden=20000), ctypes.byref(cfg), B, T) == 0
    assert b"LDS" in lib.sbk_last_error()
    assert call(tn_p=None) == -22 and b"NULL" in lib.sbk_last_error()
    assert call(tn_p=None, B=0) == 0  # empty batch
    # the binding passes lm_weight on: the entry is the one place that refuses it
    with pytest.raises(native.SbkError, match="lm_weight"):
        native.transducer_beam_search(prep, tn, 0, 4, 3, lm=lm, lm_weight=0.0)


def test_transducer_lm_python_refusals(backend):
    from speechbrain_amd.lobes.models.RNNLM import RNNLM
    from speechbrain_amd.nnet.RNN import GRU

    native, dev = backend
    meta, cases = _golden()
    case, sd = meta[0], cases[0]
    cfg = case["cfg"]
    tn = torch.from_numpy(sd["tn"]).to(dev)
    with pytest.raises(NotImplementedError, match="transducer beam search.*LM fusion.*Linear"):
        _lm_searcher(cfg, sd, dev, lm=torch.nn.Linear(2, 2))(tn)
    with pytest.raises(NotImplementedError, match="GRU"):
        RNNLM(output_neurons=10, rnn_class=GRU)
    with pytest.raises(NotImplementedError, match="LM fusion.*3 DNN blocks"):
        _lm_searcher(cfg, sd, dev, lm=RNNLM(output_neurons=10, embedding_dim=4, rnn_neurons=8, dnn_blocks=3, dnn_neurons=8))(tn)
    with pytest.raises(NotImplementedError, match="LM fusion.*Sigmoid"):
        _lm_searcher(cfg, sd, dev, lm=RNNLM(output_neurons=10, embedding_dim=4, rnn_neurons=8, dnn_neurons=8,
                                            activation=torch.nn.Sigmoid))(tn)
    small = RNNLM(output_neurons=cfg["V"] - 1, embedding_dim=4, rnn_neurons=8, dnn_neurons=8).to(dev)
    with pytest.raises(ValueError, match="fewer than"):
        _lm_searcher(cfg, sd, dev, lm=small)(tn)
    greedy = _searcher(cfg, sd, dev, lm_module=_lm(cfg, sd, dev), lm_weight=0.5)
    with pytest.raises(NotImplementedError, match="LM fusion"):
        greedy(tn)
