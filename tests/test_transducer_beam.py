"""Transducer beam search (csrc/transducer.hip, speechbrain_amd/decoders/transducer.py) against fixtures the reference wrote
(tools/make_transducer_beam_golden.py), on the CPU emulator and on the MI355X (the `backend` fixture); the host restatement
(tests/transducer_beam_host_ref.py) pinned to the same fixtures and used as the yardstick at shapes beyond them; the bound on
the expansions of a frame; and the refusals."""
import ctypes
import json
import os
import warnings

import numpy as np
import pytest
import torch

import transducer_beam_host_ref as host_ref
import transducer_host_ref
from test_transducer import _close, _searcher

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MIN_MARGIN = 1e-3  # token identity is demanded of searches whose every decision has this margin (fp32 noise is ~1e-6)
_cache = {}


def _golden():
    if "golden" not in _cache:
        z = np.load(os.path.join(GOLD, "transducer_beam.npz"))
        meta = json.loads(str(z["meta"]))
        cases = [{k[len(f"c{i}."):]: z[k] for k in z.files if k.startswith(f"c{i}.")} for i in range(len(meta))]
        _cache["golden"] = (meta, cases)
    return _cache["golden"]


def _beam_searcher(cfg, sd, dev, **kw):
    s = _searcher(cfg, sd, dev, beam_size=cfg["beam"], state_beam=cfg["state_beam"], expand_beam=cfg["expand_beam"], **kw)
    s.nbest = cfg["nbest"]
    return s


def _decode(native, s, tn, **kw):
    """The binding's raw results as host lists: (nbest tokens, nbest scores, status, expansions)"""
    prep = s._prepare(tn.device)
    tok, ln, sc, cnt, st, ex = native.transducer_beam_search(prep, tn, s.blank_id, s.beam_size, s.nbest, s.state_beam,
                                                             s.expand_beam, act=s.tjoint.act_code, **kw)
    tok, ln, sc, cnt = tok.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy()
    nb = [[tok[b, k, :ln[b, k]].tolist() for k in range(cnt[b])] for b in range(len(cnt))]
    return nb, [sc[b, :cnt[b]].tolist() for b in range(len(cnt))], st.cpu().tolist(), ex.cpu().tolist()


def test_beam_fixture_margins_make_token_identity_fair():
    meta, cases = _golden()
    names = {c["name"] for c in meta}
    assert {"beam2_gelu", "beam10_whole_row_tanh", "wide_v70", "odd_sizes", "one_frame", "blank_dominated",
            "blank_near_zero", "padded_b3", "tight_beams", "loose_beams", "dense_l2_nobias"} <= names
    for case, sd in zip(meta, cases):
        assert case["path_agrees"] and case["margin"] >= MIN_MARGIN, case["name"]
        assert int(sd["expansions"].max()) < 4 * case["cfg"]["beam"], case["name"]  # under the cap of the default
        assert int(sd["expansions"].min()) >= 1
    by = {c["name"]: (c, sd) for c, sd in zip(meta, cases)}
    assert by["blank_near_zero"][1]["expansions"].mean() > 2 * by["blank_dominated"][1]["expansions"].mean()
    assert any(len(n) < by["padded_b3"][0]["cfg"]["nbest"] for c in meta for n in c["nbest"])  # nbest > len(B) occurs


def test_beam_host_restatement_matches_reference():
    meta, cases = _golden()
    for case, sd in zip(meta, cases):
        cfg = case["cfg"]
        got = host_ref.beam_search(transducer_host_ref.Network(sd, cfg["act"]), sd["tn"], 0, cfg["beam"], cfg["nbest"],
                                   cfg["state_beam"], cfg["expand_beam"])
        assert got["nbest"] == case["nbest"], case["name"]
        assert np.array_equal(got["expansions"], sd["expansions"]), case["name"]
        for x, y in zip(got["scores"], case["scores"]):
            _close(x, y, what=(case["name"], "scores"))
        _close(got["mean"], case["mean"], what=(case["name"], "mean"))


def test_transducer_beam_kernel_matches_reference(backend):
    native, dev = backend
    meta, cases = _golden()
    for case, sd in zip(meta, cases):
        cfg = case["cfg"]
        s = _beam_searcher(cfg, sd, dev)
        tn = torch.from_numpy(sd["tn"]).to(dev)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # (a search that reaches the cap warns)
            best, mean, nbest, scores, (status, expansions) = s.transducer_beam_search_decode(tn, return_status=True)
        assert nbest == case["nbest"], case["name"]
        assert best == [n[0] for n in case["nbest"]]
        assert all(isinstance(x, float) for row in scores for x in row) and isinstance(mean, torch.Tensor)
        for x, y in zip(scores, case["scores"]):
            _close(x, y, what=(case["name"], "scores"))
        _close(float(mean), case["mean"], what=(case["name"], "mean"))
        assert status == [0] * len(nbest), case["name"]
        assert expansions == sd["expansions"].sum(axis=1).tolist(), case["name"]


def test_transducer_beam_agrees_with_greedy_on_blank_dominated_input(backend):
    """Where the blank dominates, the best hypothesis is greedy's (same searcher object, beam_size switched).  The beam's
    score also counts the blank's log-probability at every frame, which greedy's does not: the un-normalised score equals
    greedy's plus the blanks' along that path (from the host restatement's joint), to the tolerance of the scores."""
    native, dev = backend
    meta, cases = _golden()
    (case, sd), = [(c, sd) for c, sd in zip(meta, cases) if c["name"] == "blank_dominated"]
    cfg = case["cfg"]
    s = _beam_searcher(cfg, sd, dev)
    tn = torch.from_numpy(sd["tn"]).to(dev)
    best, _, nbest, scores = s(tn)
    s.beam_size, s.searcher = 1, s.transducer_greedy_decode
    greedy, _, _, _ = s(tn)
    assert best == greedy
    B, T, J = tn.shape
    st = [torch.empty(B, J, device=dev), torch.empty(cfg["L"], B, cfg["H"], device=dev),
          torch.empty(cfg["L"], B, cfg["H"], device=dev)]
    _, _, gscore = native.transducer_greedy(s._prepare(dev), tn, st[0], st[1], st[2], 0, 5, act=s.tjoint.act_code)
    net = transducer_host_ref.Network(sd, cfg["act"])
    for b in range(B):  # the blanks along greedy's path
        out, h, c = net.pn_step(0, np.zeros((cfg["L"], cfg["H"]), np.float32), np.zeros((cfg["L"], cfg["H"]), np.float32))
        blanks = 0.0
        for t in range(T):
            while True:
                lp = net.joint(sd["tn"][b, t], out)
                k = int(np.argmax(lp))
                if k == 0:
                    blanks += float(lp[0])
                    break
                out, h, c = net.pn_step(k, h, c)
        _close(scores[b][0] * (len(best[b]) + 1), float(gscore[b]) + blanks, what=("un-normalised score", b))


def _random_case(seed, B, T, beam, V, L, J=12, H=16, act="gelu", sharpen=3.0, shift=5.0):
    """Random weights by the reference's state_dict names (one-hot embedding), the classifier sharpened and the blank row
    shifted as the fixture's are."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *shape, k=1.0: ((torch.rand(*shape, generator=g) * 2 - 1) * k).numpy()  # noqa: E731
    sd = {"emb.Embedding.weight": torch.cat([torch.zeros(1, V - 1), torch.eye(V - 1)]).numpy()}
    k = 2.0 / np.sqrt(H)
    for l in range(L):
        sd[f"dec.rnn.weight_ih_l{l}"] = u(4 * H, V - 1 if l == 0 else H, k=k)
        sd[f"dec.rnn.weight_hh_l{l}"] = u(4 * H, H, k=k)
        sd[f"dec.rnn.bias_ih_l{l}"], sd[f"dec.rnn.bias_hh_l{l}"] = u(4 * H, k=k / 2), u(4 * H, k=k / 2)
    sd["proj_dec.w.weight"], sd["proj_dec.w.bias"] = u(J, H, k=k / 2), u(J, k=k / 2)
    sd["transducer_lin.w.weight"] = u(V, J, k=sharpen / np.sqrt(J))
    bias = u(V, k=1.0 / np.sqrt(J))
    bias[0] += shift
    sd["transducer_lin.w.bias"] = bias
    sd["tn"] = torch.randn(B, T, J, generator=g).numpy()
    cfg = dict(V=V, emb=None, H=H, L=L, J=J, proj_bias=True, cls_bias=True, act=act, beam=beam, nbest=5, state_beam=2.3,
               expand_beam=2.3)
    return cfg, sd


def _draw(key, **kw):
    """The first of at most 20 seeds whose search, by the host restatement, stays under the cap with every decision made by
    MIN_MARGIN; computed once per parameter set and shared by the backends."""
    if key not in _cache:
        for seed in range(20):
            cfg, sd = _random_case(1000 * (1 + sorted(SHAPES).index(key)) + seed, **kw)
            try:
                ref = host_ref.beam_search(transducer_host_ref.Network(sd, cfg["act"]), sd["tn"], 0, cfg["beam"], cfg["nbest"],
                                           cfg["state_beam"], cfg["expand_beam"])
            except host_ref.ExpansionCap:
                continue
            some_tokens = any(len(h) > 0 for n in ref["nbest"] for h in n)  # (an all-blank search tests little)
            if ref["margin"] >= MIN_MARGIN and int(ref["expansions"].max()) < 4 * cfg["beam"] and some_tokens:
                _cache[key] = (cfg, sd, ref)
                break
        else:
            pytest.fail(f"{key}: none of 20 seeds stays under the cap with margins above {MIN_MARGIN}")
    return _cache[key]


SHAPES = {"b1_t3_beam3": dict(B=1, T=3, beam=3, V=10, L=1),
          "b5_t37_beam3_v64": dict(B=5, T=37, beam=3, V=64, L=1, sharpen=8.0, shift=16.0),
          "b1_t3_beam16_v65": dict(B=1, T=3, beam=16, V=65, L=1),
          "b5_t3_beam16_v64_l2": dict(B=5, T=3, beam=16, V=64, L=2),
          "b1_t37_beam3_v65_l4": dict(B=1, T=37, beam=3, V=65, L=4, act="tanh", sharpen=6.0, shift=12.0)}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_transducer_beam_kernel_matches_host_restatement_beyond_the_fixture(backend, name):
    native, dev = backend
    cfg, sd, ref = _draw(name, **SHAPES[name])
    s = _beam_searcher(cfg, sd, dev)
    nb, sc, status, expansions = _decode(native, s, torch.from_numpy(sd["tn"]).to(dev))
    assert status == [0] * len(nb)
    assert nb == ref["nbest"]
    assert expansions == ref["expansions"].sum(axis=1).tolist()
    for x, y in zip(sc, ref["scores"]):
        _close(x, y, what=(name, "scores"))


def test_transducer_beam_expansion_cap_ends_the_search(backend):
    """Blank pushed out of every top-k (the reference would never leave the first frame), and NaN frames: the search ends at
    max_expansions per frame, says so in the status word and in a warning, and stays within max_tokens.  Both inputs are
    bounded by construction; the tokens are unspecified."""
    native, dev = backend
    meta, cases = _golden()
    case, sd = meta[0], dict(cases[0])
    cfg = dict(case["cfg"], beam=4, nbest=5)
    sd["transducer_lin.w.bias"] = sd["transducer_lin.w.bias"].copy()
    sd["transducer_lin.w.bias"][0] -= 200.0
    s = _beam_searcher(cfg, sd, dev)
    tn = torch.from_numpy(sd["tn"][:, :8].copy()).to(dev)
    T = tn.shape[1]
    nb, sc, status, expansions = _decode(native, s, tn, max_expansions=8)
    assert all(st & native.TBEAM_CAPPED for st in status)
    assert expansions == [8 * T] * len(nb)
    assert all(1 <= len(n) <= 5 and all(len(h) <= 8 * T for h in n) for n in nb)
    nb, sc, status, _ = _decode(native, s, tn, max_expansions=8, max_tokens=5)
    assert all(st & native.TBEAM_CAPPED and st & native.TBEAM_TRUNCATED for st in status)
    assert all(len(h) <= 5 for n in nb for h in n)
    with pytest.warns(UserWarning, match=r"utterances \[0, 1, 2\] reached the bound"):
        best, _, nbest, _ = s.transducer_beam_search_decode(tn, max_expansions=8)
    assert len(best) == tn.shape[0]
    # NaN frames
    s = _beam_searcher(cfg, dict(cases[0]), dev)
    bad = torch.from_numpy(cases[0]["tn"][:, :12].copy())
    bad[0, 3:9] = float("nan")
    bad[1, :, 2] = float("nan")
    nb, sc, status, expansions = _decode(native, s, bad.to(dev), max_expansions=8)
    assert len(nb) == bad.shape[0] and all(len(n) >= 1 and all(len(h) <= 8 * 12 for h in n) for n in nb)
    assert all(e <= 8 * 12 for e in expansions) and status[2] == 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (it may warn; it returns)
        best, _, _, _ = s.transducer_beam_search_decode(bad.to(dev), max_expansions=8)
    assert len(best) == bad.shape[0]
    empty = s.transducer_beam_search_decode(torch.zeros(0, 4, tn.shape[2], device=dev))
    assert empty[0] == [] and empty[2] == [] and empty[3] == []


def test_transducer_beam_bad_arguments_are_reported(backend):
    native, dev = backend
    lib = native.load()
    meta, cases = _golden()
    case, sd = meta[0], cases[0]
    s = _beam_searcher(case["cfg"], sd, dev)
    prep = s._prepare(dev)
    B, T, J, V = 2, 5, case["cfg"]["J"], case["cfg"]["V"]
    tn = torch.zeros(B, T, J, device=dev)
    good = dict(blank=0, beam_size=4, nbest=3, state_beam=2.3, expand_beam=2.3, max_expansions=16, max_tokens=T * 16,
                act=native.ACT_GELU)
    nbytes = lib.sbk_transducer_beam_workspace_bytes(ctypes.byref(prep.W), ctypes.byref(native.TransducerBeamConfig(**good)), B, T)
    assert nbytes > 0
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 16
    tok = torch.zeros(B, 3, T * 16, dtype=torch.int32, device=dev)
    ln, cnt, st = (torch.zeros(B, 3, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                   torch.zeros(B, dtype=torch.int32, device=dev))
    sc = torch.zeros(B, 3, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(cfg, W=prep.W, tn_p=p(tn), ws_p=ctypes.c_void_p(wp), ws_bytes=nbytes, tok_p=p(tok), B=B):
        return lib.sbk_transducer_beam_search_f32(ctypes.byref(W), ctypes.byref(native.TransducerBeamConfig(**cfg)), tn_p, ws_p,
                                                  ws_bytes, tok_p, p(ln), p(sc), p(cnt), p(st), B, T, None)

    assert call(good) == 0
    for bad, word in ((dict(beam_size=1), b"beam_size 1 < 2"), (dict(beam_size=V + 1), b"above the vocabulary"),
                      (dict(beam_size=native.TRANSDUCER_MAX_BEAM + 1), b"above the maximum"), (dict(nbest=0), b"nbest"),
                      (dict(blank=V), b"blank"), (dict(act=1), b"activation"), (dict(max_expansions=0), b"max_expansions"),
                      (dict(max_tokens=0), b"max_tokens"), (dict(max_expansions=100000), b"LDS")):
        assert call(dict(good, **bad)) == -22 and word in lib.sbk_last_error(), bad
    assert call(good, tn_p=None) == -22 and b"NULL" in lib.sbk_last_error()
    assert call(good, ws_p=None) == -22 and b"NULL" in lib.sbk_last_error()
    assert call(good, tok_p=None) == -22 and b"NULL" in lib.sbk_last_error()
    assert call(good, ws_bytes=nbytes - 1) == -22 and b"workspace" in lib.sbk_last_error()
    assert call(good, tn_p=None, B=0) == 0  # empty batch
    assert lib.sbk_transducer_beam_search_f32(None, None, None, None, 0, None, None, None, None, None, 1, 1, None) == -22
    assert native.TRANSDUCER_MAX_BEAM >= 16
    # the Python mirror
    with pytest.raises(ValueError, match="beam_size=11"):
        _beam_searcher(dict(case["cfg"], beam=V + 1), sd, dev)(tn)
    wide = dict(case["cfg"], beam=native.TRANSDUCER_MAX_BEAM + 1)
    with pytest.raises(NotImplementedError, match=f"beam_size={native.TRANSDUCER_MAX_BEAM + 1}"):
        _beam_searcher(wide, sd, dev)(tn)
    with pytest.raises(NotImplementedError, match="transducer beam search"):
        _beam_searcher(case["cfg"], sd, dev, lm_module=torch.nn.Linear(2, 2), lm_weight=0.5)(tn)


def test_transducer_beam_searcher_call_decodes(backend):
    """Before beam search was built, calling a searcher with beam_size 4 raised NotImplementedError."""
    native, dev = backend
    meta, cases = _golden()
    (case, sd), = [(c, sd) for c, sd in zip(meta, cases) if c["name"] == "beam4_leaky_relu"]
    s = _beam_searcher(case["cfg"], sd, dev)
    assert s.beam_size == 4 and s.searcher == s.transducer_beam_search_decode
    best, mean, nbest, scores = s(torch.from_numpy(sd["tn"]).to(dev))
    assert best == [n[0] for n in case["nbest"]] and len(nbest) == len(scores) == sd["tn"].shape[0]
