"""The CTC prefix scorer kernels (csrc/ctc_prefix.hip: ctc_score_step<NB>, ctc_same_token, ctc_advance and the state
tables between them) beyond the one shape of test_scorer_step_protocol_vs_oracle: every beam dispatch and beam tile, V past
one 256-token block, T over every chunk / segment / lane-run / load-round edge and into the raised LDS window, `start` walking
over chunk and segment edges, blank != 0, eos == blank, the attention window, the capacity errors and the underflow limit.

native.CTCStepScorer is driven directly, step by step, against tests/ctc_prefix_ref.py (float64, log domain, true -inf), which
this file first pins to oracle.sb_oracle.CTCPrefixScorer (float32) and to tests/golden/ctc_prefix.npz (written by the
reference's own CTCPrefixScore, blank 3 / eos 1 and ctc_window_size 4 with recorded attention).  The (parent, token) pairs of
the beam update are chosen on the host from the REFERENCE's scores and fed to both sides, so ties cannot fork the two.

Inputs.  *flat*: log_softmax(scale * randn).  *peaky*: blank near 1 on most frames, a planted token path that spikes every few
frames, every other token at -10 .. -40; log-probabilities are floored at -60 so that expf of every entry is a NORMAL float
(exp(-60) = 8.8e-27): the kernels keep linear posteriors in fp32, an entry below about -87 is a denormal or zero there and a
number in the float64 reference -- that limit has its own test (test_underflow_limit) and must not leak into the others.

Tolerance.  For a live entry (reference > -1e19)
    |got - ref| <= 2^-23 * (|psi| + |psi_prev|)  +  C * T * 2^-24
the first term is the fp32 rounding of the two numbers the output is the difference of, the second the accumulation over
the frames and the advances.  `c` below is (max |got - ref| - first term) / (T * 2^-24) per case, measured for (a) the float32
oracle (materialises [T,2,n_bh,V]: where it is blank, the case has a window or is too large for it), (b) the kernels on the
CPU emulator, (c) the kernels on the MI355X:

    case                                   (a) oracle f32   (b) emulator   (c) MI355X
    fixture shape, beams 4 / 10                 2.8 .. 6.4        --            --
    B=1 T=1000 V=64 beam 4  scale 3                 62.3        15.1          15.1
    B=1 T=600  V=64 beam 4  scale 6                 95.5       0.001         0.001
    B=1 T=1100 V=64 beam 4  scale 6                129.1       0.001         0.001
    B=1 T=200  V=64 beam 33 scale 6                 98.0       0.004         0.004
    B=1 T=1100 V=64 beam 33 scale 6                175.4       0.001         0.001
    beams 1 .. 33, T=40 V=70                          --     0 .. 17.0     0 .. 17.0   (largest: beams 2 and 33)
    V = 255 .. 1000, beam 5                           --     0 .. 18.5     0 .. 18.5   (largest: V=1000)
    T = 1 .. 257, flat and peaky                      --     0 .. 14.6     0 .. 14.6
    T = 1100 flat / peaky                             --    39.7 / 48.3   39.7 / 48.3
    depth 42 steps, T=300                             --       0.002         0.009
    blank / eos indices                               --     0 .. 13.1     0 .. 13.1
    window 3 / 8, scale 1 and 3                       --     0.2 .. 3.0    0.2 .. 3.0
    underflow limit (the 24 ordinary tokens)          --         2.2           2.2

The largest figures all belong to the <eos> column at step 0, psi[eos] = the blank's cumulative sum at the last frame: a
serial fp32 sum of T terms whose error grows with T * |psi|, in the kernel (ctc_init_kernel) as in torch.cumsum -- the same
order of summation on the emulator and on the hardware, hence the equal figures.  The kernels need less than the float32
oracle wherever both were measured.

C = 200: about 4x the largest kernel figure, 48.3.

Each case also asserts that the reference alone keeps at least three quarters of the non-blank entries live at every compared
step -- except the steps whose frame range is empty by construction (the empty attention window and the scores after it),
where all-dead is the point."""
import os

import numpy as np
import pytest
import torch

import ctc_prefix_ref
from oracle import sb_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C = 200.0
ATT_W = 0.4  # comb = lp + ATT_W * delta


# ============================================================================================================== inputs
def flat_inputs(seed, B, T, V, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(scale * torch.randn(B, T, V, generator=g), -1)


def peaky_inputs(seed, B, T, V, blank, lo=-40.0, hi=-10.0, floor=-60.0, low_tokens=()):
    """Blank near 1, a planted path spiking every 2..6 frames (blank at e^-5 there), the rest uniform in [lo, hi]; tokens
    listed in `low_tokens` lie in [-120, -90] instead (test_underflow_limit).  Floored at `floor` (see the module docstring)."""
    g = torch.Generator().manual_seed(seed)
    x = lo + (hi - lo) * torch.rand(B, T, V, generator=g)
    for c in low_tokens:
        x[:, :, c] = -120.0 + 30.0 * torch.rand(B, T, generator=g)
    x[:, :, blank] = 0.0
    pool = [c for c in range(V) if c != blank and c not in low_tokens]
    for b in range(B):
        t = int(torch.randint(0, 3, (1,), generator=g))
        while t < T:
            x[b, t, pool[int(torch.randint(0, len(pool), (1,), generator=g))]] = 5.0
            t += int(torch.randint(2, 7, (1,), generator=g))
    logp = torch.log_softmax(x, -1)
    return logp if floor is None else logp.clamp_min(floor)


# ============================================================================================================== the two sides
class _Native:
    def __init__(self, backend, logp, lens, blank, eos, window):
        native, self.dev = backend
        self.sc = native.CTCStepScorer(logp.clone().to(self.dev), torch.as_tensor(lens, dtype=torch.int32).to(self.dev), blank,
                                       eos, window)

    def _win(self, win):
        return None if win is None else torch.tensor(win, dtype=torch.int32).to(self.dev)

    def score(self, inp, step, win):
        return self.sc.score(torch.from_numpy(inp).to(self.dev), step, self._win(win)).cpu().double().numpy()

    def permute(self, parent, token, inp, step, win):
        self.sc.permute(*(torch.from_numpy(a).to(self.dev) for a in (parent, token, inp)), step, self._win(win))


class _Oracle:
    """oracle.sb_oracle.CTCPrefixScorer in float32 behind the same two calls (no attention window)."""

    def __init__(self, logp, lens, blank, eos, beam):
        self.o = O.CTCPrefixScorer(logp.clone(), torch.as_tensor(lens, dtype=torch.int32), blank, eos)
        self.beam, self.state = beam, None

    def score(self, inp, step, win):
        assert win is None and step == self.o.prefix_len + 1
        delta, self.new = self.o.step(torch.from_numpy(inp), self.state, self.beam)
        return delta.double().numpy()

    def permute(self, parent, token, inp, step, win):
        cand = torch.from_numpy((parent % self.beam) * self.o.V + token).view(self.o.B, self.beam)
        self.state = self.o.permute(self.new, cand, self.beam)


# ============================================================================================================== the driver
def _bos(blank, eos):
    return next(c for c in (1, 2, 3) if c not in (blank, eos))


def _select(lp, dref, inp, B, beam, V, step, blank, eos, allow_dead, events, allowed=None):
    """The beam update from the REFERENCE's scores: the `beam` best live (parent, token) pairs of every utterance (at step 0
    only the first beam is live), then the forced events: a hypothesis repeats its last token (steps 2, 4, 7, 9, ..), all
    children come from one parent (steps 3, 10, ..), the last parent -- in the second or third tile of 16 when beam > 16 --
    feeds child 0 (steps 1, 4, 7, ..).  A dead pair is never chosen unless the case is about that."""
    comb = lp + ATT_W * dref
    dead = dref <= -1e19
    if allowed is not None:
        dead = dead | ~allowed[None, :]
    comb = np.where(dead, lp - 1e6 if allow_dead else -np.inf, comb)
    if eos != blank:
        comb[:, blank] = -np.inf
    flat = comb.reshape(B, beam * V).copy()
    if step == 0:
        flat[:, V:] = -np.inf
    cand = np.argsort(-flat, axis=1, kind="stable")[:, :beam]
    rows = comb.reshape(B, beam, V)
    last = inp.reshape(B, beam)
    for b in range(B):
        if step == 0:
            continue
        if step % 3 == 1 and beam > 1:
            j = beam - 1
            cand[b, 0] = j * V + int(np.argmax(rows[b, j]))
            events["late_parent"] += 1
        if step % 7 == 3 and beam > 1:
            j = cand[b, 0] // V
            cand[b] = j * V + np.argsort(-rows[b, j], kind="stable")[:beam]
            events["one_parent"] += 1
        if step % 5 in (2, 4):
            k = 0 if step % 5 == 2 else beam - 1
            j = cand[b, k] // V
            if rows[b, j, last[b, j]] > -1e5:
                cand[b, k] = j * V + last[b, j]
                events["repeat"] += 1
    if not allow_dead:
        assert np.all(np.take_along_axis(flat if step == 0 else comb.reshape(B, beam * V), cand, 1) > -1e5), "dead pair chosen"
    parent = (cand // V + np.arange(B)[:, None] * beam).reshape(-1)
    return parent.astype(np.int64), (cand % V).reshape(-1).astype(np.int64)


def drive(make_side, logp, lens, blank, eos, beam, steps, seed, window=0, wins=None, allow_dead=False, dead_ok_from=None,
          allowed=None, upper=None, c_bound=C):
    """Run `steps` score / permute rounds on the float64 reference and on `make_side()`; compare every step.  Returns the
    measured figures {c, err, psi_max, events}."""
    B, T, V = logp.shape
    ref = ctc_prefix_ref.CTCPrefixRef(logp.numpy(), lens, blank, eos, window)
    hi = None if upper is None else ctc_prefix_ref.CTCPrefixRef(upper.numpy(), lens, blank, eos, window)
    side = make_side()
    g = torch.Generator().manual_seed(seed)
    n = B * beam
    inp = np.full(n, _bos(blank, eos), dtype=np.int64)
    events = {"repeat": 0, "one_parent": 0, "late_parent": 0}
    fig = {"c": 0.0, "err": 0.0, "psi_max": 0.0, "events": events}
    nonblank = np.ones(V, dtype=bool)
    if eos != blank:
        nonblank[blank] = False
    for step in range(steps):
        win = None if wins is None else wins[step]
        lp = torch.log_softmax(3.0 * torch.randn(n, V, generator=g), -1).double().numpy()
        dref = ref.score(inp, step, win)
        got = side.score(inp, step, win)
        live = dref > -1e19
        assert not np.isnan(got).any() and not np.isposinf(got).any(), step
        if dead_ok_from is None or step < dead_ok_from:
            assert live[:, nonblank].mean() >= 0.75, (step, float(live[:, nonblank].mean()))
        psi, psi_prev = ctc_prefix_ref.sentinel(ref.psi), ctc_prefix_ref.sentinel(ref.psi_prev)[:, None]
        rounding = 2.0 ** -23 * (np.abs(psi) + np.abs(psi_prev))
        bound = rounding + c_bound * T * 2.0 ** -24
        if hi is not None:  # (test_underflow_limit: the kernels may lose a token, never invent probability)
            dhi = hi.score(inp, step, win)
            assert not np.any((got > -1e19) & ~live), step
            assert np.all((got - dhi)[live] <= bound[live]), (step, float((got - dhi)[live].max()))
            chk = live & allowed[None, :]
            assert np.array_equal(got[:, allowed] > -1e19, live[:, allowed]), step
        else:
            assert np.array_equal(got > -1e19, live), step
            chk = live
            if (~live).any():
                assert float(np.abs(got[~live] / dref[~live] - 1.0).max()) <= 1e-5, step
        err = np.abs(got - dref)
        if chk.any():
            fig["err"] = max(fig["err"], float(err[chk].max()))
            fig["c"] = max(fig["c"], float(((err - rounding)[chk] / (T * 2.0 ** -24)).max()))
            fig["psi_max"] = max(fig["psi_max"], float(np.abs(psi[chk & (psi > -1e19)]).max(initial=0.0)))
            bad = chk & (err > bound)
            assert not bad.any(), (step, float(err[bad].max()), float(bound[bad].min()), fig["c"])
        parent, token = _select(lp, dref, inp, B, beam, V, step, blank, eos, allow_dead, events, allowed)
        side.permute(parent, token, inp, step, win)
        ref.permute(parent, token)
        if hi is not None:
            hi.permute(parent, token)
        inp = token
    print(f"\n    figures: c = {fig['c']:.3f}  max|err| = {fig['err']:.3e}  max|psi| = {fig['psi_max']:.1f}  {events}")
    return fig


def _case(backend, logp, lens, blank, eos, beam, steps, seed, **kw):
    return drive(lambda: _Native(backend, logp, lens, blank, eos, kw.get("window", 0)), logp, lens, blank, eos, beam, steps,
                 seed, **kw)


# ============================================================================================================== 1. pinning
def _fixture_shape():
    """The inputs of test_scorer_step_protocol_vs_oracle: B=3, T=37, V=50, ragged lengths, blank 0, eos 2."""
    logp = flat_inputs(21, 3, 37, 50, scale=1.0)
    return logp, torch.round(37 * torch.tensor([1.0, 0.62, 0.85])).int().numpy()


def _oracle_bound(T, psi_max):
    """What float32 rounding of the oracle allows on top of the output term: its recurrences and log-sums are contractions
    (weights that sum to one), so an error made at one frame is never amplified, and each of the T frames adds at most three
    roundings (sum, exp / log, add) of a number no larger than the largest |log-probability| in play."""
    return 3.0 * T * 2.0 ** -24 * max(psi_max, 1.0)


@pytest.mark.parametrize("shape", ["fixture", "blank_mid"])
def test_reference_agrees_with_float32_oracle(shape):
    """tests/ctc_prefix_ref.py against oracle.sb_oracle.CTCPrefixScorer run in float32, entry for entry (live pattern,
    live values, sentinel values), at the shape of the existing kernel test (beams 4 and 10, six steps) and at one with
    blank 7 / eos 4 and ragged lengths, where the padding column (0) is an ordinary token."""
    logp, lens = _fixture_shape()
    blank, eos = (0, 2) if shape == "fixture" else (7, 4)
    for beam in (4, 10):
        # C of the kernels does not apply to the oracle: its own bound, expressed in the same form
        c_oracle = _oracle_bound(37, 400.0) / (37 * 2.0 ** -24)
        fig = drive(lambda: _Oracle(logp, lens, blank, eos, beam), logp, lens, blank, eos, beam, 6, 5, c_bound=c_oracle)
        assert fig["psi_max"] <= 400.0 and fig["events"]["repeat"] >= 2


@pytest.mark.parametrize("mode", ["blank3_eos1", "window4"])
def test_reference_and_oracle_agree_with_the_recorded_reference(mode):
    """tests/golden/ctc_prefix.npz (oracle/make_golden.py: golden_ctc_prefix): the reference's own CTCPrefixScore over five
    steps at B=2, T=40, V=20, once with blank 3 / eos 1 and once with ctc_window_size 4 and a recorded attention matrix --
    the two modes the model-level goldens never reach.  The float64 restatement must reproduce the recorded psi - psi_prev
    at the recorded candidates within float32 rounding of the reference; so must the float32 oracle where it has the mode."""
    g = np.load(os.path.join(GOLD, "ctc_prefix.npz"))
    logp, lens = torch.from_numpy(g["logp"]), g["enc_len"]
    blank, eos, window, beam = (int(v) for v in g[f"{mode}/cfg"])
    B, T, V = logp.shape
    deltas, cands, attn = g[f"{mode}/delta"], g[f"{mode}/cand"], g[f"{mode}/attn"]
    sides = [ctc_prefix_ref.CTCPrefixRef(logp.numpy(), lens, blank, eos, window)]
    if window == 0:
        sides.append(_Oracle(logp, lens, blank, eos, beam))
    inp = np.full(B * beam, int(g[f"{mode}/bos"]), dtype=np.int64)
    for step in range(deltas.shape[0]):
        win = None
        if window > 0:
            peak = attn[step].argmax(1)
            win = (int(peak.min()), int(peak.max()))
        rec = deltas[step].astype(np.float64)
        live = rec > -1e19
        assert live.mean() >= 0.5, step
        parent = (cands[step] // V + np.arange(B)[:, None] * beam).reshape(-1).astype(np.int64)
        token = (cands[step] % V).reshape(-1).astype(np.int64)
        for s in sides:
            got = s.score(inp, step, win)
            assert np.array_equal(got > -1e19, live), (step, type(s).__name__)
            tol = 2.0 ** -22 * np.abs(rec) + 2 * _oracle_bound(T, float(np.abs(rec[live]).max()))
            assert np.all(np.abs(got - rec)[live] <= tol[live]), (step, type(s).__name__, float(np.abs(got - rec)[live].max()))
            assert float(np.abs(got[~live] / rec[~live] - 1.0).max()) <= 1e-5
            if isinstance(s, _Oracle):
                s.permute(parent, token, inp, step, win)
            else:
                s.permute(parent, token)
        inp = token


# ============================================================================================================== 2. the probe
@pytest.mark.parametrize("T,beam,scale", [(1000, 4, 3.0), (600, 4, 6.0), (1100, 4, 6.0), (200, 33, 6.0), (1100, 33, 6.0)])
def test_advance_scan_over_a_wide_dynamic_range(backend, T, beam, scale):
    """Regression: B=1, V=64, logits scale * randn (seed 0).  The first score after an advance was off by 1e2 .. 4e2 nats
    (float32 oracle and float64 reference agreed with each other, emulator and kernel source did not): ctc_advance's scan
    composes the per-frame affine maps of up to 32 lanes' runs, and the entries of such a map -- the all-token path a, the
    all-blank path d, the mixed paths c, v0, v1 -- shared exponents.  Over a few hundred frames of posteriors with a real
    dynamic range they drift more than 2^126 apart, the smaller one flushed to zero, and the next run of frames could favour
    exactly the flushed path: the state was wrong from a lane boundary on.  Each entry now has its own exponent."""
    logp = flat_inputs(0, 1, T, 64, scale=scale)
    _case(backend, logp, [T], 0, 2, beam, 6, 0)


# ============================================================================================================== 3. shapes
@pytest.mark.parametrize("beam", [1, 2, 4, 5, 10, 11, 16, 17, 32, 33])
def test_beam_dispatch_and_tiles(backend, beam):
    """ctc_score_step<1 / 4 / 10 / 16> on either side of every dispatch threshold, and one, two and three tiles of 16 beams
    (blockIdx.z, the j0 offset into the [frame][beam] table and its row pitch); a parent of the last tile feeds child 0."""
    logp = flat_inputs(100 + beam, 2, 40, 70)
    fig = _case(backend, logp, [40, 33], 0, 2, beam, 6, beam)
    assert fig["events"]["repeat"] >= 2 and (beam == 1 or fig["events"]["late_parent"] >= 2 and fig["events"]["one_parent"] >= 1)


@pytest.mark.parametrize("V", [255, 256, 257, 1000])
def test_vocabulary_blocks(backend, V):
    """blockIdx.x of ctc_score_step / ctc_score_delta: one block exactly full, one token short of it, one token into the
    second, four blocks with a ragged last one."""
    _case(backend, flat_inputs(V, 2, 40, V), [31, 40], 0, 2, 5, 5, V)


FRAMES = [(T, "flat") for T in (1, 2, 16, 17, 32, 33, 63, 64, 65, 256, 257, 1100)] + \
    [(T, "peaky") for T in (64, 65, 256, 257, 1100)]


def _frames_case(backend, T, family):
    B, V, beam = 2, 30, 4
    logp = flat_inputs(T, B, T, V) if family == "flat" else peaky_inputs(T, B, T, V, 0)
    lens = [T, max(1, T - T // 3)] if T > 2 else [T, T]
    return _case(backend, logp, lens, 0, 2, beam, min(6, T), T)


@pytest.mark.parametrize("T,family", FRAMES)
def test_frame_edges(backend, T, family):
    """T on either side of the chunk of 16 table entries and the 32-frame scale segment of ctc_score_step, the 64 lanes of
    ctc_same_token and of ctc_advance's scan (frames per lane going from 1 to 2), the 256-frame load round of ctc_advance;
    T = 1100, where the [T][16] table of ctc_score_step needs more than the default 64 KiB of dynamic LDS (the raised window;
    the emulator finishes it in under a second, so it has no GPU-only sibling).  T = 1 and 2 leave one and two steps before
    the prefix is as long as the utterance.  Flat and peaky posteriors."""
    _frames_case(backend, T, family)


def test_depth_and_a_ragged_batch_that_runs_out_of_frames(backend):
    """42 steps at T=300, beam 4: `start` walks over the chunk edges (16, 17, 32, 33) of the score kernel and the segment
    edge, ctc_advance's lane runs shrink from 5 frames to 4.  One utterance of the batch has 20 frames: from step 20 on
    start >= end for it, every token is dead, its hypotheses are extended all the same (dead pairs, compared by the sentinel
    rule: dead minus dead is 0) while the other three go on."""
    logp = flat_inputs(300, 4, 300, 30)
    fig = _case(backend, logp, [300, 20, 300, 257], 0, 2, 4, 42, 300, allow_dead=True)
    assert fig["events"]["repeat"] >= 10 and fig["events"]["one_parent"] >= 5


@pytest.mark.parametrize("blank,eos,lens", [(0, 2, [40, 40, 40]), (15, 2, [40, 40, 40]), (29, 1, [40, 40, 40]),
                                            (3, 3, [40, 40, 40]), (0, 0, [40, 23, 31]), (15, 2, [40, 23, 31]),
                                            (29, 0, [40, 23, 31]), (29, 29, [40, 23, 31])])
def test_blank_and_eos_indices(backend, blank, eos, lens):
    """Blank at 0, in the middle and at V-1; eos == blank (the blank column is then the eos score, not masked); ragged
    lengths with blank != 0, where the length clip of the score kernels is off and column 0 -- an ordinary token -- carries
    the padding (P = 1 on the padded frames) while the blank dies there."""
    _case(backend, flat_inputs(7 + blank, 3, 40, 30), lens, blank, eos, 5, 6, 11 + eos)


WINDOWS = {3: [(20, 39), (4, 20), (15, 22), None, (10, 12), (2, 30), (0, 3)],
           8: [(20, 39), (4, 20), (15, 22), None, (20, 22), (2, 30), (25, 39), (0, 39), (14, 20), (0, 1)]}


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("window", [3, 8])
def test_attention_window(backend, window, scale):
    """ctc_window_size 3 and 8 with {min, max} attention peaks that clip the frame range on the left, on the right, on both
    sides, not at all (no attention: every frame), and -- last -- to an empty range (max + window <= step), after which
    every score is dead (sentinel rule); `score` and `permute` take the same window.

    Regression at scale 3.0: the gamma table ctc_score_step reads is scaled per 32-frame segment by the segment's LARGEST
    entry; at 8 nats per frame the entries of frames 16..31 lie more than 126 bits below frame 0's and are flushed to zero
    when the table is built -- harmless while frame 0 is scored too, but a window that starts (or ends) inside the segment
    leaves that maximum outside: at step 0, window (20, 39), every token of utterance 0 came out 1.1e2 .. 1.5e2 nats too
    low (only frames [33, 40) counted).  With a window the score kernels now scale by the largest entry among the SCORED
    frames, from the unscaled block-float state.  Scale 1.0 (1.5 nats per frame) never flushed."""
    wins = WINDOWS[window]
    logp = flat_inputs(50 + window, 2, 40, 30, scale=scale)
    _case(backend, logp, [40, 34], 0, 2, 4, len(wins) + 1, window, window=window, wins=wins + [None], allow_dead=True,
          dead_ok_from=len(wins) - 1)


def test_capacity_limits_name_lds(backend):
    """T beyond what ctc_advance (7 * T * 4 B > 64 KiB: T > 2340) or ctc_psi_step (160 KiB: T > 2487) can hold must raise
    SbkError with a message that names LDS; T = 2400 still scores."""
    native, dev = backend
    for T, fails_in_score in ((2400, False), (2500, True)):
        logp = flat_inputs(T, 1, T, 8, scale=1.0)
        sc = native.CTCStepScorer(logp.to(dev), torch.tensor([T], dtype=torch.int32).to(dev), 0, 2)
        inp = torch.ones(1, dtype=torch.int64).to(dev)
        if fails_in_score:
            with pytest.raises(native.SbkError, match="LDS"):
                sc.score(inp, 0)
            continue
        ref = ctc_prefix_ref.CTCPrefixRef(logp.numpy(), [T], 0, 2)
        got, dref = sc.score(inp, 0).cpu().double().numpy(), ref.score(np.ones(1, dtype=np.int64), 0)
        live = dref > -1e19
        assert np.array_equal(got > -1e19, live)
        assert np.all(np.abs(got - dref)[live] <= 2.0 ** -23 * np.abs(dref[live]) + C * T * 2.0 ** -24)
        with pytest.raises(native.SbkError, match="LDS"):
            sc.permute(torch.zeros(1, dtype=torch.int64).to(dev), torch.full((1,), 3).to(dev), inp, 0)


def test_underflow_limit(backend):
    """Log-probabilities below -90: six of 30 tokens lie in [-120, -90] on every frame, where expf is zero or a denormal
    that the block-float tables flush.  The LIMIT: such a token may come out dead (-1e20) although the reference has a finite
    (hopeless) score for it.  What must hold all the same: no NaN or +inf, nothing live that the reference has dead, no score
    above the reference by more than the tolerance -- where "the reference" for this one-sided check is the float64 scorer
    on posteriors raised by 2^-150 each, half the spacing of fp32 denormals: expf rounds to the nearest denormal, which may
    lie ABOVE the true value by that much (a factor 1.16 was measured on the exact posteriors, 0.15 nats) -- and the other
    24 tokens, which the beam update is restricted to, agree both ways within the tolerance."""
    V, low = 30, (4, 9, 14, 19, 24, 28)
    logp = peaky_inputs(90, 2, 70, V, 0, floor=None, low_tokens=low)
    assert float(logp[:, :, list(low)].max()) < -90.0
    allowed = np.ones(V, dtype=bool)
    allowed[list(low)] = False
    upper = torch.logaddexp(logp.double(), torch.tensor(-150.0 * np.log(2.0), dtype=torch.float64))
    _case(backend, logp, [70, 61], 0, 2, 4, 6, 90, allowed=allowed, upper=upper)
