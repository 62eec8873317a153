"""The feature front-end (csrc/fbank.hip, the row kernels behind it) beyond its two fixture configurations.

Every test runs on the CPU emulator of the kernel sources and, marked ``gpu``, on the MI355X.  The yardstick is a
float64 restatement in plain torch, written here: ``torch.stft`` in double -> ``|.|^2`` -> ``@ fbank_matrix`` (the
module's own buffer; ``_filter_matrix`` is pinned to the reference by the goldens) -> ``10 log10(clamp(amin))`` ->
per-utterance ``max - top_db`` floor -> optional ``(x - mean) / max(std, eps)``.  ``test_restatement_matches_golden``
pins that restatement to the reference's own outputs first.

What the fixtures never reach and these do: FFT pass orders with a radix-3 butterfly, a radix-2 pass that is not the
last one and a pure ``[2]``; dynamic LDS above the 64 KiB default window (n_fft 800 / 1024 / 1600 -- only the device
can refuse those launches); every ``T % 4`` of the 4-frames-per-workgroup tiling, ``T == 1`` and signals shorter than
half a frame; utterances of one batch more than ``top_db`` apart; ``n_mels`` above 64 (two loop trips per lane),
small counts, and filters narrower than one FFT bin; ``amplitude_to_db``, ``spectral_magnitude``, ``log_softmax``
and ``input_norm_global_masked`` called directly.

Tolerances are the project's stated ones (Fbank 1e-3 dB; STFT and Whisper log-mel 2e-4; batch
invariance 8e-5), each measured against float64.  Where none was stated the bound is derived from the fp32 format
in the test's docstring.  Every test prints the error it saw before it asserts (``pytest -s``); the largest per
group are tabulated in DESIGN.md section 3.
"""
import math
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP = 2.0 ** -23  # spacing of fp32 numbers in [1, 2)


def _md(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def _seen(what, dev, err):
    print(f"[frontend_shapes] {what} {dev.type} max|d|={err:.3g}")
    return err


# ------------------------------------------------------------------------------------------- float64 restatements
def ref_mel_power(fe, wav):
    """[B,N] -> float64 mel power [B,T,n_mels] of a FbankFrontend (window already padded to n_fft)."""
    spec = torch.stft(wav.cpu().double(), fe.n_fft, fe.hop, fe.n_fft, fe.window.cpu().double(), center=True,
                      pad_mode="constant", return_complex=True)
    return (spec.abs() ** 2).transpose(1, 2) @ fe.fbank_matrix.cpu().double()


def ref_db(power, amin, top_db, mult=10.0, db_offset=0.0):
    """dB with the per-utterance floor: also returns each utterance's floor."""
    db = mult * torch.log10(torch.clamp(power, min=amin)) - db_offset
    floor = db.reshape(db.shape[0], -1).amax(dim=1) - top_db
    return torch.maximum(db, floor.reshape(-1, *([1] * (db.dim() - 1)))), floor


def ref_fbank(fe, wav, mean=None, std=None, eps=1e-10):
    out, _ = ref_db(ref_mel_power(fe, wav), fe.amin, fe.top_db)
    if mean is not None:
        out = (out - mean.cpu().double()) / torch.clamp(std.cpu().double(), min=eps)
    return out


def ref_whisper_log_mel(audio, filters, n_fft=400, hop=160):
    """tests/test_whisper.py::torch_log_mel in double."""
    stft = torch.stft(audio.double(), n_fft, hop, window=torch.hann_window(n_fft).double(), return_complex=True)
    mel = filters.double() @ (stft[..., :-1].abs() ** 2)
    log_spec = torch.clamp(mel, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.max() - 8.0)
    return (log_spec + 4.0) / 4.0


def _frontend(dev, sr, n_fft, win_ms, n_mels, hop_ms=10, **kw):
    from speechbrain_amd.processing.features import FbankFrontend

    return FbankFrontend(sample_rate=sr, win_length=win_ms, hop_length=hop_ms, n_fft=n_fft, n_mels=n_mels, **kw).to(dev)


def test_restatement_matches_golden():
    """The float64 restatement against the REFERENCE's outputs (tests/golden/fbank.npz): both configurations at
    1e-3 dB and the normed output at 2e-4, the tolerances of test_kernels.py::test_fbank_golden.  No kernel runs."""
    g = np.load(os.path.join(GOLD, "fbank.npz"))
    wav = torch.from_numpy(g["wav"])
    dev = torch.device("cpu")
    for tag, n_fft, win in (("L", 512, 32), ("S", 400, 25)):
        fe = _frontend(dev, 16000, n_fft, win, 80)
        assert _seen(f"restatement {tag}", dev, _md(ref_fbank(fe, wav), torch.from_numpy(g["fbank_" + tag]))) <= 1e-3
    fe = _frontend(dev, 16000, 512, 32, 80)
    normed = ref_fbank(fe, wav, torch.from_numpy(g["norm_mean"]), torch.from_numpy(g["norm_std"]))
    assert _seen("restatement normed", dev, _md(normed, torch.from_numpy(g["normed_L"]))) <= 2e-4


# ------------------------------------------------------------------------------------------- 1. FFT factorizations
# (sample_rate, n_fft, win_ms, hop_ms, n_mels, f_min, f_max, radices): the pass orders are asserted, so a change of
# factor_radices cannot quietly take a path out of the sweep.  LDS: n_fft 800 needs ~67 KiB (just past the default
# window), 1024 ~82 KiB, 1600 ~131 KiB.  8 kHz / n_fft 240 / 128 mels: 121 bins for 128 filters, so runs of 0 and 1.
# n_fft 2 (1 kHz, 2 ms): bins at 0 and 500 Hz only; f_max above Nyquist puts the one filter's slope on bin 1.
FACTORIZATIONS = [
    (16000, 400, 25, 10, 80, 0, None, [4, 4, 5, 5]),
    (16000, 480, 25, 10, 40, 0, None, [4, 4, 2, 3, 5]),
    (16000, 384, 20, 10, 23, 0, None, [4, 4, 4, 2, 3]),
    (8000, 240, 25, 10, 128, 0, None, [4, 4, 3, 5]),
    (16000, 512, 32, 10, 80, 0, None, [4, 4, 4, 4, 2]),  # win == n_fft (as at 400, 1024, 1600): no window padding
    (16000, 768, 32, 10, 128, 0, None, [4, 4, 4, 4, 3]),
    (16000, 360, 20, 10, 40, 100, 6000, [4, 2, 3, 3, 5]),
    (16000, 800, 40, 10, 80, 0, None, [4, 4, 2, 5, 5]),
    (16000, 1024, 64, 10, 128, 0, None, [4, 4, 4, 4, 4]),
    (16000, 1600, 100, 10, 80, 0, None, [4, 4, 4, 5, 5]),
    (1000, 2, 2, 1, 1, 0, 1000, [2]),
]
_FACT_IDS = [f"sr{c[0]}-nfft{c[1]}-win{c[2]}ms-mels{c[4]}" for c in FACTORIZATIONS]


def _three_levels(n, seed, silent=0):
    """Noise at 0.1 whose last `silent` samples are zero, the same 80 dB lower (x 1e-4: its loudest value is the
    first one's floor), and silence."""
    a = 0.1 * torch.randn(n, generator=torch.Generator().manual_seed(seed))
    a[n - silent:] = 0
    return torch.stack([a, a * 1e-4, torch.zeros(n)])


@pytest.mark.parametrize("sr,n_fft,win_ms,hop_ms,n_mels,f_min,f_max,radices", FACTORIZATIONS, ids=_FACT_IDS)
def test_fbank_factorizations(backend, sr, n_fft, win_ms, hop_ms, n_mels, f_min, f_max, radices):
    """Fbank within 1e-3 dB of float64 at every pass order; a batch whose utterances are 80 dB apart.

    The floor checks: no value of an utterance lies under its OWN max - top_db; every utterance's minimum is the
    restatement's; and where the floor binds -- utterance 0, whose silent tail sits at -100 dB under a floor near
    -70 dB -- the minimum IS max - top_db.  (It cannot bind in the other two: the amin clamp at -100 dB lies above
    their floors of about -150 and -180 dB.)  A floor taken over the batch would lift utterance 1 wholesale."""
    nat, dev = backend
    fe = _frontend(dev, sr, n_fft, win_ms, n_mels, hop_ms=hop_ms, f_min=f_min, f_max=f_max)
    assert fe.radices == radices
    silent = n_fft + 2 * fe.hop  # some frames lie wholly inside the silent tail
    N = silent + 8 * fe.hop + fe.hop // 2 + 5
    wav = _three_levels(N, n_fft, silent)
    out = fe(wav.to(dev)).cpu()
    ref = ref_fbank(fe, wav)
    assert out.shape == (3, 1 + N // fe.hop, n_mels)
    assert _seen(f"fbank n_fft={n_fft}", dev, _md(out, ref)) <= 1e-3
    assert torch.all(out[2] == -100.0)
    for b in range(3):
        assert float(out[b].min()) >= float(out[b].max()) - fe.top_db - 1e-3, b
        assert abs(float(out[b].min()) - float(ref[b].min())) <= 1e-3, b
    assert abs(float(out[0].min()) - (float(out[0].max()) - fe.top_db)) <= 1e-3
    assert float(out[1].max()) <= float(out[0].min()) + 1e-3  # the batch really spans more than top_db


# ------------------------------------------------------------------------------------------- 2. frame and tile edges
@pytest.mark.parametrize("n_fft", [400, 480])
def test_fbank_frame_and_tile_edges(backend, n_fft):
    """One workgroup handles 4 frames: T = 1 + N // hop over every T % 4, T in {1, 2, 5}, and signals shorter than a
    hop or than half a frame (N = 1, hop - 1, hop, n_fft // 2 - 1).  Float64 within 1e-3 dB, and batch invariance
    within 8e-5 (test_fbank_known_answers' figure): row b of a batch equals the same waveform run alone."""
    nat, dev = backend
    fe = _frontend(dev, 16000, n_fft, 25, 40)
    hop = fe.hop
    seen_T, worst, worst_inv = set(), 0.0, 0.0
    for N in (1, hop - 1, hop, n_fft // 2 - 1, 4 * hop + 3, 5 * hop + hop - 1, 6 * hop, 7 * hop + 1):
        g = torch.Generator().manual_seed(N)
        wav = torch.stack([0.1 * torch.randn(N, generator=g), 1e-3 * torch.randn(N, generator=g),
                           0.3 * torch.rand(N, generator=g)])
        out = fe(wav.to(dev)).cpu()
        T = 1 + N // hop
        seen_T.add(T)
        assert out.shape == (3, T, 40), N
        err = _md(out, ref_fbank(fe, wav))
        worst = max(worst, err)
        assert err <= 1e-3, (N, err)
        for b in range(3):
            inv = _md(fe(wav[b:b + 1].contiguous().to(dev)), out[b:b + 1])
            worst_inv = max(worst_inv, inv)
            assert inv <= 8e-5, (N, b, inv)
    assert {1, 2, 5} <= seen_T and {t % 4 for t in seen_T} == {0, 1, 2, 3}
    _seen(f"fbank edges n_fft={n_fft}", dev, worst)
    _seen(f"fbank edges n_fft={n_fft} batch invariance", dev, worst_inv)


# ------------------------------------------------------------------------------------------- 3. narrow-band input
NARROW_CAP = 1e-6  # compare where the float64 mel power is at least this fraction of its frame's largest


def _tone_batch(n_fft=400, sr=16000, n=2000):
    """A 0.5-amplitude sine at an exact bin centre (bin 25 of 400: 1000 Hz) and one midway between two bins
    (1020 Hz), each over white noise 40 dB below the tone's power."""
    t = torch.arange(n, dtype=torch.float64) / sr
    noise = torch.randn(2, n, generator=torch.Generator().manual_seed(40)) * math.sqrt(0.125 * 1e-4)
    tones = torch.stack([torch.sin(2 * math.pi * 25 * sr / n_fft * t), torch.sin(2 * math.pi * 25.5 * sr / n_fft * t)])
    return (0.5 * tones).float() + noise


@pytest.mark.parametrize("n_mels", [23, 40])
def test_narrow_band_restatement_keeps_the_cap(n_mels):
    """The cap is a condition on the INPUT, settled by the float64 restatement alone: at least 95 % of all mel
    values lie within 60 dB of their frame's largest (99.0 % at 23 filters, 95.8 % at 40; at 80 the low filters are
    narrower than a bin and only 88.7 % do, so 80 is not used here), and the comparison below skips the rest."""
    fe = _frontend(torch.device("cpu"), 16000, 400, 25, n_mels)
    p = ref_mel_power(fe, _tone_batch())
    assert float((p >= NARROW_CAP * p.amax(dim=2, keepdim=True)).double().mean()) >= 0.95


@pytest.mark.parametrize("n_mels", [23, 40])
def test_fbank_narrow_band(backend, n_mels):
    """A tone puts nearly all of a frame's energy into two or three bins; every other bin is what the window's side
    lobes and the noise leave.  fp32 rounding is relative to the frame's energy, not the bin's, so bins more than
    60 dB under the frame's largest are not compared; the rest agree within 1e-3 dB."""
    nat, dev = backend
    fe = _frontend(dev, 16000, 400, 25, n_mels)
    wav = _tone_batch()
    p = ref_mel_power(fe, wav)
    keep = p >= NARROW_CAP * p.amax(dim=2, keepdim=True)
    assert float(keep.double().mean()) >= 0.95
    out = fe(wav.to(dev)).cpu().double()
    ref, _ = ref_db(p, fe.amin, fe.top_db)
    assert out.shape == ref.shape
    assert _seen(f"fbank narrow band n_mels={n_mels}", dev, float((out - ref).abs()[keep].max())) <= 1e-3


# ------------------------------------------------------------------------------------------- 4. fused normalisation
@pytest.mark.parametrize("n_mels", [23, 80])
def test_fbank_fused_norm(backend, n_mels):
    """(x - mean) / max(std, eps) in the floor pass, with std entries of 0 and 1e-3 under norm_eps = 1e-2 and T = 7.
    The dB tolerance carried through the division: |d| * max(std, eps) <= 1e-3 for every element (for the fixture's
    std >= 5 that is its 2e-4)."""
    nat, dev = backend
    fe = _frontend(dev, 16000, 480, 25, n_mels)
    N = 6 * fe.hop + 17
    wav = _three_levels(N, 4)
    mean = torch.linspace(-60, -20, n_mels)
    std = torch.linspace(5, 15, n_mels)
    std[0], std[n_mels // 2], std[-1] = 0.0, 1e-3, 1e-2
    eps = 1e-2
    out = fe(wav.to(dev), mean.to(dev), std.to(dev), eps).cpu()
    ref = ref_fbank(fe, wav, mean, std, eps)
    assert out.shape == (3, 7, n_mels)
    scaled = (out.double() - ref).abs() * torch.clamp(std.double(), min=eps)
    assert _seen(f"fbank fused norm n_mels={n_mels} (dB units)", dev, float(scaled.max())) <= 1e-3
    assert _md(out[:, :, 1:n_mels // 2], ref[:, :, 1:n_mels // 2]) <= 2e-4  # columns with std >= 5


# ------------------------------------------------------------------------------------------- 5. STFT
@pytest.mark.parametrize("sr,n_fft,win_ms,hop_ms", [c[:4] for c in FACTORIZATIONS], ids=_FACT_IDS)
def test_stft_factorizations(backend, sr, n_fft, win_ms, hop_ms):
    """STFT module vs float64 torch.stft given the UNPADDED window and win_length (so the module's centring of a
    short window is checked too), 2e-4 absolute at unit-variance input; silence gives zeros exactly."""
    nat, dev = backend
    from speechbrain_amd.processing.features import STFT

    st = STFT(sample_rate=sr, win_length=win_ms, hop_length=hop_ms, n_fft=n_fft).to(dev)
    N = 9 * st.hop_length + 3 if n_fft > 2 else 41
    wav = torch.randn(2, N, generator=torch.Generator().manual_seed(n_fft + 1))
    out = st(wav.to(dev)).cpu()
    ref = torch.view_as_real(torch.stft(wav.double(), n_fft, st.hop_length, st.win_length,
                                        torch.hamming_window(st.win_length).double(), center=True, pad_mode="constant",
                                        return_complex=True)).transpose(2, 1)
    assert out.shape == (2, 1 + N // st.hop_length, n_fft // 2 + 1, 2) == tuple(ref.shape)
    assert _seen(f"stft n_fft={n_fft}", dev, _md(out, ref)) <= 2e-4
    assert torch.all(st(torch.zeros(2, N, device=dev)).cpu() == 0.0)


# ------------------------------------------------------------------------------------------- 6. staged path
@pytest.mark.parametrize("n_fft,win_ms,n_mels", [(480, 25, 40), (1024, 64, 80)])
def test_staged_vs_fused_and_float64(backend, n_fft, win_ms, n_mels):
    """Fbank.forward_staged (STFT -> spectral_magnitude -> Filterbank, which calls amplitude_to_db) against the fused
    kernel and float64, all within 1e-3 dB."""
    nat, dev = backend
    from speechbrain_amd.lobes.features import Fbank

    fb = Fbank(n_fft=n_fft, n_mels=n_mels, win_length=win_ms).to(dev)
    wav = _three_levels(9 * 160 + 3, n_fft + 2)
    staged, fused = fb.forward_staged(wav.to(dev)).cpu(), fb(wav.to(dev)).cpu()
    ref = ref_fbank(fb.fused, wav)
    assert _seen(f"staged n_fft={n_fft} vs float64", dev, _md(staged, ref)) <= 1e-3
    assert _seen(f"staged n_fft={n_fft} vs fused", dev, _md(staged, fused)) <= 1e-3
    assert _md(fused, ref) <= 1e-3


@pytest.mark.parametrize("per_utt", [1, 37, 64 * 256 + 5])
@pytest.mark.parametrize("mult,db_offset", [(10.0, 0.0), (20.0, 7.5)])
def test_amplitude_to_db(backend, per_utt, mult, db_offset):
    """native.amplitude_to_db alone: 64 tiles per utterance whatever per_utt is (so empty tiles below 16 384
    elements), levels 100 dB apart in one batch, values under amin, an all-zero utterance.

    Bound 5e-5 dB: |v| < 256 here, where fp32 numbers are 1.53e-5 apart.  log10 is taken in double and rounded to
    fp32 (relative 6e-8, times |v| <= 200: 1.2e-5); the product with the multiplier and the subtraction of the
    offset round once each (7.6e-6 each): 2.7e-5 in all, and the floor is a maximum of such values."""
    nat, dev = backend
    g = torch.Generator().manual_seed(per_utt)
    x = torch.stack([10.0 ** (4 * torch.rand(per_utt, generator=g) - 2),       # 1e-2 .. 1e2
                     10.0 ** (4 * torch.rand(per_utt, generator=g) - 12),      # 1e-12 .. 1e-8: partly under amin
                     torch.zeros(per_utt),
                     10.0 ** (14 * torch.rand(per_utt, generator=g) - 11)])    # 140 dB of range: the floor binds
    ref, floor = ref_db(x.double(), 1e-10, 80.0, mult, db_offset)
    out = nat.amplitude_to_db(x.clone().to(dev), mult, 1e-10, db_offset, 80.0).cpu()
    assert out.shape == x.shape
    assert _seen(f"amplitude_to_db per_utt={per_utt} mult={mult}", dev, _md(out, ref)) <= 5e-5
    assert torch.all(out[2] == mult * -10.0 - db_offset)
    for b in range(4):
        assert float(out[b].min()) >= float(floor[b]) - 5e-5, b


@pytest.mark.parametrize("power", [1, 0.5, 2])
@pytest.mark.parametrize("log", [False, True])
def test_spectral_magnitude(backend, power, log):
    """(re^2 + im^2)^power, eps added before a fractional power, optional log(. + eps); n = 273 is no multiple of
    256, one bin is exactly zero.

    Bounds: re^2 + im^2 carries at most 1.5 ulp, raised to the power at most 3, powf one more: relative 4 ulp
    (4.8e-7), asserted as 1e-6.  The logarithm turns that into an absolute 1e-6 and adds up to two ulp of its own
    value (|log| <= 33 at the zero bin): 1e-6 + 3 ulp * max(|ref|, 1)."""
    nat, dev = backend
    x = torch.randn(3, 7, 13, 2, generator=torch.Generator().manual_seed(9))
    x[1, 2, 3] = 0.0
    assert (x.numel() // 2) % 256 != 0
    eps = 1e-14
    v = (x.double() ** 2).sum(-1)
    if power < 1:
        v = v + eps
    ref = v ** power
    out = nat.spectral_magnitude(x.to(dev), power, log, eps).cpu().double()
    assert out.shape == ref.shape
    if log:
        ref = torch.log(ref + eps)
        tol = 1e-6 + 3 * ULP * torch.clamp(ref.abs(), min=1.0)
    else:
        tol = 1e-6 * ref.abs() + 1e-30
    ratio = float(((out - ref).abs() / tol).max())
    _seen(f"spectral_magnitude power={power} log={log} (fraction of bound)", dev, ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------- 7. Whisper log-mel
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("T", [1, 34, 35, 37])
def test_whisper_log_mel_shapes(backend, n_mels, T):
    """WhisperLogMel.log_mel_spectrogram vs the float64 restatement at 2e-4: T = N // hop off the 4-frame tiles of
    the frames kernel and the 32-frame tiles of the transposing floor kernel; T = 1 is N = n_fft // 2 + 1, the
    shortest signal reflect padding accepts, where the mirrored indices reach both ends of the signal.  The loud
    utterance sets the batch-wide floor of the quiet and the silent one."""
    nat, dev = backend
    from speechbrain_amd.integrations.huggingface.whisper import WhisperLogMel

    fe = WhisperLogMel(n_mels=n_mels).to(dev)
    N = 201 if T == 1 else 160 * T + 5
    g = torch.Generator().manual_seed(T)
    wav = torch.stack([0.5 * torch.randn(N, generator=g), 1e-3 * torch.randn(N, generator=g), torch.zeros(N)])
    out = fe.log_mel_spectrogram(wav.to(dev)).cpu()
    ref = ref_whisper_log_mel(wav, fe._mel_filters.cpu())
    assert out.shape == (3, n_mels, T) == tuple(ref.shape)
    assert _seen(f"whisper n_mels={n_mels} T={T}", dev, _md(out, ref)) <= 2e-4
    assert float(out[2].max()) == pytest.approx(float(ref[2].max()), abs=2e-4)
    assert float(out[2].min()) == float(out[2].max())  # silence sits on the floor the loud utterance set


def test_whisper_log_mel_past_the_default_lds_window(backend):
    """n_fft 1024 (hop 256): about 82 KiB of dynamic LDS through the Whisper entry, reflect padding included."""
    nat, dev = backend
    from speechbrain_amd.integrations.huggingface.whisper import WhisperLogMel

    fe = WhisperLogMel(n_mels=80, n_fft=1024, hop_length=256).to(dev)
    N = 256 * 9 + 5
    g = torch.Generator().manual_seed(1024)
    wav = torch.stack([0.5 * torch.randn(N, generator=g), 1e-3 * torch.randn(N, generator=g)])
    out = fe.log_mel_spectrogram(wav.to(dev)).cpu()
    ref = ref_whisper_log_mel(wav, fe._mel_filters.cpu(), 1024, 256)
    assert out.shape == (2, 80, 9) == tuple(ref.shape)
    assert _seen("whisper n_fft=1024", dev, _md(out, ref)) <= 2e-4


def test_whisper_log_mel_refuses_too_short(backend):
    nat, dev = backend
    from speechbrain_amd.integrations.huggingface.whisper import WhisperLogMel

    fe = WhisperLogMel(n_mels=80).to(dev)
    with pytest.raises(nat.SbkError, match="reflect padding needs"):
        fe.log_mel_spectrogram(torch.randn(1, 200).to(dev))


# ------------------------------------------------------------------------------------------- 8. refusals
def test_refusals_launch_nothing(backend):
    """Unsupported configurations are errors raised before any launch: the profiler (which records the front-end's
    launches under "fbank" / "whisper_log_mel") has seen none afterwards."""
    nat, dev = backend
    from speechbrain_amd.lobes.features import Fbank
    from speechbrain_amd.processing.features import STFT, FbankFrontend

    with pytest.raises(ValueError, match="prime factor"):
        FbankFrontend(n_fft=14, win_length=0.5)
    with pytest.raises(ValueError, match="prime factor"):
        STFT(sample_rate=16000, n_fft=14, win_length=0.5)
    with pytest.raises(ValueError, match="longer than n_fft"):
        FbankFrontend(n_fft=400, win_length=32)
    with pytest.raises(ValueError, match="longer than n_fft"):
        STFT(sample_rate=16000, n_fft=400, win_length=32)
    with pytest.raises(ValueError, match="longer than n_fft"):
        Fbank(n_fft=400, win_length=32)

    wav = torch.randn(2, 2000, generator=torch.Generator().manual_seed(8)).to(dev)
    nat.prof_reset()
    nat.prof_enable(True)
    try:
        big = FbankFrontend(n_fft=2048, win_length=128, n_mels=80).to(dev)
        lds = 2048 * 8 + 4 * 2 * 2048 * 8 + 4 * 1025 * 4 + big.mel_w.numel() * 4 + 16
        with pytest.raises(nat.SbkError, match=f"needs {lds} B of LDS"):
            big(wav)
        with pytest.raises(nat.SbkError, match=f"needs {lds - big.mel_w.numel() * 4} B of LDS"):
            STFT(sample_rate=16000, n_fft=2048, win_length=128).to(dev)(wav)
        fe = FbankFrontend(n_fft=400, n_mels=40).to(dev)
        with pytest.raises(nat.SbkError, match="both mean and std"):
            fe(wav, norm_mean=torch.zeros(40, device=dev))
        with pytest.raises(nat.SbkError, match="both mean and std"):
            fe(wav, norm_std=torch.ones(40, device=dev))
        assert not {"fbank", "whisper_log_mel"} & set(nat.prof_report())
        fe(wav)  # ... and the probe itself works: a launch that happens is seen
        assert nat.prof_report()["fbank"]["count"] == 1
    finally:
        nat.prof_enable(False)
        nat.prof_reset()


# ------------------------------------------------------------------------------------------- 9. log_softmax
def _ref_log_softmax(x, temperature, weight):
    # temperature and weight cross the C ABI as fp32
    t, w = (float(torch.tensor(v, dtype=torch.float32)) for v in (temperature, weight))
    return w * torch.log_softmax(x.double() / t, dim=-1)


@pytest.mark.parametrize("rows,V", [(3, 1), (5, 31), (2, 257), (4, 1025), (1, 5000), (2, 70000)])
@pytest.mark.parametrize("temperature,weight", [(1.0, 1.0), (0.7, 1.0), (2.0, 0.5), (0.7, 0.5)])
def test_log_softmax_vs_float64(backend, rows, V, temperature, weight):
    """weight * log_softmax(x / temperature) vs float64: inputs of scale 8, per row one -inf entry and one entry 10
    above the rest (V > 1).  Finite entries within 1e-5, -inf stays -inf, exp(out / weight) sums to 1 within 1e-5."""
    nat, dev = backend
    x = 8.0 * torch.randn(rows, V, generator=torch.Generator().manual_seed(V))
    if V > 1:
        for r in range(rows):
            x[r, (5 * r + 3) % V] = float(x[r].max()) + 10.0
            x[r, (5 * r + 4) % V] = -math.inf
    ref = _ref_log_softmax(x, temperature, weight)
    out = nat.log_softmax(x.to(dev), temperature, weight).cpu()
    assert out.shape == x.shape
    inf = torch.isinf(x)
    assert torch.all(out[inf] == -math.inf) and torch.all(torch.isfinite(out[~inf]))
    err = float((out.double() - ref)[~inf].abs().max())
    assert _seen(f"log_softmax {rows}x{V} T={temperature} w={weight}", dev, err) <= 1e-5
    total = torch.exp(out.double() / float(torch.tensor(weight, dtype=torch.float32))).sum(-1)
    assert float((total - 1.0).abs().max()) <= 1e-5


@pytest.mark.parametrize("V", [1, 257, 70000])
def test_log_softmax_all_equal_row(backend, V):
    """A constant row is -log(V) * weight, the same bits in every column, whatever the constant and the temperature."""
    nat, dev = backend
    x = torch.stack([torch.full((V,), 3.25), torch.full((V,), -40.0)])
    out = nat.log_softmax(x.to(dev), 0.7, 0.5).cpu()
    assert _seen(f"log_softmax all-equal V={V}", dev, float((out.double() + 0.5 * math.log(V)).abs().max())) <= 1e-5
    assert torch.all(out == out[:, :1])


# ------------------------------------------------------------------------------------------- 10. masked global norm
@pytest.mark.parametrize("C", [23, 80, 257])
def test_input_norm_global_masked(backend, C):
    """Called directly: n_valid of 0, T and in between; frames from n_valid[b] on come back bit-equal to the input,
    valid frames are (x - mean) / max(std, eps) within 1e-5 relative to float64 (std entries under eps included)."""
    nat, dev = backend
    B, T, eps = 4, 7, 1e-3
    g = torch.Generator().manual_seed(C)
    x = 20.0 * torch.randn(B, T, C, generator=g) - 40.0
    mean = torch.linspace(-60, -20, C)
    std = torch.linspace(5, 15, C)
    std[0], std[C // 2] = 0.0, 1e-5
    n_valid = torch.tensor([0, T, 3, T - 1], dtype=torch.int32)
    out = nat.input_norm_global_masked(x.to(dev), mean.to(dev), std.to(dev), n_valid.to(dev), eps).cpu()
    ref = (x.double() - mean.double()) / torch.clamp(std.double(), min=eps)
    valid = torch.arange(T)[None, :] < n_valid[:, None]
    assert out.shape == x.shape
    assert torch.equal(out[~valid].view(torch.int32), x[~valid].view(torch.int32))
    rel = (out.double() - ref).abs()[valid] / ref.abs()[valid].clamp(min=1e-30)
    assert _seen(f"input_norm_global_masked C={C} (relative)", dev, float(rel.max())) <= 1e-5
