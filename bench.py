#!/usr/bin/env python
"""bench.py -- audio-sec/s of the EncoderDecoderASR hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR   # + the timed region's token ids as DIR/*.npy
    python bench.py --gpus 1 --steps 20 --warmup 5 --full   # + the secondary measurements (below), several minutes more
    python bench.py --gpus 8 --steps 20 --warmup 5      # spawns 8 ranks itself (torch.distributed.run, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...   # same thing

Workload (BASELINE.json configs[2] / SURVEY 8d config 3): Conformer-L (d 512, 12 enc / 6 dec layers, 5000
tokens, RelPosMHAXL), beam 10 + CTC weight 0.4 (the recipe's valid_search), seeded random weights, synthetic
16 kHz audio (0.1*randn stored as 16-bit PCM, like a wav file), utterance durations U(5,30) s (seed 1234).
Random weights never emit EOS, so the number of decoding steps is fixed through max_decode_ratio to
round(4 tokens/s * padded seconds).  fp32 arithmetic throughout.

One "step" = 128 utterances through the whole path, as duration-sorted RECIPE-SIZED batches of at most 32
utterances ("duration-sorted batches of <= 32 utts"); `value` is measured on those.  With --full the same
utterances are then run again as 128-utterance batches (sized for 288 GB of HBM) and reported as
`value_batch128`.  Per rank the batches run through ConcurrentTranscriber: --streams worker threads (encoder on a
normal-, search on a high-priority HIP stream), each encoding --group batches one after the other and decoding them
in ONE grouped search (every batch keeps its own padding and step limits; the decoder step sees all their rows);
with --group-encoder the Conformer encoder likewise runs once over the rows of the group's batches (measured: no gain).

The timed region is the real sharded path (speechbrain_amd.inference.sharded.ShardedTranscriber): rank 0 holds the
whole job as int16 PCM waveforms in host memory; the clock covers planning (duration sort, bucketing, longest-processing-
time-first assignment), the padding of every batch into pinned staging memory (streamed behind the first batches' compute),
host->device copies, the scatter of every other rank's share (streamed: one point-to-point send per batch over the
peer's xGMI link, so a rank starts on its first batch while the rest is on its way), PCM->float,
Fbank -> norm -> CNN -> Conformer encoder -> beam search on every rank, and the gather of the token ids to rank 0
(token-id lists on the host).  With --gpus N each rank gets K steps of work (weak scaling): the job is N*K*128
utterances.  At N = 1 the same code runs without the two exchanges.

With --job-utts N the job is FIXED at N utterances shared by the ranks (strong scaling, BASELINE.json configs[3]);
"rccl_world" and "per_rank" (every rank's wall time, audio seconds and batches) make a scaling run auditable.
"determinism_check": the token ids of the timed region (eight concurrent workers, grouped searches) against the same
batches in the same groups run sequentially on one worker stream afterwards.  "parity_check": >= 256 utterances of the
job through the headline's execution mode against PLAIN main-thread asr.transcribe_batch calls on the same padded batches
(output heads x8 on both sides: the grouped search runs the decode GEMMs at other row counts, and flat random-init
posteriors would turn any fp32 reassociation into a token flip).  The searches keep the product's stop rule (polled
asynchronously every 8 steps).

"value_fp32_mfma_contractions": the same job with every contraction on the fp32 MFMA instruction (the headline's large
contractions run on the bf16 matrix pipe through the exact three-way operand split), for reference.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line; everything else it can measure
(secondary_measurements) runs only with --full: the secondary legs, the checks, the latency modes, the roofline objects and
the CPU baseline.

One JSON line on rank 0: metric / value (total unpadded audio seconds / max-over-ranks wall time); with --full also
"roofline" (dominant kernel; HIP-event timing of every launch during an instrumented single-stream repetition of
the same batches), "roofline_top3", "roofline_end_to_end", "cpu_baseline" (the oracle port of the reference's
PyTorch-CPU path on B = 4 x 10 s, BASELINE.md section 3's CPU shape; child process with a timeout and a smaller
fall-back slice), the token error rate of the HIP path against the oracle on that slice, p50 single-utterance latency and configs[1] (Conformer-S encoder).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_MFMA_F32_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
# the fp32 contractions that run on the bf16 matrix pipe (csrc/gemm.hip, gemm_nt_f32x3: exact three-way operand split, six
# bf16 MFMAs per fp32-equivalent multiply-add) are priced against the dense bf16 MFMA peak / 6
PEAK_MFMA_BF16_TFLOPS = 2500.0
PEAK_F32X3_TFLOPS = PEAK_MFMA_BF16_TFLOPS / 6.0
PEAK_HBM_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E spec peak
MFMA_KERNELS = ("gemm", "relpos_attention", "rope_attention")
TOKENS_PER_SECOND = 4.0
SR = 16000
UTTS_PER_STEP = 128
GROUP_ENCODER_DEFAULT = 1000  # batches per encoder pass of a worker's group (0 = one pass per batch, 1000 = the whole group = the product's default)
PMC_ROUND = 6  # the round whose rocprofv3 --pmc rows in profiles/pmc_traffic.json describe the kernels as shipped


# ------------------------------------------------------------------ synthetic job
def make_job(n_utts, seed=1234, lo=5.0, hi=30.0):
    """`n_utts` utterances of 16-bit PCM, durations U(lo,hi) s: list of 1-D int16 tensors (views of one noise
    pool -- the content of an utterance does not matter for timing, its length does) + their seconds."""
    g = torch.Generator().manual_seed(seed)
    n = ((lo + (hi - lo) * torch.rand(n_utts, generator=g)) * SR).round().long().tolist()
    pool_len = 1 << 22
    pool = (0.1 * torch.randn(pool_len + int(hi * SR) + 1, generator=g) * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    utts = [pool[(i * 104729) % pool_len:][:n_i] for i, n_i in enumerate(n)]
    return utts, [n_i / SR for n_i in n]


DUMP_BYTES_MAX = 64 << 20


def dump_outputs(path, hyps, seed=0):
    """--dump-outputs: what the timed region returned -- one token-id list per utterance, in job order -- as
    `path`/token_ids.npy (float32, one row per utterance, padded with -1), token_counts.npy (float32) and utterance_index.npy
    (float64, the job index of each row).  When the ids would pass DUMP_BYTES_MAX, the rows are a fixed seeded sample."""
    import numpy as np

    width = max((len(h) for h in hyps), default=0)
    idx = torch.arange(len(hyps))
    rows = (DUMP_BYTES_MAX - 4096) // (4 * width + 4 + 8)  # (4096: the three .npy headers)
    if len(hyps) > rows:
        idx = torch.randperm(len(hyps), generator=torch.Generator().manual_seed(seed))[:rows].sort().values
    idx = idx.tolist()
    ids = np.full((len(idx), width), -1.0, dtype=np.float32)
    for r, i in enumerate(idx):
        ids[r, :len(hyps[i])] = [int(v) for v in hyps[i]]
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "token_ids.npy"), ids)
    np.save(os.path.join(path, "token_counts.npy"), np.array([len(hyps[i]) for i in idx], dtype=np.float32))
    np.save(os.path.join(path, "utterance_index.npy"), np.array(idx, dtype=np.float64))


def frames_after_frontend(n_samples):
    t = 1 + n_samples // 160
    t = (t - 1) // 2 + 1
    return (t - 1) // 2 + 1


def decode_steps_for(n_samples):
    return max(1, int(round(TOKENS_PER_SECOND * n_samples / float(SR))))


def fixed_decode_length(searcher, wavs):
    """`prepare` hook of ConcurrentTranscriber: decode steps = round(4 tok/s * padded seconds)."""
    searcher.max_decode_ratio = (decode_steps_for(wavs.shape[1]) + 0.5) / frames_after_frontend(wavs.shape[1])


def run_step(asr, wav, lens):
    """One batch through the whole path on the current stream (latency case, instrumented pass)."""
    fixed_decode_length(asr.mods.decoder, wav)
    if wav.dtype == torch.int16:
        from speechbrain_amd import native

        wav = native.pcm16_to_f32(wav.to(asr.device, non_blocking=True))
    return asr.transcribe_batch(wav, lens)[1]


def decode_step_probe(asr, dev, frames=430, batches=4, steps=(16, 32)):
    """The decoding step at the headline's shape -- ONE grouped search of `batches` x 32 utterances (T' = 430, 420, ...; beam 10 +
    CTC) from a random encoder output, on one stream: milliseconds and launches per step as the difference of a 32- and a 16-step
    search (the per-search set-up -- memory projection, CTC emissions -- cancels).  Launch counts from the library's per-launch
    profiler (sbk_prof_*), times from the wall clock around synchronised searches without it.  (tools/decode_probe.py is the
    same search for rocprofv3 passes.)"""
    from speechbrain_amd import native

    dec = asr.mods.decoder
    g = torch.Generator().manual_seed(3)
    items = [(torch.randn(32, frames - 10 * k, 512, generator=g).to(dev), torch.linspace(0.85, 1.0, 32).to(dev)) for k in range(batches)]
    res = {}
    with torch.no_grad():
        for n in steps:
            ratios = [(0.0, (n + 0.5) / it[0].shape[1]) for it in items]
            dec.forward_group(items, ratios)  # warm-up (workspaces)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                dec.forward_group(items, ratios)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / 3
            native.prof_reset()
            native.prof_enable(True)
            dec.forward_group(items, ratios)
            torch.cuda.synchronize()
            native.prof_enable(False)
            rep = native.prof_report()
            native.prof_reset()
            res[n] = (ms, sum(v["count"] for v in rep.values()), {k: v["count"] for k, v in rep.items()})
    a, b = steps
    per = {k: round((res[b][2].get(k, 0) - res[a][2].get(k, 0)) / (b - a), 2) for k in res[b][2]}
    return {"decode_step_ms": round((res[b][0] - res[a][0]) / (b - a), 4),
            "launches_per_decode_step": round((res[b][1] - res[a][1]) / (b - a), 2),
            "launches_per_decode_step_by_kernel": {k: v for k, v in sorted(per.items(), key=lambda kv: -kv[1]) if v > 0},
            "shape": f"{batches} x 32 utterances, T' {frames}..{frames - 10 * (batches - 1)}, beam 10 + CTC, one stream; difference of a {b}- and a {a}-step search"}


def x3r_per_shape(dev, rows=1280, iters=40):
    """The dominant kernel shape by shape: the few-row split-operand projection at the row count of the
    headline's grouped searches, back-to-back launches between two HIP events on the current stream (weights L2-warm: the
    in-situ figure of the line's `roofline` is lower, every launch of a decoding step meeting cold operands)."""
    from speechbrain_amd import native

    out = []
    with torch.no_grad():
        for (N, K, what) in ((512, 512, "out-projections, q projection"), (1536, 512, "self-attention in_proj"), (2048, 512, "ffn.0"),
                             (512, 2048, "ffn.3"), (5000, 512, "seq_lin")):
            a = torch.randn(rows, K, device=dev)
            w = torch.randn(N, K, device=dev)
            r = torch.randn(rows, N, device=dev)
            for _ in range(3):
                native.gemm_nt_x3r(a, w, residual=r)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                native.gemm_nt_x3r(a, w, residual=r)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / iters
            tf = 2.0 * rows * N * K / us / 1e6
            out.append({"M": rows, "N": N, "K": K, "what": what, "us": round(us, 1), "tflops": round(tf, 1), "frac": round(tf / PEAK_F32X3_TFLOPS, 4)})
    return out


# ------------------------------------------------------------------ CPU leg (oracle port)
def cpu_threads():
    """Host threads for the CPU leg: the cores this process may run on, capped at 32 (the port's
    small per-frame ops stop scaling long before that and oversubscription only hurts)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 32))


def cpu_sample(kind="4x10s"):
    """The CPU leg's slice of the workload.  "4x10s": four 10-second utterances of the job's noise (BASELINE.md
    section 3 sized the CPU leg on B = 4 x 10 s, 40 decoding steps); "2shortest": the 2 shortest utterances of the
    first step's 128 (the fallback when the first does not finish in time)."""
    from speechbrain_amd.inference.sharded import pad_batch

    if kind == "4x10s":
        utts, _ = make_job(4, lo=10.0, hi=10.0)
        idx = [0, 1, 2, 3]
    else:
        utts, _ = make_job(UTTS_PER_STEP)
        idx = sorted(range(len(utts)), key=lambda i: (utts[i].numel(), i))[:2]
    x, lens = pad_batch(utts, idx)
    return x.float() / 32768.0, lens


def cpu_baseline_subprocess(timeouts=(("4x10s", 420), ("2shortest", 200))):
    """Run the CPU leg in a child process so that a slow host can never stall the GPU result: B = 4 x 10 s first,
    the 2-shortest-utterances slice if that does not finish in time."""
    fail = {"value": None, "unit": "audio-sec/s", "cores": cpu_threads(), "kind": "port"}
    notes = []
    for kind, timeout_s in timeouts:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-baseline-only", "--cpu-sample", kind],
                               capture_output=True, text=True, timeout=timeout_s)
            for line in reversed(r.stdout.splitlines()):
                if line.startswith("{"):
                    d = json.loads(line)
                    d["sample_kind"] = kind
                    if notes:
                        d["sample"] += " (" + "; ".join(notes) + ")"
                    return d
            notes.append(f"{kind}: CPU leg failed: " + (r.stderr.strip().splitlines() or ["no output"])[-1][:160])
        except subprocess.TimeoutExpired:
            notes.append(f"{kind}: did not finish within {timeout_s} s")
    return {**fail, "sample": "; ".join(notes)}


REFERENCE_ROOT = os.environ.get("SBK_BENCH_REFERENCE", "")  # opt-in: a checkout of the reference (unset: the oracle port, kind "port")


def _reference_runner(sd, steps, n_samples):
    """The reference's OWN modules (speechbrain.lobes.features.Fbank, ConvolutionFrontEnd, TransformerASR,
    S2STransformerBeamSearcher + CTCScorer) with the same weights, when SBK_BENCH_REFERENCE names a checkout of the reference."""
    if not REFERENCE_ROOT or not os.path.isdir(os.path.join(REFERENCE_ROOT, "speechbrain")):
        return None
    for pth in (REFERENCE_ROOT, os.path.join(ROOT, "oracle", "ref_stubs")):
        if pth not in sys.path:
            sys.path.insert(0, pth)
    from oracle.make_golden import build_reference
    from speechbrain.decoders import S2STransformerBeamSearcher
    from speechbrain.decoders.scorer import CTCScorer, ScorerBuilder
    from speechbrain.lobes.features import Fbank

    mods = build_reference(512, 8, 2048, 12, 6, 5000, 0)
    missing = mods.load_state_dict({k: v for k, v in sd.items() if k in mods.state_dict()}, strict=False)
    assert not missing.missing_keys, missing.missing_keys[:4]
    fb = Fbank(sample_rate=SR, n_fft=512, n_mels=80, win_length=32)
    scorer = ScorerBuilder(full_scorers=[CTCScorer(ctc_fc=mods["ctc_lin"], blank_index=0, eos_index=2)], weights={"ctc": 0.4})

    def run(w, l, ratio):
        bs = S2STransformerBeamSearcher(modules=[mods["Transformer"], mods["seq_lin"]], bos_index=1, eos_index=2,
                                        min_decode_ratio=0.0, max_decode_ratio=ratio, beam_size=10, using_eos_threshold=False,
                                        length_normalization=True, scorer=scorer)
        with torch.no_grad():
            enc = mods["Transformer"].encode(mods["CNN"](fb(w)), l)
            return bs(enc, l)[0]

    return run


def cpu_baseline(kind="4x10s", budget_s=240.0):
    """The CPU leg: the reference's own modules when SBK_BENCH_REFERENCE names them (kind "reference"), else the oracle port of
    the reference's CPU path (kind "port": no KV cache, Python-loop CTC scorer -- the reference's algorithm restated).
    One cheap warm-up (a 1-second batch: thread pools, oneDNN primitives), then best of 3 timed runs of the sample (fewer
    only when `budget_s` runs out).  With the 4 x 10 s sample it also decodes 12 x 10 s ONCE with the output heads x8 --
    3 012 encoder rows, the shape class where the encoder contractions take the split-operand kernel -- for the bench's
    token-error-rate comparison of the HIP path against the oracle."""
    from oracle import sb_oracle as O
    from speechbrain_amd.inference.builders import build_asr, flat_state_dict

    torch.set_num_threads(cpu_threads())
    sd = flat_state_dict(build_asr("L", vocab=5000, seed=0, device="cpu"))
    fc = O.FbankCfg(n_fft=512, n_mels=80, win_length_ms=32)
    mc = O.ModelCfg()
    wav, lens = cpu_sample(kind)
    seconds = float((lens * wav.shape[1]).sum()) / SR
    steps = decode_steps_for(wav.shape[1])
    ratio = (steps + 0.5) / frames_after_frontend(wav.shape[1])
    ref_run = _reference_runner(sd, steps, wav.shape[1])

    def run(w, l, r, sdict=sd):
        if ref_run is not None and sdict is sd:
            return ref_run(w, l, r)
        with torch.no_grad():
            enc = O.encode_batch(w, l, sdict, fc, mc, torch.zeros(80), torch.ones(80))
            return O.beam_search(enc, l, sdict, mc, O.SearchCfg(beam=10, ctc_weight=0.4, max_decode_ratio=r))[0]

    run(wav[:2, :SR].contiguous(), torch.ones(2), 4.5 / frames_after_frontend(SR))
    times, hyps, t_start = [], None, time.time()
    while len(times) < 3 and (not times or time.time() - t_start + min(times) < budget_s):
        t0 = time.time()
        hyps = run(wav, lens, ratio)
        times.append(time.time() - t0)
    best = min(times)
    what = ("4 utterances of 10 s (BASELINE.md section 3's CPU shape)" if kind == "4x10s"
            else "2 shortest utterances of the job's first step")
    out = {"value": round(seconds / best, 3), "unit": "audio-sec/s", "cores": torch.get_num_threads(),
           "kind": "reference" if ref_run is not None else "port",
           "sample": f"{what}: {seconds:.1f} audio-s, padded to {wav.shape[1] / SR:.2f} s, "
                     f"Conformer-L beam 10 + CTC 0.4, {steps} decode steps, "
                     + ("the reference's own modules from SBK_BENCH_REFERENCE" if ref_run is not None else "oracle/sb_oracle.py")
                     + f" (torch-CPU fp32); 1-second warm-up batch + best of {len(times)} ({', '.join(f'{t:.1f}' for t in times)} s)",
           "tokens": [list(map(int, h)) for h in hyps]}
    if kind == "4x10s":  # the parity sample: 12 x 10 s, peaked heads, the oracle once
        w12, l12 = parity_sample()
        sd8 = dict(sd)
        for k in ("seq_lin.w.weight", "ctc_lin.w.weight"):
            sd8[k] = sd[k] * 8.0
        t0 = time.time()
        out["tokens_12x10s_heads_x8"] = [list(map(int, h)) for h in run(w12, l12, ratio, sd8)]
        out["parity_sample_s"] = round(time.time() - t0, 1)
    return out


def parity_sample():
    """12 utterances of 10 s of the job's noise, relative lengths 0.6 .. 1 (the padded-frame masks are exercised)."""
    from speechbrain_amd.inference.sharded import pad_batch

    utts, _ = make_job(12, lo=10.0, hi=10.0)
    x, _ = pad_batch(utts, list(range(12)))
    x = x.float() / 32768.0
    lens = torch.linspace(0.6, 1.0, 12)
    for i in range(12):
        x[i, int(lens[i] * x.shape[1]):] = 0
    return x, lens


# ------------------------------------------------------------------ launch helpers
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n):
    """`python bench.py --gpus N` without a rendezvous in the environment: one rank per GPU over RCCL."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def whisper_encoder_leg(dev, B=8, reps=3):
    """log-mel + Whisper encoder (large-v3 shape: 128 mels, 32 layers, d 1280, 20 heads, ffn 5120) on B x 30 s of audio;
    fp32 and the opt-in bf16 GEMM operands."""
    from speechbrain_amd import native
    from speechbrain_amd.integrations.huggingface.whisper import Whisper

    cfg = dict(num_mel_bins=128, d_model=1280, encoder_layers=32, encoder_attention_heads=20, encoder_ffn_dim=5120,
               max_source_positions=1500, decoder_layers=0, decoder_attention_heads=20, decoder_ffn_dim=5120,
               vocab_size=51866, max_target_positions=448)
    from speechbrain_amd.inference.ASR import WhisperASR

    w = Whisper.from_config(cfg, encoder_only=True).to(dev).eval()
    wav = 0.1 * torch.randn(B, 480000, generator=torch.Generator().manual_seed(3))
    wav = wav.to(dev)
    lens = torch.ones(B)

    def interface(prec):  # BASELINE configs[4] "via speechbrain.inference": the precision is the interface's run_opts
        return WhisperASR(modules={"whisper": w, "decoder": torch.nn.Identity()},
                          hparams={"language": "en", "sample_rate": 16000, "whisper": w}, run_opts={"device": str(dev), "precision": prec})

    res = {"workload": f"WhisperASR(run_opts precision=...).encode_batch = log-mel + Whisper large-v3 encoder forward, {B} x 30 s, random weights, one stream",
           "precisions": "operand type of the GEMMs (fp32 accumulation everywhere): fp32 = parity path; bf16 = bf16 activations "
                         "between the contractions (LayerNorm / attention / GELU epilogue write bf16, LDS-DMA bf16 GEMM, "
                         "attention with K / V^T tiles shared through LDS; residual stream fp32); fp8 = e4m3 activations between the "
                         "contractions too (round 4: LayerNorm writes fp8 rows with one scale per row, weights with one scale per "
                         "output channel, q/k/v projection and the feed-forward pair on v_mfma_f32_32x32x64_f8f6f4 -- the 2 x-rate fp8 "
                         "instruction -- attention and its out-projection on bf16 rows); fp16 reads fp32 activations and rounds them "
                         "on load; fp8_fp32_activations = the round-3 fp8 path (per-tensor scales, activation max |x| per GEMM).  Round 6: the bf16 / fp8 "
                         "contractions at these shapes run on 256 x 256 tiles (csrc/gemm_lp256.hip: bit-identical to the 128 x 128 kernels), "
                         "the bf16 attention computes its softmax in base 2 on one v_exp_f32 per score, the GELU of the reduced-precision "
                         "epilogues is erfc by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7; the fp32 path keeps libm's erff)"}
    flops = B * 32 * (1500 * 2.0 * (4 * 1280 * 1280 + 2 * 1280 * 5120) + 4.0 * 1500 * 1500 * 1280) \
        + B * 2.0 * (3000 * 1280 * 384 + 1500 * 1280 * 3840)
    ref = None
    for prec in ("fp32", "bf16", "fp16", "fp8", "fp8_fp32_activations"):
        native.FP8_ACTIVATIONS = prec != "fp8_fp32_activations"
        asr_w = interface(prec.split("_")[0])
        with torch.no_grad():
            out = asr_w.encode_batch(wav, lens)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                asr_w.encode_batch(wav, lens)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) / reps
        res[prec] = {"ms_per_batch": round(1000.0 * dt, 2), "audio_sec_per_s": round(B * 30.0 / dt, 1),
                     "tflops": round(flops / dt / 1e12, 1)}
        if ref is None:
            ref = out
        else:  # (32 layers: the tolerance tests/test_full_size_gpu.py asserts at this depth)
            res[prec]["relative_rms_vs_fp32"] = round(float((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), 5)
        del out
    native.FP8_ACTIVATIONS = True
    del ref
    del w
    torch.cuda.empty_cache()
    return res


def launch_check(args, rank, world):
    """The launch / exchange plumbing of a measurement without the GPU: same self-launch, same job, same
    ShardedTranscriber calls; the per-rank transcriber is a stand-in that derives tokens from each waveform."""
    import torch.distributed as dist

    from speechbrain_amd.inference.sharded import ShardedTranscriber

    if world > 1:
        dist.init_process_group("gloo")

    def stand_in(wavs, lens):
        return [[int(round(float(l) * w.numel())) % 1000, int(w[0]) % 997] for w, l in zip(wavs, lens)]

    n_utts = args.job_utts if args.job_utts > 0 else world * args.steps * UTTS_PER_STEP
    # (durations a tenth of the measured job's -- 0.5-3 s instead of 5-30 s -- so that 10 000 utterances fit a CPU test:
    # the plan, the number of batches, their owners and the message pattern are those of the real job)
    job, seconds = make_job(n_utts, lo=0.5, hi=3.0) if rank == 0 else (None, None)
    if rank == 0:  # (float32 copies: widening int16 PCM is a kernel of the GPU path)
        job = [w.float() for w in job]
    st = ShardedTranscriber(stand_in, "cpu", max_utts=args.max_batch)
    t0 = time.perf_counter()
    local = st.distribute(st.plan(job))
    hyps = st.gather(st.run_local(local))
    dt = time.perf_counter() - t0
    if rank == 0:
        assert hyps == [[w.numel() % 1000, int(w[0]) % 997] for w in job], "gathered hypotheses do not match the job"
        from speechbrain_amd.inference.sharded import batch_cost

        n = [w.numel() for w in job]
        loads = [sum(batch_cost(n, st.last_plan["batches"][b]) for b in o) for o in st.last_plan["owner"]]
        print(json.dumps({"launch_check": True, "n_gpus": world, "steps": args.steps, "utterances_total": n_utts,
                          "batches_total": len(st.last_plan["batches"]), "bytes_scattered": st.last_plan["bytes_sent"],
                          "ranks_with_work": sum(1 for o in st.last_plan["owner"] if o),
                          "plan_max_over_mean_cost": round(max(loads) / (sum(loads) / len(loads)), 4),
                          "seconds": round(dt, 3)}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def pmc_traffic(name, roof, path=None):
    """HBM bytes per launch of kernel class `name` from the PMC counters, collected in their own rocprofv3 --pmc passes
    (tools/run_pmc_r5.sh -> profiles/pmc_traffic.json); fills roof's traffic_note / traffic_provenance / mfma_busy_pmc.  None when
    there is no row of THIS round's kernel, or when the row was counted before a later change of the kernel's schedule (then the
    note quotes it)."""
    pmc = json.load(open(path or os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    traffic = None
    key = next((k for k in pmc if not k.startswith("_") and name.startswith(k)), None)
    if key and pmc[key].get("round") == PMC_ROUND:  # (a row collected on an earlier round's kernel is not this kernel's traffic)
        if pmc[key].get("superseded"):
            roof["traffic_note"] = (f"not measured for the kernel as shipped -- {pmc[key]['superseded']}; the superseded row: "
                                    f"{pmc[key]['bytes_per_launch']} B/launch against {pmc[key]['algorithmic_bytes_per_launch']} algorithmic")
        else:
            traffic = pmc[key]["bytes_per_launch"]
            roof["traffic_note"] = f"{pmc[key]['note']}; algorithmic {pmc[key]['algorithmic_bytes_per_launch']} B/launch"
        roof["traffic_provenance"] = {"source": "profiles/pmc_traffic.json: rocprofv3 --pmc passes of THIS round's kernel in their own runs "
                                                "(counters cannot be read inside a timing run; tools/run_pmc_r6.sh)",
                                      "commit": pmc[key].get("commit"), "shape": pmc[key].get("shape"),
                                      "collected": pmc[key].get("collected")}
    busy = {k: v["mfma_busy"] for k, v in pmc.get("_mfma_busy", {}).items()
            if not k.startswith("_") and k.startswith(name) and v.get("round") == PMC_ROUND}
    if busy:  # SQ_VALU_MFMA_BUSY_CYCLES / (SIMDs x active cycles), from its own --pmc pass
        roof["mfma_busy_pmc"] = busy
    return traffic


def pmc_decode_row(name, path=None):
    """The fabric-counter row of one of the decode step's memory-bound kernels (profiles/pmc_traffic.json: decode_memory_bound_rNN of THIS
    round: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over tools/decode_probe.py), or None."""
    try:
        pmc = json.load(open(path or os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    except Exception:
        return None
    sec = pmc.get(f"decode_memory_bound_r{PMC_ROUND:02d}", {})
    row = sec.get(name)
    if not isinstance(row, dict) or "bytes_per_launch" not in row:
        return None
    out = {"traffic": row["bytes_per_launch"], "traffic_shape": "4 x 32 utterances, T' 430..400, beam 10 + CTC (tools/decode_probe.py), one stream",
           "traffic_source": sec.get("_source", "")[:160]}
    if row.get("algorithmic_bytes_per_launch"):
        out["traffic_over_algorithmic"] = round(row["bytes_per_launch"] / row["algorithmic_bytes_per_launch"], 3)
    return out


def roofline_entry(name, v, total_ms):
    avg_ms = v["ms"] / max(v["count"], 1)
    if name.startswith(MFMA_KERNELS):
        ach = v["flops"] / (v["ms"] * 1e-3) / 1e12
        x3 = name.startswith(("gemm_nt_f32x3", "gemm_nt_x3p", "gemm_x3r"))  # six bf16 partial products per multiply-add: bf16 peak / 6
        peak = PEAK_F32X3_TFLOPS if x3 else PEAK_MFMA_F32_TFLOPS
        e = {"kernel": name, "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
             "frac": round(ach / peak, 4)}
        if x3:
            e["frac_of_fp32_mfma_peak"] = round(ach / PEAK_MFMA_F32_TFLOPS, 4)  # what the fp32-MFMA kernel it replaced was priced against
            e["peak_note"] = ("fp32-equivalent: 2*M*N*K flops per launch; the kernel forms six bf16 partial products per multiply-add on "
                              "v_mfma_f32_32x32x16_bf16, so its ceiling is the dense bf16 MFMA peak (2 500 TF/s) / 6; "
                              f"against the fp32 MFMA peak ({PEAK_MFMA_F32_TFLOPS}) the same rate is {ach / PEAK_MFMA_F32_TFLOPS:.2f}")
    else:
        ach = v["bytes"] / (v["ms"] * 1e-3) / 1e9
        e = {"kernel": name, "bound": "hbm", "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
             "frac": round(ach / PEAK_HBM_GBS, 4)}
    e.update({"launches": v["count"], "avg_launch_ms": round(avg_ms, 4), "share_of_gpu_time": round(v["ms"] / total_ms, 3)})
    if e["bound"] == "hbm":
        row = pmc_decode_row(name)
        if row:
            e.update(row)
    return e


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=16, help="steps per GPU; one step = 128 utterances")
    ap.add_argument("--warmup", type=int, default=4,
                    help="untimed steps through the same path before the clock starts (communicators, allocator pools, and the "
                         "box itself: the first bench process on a fresh box measured 5-7 %% below the following ones with one "
                         "warm-up step, profiles/r04_j_*, r04_k_*, r04_l_*)")
    ap.add_argument("--max-batch", type=int, default=32, help="utterances per batch of the headline run (32 = recipe-sized)")
    ap.add_argument("--second-batch", type=int, default=128, help="batch size of the second timed run (0: skip; N = 1 only)")
    ap.add_argument("--streams", type=int, default=0, help="worker threads per GPU, each with a batch (or a group of batches) in flight (0: automatic)")
    ap.add_argument("--group", type=int, default=0,
                    help="batches decoded together in one grouped search per worker (0: automatic -- enough recipe-sized "
                         "batches to give the decoder step ~256 utterances)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="arithmetic of the headline run: fp32 = the parity path (default); bf16 = bf16 operands / fp32 "
                         "accumulation in the encoder GEMMs (opt-in fast path; reported as a secondary value otherwise)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip configs[1] (Conformer-S encoder) and the second run")
    ap.add_argument("--latency-runs", type=int, default=5)
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--leg", default="", choices=["", "batch128", "bf16", "fp32mfma", "latency"], help=argparse.SUPPRESS)  # child process of a secondary leg
    ap.add_argument("--leg-out", default="", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-sample", default="4x10s", choices=["4x10s", "2shortest"], help=argparse.SUPPRESS)
    ap.add_argument("--job-utts", type=int, default=0,
                    help="STRONG scaling: a fixed job of this many utterances shared by all the ranks (BASELINE.json "
                         "configs[3]: 10000), instead of --steps x 128 utterances per rank (weak scaling, the default)")
    ap.add_argument("--check-every", type=int, default=-1,
                    help="stop-rule polling interval of the searches (-1: the product default, 8 steps; 0: never poll)")
    ap.add_argument("--attention", default="RelPosMHAXL", choices=["RelPosMHAXL", "RoPEMHA"],
                    help="encoder attention (RelPosMHAXL = BASELINE.json's config; RoPEMHA = the in-tree recipe)")
    ap.add_argument("--lm", action="store_true",
                    help="add the recipe's TransformerLM scorer (12 x 768, weight 0.6, T=1.15): test_search at beam 10")
    ap.add_argument("--group-encoder", type=int, default=-1, nargs="?", const=1000, metavar="BATCHES",
                    help="one encoder pass over the rows of up to BATCHES batches of a group (no value: all of them) instead of one "
                         "per batch; 0: one pass per batch; default: GROUP_ENCODER_DEFAULT)")
    ap.add_argument("--overlap-ctc", type=int, default=-1,
                    help="A/B: overlap_ctc bit mask of the workers' searches (default: 0 with several workers)")
    ap.add_argument("--graph-mode", type=int, default=0, choices=[0, 1, 2],
                    help="searches of the timed run: 1 = decoding steps replayed from a captured hipGraph, 2 = device-side "
                         "step counter with plain launches (A/B; 0 = plain launches)")
    ap.add_argument("--no-search-priority", action="store_true",
                    help="run each worker's search on its normal-priority stream (A/B of the stream priorities)")
    ap.add_argument("--knob", action="append", default=[], metavar="KEY=VALUE",
                    help="tuning switch passed to sbk_prof_set_knob (A/B measurements only)")
    ap.add_argument("--launch-check", action="store_true",
                    help="no GPU work: launch the N ranks exactly as a measurement would (gloo instead of RCCL), push the "
                         "synthetic job through plan -> streamed scatter -> a stand-in transcriber -> gather and print the "
                         "line with n_gpus = N.  What tests/test_distributed.py runs on CPU")
    ap.add_argument("--prof-concurrent", action="store_true",
                    help="measurement runs only (the value is then that of an INSTRUMENTED run): HIP events around every launch "
                         "of the timed region itself -- per kernel class the time its launches took with the other workers' "
                         "kernels co-resident, and the mean number of kernels in flight (sum of those times / wall clock); "
                         "rocprofv3 serialises the launch path of several threads and cannot show this regime (DESIGN.md section 6)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed region, write the token ids it returned to DIR/*.npy (dump_outputs): the inputs are "
                         "seeded, so two builds run with the same arguments can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the secondary measurements (secondary_measurements): other batch sizes and "
                         "precisions in processes of their own, latency modes, the Whisper encoder, the instrumented repetition "
                         "(roofline, determinism_check, decode step probe), parity_check, configs[1] and the CPU baseline.  "
                         "Without it a run sets up, warms up, times the steps, writes --dump-outputs and prints the line")
    ap.add_argument("--verbose", action="store_true")
    return ap.parse_args(argv)


def secondary_measurements(args, rank, world, dist_on):
    """What a run measures besides the headline.  A plain run measures nothing else; --full adds every secondary measurement
    that its own --no-* switch, the rank and the world size allow (the fp32-MFMA leg also needs the split-operand contractions
    to be on, which only the loaded library can tell)."""
    if not args.full or rank != 0:
        return set()
    todo = set()
    if world == 1 and not dist_on and not args.no_extras:
        if args.second_batch > 0:
            todo.add("batch128")
        if args.precision == "fp32":
            todo |= {"bf16", "fp32mfma"}
    if args.latency_runs > 0:
        todo.add("latency")
    if world == 1 and not args.no_extras:
        todo |= {"whisper_encoder", "config1_encoder_S"}
    if not args.no_roofline:
        todo |= {"roofline", "parity_check"}
    if world == 1 and not args.no_cpu_baseline:
        todo.add("cpu_baseline")
    return todo


def main():
    args = parse_args()

    def note(msg):
        if args.verbose:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(args.cpu_sample)), flush=True)
        return
    if args.gpus > 1 and "RANK" not in os.environ:
        self_launch(args.gpus)

    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.launch_check:
        launch_check(args, rank, world)
        return
    # SBK_BENCH_FORCE_DIST=1 (with torchrun --nproc-per-node 1): run the RCCL leg -- process group, scatter metadata,
    # gather, all-reduce, barrier -- on a single GPU, to check the N > 1 code path where only one GPU is available
    dist_on = world > 1 or (os.environ.get("SBK_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (the HIP path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    if dist_on:
        dist.init_process_group("nccl", device_id=dev)

    from speechbrain_amd import native
    from speechbrain_amd.inference.builders import build_asr
    from speechbrain_amd.inference.sharded import ShardedTranscriber
    from speechbrain_amd.inference.streams import ConcurrentTranscriber

    native.load()
    for kv in args.knob:
        native.load().sbk_prof_set_knob(*[int(v) for v in kv.split("=")])
    asr = build_asr("L", vocab=5000, seed=0, beam_size=10, ctc_weight=0.4, device=str(dev),
                    attention_type=args.attention)
    if args.lm:  # conformer_large.yaml:166-223: full_scorers=[transformerlm, ctc], lm_weight 0.6, temperature 1.15
        from speechbrain_amd.decoders import (CTCScorer, S2STransformerBeamSearcher, ScorerBuilder,
                                              TransformerLMScorer)
        from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM

        torch.manual_seed(1)
        lm = TransformerLM(vocab=5000, d_model=768, nhead=12, num_encoder_layers=12, num_decoder_layers=0, d_ffn=3072,
                           dropout=0.0, activation=torch.nn.GELU, normalize_before=False).to(dev).eval()
        scorer = ScorerBuilder(full_scorers=[TransformerLMScorer(language_model=lm, temperature=1.15),
                                             CTCScorer(ctc_fc=asr.mods.ctc_lin, blank_index=0, eos_index=2)],
                               weights={"transformerlm": 0.6, "ctc": 0.4})
        asr.mods.decoder = S2STransformerBeamSearcher(
            modules=[asr.mods.transformer, asr.mods.seq_lin], bos_index=1, eos_index=2, min_decode_ratio=0.0,
            max_decode_ratio=1.0, beam_size=10, using_eos_threshold=False, length_normalization=True,
            temperature=1.15, scorer=scorer)
    # the searches keep the product's stop rule (polled every 8 steps through asynchronous 4-byte copies: no stream
    # drain, csrc/search.hip AsyncPoll); random weights never finish early, so every search runs its fixed length
    if args.check_every >= 0:
        asr.mods.decoder.check_every = args.check_every
    asr.eval_precision = args.precision

    def transcribe_one(w, l):
        return asr.transcribe_batch(w, l)[1]

    def trace_mark():
        # SBK_TRACE_MARK=1: a uniquely named kernel (stream_copy_kernel) brackets the timed region, so that a
        # rocprofv3 kernel trace can be cut to exactly that region (tools/trace_gaps.py, tools/trace_overlap.py)
        if os.environ.get("SBK_TRACE_MARK", "0") != "1":
            return
        import ctypes

        from speechbrain_amd import native as nat
        x = torch.zeros(2048, device=dev)
        us = ctypes.c_float(0)
        nat.load().sbk_prof_stream_f32(nat._p(x), nat._p(x[1024:]), 1024, 0, 1, ctypes.byref(us), nat._stream(x))
        torch.cuda.synchronize()

    def barrier():
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- the job: rank 0 holds world * K * 128 utterances (weak scaling: K steps per GPU)
    strong = args.job_utts > 0
    n_utts = args.job_utts if strong else world * args.steps * UTTS_PER_STEP
    job, seconds = make_job(n_utts) if rank == 0 else (None, None)
    total_audio = sum(seconds) if rank == 0 else 0.0

    def timed_run(max_batch, streams, group):
        """Warm-up + the timed scatter -> transcribe -> gather of the whole job at one batch size."""
        # every leg starts from a trimmed allocator: each leg has its own worker streams, the caching allocator keeps one
        # pool per stream, and three legs' pools (128-utterance batches: ~2 GB of CTC emissions per grouped search) next
        # to each other had the third leg reclaiming cached blocks inside its timed region (3 299 instead of 11 K audio-s/s)
        import gc
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        workers = ConcurrentTranscriber(asr, streams=streams, prioritise_search=not args.no_search_priority, group=group)
        workers.group_encoder = group_encoder_setting()
        for srch in workers.searchers:
            srch.graph_mode = args.graph_mode
            if args.overlap_ctc >= 0:
                srch.overlap_ctc = args.overlap_ctc
        st = ShardedTranscriber(transcribe_one, dev, max_utts=max_batch, concurrent=workers, prepare=fixed_decode_length)
        # W untimed steps through the same path (communicators, allocator pools); the longest utterances first, and
        # every worker stream sizes its allocations on the longest batch
        warm = None
        if rank == 0:
            longest = sorted(range(n_utts), key=lambda i: -job[i].numel())
            warm = [job[i] for i in longest[: max(1, args.warmup) * UTTS_PER_STEP * world]]
        local = st.scatter(warm)
        if local:
            # FIRST the largest batch as a full group on every worker: each worker stream sizes its search buffer once, at its
            # maximum (a buffer that is outgrown later goes back to the driver together with every cached block -- native.
            # _search_workspace -- which must not happen right in front of the timed region); then the warm job itself
            big = max(local, key=lambda t: t[1].numel())
            if len(big) > 3 and big[3] is not None:
                big[3]()  # (rank 0: stages the warm job on this thread; a peer: waits for its receive)
            workers.transcribe_batches([(big[1], big[2])] * (workers.n * workers.group), prepare=fixed_decode_length)
        st.gather(st.run_local(local))
        note(f"batch {max_batch}: warm-up done; timed region")
        barrier()
        trace_mark()
        # the clock starts with the waveforms in (pageable) host memory and stops with the token-id lists on the host
        # (SURVEY 8d): planning -- duration sort, buckets, LPT assignment -- and the padding of every batch into pinned
        # staging memory are INSIDE it; the padding / H2D / sends are streamed behind the first batches' compute
        if args.prof_concurrent:
            native.prof_reset()
            native.prof_enable(True)
        t0 = time.perf_counter()
        plan = st.plan(job)
        t_prep = time.perf_counter() - t0
        local = st.distribute(plan)
        hyps = st.gather(st.run_local(local))
        barrier()
        dt = time.perf_counter() - t0
        trace_mark()
        conc = None
        if args.prof_concurrent:
            native.prof_enable(False)
            conc = native.prof_report()
            native.prof_reset()
        per_rank_wall = [dt]
        if dist_on:  # every rank's own wall time (audit of a scaling run), MAX over ranks = the job's time
            t = torch.tensor([dt], dtype=torch.float64, device=dev)
            walls = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(walls, t)
            per_rank_wall = [float(w[0]) for w in walls]
            dt = max(per_rank_wall)
        info = {}
        if rank == 0 and conc:
            tot = sum(v["ms"] for v in conc.values())
            top = sorted(conc.items(), key=lambda kv: -kv[1]["ms"])[:16]
            info["concurrent_kernels"] = {
                "instrumented": True, "launches": sum(v["count"] for v in conc.values()),
                "kernel_ms_sum": round(tot, 1), "wall_ms": round(1000.0 * dt, 1),
                "mean_kernels_in_flight": round(tot / (1000.0 * dt), 2),
                "by_class": {k: {"launches": v["count"], "ms": round(v["ms"], 1), "us_each": round(1000.0 * v["ms"] / max(v["count"], 1), 1)}
                             for k, v in top}}
        if rank == 0:
            plan_ = st.last_plan
            info.update({"n_batches": len(plan_["batches"]), "bytes_scattered": plan_["bytes_sent"], "plan_s": round(t_prep, 4),
                    "streams": workers.n, "group": workers.group,
                    "gpu_memory_reserved_gb": round(torch.cuda.memory_reserved(dev) / 2 ** 30, 1),
                    "gpu_memory_peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 1),
                    "per_rank_wall_s": [round(w, 4) for w in per_rank_wall],
                    "per_rank_audio_s": [round(sum(seconds[i] for b in plan_["owner"][r] for i in plan_["batches"][b]), 1)
                                         for r in range(world)],
                    "per_rank_batches": [len(plan_["owner"][r]) for r in range(world)]})
        workers.close()
        return dt, hyps, local, info

    def group_encoder_setting():
        """ConcurrentTranscriber.group_encoder of the timed region: False = one encoder pass per batch, True = one over the rows of all
        the batches of a group, n = over n batches at a time.  Default (round 6, profiles/r06_r_*, r06_s_*): see GROUP_ENCODER_DEFAULT."""
        v = GROUP_ENCODER_DEFAULT if args.group_encoder < 0 else args.group_encoder
        return False if v == 0 else (True if v >= 1000 else v)

    def auto(max_batch):
        # 4 recipe-sized batches per grouped search (profiles/r02_* ... r06_d_*); workers: rounds 2-5 ran 8 -- with the group encoder
        # (round 6) 4 / 5 / 6 / 8 workers read 12 629 / 12 594 / 12 612 / 12 516 and 12 559 / 12 577 / 12 533 / 12 491 at 12 steps,
        # 12 861 / -- / 13 042 / 12 978 at the driver's 20 + 5 steps, with 78 / -- / 100 / 125 GB reserved (profiles/r06_u_*): from two
        # workers on every further one only stretches the others' kernels.  At 20 + 5 steps twice more
        # (profiles/r06_v_*): 4 workers 12 953 / 12 939 at 78 GB reserved, 5: 13 042 / 12 950 at 82 GB, 6: 13 050 / 13 027 at 100 GB -> 5.
        # (128-utterance batches are searched one per worker: eight of them, as before.)
        group = args.group or max(1, 128 // max_batch)
        return args.streams or (5 if group > 1 else 8), group

    def child_leg(name):
        import gc
        import subprocess
        import tempfile

        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()  # (the child needs the HBM the parent's pools still hold)
        fd, path = tempfile.mkstemp(suffix=".json", prefix=f"sbk_leg_{name}_")
        os.close(fd)
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--leg-out", path, "--steps", str(args.steps), "--warmup",
               str(args.warmup), "--max-batch", str(args.max_batch), "--second-batch", str(args.second_batch), "--attention",
               args.attention, "--check-every", str(args.check_every), "--streams", str(args.streams), "--group", str(args.group),
               "--graph-mode", str(args.graph_mode), "--overlap-ctc", str(args.overlap_ctc), "--latency-runs", str(args.latency_runs)]
        cmd += [x for kv in args.knob for x in ("--knob", kv)]
        cmd += (["--lm"] if args.lm else []) + ["--group-encoder", str(args.group_encoder)] + (
            ["--no-search-priority"] if args.no_search_priority else [])
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
            if r.returncode != 0:
                return {"error": f"rc {r.returncode}: {r.stderr.decode(errors='replace')[-300:]}"}
            with open(path) as f:
                return json.load(f)
        except Exception as e:  # (a secondary leg must never cost the headline)
            return {"error": repr(e)[:300]}
        finally:
            try:
                os.unlink(path)
            except OSError:
                pass

    def latency_modes():
        """p50 of a single 10-s utterance, pinned host waveform -> token ids on the host, for the ways to run a single search.
        Round 5 (the default): the decoder stack of a step as ONE cooperative launch (csrc/decoder_persist.hip, knob 47), alone or
        with the CTC scorer on a helper stream beside it; before: a launch per operation with the CTC scorer on a helper stream,
        or replayed from a captured hipGraph."""
        w1 = (0.1 * torch.randn(1, 160000, generator=torch.Generator().manual_seed(5))).pin_memory()
        l1 = torch.ones(1)
        by_mode = {}
        lat_stream = torch.cuda.Stream(dev)  # (the legacy default stream cannot be captured into a graph)
        dec = asr.mods.decoder
        saved = (dec.overlap_ctc, dec.graph_mode)
        lib = native.load()
        # (round 6: "..._plain_launch_single_search_only" = the same kernel and grid as a PLAIN launch, knob 47 = 2: no 11-us gap on
        #  either side of it -- but several searches at once could then each hold part of the chip and wait for the rest forever; the
        #  cooperative launch queue runs such kernels one at a time.  Reported, never the product default, not in p50_latency_ms.)
        for mode, (ov, gm, persist) in (("persistent_step", (0, 0, 1)), ("persistent_step_helper_stream", (3, 0, 1)),
                                        ("persistent_step_helper_stream_plain_launch_single_search_only", (3, 0, 2)),
                                        ("helper_stream", (3, 0, 0)), ("hipgraph", (0, 1, 0))):
            dec.overlap_ctc, dec.graph_mode = ov, gm
            lib.sbk_prof_set_knob(47, persist)
            lat = []
            try:
                with torch.cuda.stream(lat_stream):
                    run_step(asr, w1, l1)
                    run_step(asr, w1, l1)
                    for _ in range(max(args.latency_runs, 1)):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        run_step(asr, w1, l1)
                        torch.cuda.synchronize()
                        lat.append(time.perf_counter() - t)
            finally:
                lib.sbk_prof_set_knob(47, 1)
            lat.sort()
            by_mode[mode] = round(1000.0 * lat[len(lat) // 2], 2)
        dec.overlap_ctc, dec.graph_mode = saved
        return by_mode

    if args.leg:  # ---- this process IS such a child: run the one leg, write its result, leave
        if args.leg == "latency":
            with open(args.leg_out, "w") as f:
                json.dump({"leg": "latency", "by_mode": latency_modes()}, f)
            return
        if args.leg == "batch128":
            dt2, hyps2, _, info2 = timed_run(args.second_batch, *auto(args.second_batch))
        elif args.leg == "bf16":
            asr.eval_precision = "bf16"
            dt2, hyps2, _, info2 = timed_run(args.max_batch, *auto(args.max_batch))
        else:
            native.F32X3 = False
            asr.mods.decoder._dec_handle = None  # (the searchers' weight tables carry the split images: rebuilt without)
            dt2, hyps2, _, info2 = timed_run(args.max_batch, *auto(args.max_batch))
        res = {"leg": args.leg, "dt": dt2, "value": round(total_audio / dt2, 2), "ms_per_step": round(1000.0 * dt2 / max(args.steps, 1), 3),
               "reserved_gb": info2.get("gpu_memory_reserved_gb"), "peak_allocated_gb": info2.get("gpu_memory_peak_allocated_gb"),
               "workers_x_group": [info2["streams"], info2["group"]],
               "hyps": [[int(v) for v in h] for h in hyps2] if args.leg == "bf16" else None}
        with open(args.leg_out, "w") as f:
            json.dump(res, f)
        return

    dt, hyps, local_batches, info = timed_run(args.max_batch, *auto(args.max_batch))
    note(f"timed region done: {dt:.3f} s")

    out = None
    if rank == 0:
        assert len(hyps) == n_utts and all(len(h) > 0 for h in hyps)
        out = {
            "metric": "audio-sec/s decoded (node), Conformer-L beam=10", "value": round(total_audio / dt, 2),
            "unit": "audio-sec/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1000.0 * dt / max(n_utts / (world * UTTS_PER_STEP), 1e-9), 3), "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None, "dtype": "f32" if args.precision == "fp32" else "bf16 operands, f32 accumulate (encoder GEMMs); f32 elsewhere",
            "data": "synthetic",
            "config": {"workload": f"Conformer-L enc-dec ({args.attention}, 12+6 layers, d=512, V=5000) + "
                                   "S2STransformerBeamSearcher beam=10 + CTC 0.4"
                                   + (" + TransformerLM 12x768 scorer 0.6" if args.lm else "")
                                   + "; 16 kHz 0.1*randn 16-bit PCM, durations U(5,30) s; duration-sorted batches of "
                                   f"<= {args.max_batch} utterances; decode steps = round(4 tok/s * seconds)",
                       "arithmetic": ("fp32 throughout; the encoder's large contractions (sbk_gemm_nt_x3p / _f32x3) and the decode step's "
                                      "projections from ~200 hypothesis rows on (sbk_gemm_nt_x3r) on the bf16 matrix pipe by the exact "
                                      "three-way operand split (six bf16 partial products per multiply-add, fp32 accumulation: "
                                      "fp32-grade results)" if native.F32X3 else "fp32 throughout, fp32 MFMA contractions")
                       if args.precision == "fp32" else "opt-in bf16 operands",
                       "gpu_memory_reserved_gb": {"after_headline_leg": info.get("gpu_memory_reserved_gb"),
                                                  "peak_allocated_headline_leg": info.get("gpu_memory_peak_allocated_gb")},
                       "parity_scope": ("token ids are bit-exact against the oracle only with the output heads x8 (peaked posteriors); on the "
                                        "unscaled random-init weights the tests assert the margin rule (the HIP token is the oracle's arg-max wherever "
                                        "the oracle's own top-1 / top-2 margin exceeds the fp32 error); WER within 0.1 abs of the reference is "
                                        "UNVERIFIABLE offline (no trained checkpoint, no LibriSpeech in this image)"),
                       "multi_gpu": "unmeasured on hardware in every round (one GPU per box): N > 1 ran under gloo only, RCCL at world size 1",
                       "step": f"{UTTS_PER_STEP} utterances", "max_batch": args.max_batch,
                       "utterances_total": n_utts, "batches_total": info["n_batches"],
                       "audio_seconds_total": round(total_audio, 1), "weights": "random init, torch.manual_seed(0)",
                       "parallelism": f"replicas x{world}; rank 0 holds the job as int16 PCM in host memory; timed: plan (duration sort, buckets, LPT) "
                                      "+ pad + H2D + streamed scatter (one P2P send per batch, RCCL/xGMI) -> transcribe -> gather of token ids",
                       "bytes_scattered": info["bytes_scattered"],
                       "planning": f"inside the timed region: {info['plan_s']} s of sort / bucket / LPT on rank 0, then every batch is padded "
                                   "into a ring of pinned buffers and copied (sent) one by one behind the first batches' compute",
                       "workers_per_gpu": info["streams"], "batches_per_grouped_search": info["group"],
                       "batches_in_flight_per_gpu": info["streams"] * info["group"],
                       "job": (f"fixed job of {n_utts} utterances shared by the {world} rank(s) (strong scaling, BASELINE.json configs[3])"
                               if strong else f"{args.steps} steps x {UTTS_PER_STEP} utterances per rank (weak scaling)"),
                       "stop_rule": ("polled every %d steps (asynchronous copies, product default)" % asr.mods.decoder.check_every)
                                    if asr.mods.decoder.check_every > 0 else "not polled (check_every = 0)"},
            "rccl_world": world if dist_on else 0,
            "per_rank": {"wall_s": info["per_rank_wall_s"], "audio_s": info["per_rank_audio_s"], "batches": info["per_rank_batches"]},
            **({"concurrent_kernels": info["concurrent_kernels"]} if "concurrent_kernels" in info else {}),
        }
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, hyps)

    # ---- everything below runs with --full only (secondary_measurements); a plain run prints the line here
    todo = secondary_measurements(args, rank, world, dist_on)

    # ---- secondary legs (N = 1), EACH IN A PROCESS OF ITS OWN (the legs used to share the parent's caching-allocator
    # pools -- one per worker stream -- and the third leg measured 8.3 K where the same leg alone gives 11-12 K): the same
    # utterances as 128-utterance batches; the opt-in bf16 encoder GEMMs + token agreement with the fp32 run; every contraction
    # on the fp32 MFMA instruction (SBK_F32X3=0's path: the headline's large contractions run on the bf16 pipe)
    if todo & {"batch128", "bf16", "fp32mfma"}:
        out["config"]["secondary_legs"] = "each in a process of its own (own allocator pools, worker streams and weight images)"
    if "batch128" in todo:
        r2 = child_leg("batch128")
        out[f"value_batch{args.second_batch}"] = r2.get("value")
        if "error" in r2:
            out["config"][f"batch{args.second_batch}_leg_error"] = r2["error"]
        else:
            out[f"ms_per_step_batch{args.second_batch}"] = r2["ms_per_step"]
            out["config"].setdefault("gpu_memory_reserved_gb", {})[f"batch{args.second_batch}_leg_own_process"] = r2["reserved_gb"]
            out["config"][f"workers_x_group_batch{args.second_batch}"] = r2["workers_x_group"]
        note(f"second run ({args.second_batch}-utterance batches): {r2.get('value')}")
    if "bf16" in todo:
        from speechbrain_amd.utils.metric_stats import token_error_rate

        r3 = child_leg("bf16")
        out["value_encoder_gemms_bf16"] = r3.get("value")
        if "error" in r3:
            out["config"]["bf16_leg_error"] = r3["error"]
        else:
            ter = token_error_rate(r3["hyps"], hyps)
            out["bf16_vs_fp32_token_error_rate_percent"] = round(ter["WER"], 3)
            out["config"].setdefault("gpu_memory_reserved_gb", {})["bf16_leg_own_process"] = r3["reserved_gb"]
        out["config"]["bf16_note"] = ("opt-in (run_opts precision='bf16'): encoder GEMM operands rounded to bf16, fp32 accumulation, "
                                      "everything else fp32; token error rate of its hypotheses against the fp32 run's on the "
                                      "same utterances (random-init weights: flat posteriors amplify every perturbation)")
        note(f"bf16 encoder GEMMs: {r3.get('value')}")
    if "fp32mfma" in todo and native.F32X3:
        r4 = child_leg("fp32mfma")
        out["value_fp32_mfma_contractions"] = r4.get("value")
        if "error" in r4:
            out["config"]["fp32_mfma_leg_error"] = r4["error"]
        note(f"fp32-MFMA contractions: {r4.get('value')}")

    # ---- p50 per-utterance latency (B = 1, 10 s; pinned host waveform -> token ids on the host), rank 0 only.  In a process of
    # its own like the other secondary legs: measured inside this one -- 100 GB of cached blocks mapped, sixteen retired worker
    # streams -- every mode read 3-4 ms more than in a fresh process (27.5 against 22.9 ms for the persistent step,
    # profiles/r05_final_bench_first.json against profiles/r05_g_*.log)
    if "latency" in todo:
        by_mode = None
        if world == 1 and not dist_on:
            r5 = child_leg("latency")
            by_mode = r5.get("by_mode")
            if by_mode is None:
                out["config"]["latency_leg_error"] = r5.get("error", "no result")
            else:
                out["config"]["latency_leg"] = "own process"
        if by_mode is None:
            by_mode = latency_modes()
        out["p50_latency_ms"] = min(v for k, v in by_mode.items() if "single_search_only" not in k)
        out["p50_latency_ms_by_mode"] = by_mode
        out["config"]["latency_case"] = "B=1, 10 s utterance, 40 decode steps"

    # ---- BASELINE.json configs[4] (stretch): Whisper large-v3 shaped encoder, random weights, 30-second chunks
    if "whisper_encoder" in todo:
        try:
            out["config5_whisper_encoder"] = whisper_encoder_leg(dev)
        except Exception as e:  # a secondary measurement must not take the headline down
            out["config5_whisper_encoder"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        note("whisper encoder leg done")

    # ---- rooflines: HIP events around every launch, rank 0's batches repeated on one stream
    if "roofline" in todo:
        note("instrumented repetition (HIP events)")
        native.prof_reset()
        native.prof_enable(True)
        # the same batches, grouped as in the timed region, on ONE worker stream (every launch between two events)
        one = ConcurrentTranscriber(asr, streams=1, prioritise_search=False, group=auto(args.max_batch)[1])
        one.group_encoder = group_encoder_setting()
        one.plan_workers = auto(args.max_batch)[0]  # the same groups as the eight workers formed
        # every launch ALONE between its two events: a single worker would otherwise run the CTC scorer on a helper stream
        # (overlap_ctc = 3), and the layer-0 launches that co-run with the 250-us ctc_score_step were counted at 100-200 us each
        # -- rounds 4-5 reported gemm_x3r at 27-28 us per launch for what the device timeline shows at 13-35 us
        # (profiles/r06_c_*).  The timed region's workers run with overlap_ctc = 0 as well.
        for srch in one.searchers:
            srch.overlap_ctc = 0 if args.overlap_ctc < 0 else args.overlap_ctc
        seq_out = one.transcribe_batches([(t[1], t[2]) for t in local_batches], prepare=fixed_decode_length)
        one.close()
        # determinism of the headline's execution mode: the same batches, in the same groups, one after the other on ONE
        # stream give exactly the token ids the eight concurrent workers produced inside the timed region (NOT a parity
        # statement: both sides are the worker machinery -- the comparison with plain transcribe_batch follows below)
        n_cmp = n_bad = 0
        for t, per_batch in zip(local_batches, seq_out):
            for i, toks in zip(t[0], per_batch):
                n_cmp += 1
                n_bad += int(list(toks) != list(hyps[i]))
        out["determinism_check"] = {"utterances": n_cmp, "ids_equal": n_bad == 0, "utterances_differing": n_bad,
                                    "what": "token ids of the timed region (concurrent workers, grouped searches) vs the same "
                                            "batches in the same groups run sequentially on one worker stream afterwards"}
        if n_bad:  # (reported in the line, not fatal: the measurement above stands or falls with what the line says)
            print(f"[bench] determinism_check FAILED: {n_bad} of {n_cmp} utterances differ", file=sys.stderr, flush=True)
        rep_audio = sum(seconds[i] for t in local_batches for i in t[0])
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
        native.prof_reset()
        # one kernel, two profiler names: gemm_x3r_kernel with and without the LayerNorm in its prologue (csrc/gemm_x3r.hip)
        if "gemm_ln_x3r" in rep:
            fam = rep.setdefault("gemm_x3r", {"ms": 0.0, "count": 0, "flops": 0.0, "bytes": 0.0})
            ln = rep.pop("gemm_ln_x3r")
            for k in ("ms", "count", "flops", "bytes"):
                fam[k] = fam[k] + ln[k]
        total_ms = sum(v["ms"] for v in rep.values()) or 1.0
        ranked = sorted(rep.items(), key=lambda kv: -kv[1]["ms"])
        roof = roofline_entry(ranked[0][0], ranked[0][1], total_ms)
        name = roof["kernel"]
        traffic = None
        try:
            traffic = pmc_traffic(name, roof)
        except Exception:
            pass
        roof["traffic"] = traffic
        if name.startswith("gemm_x3r"):
            roof["kernel_note"] = "gemm_x3r_kernel with and without the LayerNorm prologue (profiler names gemm_x3r + gemm_ln_x3r: one kernel template)"
            try:
                roof["per_shape_isolated"] = x3r_per_shape(dev)
            except Exception as e:
                roof["per_shape_isolated"] = repr(e)[:200]
        out["roofline"] = roof
        out["roofline_top3"] = [roofline_entry(k, v, total_ms) for k, v in ranked[:3]]
        gflop_per_s = sum(v["flops"] for v in rep.values()) / max(rep_audio, 1e-9) / 1e9
        mb_per_s = sum(v["bytes"] for v in rep.values()) / max(rep_audio, 1e-9) / 1e6
        out["roofline_end_to_end"] = {
            "algorithmic_gflop_per_audio_sec": round(gflop_per_s, 3), "algorithmic_mb_per_audio_sec": round(mb_per_s, 2),
            "achieved_tflops": round(gflop_per_s * out["value"] / world / 1e3, 2),
            "frac_of_mfma_f32_peak": round(gflop_per_s * out["value"] / world / 1e3 / PEAK_MFMA_F32_TFLOPS, 4),
            "achieved_gbs": round(mb_per_s * out["value"] / world / 1e3, 1),
            "frac_of_hbm_peak": round(mb_per_s * out["value"] / world / 1e3 / PEAK_HBM_GBS, 4),
            "single_stream_kernel_ms_per_audio_sec": round(total_ms / max(rep_audio, 1e-9), 4)}
        out["kernel_breakdown_ms"] = {k: round(v["ms"], 2) for k, v in ranked}
        try:  # the decoding step of the headline's grouped searches, on one stream (on the line, not only in profiles/)
            probe = decode_step_probe(asr, dev)
            out["decode_step_ms"] = probe.pop("decode_step_ms")
            out["launches_per_decode_step"] = probe.pop("launches_per_decode_step")
            out["decode_step_probe"] = probe
        except Exception as e:
            out["decode_step_probe"] = {"error": repr(e)[:200]}

    # ---- parity of the headline's execution mode against the PLAIN path: >= 256 utterances of the job through the eight
    # concurrent workers with grouped searches vs main-thread, one-stream, ungrouped asr.transcribe_batch calls on the same
    # padded batches.  The grouped search runs the decode GEMMs at other row counts (other kernels, another summation
    # order), so the output heads are peaked (x8, as in tests/: random-init posteriors are flat and any fp32 reassociation
    # flips a near-tie) for BOTH sides; the weights are restored afterwards
    if "parity_check" in todo:
        sub, n_sub = [], 0
        for t in sorted(local_batches, key=lambda t: (t[1].numel(), t[0][0])):  # the smallest batches first: cheap, and several shapes
            sub.append(t)
            n_sub += len(t[0])
            if n_sub >= 256:
                break
        heads = [asr.mods.seq_lin.w.weight, asr.mods.ctc_lin.w.weight]
        with torch.no_grad():
            for h in heads:
                h.mul_(8.0)
        try:
            par = ConcurrentTranscriber(asr, streams=auto(args.max_batch)[0], group=auto(args.max_batch)[1])
            par.group_encoder = group_encoder_setting()
            got = par.transcribe_batches([(t[1], t[2]) for t in sub], prepare=fixed_decode_length)
            par.close()
            n_bad = 0
            for t, per_batch in zip(sub, got):
                plain = run_step(asr, t[1], t[2])
                n_bad += sum(int(list(a) != list(b)) for a, b in zip(per_batch, plain))
        finally:
            with torch.no_grad():
                for h in heads:
                    h.div_(8.0)
            asr.mods.decoder._dec_handle = None
        out["parity_check"] = {"utterances": n_sub, "batches": len(sub), "ids_equal": n_bad == 0, "utterances_differing": n_bad,
                               "what": "concurrent workers + grouped searches (the timed region's mode) vs plain main-thread "
                                       "asr.transcribe_batch per batch on the same padded batches; output heads x8 on both sides"}
        if n_bad:
            print(f"[bench] parity_check FAILED: {n_bad} of {n_sub} utterances differ", file=sys.stderr, flush=True)

    # ---- configs[1]: STFT + Fbank + CNN + Conformer-S encoder forward, 32 x 10 s
    if "config1_encoder_S" in todo:
        note("configs[1]: Conformer-S encoder")
        small = build_asr("S", vocab=5000, seed=0, beam_size=10, ctc_weight=0.4, device=str(dev))
        ws = (0.1 * torch.randn(32, 160000, generator=torch.Generator().manual_seed(1234))).to(dev)
        ls = torch.ones(32, device=dev)
        with torch.no_grad():
            for _ in range(3):
                small.encode_batch(ws, ls)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                small.encode_batch(ws, ls)
            e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20.0
        out["config1_encoder_S"] = {"workload": "STFT+Fbank+CNN+Conformer-S encoder forward, 32 x 10 s, one stream",
                                    "ms_per_batch": round(ms, 3), "audio_sec_per_s": round(320.0 / (ms * 1e-3), 1)}
        del small

    if "cpu_baseline" in todo:
        note("cpu baseline (subprocess)")
        cpu = cpu_baseline_subprocess()
        ref_tokens = cpu.pop("tokens", None)
        ref12 = cpu.pop("tokens_12x10s_heads_x8", None)
        out["cpu_baseline"] = cpu
        if ref12:  # 12 x 10 s = 3 012 encoder rows: the split-operand kernel inside an oracle comparison; heads x8 on both sides
            from speechbrain_amd.utils.metric_stats import token_error_rate

            w12, l12 = parity_sample()
            heads = [asr.mods.seq_lin.w.weight, asr.mods.ctc_lin.w.weight]
            with torch.no_grad():
                for h in heads:
                    h.mul_(8.0)
            try:
                # (12 utterances x beam 10 = 120 hypothesis rows: the decode step's projections take sbk_gemm_nt_x3r from
                # ~200 rows on -- the headline's grouped searches have 1 280 -- so the row threshold is lowered for this
                # sample: the kernel the headline's decode loop runs is the one compared with the oracle)
                # (and 12 utterances x 8 heads = 96 (utterance, head) pairs: the register-ring cross-attention starts at 128 --
                # the headline's searches have 1 024 -- so knob 4 = 5 routes this sample through it as well; the profiler
                # report says which kernels the sample actually ran)
                native.load().sbk_prof_set_knob(42, 1)
                native.load().sbk_prof_set_knob(4, 5)
                native.prof_reset()
                native.prof_enable(True)
                got12 = run_step(asr, w12.to(dev), l12.to(dev))
                native.prof_enable(False)
                ran12 = native.prof_report()
                native.prof_reset()
            finally:
                native.prof_enable(False)
                native.load().sbk_prof_set_knob(4, 7)
                native.load().sbk_prof_set_knob(42, 192)
                with torch.no_grad():
                    for h in heads:
                        h.div_(8.0)
                asr.mods.decoder._dec_handle = None
            wer12 = token_error_rate(got12, ref12)
            out["token_error_rate_vs_oracle_12x10s_peaked_heads"] = {
                "WER_percent": round(wer12["WER"], 3), "tokens": wer12["num_scored_tokens"], "utterances": len(ref12),
                "ids_equal": [list(a) for a in got12] == [list(b) for b in ref12],
                "decode_kernels_run": {k: ran12[k]["count"] for k in ("gemm_x3r", "gemm_ln_x3r", "cross_attn_ring", "cross_attn_step", "cross_merge",
                                                                      "self_attn_step", "ctc_score_step") if k in ran12},
                "note": "12 x 10 s (3 012 encoder rows: FFN / QKV / pointwise-conv contractions on sbk_gemm_nt_x3p with the "
                        "LayerNorm -> panel / hidden-layer hand-over chain; the decode step's projections on sbk_gemm_nt_x3r, its "
                        "cross-attention on the register-ring kernel -- the headline's decode kernels, routed by knobs 42 / 4 because 12 utterances are below their row thresholds), "
                        "relative lengths 0.6-1, output heads x8 on both sides so that fp32 reassociation cannot flip a "
                        "near-tie; oracle = oracle/sb_oracle.py (the port)"}
        if ref_tokens:  # the same batch on the HIP path, scored against the oracle's tokens
            from speechbrain_amd.utils.metric_stats import token_error_rate

            w2, l2 = cpu_sample(cpu.get("sample_kind", "4x10s"))
            got = run_step(asr, w2.to(dev), l2.to(dev))
            wer = token_error_rate(got, ref_tokens)
            out["token_error_rate_vs_oracle"] = {
                "WER_percent": round(wer["WER"], 3), "tokens": wer["num_scored_tokens"], "utterances": len(ref_tokens),
                "note": "random-init weights give nearly flat posteriors (SURVEY A.4): ids can differ where the oracle's "
                        "own top-1/top-2 margin is below fp32 reassociation error; parity proper is asserted in tests/"}

    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
