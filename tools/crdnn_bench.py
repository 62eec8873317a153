"""CRDNN encoder time at the train_BPE_1000.yaml shape (2 CNN blocks 128 / 256, 4 x 1024 bidirectional LSTM, 2 x 512 DNN; n_mels
40, time pooling 4) -- random weights, fp32, 32 x 10 s from PCM -- in HIP events, with the parts next to their comparators in
the same run, alternating:

  encoder  p50 per batch (Fbank + CRDNN from PCM) and audio-sec/s; the kernel-time shares of the CNN (contractions, patch
           matrices, frame passes), the input projections, the recurrence and the DNN from the library's per-launch timing, each
           part of the model timed in a pass of its own (their contractions are launches of the same kernels).
  convs    each convolution with Cin >= 128 (patch matrix + contraction, native.crdnn_conv) in TFLOP/s next to native.gemm_nt on
           the plain product of the same size [B*T*F, 9 Cin] x [Cout, 9 Cin], issued in the same chunks of rows.
           RECORDED expectation: the convolution reaches at least half of the plain product's rate (the patch pass moves 9 x the
           activation, the same order of time as the contraction).
  lstm     per LSTM layer (input 2560 for layer 0, 2048 after) at B 32 and B 1, T' = 250: the input projection and the
           recurrence (step launches, the one route of csrc/rnn.hip) in us per step.
           RECORDED expectations: a step at B 32 takes at most 20 us (32 MiB of W_hh from the Infinity Cache plus a launch
           boundary); the recurrence is the largest share of the encoder's kernel time.
  torch    torch.nn.LSTM (one bidirectional layer, the same sizes) on the same device, if it runs there; last, in its own
           process: a failure is recorded and ends the run.  RECORDED expectation: native.rnn_layer is faster at B 32.

Every GPU step runs in a fresh child process under its own time limit, one at a time; the first step that fails or runs out of
time ends the run (nothing more is started on the GPU) and is recorded.  ``--headline NAME=FILE`` copies the JSON result line of
a ``bench.py`` run into the result.  One JSON line per run, also written to profiles/crdnn_bench.json.  A job for a GPU visit.

    python tools/crdnn_bench.py [--steps 3] [--warmup 1] [--headline this=a.json ...]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TIMEOUT_S = 240
N_MELS, T_FEAT, T_RNN, H = 40, 1001, 250, 1024


def event_ms(torch, fn, steps, warmup):
    """Sorted per-call times (ms) of ``steps`` calls, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out)


def med(v):
    return v[len(v) // 2]


def build_model(torch):
    from speechbrain_amd.lobes.models.CRDNN import CRDNN
    from speechbrain_amd.nnet.RNN import LSTM

    torch.manual_seed(3)
    return CRDNN(input_shape=[None, None, N_MELS], cnn_blocks=2, cnn_channels=[128, 256], inter_layer_pooling_size=[2, 2],
                 time_pooling=True, time_pooling_size=4, rnn_class=LSTM, rnn_layers=4, rnn_neurons=H, rnn_bidirectional=True,
                 rnn_re_init=True, dnn_blocks=2, dnn_neurons=512).to("cuda:0").eval()


def encoder_step(args):
    import torch

    from speechbrain_amd import native
    from speechbrain_amd.lobes.features import Fbank

    native.load()
    B = args.batch
    m = build_model(torch)
    fbank = Fbank(sample_rate=16000, n_fft=400, n_mels=N_MELS).to("cuda:0")
    wav = (0.1 * torch.randn(B, 160000, generator=torch.Generator().manual_seed(5))).cuda()
    res = {"batch": B, "seconds": 10.0}
    with torch.no_grad():
        run = lambda: m(fbank(wav))  # noqa: E731
        feats = fbank(wav)
        res["feature_frames"], res["encoder_frames"] = int(feats.shape[1]), int(m(feats).shape[1])
        ms = event_ms(torch, run, args.steps, args.warmup)
        res["p50_ms"], res["min_ms"], res["max_ms"] = round(med(ms), 2), round(ms[0], 2), round(ms[-1], 2)
        res["audio_sec_per_sec"] = round(B * 10.0 / (med(ms) / 1e3), 1)
        native.prof_reset()
        native.prof_enable(True)
        run()
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
    total = sum(v["ms"] for v in rep.values())
    res["kernel_ms"] = round(total, 2)
    res["kernels_ms"] = {k: [v["count"], round(v["ms"], 3)] for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}
    # the contractions of the three parts are launches of the same kernels: each part is timed in a pass of its own
    def part_ms(fn):
        native.prof_reset()
        native.prof_enable(True)
        with torch.no_grad():
            y = fn()
        torch.cuda.synchronize()
        native.prof_enable(False)
        return y, {k: v["ms"] for k, v in native.prof_report().items()}

    is_gemm = lambda k: "gemm" in k or "split" in k  # noqa: E731
    x_cnn, cnn = part_ms(lambda: m.cnn_forward(feats))
    x_rnn, rnn = part_ms(lambda: m.rnn_forward(x_cnn))

    def dnn_fn():
        y = x_rnn
        for block in m["DNN"].values():
            y = block(y)
        return y

    _, dnn = part_ms(dnn_fn)
    parts = sum(sum(d.values()) for d in (cnn, rnn, dnn)) + sum(v["ms"] for k, v in rep.items() if "fbank" in k)
    share = lambda d, pred: round(sum(v for k, v in d.items() if pred(k)) / parts, 4)  # noqa: E731
    res["parts_kernel_ms"] = round(parts, 2)
    res["share_cnn_contractions"] = share(cnn, is_gemm)
    res["share_cnn_patch_matrix"] = share(cnn, lambda k: k.startswith("crdnn_im2col"))
    res["share_cnn_frame_passes"] = share(cnn, lambda k: k.startswith("crdnn_conv1") or k.startswith("crdnn_norm_pool"))
    res["share_input_projections"] = share(rnn, is_gemm)
    res["share_recurrence"] = share(rnn, lambda k: k.startswith("rnn_"))
    res["share_dnn"] = share(dnn, lambda k: True)
    res["share_front_end"] = round(sum(v["ms"] for k, v in rep.items() if "fbank" in k) / parts, 4)
    res["share_cnn"] = round(res["share_cnn_contractions"] + res["share_cnn_patch_matrix"] + res["share_cnn_frame_passes"], 4)
    big = max(("recurrence", res["share_recurrence"]), ("cnn", res["share_cnn"]), ("input projections", res["share_input_projections"]),
              ("dnn", res["share_dnn"]), key=lambda kv: kv[1])[0]
    res["expectation the recurrence is the largest share"] = "met" if big == "recurrence" else f"missed ({big} is)"
    return res


def convs_step(args):
    import torch

    from speechbrain_amd import native

    native.load()
    B, out = args.batch, []
    gen = torch.Generator().manual_seed(7)
    for name, F, Cin, Cout in (("block_0.conv_2", 40, 128, 128), ("block_1.conv_1", 20, 128, 256), ("block_1.conv_2", 20, 256, 256)):
        x = torch.randn(B, T_FEAT, F, Cin, generator=gen).cuda()
        wk = (torch.randn(Cout, 9 * Cin, generator=gen) / (9 * Cin) ** 0.5).cuda()
        bias = torch.randn(Cout, generator=gen).cuda()
        M, K = B * T_FEAT * F, 9 * Cin
        rows = min(M, (native.CRDNN_COL_BYTES // (F * K * 4)) * F)  # the rows of one chunk of native.crdnn_conv
        a = torch.randn(rows, K, generator=gen).cuda()
        y = torch.empty(M, Cout, device="cuda:0")
        conv = lambda: native.crdnn_conv(x, wk, bias)  # noqa: E731
        # the plain product of the same size, in the same chunks of rows (the operand chunk is reused: the product is the same work)
        plain = lambda: [native.gemm_nt(a[:min(rows, M - r0)], wk, bias, out=y[r0:r0 + min(rows, M - r0)]) for r0 in range(0, M, rows)]  # noqa: E731
        t = {"conv": [], "plain": []}
        for _ in range(2):  # alternate
            t["conv"] += event_ms(torch, conv, args.steps, args.warmup)
            t["plain"] += event_ms(torch, plain, args.steps, args.warmup)
        gflop = 2.0 * M * K * Cout / 1e9
        c, p = med(sorted(t["conv"])), med(sorted(t["plain"]))
        r = {"conv": name, "M": M, "K": K, "N": Cout, "gflop": round(gflop, 1), "conv_ms": round(c, 2), "conv_tflops": round(gflop / c, 1),
             "plain_gemm_chunk_rows": rows, "plain_gemm_ms": round(p, 2), "plain_gemm_tflops": round(gflop / p, 1)}
        r["expectation conv at least half the plain product's rate"] = "met" if c <= 2.0 * p else "missed"
        out.append(r)
        del x, a
    return out


def lstm_step(args):
    import torch

    from speechbrain_amd import native

    native.load()
    gen = torch.Generator().manual_seed(9)
    out = []
    w_hh = (torch.randn(2, 4 * H, H, generator=gen) / H ** 0.5).cuda()
    b_ih, b_hh = torch.randn(2, 4 * H, generator=gen).cuda(), torch.randn(2, 4 * H, generator=gen).cuda()
    for layer, In in (("layer 0", 2560), ("layers 1-3", 2 * H)):
        w_ih = (torch.randn(2 * 4 * H, In, generator=gen) / In ** 0.5).cuda()
        for B in (32, 1):
            x = torch.randn(B, T_RNN, In, generator=gen).cuda()
            xp = native.gemm_nt(x, w_ih).view(B, T_RNN, 2, 4 * H)
            proj = lambda: native.gemm_nt(x, w_ih)  # noqa: E731
            rec = lambda: native.rnn_layer(xp, w_hh, b_ih, b_hh, route=1)  # noqa: E731
            runs = [med(event_ms(torch, rec, args.steps, args.warmup)) for _ in range(3)]  # three repeated measurements
            p = med(event_ms(torch, proj, args.steps, args.warmup))
            r = {"layer": layer, "B": B, "T": T_RNN, "H": H, "D": 2, "route": native.rnn_layer_route(B, T_RNN, H, 2),
                 "input_projection_ms": round(p, 3), "recurrence_ms_repeated": [round(v, 3) for v in runs],
                 "recurrence_us_per_step": round(med(sorted(runs)) * 1e3 / T_RNN, 2)}
            if B == 32:
                r["expectation a step takes at most 20 us"] = "met" if r["recurrence_us_per_step"] <= 20.0 else "missed"
            out.append(r)
    return out


def torch_step(args):
    import torch

    from speechbrain_amd import native

    native.load()
    gen = torch.Generator().manual_seed(9)
    out = []
    for B in (32, 1):
        m = torch.nn.LSTM(2 * H, H, 1, batch_first=True, bidirectional=True).to("cuda:0").eval()
        x = torch.randn(B, T_RNN, 2 * H, generator=gen).cuda()
        w_ih = torch.cat([m.weight_ih_l0, m.weight_ih_l0_reverse]).detach().contiguous()
        w_hh = torch.stack([m.weight_hh_l0, m.weight_hh_l0_reverse]).detach().contiguous()
        b_ih = torch.stack([m.bias_ih_l0, m.bias_ih_l0_reverse]).detach().contiguous()
        b_hh = torch.stack([m.bias_hh_l0, m.bias_hh_l0_reverse]).detach().contiguous()
        with torch.no_grad():
            ours = lambda: native.rnn_layer(native.gemm_nt(x, w_ih).view(B, T_RNN, 2, 4 * H), w_hh, b_ih, b_hh)[0]  # noqa: E731
            theirs = lambda: m(x)[0]  # noqa: E731
            diff = float((ours() - theirs()).abs().max())
            t = {"ours": [], "torch": []}
            for _ in range(2):
                t["ours"] += event_ms(torch, ours, args.steps, args.warmup)
                t["torch"] += event_ms(torch, theirs, args.steps, args.warmup)
        r = {"B": B, "T": T_RNN, "in": 2 * H, "H": H, "projection_plus_rnn_layer_ms": round(med(sorted(t["ours"])), 3),
             "torch_nn_lstm_ms": round(med(sorted(t["torch"])), 3), "max_abs_diff": diff}
        if B == 32:
            r["expectation rnn_layer faster than torch.nn.LSTM"] = "met" if r["projection_plus_rnn_layer_ms"] < r["torch_nn_lstm_ms"] else "missed"
        out.append(r)
    return out


STEPS = {"encoder": encoder_step, "convs": convs_step, "lstm": lstm_step, "torch": torch_step}


def child(step, args):
    """A fresh process for one GPU step, under its own time limit -> (result or None, error text or None)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--batch", str(args.batch)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return None, f"{step}: no result within {STEP_TIMEOUT_S} s"
    if p.returncode != 0:
        return None, f"{step}: exit status {p.returncode}: {p.stderr.strip()[-400:]}"
    return json.loads(p.stdout.strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process: " + " | ".join(STEPS))
    ap.add_argument("--headline", action="append", default=[], metavar="NAME=FILE",
                    help="a file whose last line is a bench.py JSON result, recorded under bench_py[NAME]")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step](args)))
        return
    res = {"workload": f"CRDNN encoder (train_BPE_1000.yaml shape), {args.batch} x 10 s from PCM, fp32, random weights",
           "steps": args.steps, "rnn_routes_in_tree": [1], "failed": None}
    for step in STEPS:
        out, err = child(step, args)
        if err:  # (nothing more is started on the GPU after a step that failed or hung)
            res["failed"] = err
            break
        res[step] = out
    bench = {}
    for item in args.headline:
        name, path = item.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
        full = json.loads(lines[-1])
        bench.setdefault(name.rstrip("0123456789_"), []).append(
            {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step")})
    if bench:
        res["bench_py"] = bench
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "crdnn_bench.json"), "w") as f:
        f.write(line + "\n")
    if res["failed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
