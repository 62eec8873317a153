"""WavLM encoder time at the wavlm-base-plus (group norm, post-norm, d 768, 12 layers) and wavlm-large (layer norm, stable,
d 1024, 24 layers) shapes -- random weights (WavLM.from_config), fp32, 32 x 10 s (T' = 499 encoder frames) -- and, in the same
run, the price of the fused gated relative-position bias: ``native.wavlm_attention`` next to plain ``native.rope_attention``
(no rotation tables: the wav2vec 2.0 / HuBERT attention) at the same B, T', H, Dh, in microseconds per launch (HIP events).

The expectation that is RECORDED as met or missed (nothing is gated on it): wavlm_attention / rope_attention <= 1.3 -- one LDS
read and one fused multiply-add per score against 128 MFMA flops and an ``exp``, at the same occupancy.

Every GPU step (one encoder shape, the attention pair) runs in a fresh child process under its own time limit; the first step
that fails or runs out of time ends the run (nothing more is started on the GPU) and is recorded.  ``--headline NAME=FILE``
copies the JSON result line of a ``bench.py`` run (e.g. this tree's and the parent commit's, from the same visit) into the result.
One JSON line per run, also written to profiles/wavlm_bench.json.  A job for a GPU visit.

    python tools/wavlm_bench.py [--steps 5] [--warmup 2] [--shapes base_plus,large] [--headline this=a.json --headline parent=b.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "base_plus": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                      feat_extract_norm="group", conv_bias=False, do_stable_layer_norm=False),
    "large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                  feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True),
}
STEP_TIMEOUT_S = 240


def p50_ms(torch, fn, steps, warmup):
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    times.sort()
    return times[len(times) // 2] * 1e3


def event_us(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def encoder_step(name, args):
    import torch

    from speechbrain_amd import native
    from speechbrain_amd.integrations.huggingface.wavlm import WavLM

    native.load()
    B, N = args.batch, int(args.seconds * 16000)
    w = WavLM.from_config({"model_type": "wavlm", **SHAPES[name]}, normalize_wav=(name == "large"), output_norm=True,
                          seed=3).to("cuda:0")
    cfg = w.model.config
    wav = (0.3 * torch.randn(B, N, generator=torch.Generator().manual_seed(5))).cuda()
    lens = torch.linspace(0.6, 1.0, B).cuda()
    res = {"shape": name, "batch": B, "seconds": args.seconds, "frames": int(w.model.feat_lengths(N)),
           "layers": cfg["num_hidden_layers"], "d": cfg["hidden_size"]}
    with torch.no_grad():
        run = lambda: w(wav, lens)  # noqa: E731
        ms = p50_ms(torch, run, args.steps, args.warmup)
        res["encoder_p50_ms"] = round(ms, 3)
        res["audio_sec_per_sec"] = round(B * args.seconds / (ms / 1e3), 1)
        native.prof_reset()
        native.prof_enable(True)
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = {k: v["ms"] / args.steps for k, v in native.prof_report().items()}
        res["encoder_kernel_ms"] = round(sum(rep.values()), 3)
        res["wavlm_attention_share_of_kernel_time"] = round(rep["wavlm_attention"] / sum(rep.values()), 4)
        res["kernels_ms"] = {k: round(v, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1])}
    return res


def attention_step(args):
    """wavlm_attention and plain rope_attention on the same qkv, key lengths and stream, alternating."""
    import torch

    from speechbrain_amd import native

    native.load()
    B, Dh = args.batch, 64
    out = []
    for name, shape in SHAPES.items():
        H, d = shape["num_attention_heads"], shape["hidden_size"]
        T = ((int(args.seconds * 16000) - 400) // 320) + 1
        gen = torch.Generator().manual_seed(11)
        qkv = torch.randn(B, T, 3 * d, generator=gen).cuda()
        x = torch.randn(B, T, d, generator=gen).cuda()
        gate_w = (torch.randn(8, Dh, generator=gen) / Dh ** 0.5).cuda()
        gate_b, gate_const = torch.zeros(8).cuda(), torch.ones(H).cuda()
        tab = native.wavlm_bias_table(torch.randn(320, H, generator=gen).cuda(), T, 320, 800)
        key_len = (torch.linspace(0.6, 1.0, B) * T).round().to(torch.int32).cuda()
        o1, o2 = torch.empty(B, T, d, device="cuda:0"), torch.empty(B, T, d, device="cuda:0")
        gated = lambda: native.wavlm_attention(qkv, x, gate_w, gate_b, gate_const, tab, key_len, H, Dh ** -0.5, out=o1)  # noqa: E731
        with native.precision_scope("fp32"):
            plain = lambda: native.rope_attention(qkv, None, None, key_len, H, Dh ** -0.5, out=o2)  # noqa: E731
            us_g, us_p = [], []
            for _ in range(3):  # alternate the two, keep each one's best of three: clock and cache state are shared
                us_g.append(event_us(torch, gated, 10 * args.steps, args.warmup))
                us_p.append(event_us(torch, plain, 10 * args.steps, args.warmup))
        flops = 4.0 * B * H * float(T) * T * Dh
        r = {"shape": name, "B": B, "T": T, "H": H, "Dh": Dh, "wavlm_attention_us": round(min(us_g), 1),
             "rope_attention_us": round(min(us_p), 1), "ratio": round(min(us_g) / min(us_p), 3),
             "wavlm_attention_tflops": round(flops / min(us_g) / 1e6, 1), "rope_attention_tflops": round(flops / min(us_p) / 1e6, 1),
             "bias_tensor_avoided_mbytes_per_layer": round(4.0 * B * H * T * T / 1e6, 1)}
        r["expectation ratio <= 1.3"] = "met" if r["ratio"] <= 1.3 else "missed"
        out.append(r)
    return out


def child(step, args):
    """A fresh process for one GPU step, under its own time limit -> (result or None, error text or None)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--batch", str(args.batch), "--seconds", str(args.seconds)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return None, f"{step}: no result within {STEP_TIMEOUT_S} s"
    if p.returncode != 0:
        return None, f"{step}: exit status {p.returncode}: {p.stderr.strip()[-400:]}"
    return json.loads(p.stdout.strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--shapes", default="base_plus,large")
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process: attention | encoder:<shape>")
    ap.add_argument("--headline", action="append", default=[], metavar="NAME=FILE",
                    help="a file whose last line is a bench.py JSON result, recorded under bench_py[NAME]")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(attention_step(args) if args.step == "attention" else encoder_step(args.step.split(":", 1)[1], args)))
        return
    res = {"workload": f"WavLM encoder, {args.batch} x {args.seconds:g} s, fp32, random weights", "steps": args.steps,
           "shapes": [], "attention": None, "failed": None}
    for step in ["attention"] + [f"encoder:{s}" for s in args.shapes.split(",") if s]:
        out, err = child(step, args)
        if err:  # (nothing more is started on the GPU after a step that failed or hung)
            res["failed"] = err
            break
        if step == "attention":
            res["attention"] = out
        else:
            res["shapes"].append(out)
    bench = {}
    for item in args.headline:
        name, path = item.split("=", 1)
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.strip().startswith("{")]
        full = json.loads(lines[-1])
        bench[name] = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step")}
    if bench:
        res["bench_py"] = bench
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "wavlm_bench.json"), "w") as f:
        f.write(line + "\n")
    if res["failed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
