"""Transformer-encoder ASR (transformer.yaml) encoder time at the recipe's shape -- the three-block convolution front end (64
channels), 12 layers, d 512, 4 heads (head dim 128), d_ffn 2048 --, random weights, fp32, 32 x 10 s (1001 feature frames, T' = 251
encoder frames).  Reports the encoder's ms per batch (front end + encode), the kernels' own time from the profiler (HIP events):
the three conv blocks, the head-dim-128 attention, and, in the same run, the two yardsticks the new kernels are held against:

  * the head-dim-64 attention at H = 8 on the same d = 512, B and T (identical FLOPs and bytes): dh128 / dh64 should be <= 1.5;
  * sbk_gemm_nt_f32 on the plain [B*T2*20 x 1600] x [1600 x 64] product block 2 contracts: block 2 should reach >= 1/4 of it;
  * the front end should stay under 10 % of the encoder's kernel time.

One JSON line, also written to profiles/transformer_bench.json.  A job for a GPU visit.

    python tools/transformer_bench.py [--steps 10] [--warmup 3]

--precision bf16 measures the head-dim-128 bf16 attention instead (bench_bf16 below) and adds its result to that file under the key
"precision_bf16"; the fp32 record stays.

    python tools/transformer_bench.py --precision bf16 [--steps 20] [--warmup 5] [--rounds 5]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def p50_ms(fn, steps, warmup):
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    times.sort()
    return round(times[len(times) // 2] * 1e3, 3)


def profiled(native, fn, steps):
    """name -> ms per call of fn (the profiler's HIP-event times, summed over the launches of one call)."""
    native.prof_reset()
    native.prof_enable(True)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    native.prof_enable(False)
    return {k: v["ms"] / steps for k, v in native.prof_report().items()}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def bench_bf16(native, args, run, n_layers, B, T, lens):
    """--precision bf16: the head-dim-128 attention launch as fp32 and as bf16 (rope_flash_t128_bf16_kernel), the head-dim-64 bf16
    kernel at H = 8 on the same d, B and T for reference, and the 12-layer encoder under "bf16" with the attention held to fp32 (the
    encoder before the kernel existed) and with the new kernel.  The comparators alternate over `--rounds` rounds in this one run;
    every figure is the median over the rounds.  Result -> key "precision_bf16" of profiles/transformer_bench.json."""
    qkv = torch.randn(B, T, 3 * 512, generator=torch.Generator().manual_seed(6)).cuda()
    kl = torch.round(lens * T).to(torch.int32)

    def attn(precision, H):
        def f():
            with native.precision_scope(precision):
                native.rope_attention(qkv, None, None, kl, H, 1 / math.sqrt(512 // H))
        return f

    launches = {"attention_dh128_fp32_ms": (attn("fp32", 4), "rope_attention"),
                "attention_dh128_bf16_ms": (attn("bf16", 4), "rope_attention_bf16"),
                "attention_dh64_h8_bf16_ms": (attn("bf16", 8), "rope_attention_bf16")}
    orig = native.rope_attention

    def held(*a, **k):  # the attention of a "bf16" encoder on the fp32 kernel
        with native.precision_scope("fp32"):
            return orig(*a, **k)

    def encoder(fn):
        def f():
            native.rope_attention = fn
            try:
                with native.precision_scope("bf16"):
                    run()
            finally:
                native.rope_attention = orig
        return f

    encoders = {"encoder_bf16_attention_fp32": encoder(held), "encoder_bf16_attention_bf16": encoder(orig)}
    with native.precision_scope("fp32"):  # the contraction of the two attention results, old and new, on the same inputs
        c32 = native.rope_attention(qkv, None, None, kl, 4, 1 / math.sqrt(128))[0]
    with native.precision_scope("bf16"):
        c16 = native.rope_attention(qkv, None, None, kl, 4, 1 / math.sqrt(128))[0]
    res = {"rounds": args.rounds, "steps": args.steps,
           "attention_dh128_bf16_vs_fp32_max_abs": float((c16 - c32).abs().max()),
           "attention_dh128_bf16_vs_fp32_rel_rms": float(((c16 - c32).double().pow(2).mean() / c32.double().pow(2).mean()).sqrt())}
    times = {k: [] for k in list(launches) + [e + "_p50_ms" for e in encoders]}
    for fn, _ in launches.values():
        fn()
    for _ in range(args.rounds):
        for k, (fn, name) in launches.items():
            times[k].append(profiled(native, fn, args.steps)[name])
        for k, fn in encoders.items():
            times[k + "_p50_ms"].append(p50_ms(fn, args.steps, args.warmup))
    res.update({k: round(median(v), 4) for k, v in times.items()})
    res["spread"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()}
    for k, fn in encoders.items():  # the kernels' own time, profiler on: a run of its own
        rep = profiled(native, fn, args.steps)
        res[k + "_kernel_ms"] = round(sum(rep.values()), 3)
        res[k + "_attention_ms_per_layer"] = round((rep.get("rope_attention", 0.0) + rep.get("rope_attention_bf16", 0.0)) / n_layers, 4)
        res[k + "_kernels_ms"] = {n: round(v, 4) for n, v in sorted(rep.items(), key=lambda kv: -kv[1])}
    gflop = 4.0 * B * T * T * 512 / 1e9
    res["attention_dh128_bf16_tflops"] = round(gflop / res["attention_dh128_bf16_ms"], 2)
    res["attention_dh128_fp32_over_bf16"] = round(res["attention_dh128_fp32_ms"] / res["attention_dh128_bf16_ms"], 3)
    res["attention_dh128_bf16_over_dh64_h8_bf16"] = round(res["attention_dh128_bf16_ms"] / res["attention_dh64_h8_bf16_ms"], 3)
    res["encoder_attention_fp32_over_bf16"] = round(res["encoder_bf16_attention_fp32_p50_ms"] / res["encoder_bf16_attention_bf16_p50_ms"], 3)
    res["expectations"] = {"bf16 launch faster than the fp32 launch": res["attention_dh128_bf16_ms"] < res["attention_dh128_fp32_ms"],
                           "bf16 encoder faster with the new kernel than with the attention held to fp32":
                               res["encoder_bf16_attention_bf16_p50_ms"] < res["encoder_bf16_attention_fp32_p50_ms"]}
    return res


def main():
    from speechbrain_amd import native
    from speechbrain_amd.inference.builders import build_transformer_modules

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--rounds", type=int, default=5, help="--precision bf16: rounds over which the comparators alternate")
    args = ap.parse_args()
    native.load()
    B = args.batch
    frames = 1 + int(args.seconds * 16000) // 160
    T1 = (frames - 1) // 2 + 1
    T = (T1 - 1) // 2 + 1
    mods = build_transformer_modules(vocab=5000, seed=41)
    cnn, tr = mods["CNN"].to("cuda:0").eval(), mods["Transformer"].to("cuda:0").eval()
    feats = torch.randn(B, frames, 80, generator=torch.Generator().manual_seed(5)).cuda()
    lens = torch.linspace(0.6, 1.0, B).cuda()
    path = os.path.join(ROOT, "profiles", "transformer_bench.json")
    if args.precision == "bf16":  # added under its own key; the fp32 record of the file stays as it is
        with torch.no_grad():
            part = bench_bf16(native, args, lambda: tr.encode(cnn(feats), lens), len(tr.encoder.layers), B, T, lens)
        print(json.dumps({"precision_bf16": part}))
        with open(path) as f:
            res = json.loads(f.read())
        res["precision_bf16"] = part
        with open(path, "w") as f:
            f.write(json.dumps(res) + "\n")
        return
    res = {"workload": f"transformer.yaml encoder, {B} x {args.seconds:g} s ({frames} feature frames, T' = {T})", "batch": B,
           "frames": T, "steps": args.steps, "precision": "fp32"}
    with torch.no_grad():
        run = lambda: tr.encode(cnn(feats), lens)  # noqa: E731
        res["encoder_p50_ms"] = p50_ms(run, args.steps, args.warmup)
        rep = profiled(native, run, args.steps)
        total = sum(rep.values())
        res["encoder_kernel_ms"] = round(total, 3)
        blocks = {"conv_block1_5x5_cin1_ms": rep.get("conv_block5_cin1", 0.0), "conv_block2_5x5_mfma_ms": rep.get("conv_block5_mfma", 0.0),
                  "conv_block3_res1x1_ms": rep.get("conv_block_res1x1", 0.0)}
        res.update({k: round(v, 4) for k, v in blocks.items()})
        front = sum(blocks.values())
        res["front_end_share_of_kernel_time"] = round(front / total, 4)
        res["attention_dh128_ms_per_layer"] = round(rep["rope_attention"] / len(tr.encoder.layers), 4)
        res["kernels_ms"] = {k: round(v, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1])}

        # yardstick 1: the same attention problem as 8 heads of 64 (same d, B, T: identical FLOPs and bytes)
        qkv = torch.randn(B, T, 3 * 512, generator=torch.Generator().manual_seed(6)).cuda()
        kl = torch.round(lens * T).to(torch.int32)
        t128 = profiled(native, lambda: native.rope_attention(qkv, None, None, kl, 4, 1 / math.sqrt(128)), args.steps)["rope_attention"]
        t64 = profiled(native, lambda: native.rope_attention(qkv, None, None, kl, 8, 1 / math.sqrt(64)), args.steps)["rope_attention"]
        res["attention_dh128_ms"], res["attention_dh64_ms"] = round(t128, 4), round(t64, 4)
        res["attention_dh128_over_dh64"] = round(t128 / t64, 3)
        gflop = 4.0 * B * T * T * 512 / 1e9
        res["attention_dh128_tflops"], res["attention_dh64_tflops"] = round(gflop / t128, 2), round(gflop / t64, 2)

        # yardstick 2: block 2's contraction as a plain GEMM through sbk_gemm_nt_f32
        M = B * T * 20
        a = torch.randn(M, 1600, generator=torch.Generator().manual_seed(7)).cuda()
        w = (torch.randn(64, 1600, generator=torch.Generator().manual_seed(8)) / 40.0).cuda()
        with native.precision_scope("fp32"):
            g = profiled(native, lambda: native.gemm_nt(a, w), args.steps)
        gemm_ms = sum(g.values())
        gf = 2.0 * M * 1600 * 64 / 1e9
        res["block2_gflop"] = round(gf, 2)
        res["block2_tflops"] = round(gf / blocks["conv_block2_5x5_mfma_ms"], 2)
        res["gemm_nt_same_product_ms"], res["gemm_nt_same_product_tflops"] = round(gemm_ms, 4), round(gf / gemm_ms, 2)
        res["gemm_nt_kernels"] = sorted(g)
        res["block2_over_gemm_nt_rate"] = round(gemm_ms / blocks["conv_block2_5x5_mfma_ms"], 3)
    res["expectations"] = {"attention_dh128_over_dh64 <= 1.5": res["attention_dh128_over_dh64"] <= 1.5,
                           "block2_over_gemm_nt_rate >= 0.25": res["block2_over_gemm_nt_rate"] >= 0.25,
                           "front_end_share_of_kernel_time < 0.10": res["front_end_share_of_kernel_time"] < 0.10}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "transformer_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
