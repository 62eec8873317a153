"""Transformer-encoder ASR (transformer.yaml) encoder time at the recipe's shape -- the three-block convolution front end (64
channels), 12 layers, d 512, 4 heads (head dim 128), d_ffn 2048 --, random weights, fp32, 32 x 10 s (1001 feature frames, T' = 251
encoder frames).  Reports the encoder's ms per batch (front end + encode), the kernels' own time from the profiler (HIP events):
the three conv blocks, the head-dim-128 attention, and, in the same run, the two yardsticks the new kernels are held against:

  * the head-dim-64 attention at H = 8 on the same d = 512, B and T (identical FLOPs and bytes): dh128 / dh64 should be <= 1.5;
  * sbk_gemm_nt_f32 on the plain [B*T2*20 x 1600] x [1600 x 64] product block 2 contracts: block 2 should reach >= 1/4 of it;
  * the front end should stay under 10 % of the encoder's kernel time.

One JSON line, also written to profiles/transformer_bench.json.  A job for a GPU visit.

    python tools/transformer_bench.py [--steps 10] [--warmup 3]
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


def main():
    from speechbrain_amd import native
    from speechbrain_amd.inference.builders import build_transformer_modules

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
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
