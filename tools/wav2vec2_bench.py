"""wav2vec 2.0 encoder time at the wav2vec2-base (group norm, d 768, 12 layers) and wav2vec2-large (layer norm, stable, d 1024,
24 layers) shapes -- random weights (Wav2Vec2.from_config), fp32, 32 x 10 s (T0 = 31 999 frames after the first convolution,
T' = 499 encoder frames).  Per shape: the encoder's ms per batch and audio-seconds per second, the kernels' own time from the
profiler (HIP events), and in the same run the yardsticks the two new kernels are held against:

  * the feature encoder (seven convolutions) should stay under 25 % of the encoder's kernel time;
  * sbk_w2v_conv0_f32 over its algorithmic bytes (read the waveform, write the activation once) should reach >= 0.5 of a plain
    device copy of the activation's size;
  * sbk_w2v_posconv_f32 should reach >= 0.25 of native.gemm_nt's rate on the plain [B*T' x cg*k] x [cg*k x cg] product.

One JSON line per run, also written to profiles/wav2vec2_bench.json.  A job for a GPU visit.

    python tools/wav2vec2_bench.py [--steps 5] [--warmup 2] [--shapes base,large]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = {
    "base": dict(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, feat_extract_norm="group",
                 conv_bias=False, do_stable_layer_norm=False),
    "large": dict(hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
                  feat_extract_norm="layer", conv_bias=True, do_stable_layer_norm=True),
}


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
    return times[len(times) // 2] * 1e3


def profiled(native, fn, steps):
    """name -> ms per call of fn (the profiler's HIP-event times, summed over the launches of one call)."""
    native.prof_reset()
    native.prof_enable(True)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    native.prof_enable(False)
    return {k: v["ms"] / steps for k, v in native.prof_report().items()}


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def run_shape(native, name, args):
    from speechbrain_amd.integrations.huggingface.wav2vec2 import Wav2Vec2

    B, N = args.batch, int(args.seconds * 16000)
    w = Wav2Vec2.from_config(SHAPES[name], normalize_wav=(name == "large"), output_norm=True, seed=3).to("cuda:0")
    cfg = w.model.config
    wav = (0.3 * torch.randn(B, N, generator=torch.Generator().manual_seed(5))).cuda()
    lens = torch.linspace(0.6, 1.0, B).cuda()
    T0, T = (N - 10) // 5 + 1, int(w.model.feat_lengths(N))
    d, G, k, C0 = cfg["hidden_size"], cfg["num_conv_pos_embedding_groups"], cfg["num_conv_pos_embeddings"], cfg["conv_dim"][0]
    cg = d // G
    res = {"shape": name, "batch": B, "seconds": args.seconds, "frames": T, "layers": cfg["num_hidden_layers"], "d": d}
    with torch.no_grad():
        run = lambda: w(wav, lens)  # noqa: E731
        ms = p50_ms(run, args.steps, args.warmup)
        res["encoder_p50_ms"] = round(ms, 3)
        res["audio_sec_per_sec"] = round(B * args.seconds / (ms / 1e3), 1)
        rep = profiled(native, run, args.steps)
        total = sum(rep.values())
        feat = profiled(native, lambda: w.model.features(wav, w.normalize_wav), args.steps)
        res["encoder_kernel_ms"] = round(total, 3)
        res["feature_encoder_kernel_ms"] = round(sum(feat.values()), 3)
        res["feature_encoder_share_of_kernel_time"] = round(sum(feat.values()) / total, 4)
        res["kernels_ms"] = {k_: round(v, 4) for k_, v in sorted(rep.items(), key=lambda kv: -kv[1])}
        # conv0 against a plain device copy of the activation's size
        c0_ms = rep["w2v_conv0"]
        c0_bytes = 4.0 * B * N + 4.0 * B * T0 * C0
        src = torch.empty(B * T0 * C0, dtype=torch.float32, device="cuda:0").normal_()
        dst = torch.empty_like(src)
        copy_ms = event_ms(lambda: dst.copy_(src), args.steps, args.warmup)
        res["conv0_ms"], res["conv0_stats_ms"] = round(c0_ms, 4), round(rep.get("w2v_conv0_stats", 0.0), 4)
        res["conv0_gbytes_per_s"] = round(c0_bytes / c0_ms / 1e6, 1)
        res["device_copy_gbytes_per_s"] = round(2.0 * src.numel() * 4 / copy_ms / 1e6, 1)
        res["conv0_over_copy_rate"] = round(res["conv0_gbytes_per_s"] / res["device_copy_gbytes_per_s"], 3)
        del src, dst
        # posconv against gemm_nt on the plain product of one group
        pc_ms = rep["w2v_posconv"]
        gf = 2.0 * B * T * d * cg * k / 1e9
        a = torch.randn(B * T, cg * k, generator=torch.Generator().manual_seed(7)).cuda()
        wg = (torch.randn(cg, cg * k, generator=torch.Generator().manual_seed(8)) / (cg * k) ** 0.5).cuda()
        with native.precision_scope("fp32"):
            g = profiled(native, lambda: native.gemm_nt(a, wg), args.steps)
        gemm_ms = sum(g.values())
        res["posconv_ms"], res["posconv_tflops"] = round(pc_ms, 4), round(gf / pc_ms, 2)
        res["gemm_nt_one_group_ms"] = round(gemm_ms, 4)
        res["gemm_nt_one_group_tflops"] = round(gf / G / gemm_ms, 2)
        res["gemm_nt_kernels"] = sorted(g)
        res["posconv_over_gemm_nt_rate"] = round(res["posconv_tflops"] / res["gemm_nt_one_group_tflops"], 3)
    res["expectations"] = {"feature_encoder_share_of_kernel_time < 0.25": res["feature_encoder_share_of_kernel_time"] < 0.25,
                           "conv0_over_copy_rate >= 0.5": res["conv0_over_copy_rate"] >= 0.5,
                           "posconv_over_gemm_nt_rate >= 0.25": res["posconv_over_gemm_nt_rate"] >= 0.25}
    return res


def main():
    from speechbrain_amd import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--shapes", default="base,large")
    args = ap.parse_args()
    native.load()
    res = {"workload": f"wav2vec 2.0 encoder, {args.batch} x {args.seconds:g} s, fp32, random weights", "steps": args.steps,
           "shapes": [run_shape(native, name, args) for name in args.shapes.split(",")]}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "wav2vec2_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
