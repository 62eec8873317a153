"""Branchformer encoder time at branchformer_large.yaml's shape (18 layers, d 512, 8 heads, csgu_linear_units 3072, kernel 31),
random weights, 32 x 10 s (T' = 251 encoder frames, features [32,251,640] as the convolutional front-end hands them over):
the encoder's ms per batch, the CSGU launches' own time (HIP events) and bytes/s over their algorithmic bytes (the fused
launch reads 2C and writes C floats per frame, the statistics pass reads C more and writes two), and -- for context, in the
same run -- the Conformer-L encoder (12 layers, d_ffn 2048) on the same features.  One JSON line, also written to
profiles/branchformer_bench.json.  A job for a GPU visit.

    python tools/branchformer_bench.py [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

COPY_TBPS = 6.3  # what a plain copy kernel reaches on this part


def build(encoder_module, layers):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR

    torch.manual_seed(41)
    tr = TransformerASR(input_size=640, tgt_vocab=5000, d_model=512, nhead=8, num_encoder_layers=layers, num_decoder_layers=0,
                        d_ffn=2048, dropout=0.1, activation=torch.nn.GELU, branchformer_activation=torch.nn.GELU,
                        encoder_module=encoder_module, csgu_linear_units=3072, kernel_size=31, attention_type="RelPosMHAXL",
                        normalize_before=True, causal=False)
    with torch.no_grad():
        for n, p in tr.named_parameters():
            if n.endswith("csgu.conv.conv.weight"):  # (drawn with std 1e-6 by the constructor)
                p.normal_(0.0, 0.1)
    return tr.to("cuda:0").eval()


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


def main():
    from speechbrain_amd import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    native.load()
    B = args.batch
    frames = 1 + int(args.seconds * 16000) // 160
    T = ((frames - 1) // 2 + 1 - 1) // 2 + 1  # two stride-2 blocks of the convolutional front-end
    feats = torch.randn(B, T, 640, generator=torch.Generator().manual_seed(5)).cuda()
    lens = torch.linspace(0.6, 1.0, B).cuda()
    res = {"workload": f"branchformer_large encoder, {B} x {args.seconds:g} s (T' = {T})", "batch": B, "frames": T,
           "steps": args.steps}
    with torch.no_grad():
        bf = build("branchformer", 18)
        res["branchformer_encoder_p50_ms"] = p50_ms(lambda: bf.encode(feats, lens), args.steps, args.warmup)
        native.prof_reset()
        native.prof_enable(True)
        for _ in range(args.steps):
            bf.encode(feats, lens)
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
        total = sum(v["ms"] for v in rep.values())
        for key in ("csgu", "csgu_stats"):
            r = rep[key]
            res[f"{key}_launch_us"] = round(1e3 * r["ms"] / r["count"], 2)
            res[f"{key}_algorithmic_TBps"] = round(r["bytes"] / (r["ms"] * 1e-3) / 1e12, 3)
        both_ms = rep["csgu"]["ms"] + rep["csgu_stats"]["ms"]
        res["csgu_both_launches_us"] = round(1e3 * both_ms / rep["csgu"]["count"], 2)
        res["csgu_both_algorithmic_TBps"] = round((rep["csgu"]["bytes"] + rep["csgu_stats"]["bytes"]) / (both_ms * 1e-3) / 1e12, 3)
        res["csgu_share_of_kernel_time"] = round(both_ms / total, 4)
        res["copy_kernel_TBps"] = COPY_TBPS
        res["branchformer_kernel_ms_by_name"] = {k: round(v["ms"] / args.steps, 3) for k, v in
                                                 sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}
        del bf
        cf = build("conformer", 12)
        res["conformer_l_encoder_p50_ms"] = p50_ms(lambda: cf.encode(feats, lens), args.steps, args.warmup)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "branchformer_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
