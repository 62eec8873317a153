"""Branchformer encoder time at branchformer_large.yaml's shape (18 layers, d 512, 8 heads, csgu_linear_units 3072, kernel 31),
random weights, 32 x 10 s (T' = 251 encoder frames, features [32,251,640] as the convolutional front-end hands them over):
the encoder's ms per batch, the CSGU launches' own time (HIP events) and bytes/s over their algorithmic bytes (the fused
launch reads 2C and writes C floats per frame, the statistics pass reads C more and writes two), and -- for context, in the
same run -- the Conformer-L encoder (12 layers, d_ffn 2048) on the same features.  One JSON line, also written to
profiles/branchformer_bench.json.  A job for a GPU visit.
``--precision bf16`` adds the reduced-precision leg under the key precision_bf16: both encoders under precision "bf16" with
sbk_relpos_attention_bf16 and, alternating, with the attention alone held to fp32 (the encoder before that kernel existed);
the attention's share of kernel time in both; and three attention launches at the encoder's shape by HIP events (relpos fp32,
relpos bf16, rope bf16 -- the last shows what the position ring costs).

    python tools/branchformer_bench.py [--steps 10] [--warmup 3] [--precision bf16]
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


def event_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e3


def attention_launches(native, B, T, steps, warmup, H=8, Dh=64):
    """relpos_attention fp32 / bf16 and rope_attention bf16 on the same qkv and key lengths, alternating; each one's best of three."""
    d, gen = H * Dh, torch.Generator().manual_seed(11)
    qkv = torch.randn(B, T, 3 * d, generator=gen).cuda()
    pos = torch.randn(2 * T - 1, d, generator=gen).cuda()
    u, v = (0.3 * torch.randn(d, generator=gen)).cuda(), (0.3 * torch.randn(d, generator=gen)).cuda()
    key_len = (torch.linspace(0.6, 1.0, B) * T).round().to(torch.int32).cuda()
    out = torch.empty(B, T, d, device="cuda:0")

    def scoped(precision, fn):
        def run():
            with native.precision_scope(precision):
                fn()
        return run

    relpos = lambda: native.relpos_attention(qkv, pos, u, v, key_len, H, Dh ** -0.5, out=out)  # noqa: E731
    runs = {"relpos_attention_fp32": scoped("fp32", relpos), "relpos_attention_bf16": scoped("bf16", relpos),
            "rope_attention_bf16": scoped("bf16", lambda: native.rope_attention(qkv, None, None, key_len, H, Dh ** -0.5, out=out))}
    us = {k: [] for k in runs}
    for _ in range(3):
        for k, fn in runs.items():
            us[k].append(event_us(fn, 10 * steps, warmup))
    best = {k: min(t) for k, t in us.items()}
    res = {"B": B, "T": T, "H": H, "Dh": Dh}
    for k, t in best.items():  # (6 flops per score and channel with the position term, 4 without)
        res[k + "_us"] = round(t, 1)
        res[k + "_tflops"] = round((4.0 if k.startswith("rope") else 6.0) * B * H * float(T) * T * Dh / t / 1e6, 1)
    res["bf16_speedup_over_fp32"] = round(best["relpos_attention_fp32"] / best["relpos_attention_bf16"], 2)
    res["ratio_to_rope_attention_bf16"] = round(best["relpos_attention_bf16"] / best["rope_attention_bf16"], 2)
    res["expectation bf16 relpos launch faster than fp32 in the same run"] = "met" if res["bf16_speedup_over_fp32"] > 1.0 else "missed"
    return res


def bf16_leg(native, models, feats, lens, steps, warmup):
    """Both encoders under precision "bf16", and -- the encoder as it ran before relpos_attention had a bf16 form -- the same with
    the attention call alone put back under "fp32" (bf16 GEMMs, fp32 attention), alternating in this run."""
    real = native.relpos_attention

    def fp32_attention(*a, **k):
        with native.precision_scope("fp32"):
            return real(*a, **k)

    res = {}
    for name, tr in models.items():
        ms, share = {"attention_fp32": [], "attention_bf16": []}, {}
        for _ in range(2):
            for mode in ms:
                native.relpos_attention = fp32_attention if mode == "attention_fp32" else real
                try:
                    with native.precision_scope("bf16"):
                        ms[mode].append(p50_ms(lambda: tr.encode(feats, lens), steps, warmup))
                        native.prof_reset()
                        native.prof_enable(True)
                        tr.encode(feats, lens)
                        torch.cuda.synchronize()
                        native.prof_enable(False)
                finally:
                    native.relpos_attention = real
                rep = native.prof_report()
                key = "relpos_attention" if mode == "attention_fp32" else "relpos_attention_bf16"
                share[mode] = round(rep[key]["ms"] / sum(v["ms"] for v in rep.values()), 4)
        res[name] = {"encoder_p50_ms_attention_fp32": min(ms["attention_fp32"]), "encoder_p50_ms": min(ms["attention_bf16"]),
                     "attention_share_of_kernel_time_before": share["attention_fp32"],
                     "attention_share_of_kernel_time_after": share["attention_bf16"],
                     "expectation encoder faster than with the fp32 attention":
                         "met" if min(ms["attention_bf16"]) < min(ms["attention_fp32"]) else "missed"}
    return res


def main():
    from speechbrain_amd import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="bf16: adds the reduced-precision leg (both encoders, the three attention launches) under precision_bf16")
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
        cf = build("conformer", 12)
        res["conformer_l_encoder_p50_ms"] = p50_ms(lambda: cf.encode(feats, lens), args.steps, args.warmup)
        if args.precision == "bf16":
            res["precision_bf16"] = {"attention": attention_launches(native, B, T, args.steps, args.warmup),
                                     **bf16_leg(native, {"branchformer": bf, "conformer_l": cf}, feats, lens, args.steps, args.warmup)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "branchformer_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
