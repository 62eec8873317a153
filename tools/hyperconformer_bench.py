"""HyperConformer encoder time at the hyperconformer_8M (10 layers, d 144, d_ffn 576) and hyperconformer_22M (10 layers, d 256,
d_ffn 1024) shapes -- random weights, fp32, 32 x 10 s (T' = 251 encoder frames) -- and, in the same run, the fused mixer
(``native.hypermix``, csrc/hypermix.hip) next to three comparators, alternating, in microseconds per call (HIP events):

  1. the composition it replaces in the reference: tests/hypermixing_host_ref.py in fp32 on the same GPU and tensors (it writes
     the two generated weight tensors [B,H,T',d_ffn/H]).  RECORDED expectation: the fused call is faster.
  2. what HyperMixing replaces in the model: norm1 + RelPosMHAXL with its projections (ConformerEncoderLayer._mha) at the same
     B, T', d, H (4 heads of 36 at d 144: the attention kernel has no head width 18) -- at T' = 251 and T' = 751 (30 s).
     Recorded without an expectation.
  3. a plain device copy: hypermix's algorithmic bytes (h read twice, residual read, out written, generator weights) over its time
     as a fraction of the copy's rate.

Every GPU step runs in a fresh child process under its own time limit, one at a time; the first step that fails or runs out of
time ends the run (nothing more is started on the GPU) and is recorded.  ``--headline NAME=FILE`` copies the JSON result line of
a ``bench.py`` run (e.g. this tree's and the parent commit's, from the same visit) into the result.  One JSON line per run, also
written to profiles/hyperconformer_bench.json.  A job for a GPU visit.

    python tools/hyperconformer_bench.py [--steps 5] [--warmup 2] [--shapes 8M,22M] [--headline this=a.json ...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"8M": dict(d=144, H=8, d_ffn=576, layers=10), "22M": dict(d=256, H=8, d_ffn=1024, layers=10)}
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
    from speechbrain_amd.lobes.models.transformer.Conformer import ConformerEncoder

    native.load()
    s, B, T = SHAPES[name], args.batch, 251
    torch.manual_seed(3)
    enc = ConformerEncoder(num_layers=s["layers"], d_model=s["d"], d_ffn=s["d_ffn"], nhead=s["H"], kernel_size=31,
                           attention_type="hypermixing").to("cuda:0").eval()
    x = torch.randn(B, T, s["d"], generator=torch.Generator().manual_seed(5)).cuda()
    key_len = (torch.linspace(0.6, 1.0, B) * T).round().long()
    pad = (torch.arange(T)[None, :] >= key_len[:, None]).cuda()
    res = {"shape": name, "batch": B, "seconds": 10.0, "frames": T, **s}
    with torch.no_grad():
        run = lambda: enc(x, src_key_padding_mask=pad)  # noqa: E731
        ms = p50_ms(torch, run, args.steps, args.warmup)
        res["encoder_p50_ms"] = round(ms, 3)
        res["audio_sec_per_sec"] = round(B * 10.0 / (ms / 1e3), 1)
        native.prof_reset()
        native.prof_enable(True)
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = {k: v["ms"] / args.steps for k, v in native.prof_report().items()}
        hm = sum(v for k, v in rep.items() if k.startswith("hypermix"))
        res["encoder_kernel_ms"] = round(sum(rep.values()), 3)
        res["hypermix_ms_per_layer"] = round(hm / s["layers"], 4)
        res["hypermix_share_of_kernel_time"] = round(hm / sum(rep.values()), 4)
        res["kernels_ms"] = {k: round(v, 4) for k, v in sorted(rep.items(), key=lambda kv: -kv[1])}
    return res


def mixer_step(args):
    """native.hypermix next to the fp32 composition, norm1 + RelPosMHAXL and a device copy, alternating in one process."""
    import torch

    import hypermixing_host_ref as R
    from speechbrain_amd import native
    from speechbrain_amd.lobes.models.transformer.Conformer import ConformerEncoderLayer
    from speechbrain_amd.nnet.attention import RelPosEncXL

    native.load()
    B, out = args.batch, []
    for name, s in SHAPES.items():
        d, H, d_ffn = s["d"], s["H"], s["d_ffn"]
        Dh, k = d // H, d_ffn // H
        torch.manual_seed(7)
        mix_layer = ConformerEncoderLayer(d, d_ffn, H, kernel_size=31, attention_type="hypermixing").to("cuda:0").eval()
        # (the attention kernel has no head width 18: at d 144 the comparator runs 4 heads of 36, the conformer_small layout)
        att_H = H if d // H in (8, 16, 32, 36, 64) else 4
        att_layer = ConformerEncoderLayer(d, d_ffn, att_H, kernel_size=31, attention_type="RelPosMHAXL").to("cuda:0").eval()
        relpos = RelPosEncXL(d).to("cuda:0")
        for T in (251, 751):
            gen = torch.Generator().manual_seed(11)
            x = torch.randn(B, T, d, generator=gen).cuda()
            key_len = (torch.linspace(0.6, 1.0, B) * T).round().to(torch.int32).cuda()
            pos = relpos(x)
            m, ln1 = mix_layer.mha_layer, mix_layer.norm1.norm
            with torch.no_grad():
                h = native.layernorm(x, ln1.weight, ln1.bias, ln1.eps)
                pe = m.positional_encoding.pe[0]
                o = torch.empty_like(x)
                fused = lambda: m.core(h, key_len, residual=x, out=o)  # noqa: E731
                g1, g2 = [t.detach() for t in m.hyper.w1_gen.tensors()], [t.detach() for t in m.hyper.w2_gen.tensors()]
                comp = lambda: R.hypermix(h, key_len, pe, g1, g2, m.layer_norm.weight, m.layer_norm.bias, 1e-5, H, residual=x)  # noqa: E731
                err = float((fused() - comp()).abs().max())
                mixed = lambda: mix_layer._mha(x, None, key_len)  # noqa: E731
                attn = lambda: att_layer._mha(x, pos, key_len)  # noqa: E731
                src = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0")
                dst = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0")
                copy = lambda: dst.copy_(src)  # noqa: E731
                us = {n: [] for n in ("fused", "comp", "mixed", "attn", "copy")}
                for _ in range(3):  # alternate, keep each one's best of three: clock and cache state are shared
                    for n, fn in (("fused", fused), ("comp", comp), ("mixed", mixed), ("attn", attn), ("copy", copy)):
                        us[n].append(event_us(torch, fn, 10 * args.steps, args.warmup))
                native.prof_reset()
                native.prof_enable(True)
                for _ in range(10):
                    fused()
                torch.cuda.synchronize()
                native.prof_enable(False)
                launches = {n: round(v["ms"] / 10 * 1e3, 1) for n, v in native.prof_report().items() if n.startswith("hypermix")}
            best = {n: min(v) for n, v in us.items()}
            alg_bytes = 4.0 * (4.0 * B * T * d + 2.0 * H * (Dh * Dh + Dh + k * Dh + k))
            copy_rate = 2.0 * (64 << 20) / best["copy"]  # bytes per microsecond, read + write
            r = {"shape": name, "B": B, "T": T, "d": d, "H": H, "Dh": Dh, "k": k, "hypermix_us": round(best["fused"], 1),
                 "hypermix_launches_us": launches, "composition_fp32_us": round(best["comp"], 1),
                 "composition_over_hypermix": round(best["comp"] / best["fused"], 2),
                 "fused_vs_composition_max_abs_diff": err,
                 "norm1_plus_hypermix_us": round(best["mixed"], 1), "norm1_plus_relpos_mha_us": round(best["attn"], 1),
                 "relpos_mha_heads": att_H,
                 "relpos_mha_over_hypermix": round(best["attn"] / best["mixed"], 2),
                 "copy_gbytes_per_s": round(copy_rate / 1e3, 1), "hypermix_algorithmic_mbytes": round(alg_bytes / 1e6, 2),
                 "hypermix_fraction_of_copy_rate": round(alg_bytes / best["fused"] / copy_rate, 3),
                 "generated_weights_avoided_mbytes": round(2 * 4.0 * B * T * d_ffn / 1e6, 1)}
            r["expectation fused faster than the composition"] = "met" if best["fused"] < best["comp"] else "missed"
            out.append(r)
    return out


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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--shapes", default="8M,22M")
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process: mixer | encoder:<shape>")
    ap.add_argument("--headline", action="append", default=[], metavar="NAME=FILE",
                    help="a file whose last line is a bench.py JSON result, recorded under bench_py[NAME]")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(mixer_step(args) if args.step == "mixer" else encoder_step(args.step.split(":", 1)[1], args)))
        return
    res = {"workload": f"HyperConformer encoder, {args.batch} x 10 s, T' = 251, fp32, random weights", "steps": args.steps,
           "shapes": [], "mixer": None, "failed": None}
    for step in ["mixer"] + [f"encoder:{s}" for s in args.shapes.split(",") if s]:
        out, err = child(step, args)
        if err:  # (nothing more is started on the GPU after a step that failed or hung)
            res["failed"] = err
            break
        if step == "mixer":
            res["mixer"] = out
        else:
            res["shapes"].append(out)
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
    with open(os.path.join(ROOT, "profiles", "hyperconformer_bench.json"), "w") as f:
        f.write(line + "\n")
    if res["failed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
