"""Greedy decoding with the GRU attention decoder at the train_BPE_1000.yaml shape (embedding 128, one GRU layer of 1024, location-
aware attention 1024 with 10 channels and kernel 100, encoder states 512, 1000 tokens) -- random weights, fp32, B 32 utterances of
T' = 250 encoder frames -- in HIP events, with the parts next to their comparators in the same run, alternating:

  greedy   native.attn_rnn_greedy (sbk_attn_rnn_greedy_f32, one C call per batch) for 40 and for 120 steps (no utterance ends: the
           output layer's eos bias is lowered), p50 of each; the time of a step is the difference over the 80 steps (the one-off
           work -- mlp_enc over the encoder states, the checks -- drops out).
  torch    the same search written here in plain torch operations on the same device and tensors (embedding, torch.gru_cell,
           conv1d, tanh, softmax, bmm, linear, argmax), alternating with the above; the share of equal tokens is recorded.
  profile  one 40-step search under the library's per-launch timing: launches per step, the kernel time of a step, the two
           kernels of sbk_attn_rnn_attend_f32 (attn_rnn_energy, attn_rnn_softmax_ctx) with their algorithmic bytes over time, next
           to a plain device copy of the same number of bytes timed in the same process before and after.
  RECORDED expectation: "faster than the torch composition; the step is launch-bound at 32 rows" -- the first half is met when
  the step takes less time than the torch composition's, the second when the kernels of a step together run for less than half
  of the step's time.

Every GPU step runs in a fresh child process under its own time limit, one at a time; the first step that fails or runs out of
time ends the run (nothing more is started on the GPU) and is recorded.  ``--headline NAME=FILE`` copies the JSON result line of
a ``bench.py`` run into the result.  One JSON line per run, also written to profiles/s2srnn_bench.json.  A job for a GPU visit.

    python tools/s2srnn_bench.py [--steps 5] [--warmup 2] [--headline this1=a.json ...]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_TIMEOUT_S = 240
EMB, HID, ATT, ENC, VOCAB, CH, KS, T_ENC = 128, 1024, 1024, 512, 1000, 10, 100, 250
SHORT, LONG = 40, 120
BOS, EOS = 0, 0


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


def build(torch, B):
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import AttentionalRNNDecoder

    torch.manual_seed(3)
    emb = Embedding(num_embeddings=VOCAB, embedding_dim=EMB)
    dec = AttentionalRNNDecoder(rnn_type="gru", attn_type="location", hidden_size=HID, attn_dim=ATT, num_layers=1, enc_dim=ENC,
                                input_size=EMB, scaling=1.0, channels=CH, kernel_size=KS, re_init=True, dropout=0.15)
    lin = Linear(input_size=HID, n_neurons=VOCAB)
    with torch.no_grad():
        dec.attn.mlp_attn.weight.mul_(8.0)
        dec.attn.conv_loc.weight.mul_(8.0)
        lin.w.weight.mul_(8.0)
        lin.w.bias[EOS] -= 50.0  # no utterance ends: every search runs the steps it is given
    for m in (emb, dec, lin):
        m.to("cuda:0").eval()
    enc = torch.randn(B, T_ENC, ENC, generator=torch.Generator().manual_seed(5)).cuda()
    enc_len = torch.full((B,), T_ENC, dtype=torch.int32, device="cuda:0")
    prep = dec.prepared(enc.device, emb=emb.Embedding.weight, fc=(lin.w.weight, lin.w.bias))
    return emb, dec, lin, enc, enc_len, prep


def torch_greedy(torch, emb, dec, lin, enc, enc_len, steps):
    """The search in plain torch operations: tokens [B,steps]."""
    F = torch.nn.functional
    a, cell = dec.attn, dec.rnn.rnn_cells[0]
    B, T, _ = enc.shape
    enc_h = F.linear(enc, a.mlp_enc.weight, a.mlp_enc.bias)
    mask = torch.arange(T, device=enc.device)[None, :] < enc_len[:, None]
    prev = mask.float() / enc_len.float()[:, None]
    tok = torch.full((B,), BOS, dtype=torch.long, device=enc.device)
    c = torch.zeros(B, ATT, device=enc.device)
    h = torch.zeros(B, HID, device=enc.device)
    out = []
    for _ in range(steps):
        x = torch.cat([emb.Embedding.weight[tok], c], dim=-1)
        h = torch.gru_cell(x, h, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)
        loc = F.linear(F.conv1d(prev[:, None, :], a.conv_loc.weight, padding=KS).transpose(1, 2), a.mlp_loc.weight, a.mlp_loc.bias)
        e = F.linear(torch.tanh(enc_h + F.linear(h, a.mlp_dec.weight, a.mlp_dec.bias)[:, None, :] + loc), a.mlp_attn.weight)[..., 0]
        prev = torch.softmax(e.masked_fill(~mask, float("-inf")) * dec.scaling, dim=-1)
        c = F.linear(torch.bmm(prev[:, None, :], enc)[:, 0], a.mlp_out.weight, a.mlp_out.bias)
        logits = F.linear(F.linear(torch.cat([c, h], dim=1), dec.proj.weight, dec.proj.bias), lin.w.weight, lin.w.bias)
        tok = logits.argmax(dim=-1)
        out.append(tok)
    return torch.stack(out, 1)


def greedy_step(args):
    import torch

    from speechbrain_amd import native

    native.load()
    B = args.batch
    emb, dec, lin, enc, enc_len, prep = build(torch, B)
    res = {"batch": B, "encoder_frames": T_ENC, "steps_short": SHORT, "steps_long": LONG}
    with torch.no_grad(), native.precision_scope("fp32"):
        ours = {n: (lambda n=n: native.attn_rnn_greedy(prep, enc, enc_len, n, BOS, EOS)) for n in (SHORT, LONG)}
        theirs = {n: (lambda n=n: torch_greedy(torch, emb, dec, lin, enc, enc_len, n)) for n in (SHORT, LONG)}
        tok, _, ran = ours[LONG]()
        assert ran == LONG, ran
        res["share_of_tokens_equal_to_the_torch_composition"] = round(float((tok.long() == theirs[LONG]()).float().mean()), 4)
        t = {("ours", n): [] for n in (SHORT, LONG)}
        t.update({("torch", n): [] for n in (SHORT, LONG)})
        for _ in range(2):  # alternate
            for n in (SHORT, LONG):
                t[("ours", n)] += event_ms(torch, ours[n], args.steps, args.warmup)
                t[("torch", n)] += event_ms(torch, theirs[n], args.steps, args.warmup)
    p50 = {k: med(sorted(v)) for k, v in t.items()}
    for who in ("ours", "torch"):
        name = "greedy" if who == "ours" else "torch_composition"
        res[f"{name}_ms_{SHORT}_steps"], res[f"{name}_ms_{LONG}_steps"] = round(p50[(who, SHORT)], 3), round(p50[(who, LONG)], 3)
        res[f"{name}_us_per_step"] = round((p50[(who, LONG)] - p50[(who, SHORT)]) * 1e3 / (LONG - SHORT), 2)
    res["expectation faster than the torch composition"] = "met" if res["greedy_us_per_step"] < res["torch_composition_us_per_step"] else "missed"
    return res


def profile_step(args):
    import torch

    from speechbrain_amd import native

    native.load()
    B = args.batch
    _, _, _, enc, enc_len, prep = build(torch, B)

    def profiled(n):
        native.prof_reset()
        native.prof_enable(True)
        with torch.no_grad(), native.precision_scope("fp32"):
            native.attn_rnn_greedy(prep, enc, enc_len, n, BOS, EOS)
        torch.cuda.synchronize()
        native.prof_enable(False)
        return native.prof_report()

    with torch.no_grad(), native.precision_scope("fp32"):
        native.attn_rnn_greedy(prep, enc, enc_len, SHORT, BOS, EOS)  # warm
    short, rep = profiled(SHORT), profiled(LONG)
    span = LONG - SHORT
    per_step = {k: ((v["count"] - short.get(k, {"count": 0})["count"]) / span, (v["ms"] - short.get(k, {"ms": 0.0})["ms"]) * 1e3 / span)
                for k, v in rep.items()}
    res = {"batch": B, "launches_per_step": round(sum(c for c, _ in per_step.values()), 2),
           "kernel_us_per_step": round(sum(us for _, us in per_step.values()), 2),
           "kernels_per_step": {k: [round(c, 2), round(us, 2)] for k, (c, us) in sorted(per_step.items(), key=lambda kv: -kv[1][1]) if c > 0}}
    attend_bytes = 0.0
    for k in ("attn_rnn_energy", "attn_rnn_softmax_ctx"):
        v = rep[k]
        us, nbytes = v["ms"] * 1e3 / v["count"], v["bytes"] / v["count"]
        attend_bytes += nbytes
        res[k] = {"us": round(us, 2), "algorithmic_MB": round(nbytes / 1e6, 2), "TB_per_s": round(nbytes / us / 1e6, 3)}
    res["attend_us"] = round(res["attn_rnn_energy"]["us"] + res["attn_rnn_softmax_ctx"]["us"], 2)
    res["attend_TB_per_s"] = round(attend_bytes / res["attend_us"] / 1e6, 3)
    # a plain device copy that moves the same number of bytes (half read, half written)
    n = int(attend_bytes // 8)
    src, dst = torch.randn(n, device="cuda:0"), torch.empty(n, device="cuda:0")
    ms = event_ms(torch, lambda: dst.copy_(src), 20, 5)
    res["device_copy_of_the_same_bytes"] = {"us": round(med(ms) * 1e3, 2), "TB_per_s": round(8.0 * n / (med(ms) * 1e3) / 1e6, 3)}
    return res


STEPS = {"greedy": greedy_step, "profile": profile_step}


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
    ap.add_argument("--step", default=None, help="(internal) run one GPU step in this process: " + " | ".join(STEPS))
    ap.add_argument("--headline", action="append", default=[], metavar="NAME=FILE",
                    help="a file whose last line is a bench.py JSON result, recorded under bench_py[NAME]")
    ap.add_argument("--reuse", default=None, metavar="FILE",
                    help="take the GPU steps' results from this earlier result file and only add the --headline entries")
    args = ap.parse_args()
    if args.step:
        print(json.dumps(STEPS[args.step](args)))
        return
    res = {"workload": f"S2SRNN greedy decoding (train_BPE_1000.yaml decoder shape), {args.batch} x {T_ENC} encoder frames, fp32, "
                       "random weights", "steps": args.steps, "failed": None}
    if args.reuse:
        with open(args.reuse) as f:
            res = json.loads(f.read().strip().splitlines()[-1])
    for step in [] if args.reuse else STEPS:
        out, err = child(step, args)
        if err:  # (nothing more is started on the GPU after a step that failed or hung)
            res["failed"] = err
            break
        res[step] = out
    if not res["failed"]:
        share = res["profile"]["kernel_us_per_step"] / res["greedy"]["greedy_us_per_step"]
        res["kernel_time_share_of_the_step"] = round(share, 3)
        res["expectation the step is launch-bound at 32 rows"] = "met" if share < 0.5 else "missed"
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
    with open(os.path.join(ROOT, "profiles", "s2srnn_bench.json"), "w") as f:
        f.write(line + "\n")
    if res["failed"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
