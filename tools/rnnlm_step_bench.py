"""Time one RNNLM scorer step (sbk_rnnlm_step_f32, csrc/rnnlm_step.hip) at the LibriSpeech RNNLM shape -- embedding 128, two LSTM layers
of 2 048, one DNN block of 512, 1 000 tokens -- for n = 320 (32 utterances x beam 10) and n = 32 hypothesis rows, against
  (a) the same LSTM stack composed from what the library had before: an explicit gather of the state (index_select), the input
      product with sbk_gemm_nt_f32 and the recurrence with sbk_lstm_f32 (native.lstm over one time step);
  (b) one torch.nn.LSTM step on the same tensors after the same index_select.
The comparators time the LSTM stack only; `lstm` is the new step's LSTM launches alone (from the library's profiler), `step` the
whole entry with the DNN block, the output layer and the log-softmax.  Blocks alternate (new, a, b, new, a, b, ...) and every figure
is the median over the blocks of a block's mean; device events around each block.

    python tools/rnnlm_step_bench.py [--rows 320 32] [--blocks 5] [--iters 50] [--out profiles/rnnlm_step_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from speechbrain_amd import native  # noqa: E402

V, E, H, L, D = 1000, 128, 2048, 2, 512


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[320, 32])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    native.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(7)
    rn = lambda *s: (torch.randn(*s, generator=gen)).to(dev)  # noqa: E731
    layers = [(rn(4 * H, E if l == 0 else H) / (E if l == 0 else H) ** 0.5, rn(4 * H, H) / H ** 0.5, rn(4 * H) * 0.1, rn(4 * H) * 0.1)
              for l in range(L)]
    prep = native.RNNLMPrepared(rn(V, E), layers, [(rn(D, H) / H ** 0.5, rn(D) * 0.1, torch.ones(D, device=dev), torch.zeros(D, device=dev), 1e-5)],
                                rn(V, D) / D ** 0.5, rn(V) * 0.1, native.ACT_LEAKY_RELU)
    ref = torch.nn.LSTM(E, H, L, batch_first=True).to(dev)
    with torch.no_grad():
        for l, ws in enumerate(layers):
            for name, w in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), ws):
                getattr(ref, f"{name}_l{l}").copy_(w)
    emb = rn(V, E)
    result = dict(shape=dict(vocab=V, embedding=E, hidden=H, layers=L, dnn=D), rows={})
    for n in args.rows:
        tokens = torch.randint(0, V, (n,), generator=gen, dtype=torch.int32).to(dev)
        parent = torch.randint(0, n, (n,), generator=gen, dtype=torch.int32).to(dev)
        plong = parent.long()
        state = [native.rnnlm_state(prep, n).normal_(generator=None).mul_(0.3), native.rnnlm_state(prep, n)]
        x = emb[tokens.long()].unsqueeze(1).contiguous()

        def new():
            native.rnnlm_step(prep, tokens, parent, state[0], state[1])

        def composed():
            h, c = state[0][:, 0].index_select(1, plong), state[0][:, 1].index_select(1, plong)
            native.lstm(x, layers, (h, c))

        def torch_lstm():
            h, c = state[0][:, 0].index_select(1, plong), state[0][:, 1].index_select(1, plong)
            ref(x, (h, c))

        fns = dict(step=new, composed=composed, torch_lstm=torch_lstm)
        with torch.no_grad():
            for fn in fns.values():  # warm up every shape the timed window uses
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(args.blocks):
                for k, fn in fns.items():
                    times[k].append(timed(fn, args.iters))
            native.prof_reset()
            native.prof_enable(True)
            for _ in range(10):
                new()
            torch.cuda.synchronize()
            native.prof_enable(False)
        lstm_us = native.prof_report()["rnnlm_lstm"]
        row = {k: dict(median_us=statistics.median(v), blocks_us=[round(t, 2) for t in v]) for k, v in times.items()}
        row["lstm"] = dict(mean_us=lstm_us["ms"] * 1e3 / 10, launches=lstm_us["count"])
        result["rows"][str(n)] = row
        print(f"n={n}: step {row['step']['median_us']:.1f} us (its LSTM launches {row['lstm']['mean_us']:.1f} us), composed "
              f"{row['composed']['median_us']:.1f} us, torch.nn.LSTM + index_select {row['torch_lstm']['median_us']:.1f} us", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
