"""EncoderASR throughput at the LibriSpeech CTC recipe's shape (d 256, 4 heads, d_ffn 1 024, 18 layers, 31 characters):
transcribe_batch of 32 x 10 s from 16-bit PCM with greedy decoding and with CTCBeamSearcher (beam 100, beam_prune_logp
-12, token_prune_min_logp -1.2, prune_history False), plus the decode kernels' own times (HIP events).  One JSON line.

    python tools/ctc_bench.py [--steps 10] [--warmup 3]
"""
import argparse
import functools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CHARS = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "-", "."]
CFG = dict(d_model=256, nhead=4, d_ffn=1024, n_enc=18, n_dec=0, n_fft=512, win_length=32)
BEAM = dict(blank_index=0, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2, prune_history=False, topk=1)


def build(decoding):
    from speechbrain_amd.dataio.encoder import CTCTextEncoder
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher, ctc_greedy_decode
    from speechbrain_amd.inference.ASR import EncoderASR
    from speechbrain_amd.inference.builders import build_modules
    from speechbrain_amd.lobes.models.transformer.TransformerASR import EncoderWrapper
    from speechbrain_amd.nnet.containers import LengthsCapableSequential

    m = build_modules(CFG, vocab=len(CHARS), seed=21)
    with torch.no_grad():
        m["ctc_lin"].w.weight.mul_(8.0)
    enc = LengthsCapableSequential(compute_features=m["compute_features"], normalize=m["normalize"], CNN=m["CNN"],
                                   transformer_encoder=EncoderWrapper(m["Transformer"]), ctc_lin=m["ctc_lin"],
                                   log_softmax=torch.nn.LogSoftmax(dim=-1))
    tok = CTCTextEncoder()
    tok.lab2ind, tok.ind2lab, tok.blank_label = {c: i for i, c in enumerate(CHARS)}, dict(enumerate(CHARS)), "<blank>"
    fn = functools.partial(ctc_greedy_decode, blank_id=0) if decoding == "greedy" else CTCBeamSearcher
    return EncoderASR(modules={"encoder": enc}, hparams={"tokenizer": tok, "decoding_function": fn,
                                                          "test_beam_search": dict(BEAM)}, run_opts={"device": "cuda:0"})


def main():
    from speechbrain_amd import native

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    native.load()
    B, n = args.batch, int(args.seconds * 16000)
    g = torch.Generator().manual_seed(3)
    pcm = (torch.randn(B, n, generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    lens = torch.ones(B)
    res = {"workload": f"EncoderASR CTC-L {B} x {args.seconds:g} s from int16 PCM", "batch": B, "steps": args.steps}
    for name in ("greedy", "beam100"):
        asr = build("greedy" if name == "greedy" else "beam")
        times = []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav = pcm.cuda(non_blocking=True).float() / 32768.0
            asr.transcribe_batch(wav, lens)
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(time.perf_counter() - t0)
        times.sort()
        p50 = times[len(times) // 2]
        res[f"{name}_p50_ms"] = round(p50 * 1e3, 3)
        res[f"{name}_audio_s_per_s"] = round(B * args.seconds / p50, 1)
        # the decode kernel alone, timed with HIP events on the same log-probabilities
        logp = asr.encode_batch(pcm.cuda().float() / 32768.0, lens)
        native.prof_reset()
        native.prof_enable(True)
        for _ in range(args.steps):
            asr.decoding_function(logp, lens.cuda())
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
        key = "ctc_greedy_decode" if name == "greedy" else "ctc_beam_search"
        res[f"{key}_kernel_ms"] = round(rep[key]["ms"] / rep[key]["count"], 4)
        res[f"{name}_frames"] = int(logp.shape[1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
