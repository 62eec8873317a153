"""Conformer-Transducer throughput at the LibriSpeech transducer recipe's shape (conformer_transducer.yaml: d 512, 8 heads,
d_ffn 2 048, 12 layers, joint 640, LSTM 512, 1 000 tokens, one-hot embedding, GELU joint) with random weights and a
sharpened classifier: EncoderDecoderASR.transcribe_batch of 32 x 10 s from 16-bit PCM (encoder + greedy decoding), the
decode kernel's own time (HIP events), and streaming-style decoding at B = 1 (one 8-frame chunk per call, the state carried
in a TransducerGreedySearcherStreamingContext).  With --beam N (N > 1) the same batch is then decoded by beam search
(beam_size N, nbest 5) in the same process: ms per batch, the beam kernel's own time, its ratio to the greedy kernel's, the
mean expansions per frame and the number of utterances that reached max_expansions.  With --lm as well, the beam search is
measured a third time fused with an RNNLM of the recipe's shape (embedding 128, two LSTM layers of 2 048, one DNN block of
512, random weights).  A random LM is noise of about -log(V) per token: at the recipe's lm_weight (0.5) it only suppresses
every token and the search makes one LM step per utterance, so the default --lm-weight is 0.01, which leaves the search on
(nearly) the path it takes without the LM and makes the difference of the two kernels the cost of the LM steps: ms per batch, the kernel's own time, the LM steps taken and the bytes of LM weights read
per second; that result is also written to profiles/transducer_lm_bench.json.  One JSON line.

    python tools/transducer_bench.py [--steps 10] [--warmup 3] [--beam 10] [--lm [--lm-steps 3]]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CFG = dict(d_model=512, nhead=8, d_ffn=2048, n_enc=12, n_dec=0, n_fft=512, win_length=32)
V, J, H = 1000, 640, 512


class _Ids:
    def decode_ids(self, ids):
        return " ".join(str(i) for i in ids)


def build():
    from speechbrain_amd.decoders.transducer import TransducerBeamSearcher
    from speechbrain_amd.inference.ASR import EncoderDecoderASR
    from speechbrain_amd.inference.builders import build_modules
    from speechbrain_amd.lobes.models.transformer.TransformerASR import EncoderWrapper
    from speechbrain_amd.nnet.containers import LengthsCapableSequential
    from speechbrain_amd.nnet.embedding import Embedding
    from speechbrain_amd.nnet.linear import Linear
    from speechbrain_amd.nnet.RNN import LSTM
    from speechbrain_amd.nnet.transducer.transducer_joint import Transducer_joint

    m = build_modules(CFG, vocab=V, seed=31)
    proj_enc = Linear(input_size=CFG["d_model"], n_neurons=J, bias=False)
    emb = Embedding(num_embeddings=V, consider_as_one_hot=True, blank_id=0)
    dec = LSTM(input_shape=[None, None, V - 1], hidden_size=H, num_layers=1)
    proj_dec = Linear(input_size=H, n_neurons=J, bias=False)
    lin = Linear(input_size=J, n_neurons=V, bias=True)
    with torch.no_grad():
        lin.w.weight.mul_(8.0)
        lin.w.bias.zero_()
        lin.w.bias[0] = 6.0  # blank-dominated decisions, as a trained model's
    enc = LengthsCapableSequential(compute_features=m["compute_features"], normalize=m["normalize"], CNN=m["CNN"],
                                   enc=EncoderWrapper(m["Transformer"]), proj_enc=proj_enc)
    searcher = TransducerBeamSearcher(decode_network_lst=[emb, dec, proj_dec], tjoint=Transducer_joint(nonlinearity=torch.nn.GELU),
                                      classifier_network=[lin], blank_id=0, beam_size=1, nbest=1)
    for x in (emb, dec, proj_dec, lin):
        x.to("cuda:0")
    return EncoderDecoderASR(modules={"encoder": enc, "decoder": searcher},
                             hparams={"tokenizer": _Ids(), "transducer_beam_search": True}, run_opts={"device": "cuda:0"})


def main():
    from speechbrain_amd import native
    from speechbrain_amd.decoders.transducer import TransducerGreedySearcherStreamingContext

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk-frames", type=int, default=8)
    ap.add_argument("--beam", type=int, default=0, help="also measure beam search with this beam_size (> 1)")
    ap.add_argument("--lm", action="store_true", help="with --beam: also measure the beam search fused with an RNNLM")
    ap.add_argument("--lm-weight", type=float, default=0.01, help="lm_weight of the LM leg (see the module's docstring)")
    ap.add_argument("--lm-steps", type=int, default=3, help="timed batches of the LM leg (after one warm-up batch)")
    args = ap.parse_args()
    native.load()
    B, n = args.batch, int(args.seconds * 16000)
    g = torch.Generator().manual_seed(3)
    pcm = (torch.randn(B, n, generator=g) * 3000).clamp(-32768, 32767).to(torch.int16)
    lens = torch.ones(B)
    asr = build()
    res = {"workload": f"EncoderDecoderASR Conformer-Transducer {B} x {args.seconds:g} s from int16 PCM, greedy",
           "batch": B, "steps": args.steps}
    times = []
    for i in range(args.warmup + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wav = pcm.cuda(non_blocking=True).float() / 32768.0
        _, toks = asr.transcribe_batch(wav, lens)
        torch.cuda.synchronize()
        if i >= args.warmup:
            times.append(time.perf_counter() - t0)
    times.sort()
    p50 = times[len(times) // 2]
    res["p50_ms"] = round(p50 * 1e3, 3)
    res["audio_s_per_s"] = round(B * args.seconds / p50, 1)
    tn = asr.encode_batch(pcm.cuda().float() / 32768.0, lens)
    res["frames"] = int(tn.shape[1])
    res["tokens_per_utterance_mean"] = round(sum(len(t) for t in toks) / B, 1)
    searcher = asr.mods.decoder
    native.prof_reset()
    native.prof_enable(True)
    for _ in range(args.steps):
        searcher(tn)
    torch.cuda.synchronize()
    native.prof_enable(False)
    rep = native.prof_report()
    res["transducer_greedy_kernel_ms"] = round(rep["transducer_greedy"]["ms"] / rep["transducer_greedy"]["count"], 4)
    # streaming-style: utterance 0 in chunks of chunk-frames encoder frames, B = 1, the context carried
    x = tn[:1].contiguous()
    chunks = [x[:, t:t + args.chunk_frames].contiguous() for t in range(0, x.shape[1], args.chunk_frames)]
    for _ in range(2):
        ctx = TransducerGreedySearcherStreamingContext()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for ch in chunks:
            searcher.transducer_greedy_decode_streaming(ch, ctx)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    res["stream_b1_chunk_frames"] = args.chunk_frames
    res["stream_b1_decode_ms_per_chunk"] = round(dt * 1e3 / len(chunks), 4)
    if args.beam > 1:
        import warnings

        warnings.simplefilter("ignore")  # (capped utterances are counted below)
        searcher.beam_size, searcher.nbest, searcher.searcher = args.beam, 5, searcher.transducer_beam_search_decode
        times = []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav = pcm.cuda(non_blocking=True).float() / 32768.0
            _, toks = asr.transcribe_batch(wav, lens)
            torch.cuda.synchronize()
            if i >= args.warmup:
                times.append(time.perf_counter() - t0)
        times.sort()
        res["beam"] = args.beam
        res["beam_p50_ms"] = round(times[len(times) // 2] * 1e3, 3)
        res["beam_tokens_per_utterance_mean"] = round(sum(len(t) for t in toks) / B, 1)
        native.prof_reset()
        native.prof_enable(True)
        for _ in range(args.steps):
            out = native.transducer_beam_search(searcher._prepare(tn.device), tn, 0, args.beam, 5, searcher.state_beam,
                                                searcher.expand_beam, act=searcher.tjoint.act_code)
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
        res["transducer_beam_kernel_ms"] = round(rep["transducer_beam"]["ms"] / rep["transducer_beam"]["count"], 4)
        res["beam_kernel_over_greedy_kernel"] = round(res["transducer_beam_kernel_ms"] / res["transducer_greedy_kernel_ms"], 2)
        res["beam_kernel_share_of_batch"] = round(res["transducer_beam_kernel_ms"] / res["beam_p50_ms"], 3)
        res["beam_expansions_per_frame_mean"] = round(float(out[5].float().mean()) / tn.shape[1], 3)
        res["beam_utterances_capped"] = int((out[4] != 0).sum())
    if args.beam > 1 and args.lm:
        from speechbrain_amd.lobes.models.RNNLM import RNNLM

        torch.manual_seed(41)
        lm = RNNLM(output_neurons=V, embedding_dim=128, rnn_layers=2, rnn_neurons=2048, dnn_blocks=1, dnn_neurons=512,
                   dropout=0.0, return_hidden=True).to("cuda:0").eval()
        searcher.lm, searcher.lm_weight = lm, args.lm_weight
        times = []
        for i in range(1 + args.lm_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav = pcm.cuda(non_blocking=True).float() / 32768.0
            _, toks = asr.transcribe_batch(wav, lens)
            torch.cuda.synchronize()
            if i >= 1:
                times.append(time.perf_counter() - t0)
        times.sort()
        res["beam_lm_p50_ms"] = round(times[len(times) // 2] * 1e3, 3)
        res["beam_lm_tokens_per_utterance_mean"] = round(sum(len(t) for t in toks) / B, 1)
        plm = searcher._prepare_lm(tn.device)
        native.prof_reset()
        native.prof_enable(True)
        for _ in range(args.lm_steps):
            out = native.transducer_beam_search(searcher._prepare(tn.device, beam=True), tn, 0, args.beam, 5, searcher.state_beam,
                                                searcher.expand_beam, act=searcher.tjoint.act_code, lm=plm, lm_weight=args.lm_weight,
                                                return_lm_steps=True)
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
        ms = rep["transducer_beam_lm"]["ms"] / rep["transducer_beam_lm"]["count"]
        steps = out[6].cpu()
        res["lm_weight"] = args.lm_weight
        res["transducer_beam_lm_kernel_ms"] = round(ms, 3)
        res["beam_lm_kernel_over_beam_kernel"] = round(ms / res["transducer_beam_kernel_ms"], 2)
        res["beam_lm_expansions_per_frame_mean"] = round(float(out[5].float().mean()) / tn.shape[1], 3)
        res["beam_lm_utterances_capped"] = int((out[4] != 0).sum())
        res["lm_steps_total"], res["lm_steps_max_per_utterance"] = int(steps.sum()), int(steps.max())
        res["lm_weight_bytes_per_step"] = int(plm.weight_bytes)
        # the LM's share of the kernel: what the fused search takes beyond the plain one (one workgroup per utterance, so the
        # kernel lasts as long as its slowest utterance; the aggregate rate counts every utterance's steps)
        # (meaningful only where both searches make about the same expansions: compare the two expansions_per_frame_mean)
        extra_s = (ms - res["transducer_beam_kernel_ms"]) * 1e-3
        if extra_s > 0:
            res["lm_step_ms_per_workgroup"] = round(extra_s * 1e3 / max(1, int(steps.max())), 4)
            res["lm_gbytes_per_s_per_workgroup"] = round(plm.weight_bytes * int(steps.max()) / extra_s / 1e9, 2)
            res["lm_gbytes_per_s_all_workgroups"] = round(plm.weight_bytes * int(steps.sum()) / extra_s / 1e9, 2)
        with open(os.path.join(ROOT, "profiles", "transducer_lm_bench.json"), "w", encoding="utf-8") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
