"""Write tests/golden/ctc_prefix_search.npz and tests/golden/pretrained_ctc_tiny/hyperparams_prefix.yaml with the
REFERENCE's own CTCPrefixBeamSearcher (decoders/ctc.py, unmodified, on the CPU).

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference), set up as
tools/make_ctc_golden.py does.

    python tools/make_ctc_prefix_golden.py

Every case stores small log-probabilities, relative lengths, the settings and per utterance the reference's top-k texts,
scores and text_frames.  A seed is kept only if (1) the fp32 run of the host restatement (tests/ctc_prefix_host_ref.py,
the kernel's number format and merge order) gives the reference's float64 texts and frames, and (2) at every pruning step
of the reference the kept and the dropped beams are more than 1e-4 apart, both at the beam_prune_logp cut and at the
beam_size cut; the seeds dropped are printed.  The yaml is the CTC model directory's hyperparams_beam.yaml with
CTCPrefixBeamSearcher as its decoding function; its expected words are the reference searcher's on the posteriors that
tests/golden/pretrained_ctc_tiny_expected.npz holds from the reference's EncoderASR.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SB_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_stubs"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.make_ctc_golden import BEAM_DECODING, CHARS, CTC_YAML, SPM, posteriors  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-4
LENS = torch.tensor([1.0, 0.8, 0.55])
PREFIX_SETTINGS = dict(beam_size=40, beam_prune_logp=-12.0, token_prune_min_logp=-3.0, prune_history=False)


def cases():
    """(name, vocab, V, scale, searcher kwargs): seeds are tried in order until one passes the two filters"""
    out = []
    for tag, vocab in (("char", CHARS), ("spm", SPM)):
        for scale, look in ((6.0, "peaked"), (1.0, "flat")):
            for beam, ph, topk in ((1, False, 1), (4, True, 3), (40, False, 3)):
                out.append((f"{tag}_{look}_b{beam}_ph{int(ph)}_k{topk}", vocab, len(vocab), scale,
                            dict(beam_size=beam, prune_history=ph, topk=topk, beam_prune_logp=-12.0)))
        out.append((f"{tag}_blankskip", vocab, len(vocab), 3.0, dict(beam_size=4, topk=3, blank_skip_threshold=0.5)))
        out.append((f"{tag}_all_tokens", vocab, len(vocab), 1.0, dict(beam_size=4, topk=3, token_prune_min_logp=-1e30)))
        out.append((f"{tag}_wide_v", vocab, len(vocab) + 3, 3.0, dict(beam_size=4, topk=3, prune_history=False)))
    return out


def reference_run(searcher, x, lens):
    """The reference's hypotheses and the smallest distance between kept and dropped beams over its pruning steps."""
    gap = [np.inf]
    scored = searcher.get_lm_beams

    def get_lm_beams(beams, *a, **k):
        res = scored(beams, *a, **k)
        s = np.sort(np.array([b.lm_score for b in res], dtype=np.float64))[::-1]
        cut = s[0] + searcher.beam_prune_logp
        live = s[s >= cut]
        gap[0] = min(gap[0], np.abs(s[np.isfinite(s)] - cut).min())
        if len(live) > searcher.beam_size:
            gap[0] = min(gap[0], live[searcher.beam_size - 1] - live[searcher.beam_size])
        return res

    searcher.get_lm_beams = get_lm_beams
    return searcher(x, lens), gap[0]


def main():
    import ctc_prefix_host_ref as H
    from speechbrain.decoders.ctc import CTCPrefixBeamSearcher

    out, meta = {}, []
    for i, (name, vocab, V, scale, kw) in enumerate(cases()):
        dropped = []
        for seed in range(700 + 20 * i, 720 + 20 * i):
            x = posteriors(seed, 3, 24, V, scale)
            s = CTCPrefixBeamSearcher(blank_index=0, vocab_list=vocab, space_token=" ", **kw)
            hyps, gap = reference_run(s, x, LENS)
            n = (x.shape[1] * LENS).numpy().astype(int)
            host = [H.prefix_search(x[b].numpy(), int(n[b]), vocab, 0, beam_size=s.beam_size,
                                    beam_prune_logp=s.beam_prune_logp, token_prune_min_logp=s.token_prune_min_logp,
                                    prune_history=s.prune_history, log_blank_skip_threshold=s.blank_skip_threshold,
                                    topk=s.topk, dtype=np.float32) for b in range(3)]
            same = all([(h.text, list(h.text_frames)) for h in hl] == [(t, fr) for t, _, fr in ho]
                       for hl, ho in zip(hyps, host))
            if same and gap > MARGIN:
                break
            dropped.append(seed)
        else:
            raise SystemExit(f"{name}: no seed passed the filters")
        res = [dict(text=[h.text for h in hl], score=[float(h.score) for h in hl],
                    text_frames=[[[w, list(f)] for w, f in h.text_frames] for h in hl]) for hl in hyps]
        out[f"case{i}_x"], out[f"case{i}_lens"] = x.numpy(), LENS.numpy()
        meta.append(dict(name=name, vocab=vocab, kwargs=kw, seed=seed, result=res))
        print(f"  {name:28s} seed {seed} (dropped {dropped}) gap {gap:.3g} {[r['text'][0][:24] for r in res]}")
    # the model directory: the reference searcher on the reference EncoderASR's posteriors
    exp = np.load(os.path.join(OUT, "pretrained_ctc_tiny_expected.npz"))
    from speechbrain.dataio.encoder import CTCTextEncoder

    tok = CTCTextEncoder()
    tok.load(os.path.join(OUT, "pretrained_ctc_tiny", "tokenizer.ckpt"))
    s = CTCPrefixBeamSearcher(blank_index=0, vocab_list=[tok.ind2lab[i] for i in range(len(tok.ind2lab))], **PREFIX_SETTINGS)
    hyps, gap = reference_run(s, torch.from_numpy(exp["logp"]), torch.from_numpy(exp["lens"]))
    assert gap > MARGIN, gap
    words = [h[0].text for h in hyps]
    dec = BEAM_DECODING.replace("CTCBeamSearcher", "CTCPrefixBeamSearcher")
    for k, v in PREFIX_SETTINGS.items():
        dec = "\n".join(f"    {k}: {v}" if line.strip().startswith(k + ":") else line for line in dec.split("\n"))
    with open(os.path.join(OUT, "pretrained_ctc_tiny", "hyperparams_prefix.yaml"), "w", encoding="utf-8") as fh:
        fh.write(CTC_YAML.replace("%DECODING%", dec).replace("tools/make_ctc_golden.py", "tools/make_ctc_prefix_golden.py"))
    print("  yaml words:", words, f"gap {gap:.3g}")
    out["meta"] = np.array(json.dumps(dict(cases=meta, yaml_words=words, yaml_scores=[float(h[0].score) for h in hyps])))
    np.savez_compressed(os.path.join(OUT, "ctc_prefix_search.npz"), **out)
    print("wrote", os.path.join(OUT, "ctc_prefix_search.npz"), os.path.getsize(os.path.join(OUT, "ctc_prefix_search.npz")), "bytes")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
