"""Host restatement of CTCBeamSearcher without a language model (the reference's decoders/ctc.py:1298-1487 semantics as
listed in DESIGN.md section 5), written from that description in plain Python / numpy.  The CPU suite pins it to
tests/golden/ctc_decode.npz, which the reference itself wrote, so that GPU tests can compare the device search against it
at shapes the fixtures do not cover, without the reference.  Test tooling only."""
import heapq
import math

import numpy as np

from speechbrain_amd.decoders.ctc import CTCHypothesis


def _merge(a, b):
    return a if not b else (b if not a else a + " " + b)


def _logaddexp(x, y):
    return np.logaddexp(np.float32(x), np.float32(y))


def beam_search(log_probs, wav_lens, blank, vocab, space_token=" ", beam_size=100, beam_prune_logp=-10.0,
                token_prune_min_logp=-5.0, prune_history=True, blank_skip_threshold=1.0, topk=1, spm_token="▁"):
    """log_probs [B,T,V] (torch or numpy), wav_lens [B] relative or None -> [[CTCHypothesis] * <= topk] * B."""
    x = np.asarray(log_probs.cpu().numpy() if hasattr(log_probs, "cpu") else log_probs, dtype=np.float32)
    B, T, _ = x.shape
    if wav_lens is None:
        lens = [T] * B
    else:
        rel = np.asarray(wav_lens.cpu().numpy() if hasattr(wav_lens, "cpu") else wav_lens, dtype=np.float32)
        lens = (np.float32(T) * rel).astype(int).tolist()
    is_spm = any(str(s).startswith(spm_token) for s in vocab)
    space = vocab.index(space_token) if (not is_spm and space_token in vocab) else -1
    skip = np.float32(math.log(blank_skip_threshold)) if blank_skip_threshold > 0 else np.float32(-np.inf)
    tmin, bprune = np.float32(token_prune_min_logp), np.float32(beam_prune_logp)
    out = []
    for b in range(B):
        # a beam: (text, partial, last_token, text_frames, partial_frames, score)
        beams = [("", "", None, [], (-1, -1), np.float32(0.0))]
        for t in range(lens[b]):
            row = x[b, t]
            if row[blank] > skip:
                continue
            kept = sorted(set(np.nonzero(row > tmin)[0].tolist()) | {int(np.argmax(row))})
            cands = {}  # key -> [fields of the last member, score]; dict order = first insertion
            for v in kept:
                if v >= len(vocab):
                    continue
                tok, p = vocab[v], row[v]
                for text, part, last, tf, pf, score in beams:
                    s = np.float32(score + p)
                    if v == blank or last == tok:
                        npf = pf if v == blank else (pf[0], t + 1)
                        nb = (text, part, tok, tf, npf)
                    elif (is_spm and tok[:1] == spm_token) or (not is_spm and v == space):
                        ntf = tf if part == "" else tf + [pf]
                        nb = (_merge(text, part), tok[1:] if is_spm else "", tok, ntf,
                              (t, t + 1) if is_spm else (-1, -1))
                    else:
                        npf = (t, t + 1) if pf[0] < 0 else (pf[0], t + 1)
                        nb = (text, part + tok, tok, tf, npf)
                    key = nb[:3]
                    if key in cands:
                        cands[key] = [nb, _logaddexp(cands[key][1], s)]
                    else:
                        cands[key] = [nb, s]
            beams = _select([c[0] + (c[1],) for c in cands.values()], bprune, beam_size)
            if prune_history:
                seen, kept_beams = set(), []
                for bm in beams:
                    key = (tuple(bm[0].split()[-1:]), bm[1], bm[2])
                    if key not in seen:
                        seen.add(key)
                        kept_beams.append(bm)
                beams = kept_beams
        final = {}
        for text, part, last, tf, pf, score in beams:
            nb = (_merge(text, part), "", None, tf if part == "" else tf + [pf], (-1, -1))
            key = nb[:3]
            final[key] = [nb, _logaddexp(final[key][1], score)] if key in final else [nb, score]
        beams = _select([c[0] + (c[1],) for c in final.values()], bprune, beam_size) if final else []
        out.append([CTCHypothesis(text=" ".join(bm[0].split()), last_lm_state=None, score=bm[5], lm_score=bm[5],
                                  text_frames=list(zip(bm[0].split(), bm[3]))) for bm in beams[:topk]])
    return out


def _select(beams, bprune, beam_size):
    """Drop beams below fp32(best + beam_prune_logp), then the best beam_size, stably."""
    if not beams:
        return []
    best = max(bm[5] for bm in beams)
    thr = np.float32(best + bprune)
    beams = [bm for bm in beams if bm[5] >= thr]
    return heapq.nlargest(beam_size, beams, key=lambda bm: bm[5])
