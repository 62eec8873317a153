"""Host restatement of CTCBeamSearcher with an n-gram language model (the semantics listed in DESIGN.md section 5), in plain
Python / numpy with no reference code.  The language model is any object with ``order``, ``start_context()``,
``score(context, word) -> (score, context)`` and ``score_partial_token(partial)`` (speechbrain_amd.decoders.ngram.NgramLM's
host walk of its own tables).  tests/test_ctc_lm.py pins it to tests/golden/ctc_decode_lm.npz, which the reference's search
wrote, so that tests/test_ctc_lm_shapes.py can use it as the yardstick at shapes the fixture does not cover."""
import heapq
import math

import numpy as np

from speechbrain_amd.decoders.ctc import CTCHypothesis


def _merge(a, b):
    return a if not b else (b if not a else a + " " + b)


def beam_search(log_probs, wav_lens, blank, vocab, lm, space_token=" ", beam_size=100, beam_prune_logp=-10.0,
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
    nhist = max(1, lm.order - 1)
    out = []
    for b in range(B):
        text_lm = {"": (0.0, lm.start_context())}  # text -> (raw LM score: a Python float, n-gram context)
        partial_lm = {}

        def fused(text, word, part, score):
            """The candidate's text after its next word, and fp32(score) + fp32(raw LM score + partial-word penalty)."""
            new_text = _merge(text, word)
            if new_text not in text_lm:
                raw, ctx = text_lm[text]
                s, ctx = lm.score(ctx, word)
                text_lm[new_text] = (raw + s, ctx)
            total = text_lm[new_text][0]
            if part:
                if part not in partial_lm:
                    partial_lm[part] = lm.score_partial_token(part)
                total += partial_lm[part]
            return new_text, np.float32(np.float32(score) + np.float32(total))

        # a beam: (text, partial, last_token, text_frames, partial_frames, score, lm_score)
        beams = [("", "", None, [], (-1, -1), np.float32(0.0), np.float32(0.0))]
        for t in range(lens[b]):
            row = x[b, t]
            if row[blank] > skip:
                continue
            kept = sorted(set(np.nonzero(row > tmin)[0].tolist()) | {int(np.argmax(row))})
            cands = {}  # (new text, partial, last token) -> [text, next word, fields of the last member, score]
            for v in kept:
                if v >= len(vocab):
                    continue
                tok, p = vocab[v], row[v]
                for text, part, last, tf, pf, score, _ in beams:
                    s = np.float32(score + p)
                    if v == blank or last == tok:
                        npf = pf if v == blank else (pf[0], t + 1)
                        word, nb = "", (part, tok, tf, npf)
                    elif (is_spm and tok[:1] == spm_token) or (not is_spm and v == space):
                        ntf = tf if part == "" else tf + [pf]
                        word, nb = part, (tok[1:] if is_spm else "", tok, ntf, (t, t + 1) if is_spm else (-1, -1))
                    else:
                        npf = (t, t + 1) if pf[0] < 0 else (pf[0], t + 1)
                        word, nb = "", (part + tok, tok, tf, npf)
                    key = (_merge(text, word), nb[0], tok)
                    if key in cands:
                        cands[key] = [text, word, nb, np.logaddexp(np.float32(cands[key][3]), s)]
                    else:
                        cands[key] = [text, word, nb, s]
            scored = []
            for text, word, nb, s in cands.values():
                new_text, ls = fused(text, word, nb[0], s)
                scored.append((new_text,) + nb + (s, ls))
            beams = _select(scored, bprune, beam_size)
            if prune_history:
                seen, kept_beams = set(), []
                for bm in beams:
                    key = (tuple(bm[0].split()[-nhist:]), bm[1], bm[2])
                    if key not in seen:
                        seen.add(key)
                        kept_beams.append(bm)
                beams = kept_beams
        final = {}
        for text, part, last, tf, pf, score, _ in beams:
            key = _merge(text, part)
            ntf = tf if part == "" else tf + [pf]
            final[key] = [text, part, ntf, np.logaddexp(np.float32(final[key][3]), score) if key in final else score]
        scored = []
        for text, word, ntf, s in final.values():
            new_text, ls = fused(text, word, "", s)
            scored.append((new_text, "", None, ntf, (-1, -1), s, ls))
        beams = _select(scored, bprune, beam_size)
        out.append([CTCHypothesis(text=" ".join(bm[0].split()), last_lm_state=None, score=bm[5], lm_score=bm[6],
                                  text_frames=list(zip(bm[0].split(), bm[3]))) for bm in beams[:topk]])
    return out


def _select(beams, bprune, beam_size):
    """Drop beams whose lm_score is below fp32(best + beam_prune_logp), then the best beam_size, stably."""
    if not beams:
        return []
    best = max(bm[6] for bm in beams)
    thr = np.float32(best + bprune)
    beams = [bm for bm in beams if bm[6] >= thr]
    return heapq.nlargest(beam_size, beams, key=lambda bm: bm[6])
