"""A plain host restatement of CTC prefix beam search without a language model, as DESIGN.md section 5 ("CTC prefix beam
search") words it: the yardstick of tests/test_ctc_prefix_search.py and the fp32 filter of tools/make_ctc_prefix_golden.py.
``dtype`` is the number format of every score (the kernel: float32; the reference: float64)."""
import numpy as np


class _Beam:
    def __init__(self, text, partial, last, frames, pf, p_b, score, neg):
        self.text, self.partial, self.last, self.frames, self.pf = text, partial, last, frames, pf
        self.p_b, self.p_nb, self.n_b, self.n_nb, self.score = p_b, neg, neg, neg, score


def prefix_search(x, n_frames, vocab, blank, space_token=" ", beam_size=100, beam_prune_logp=-10.0,
                  token_prune_min_logp=-5.0, prune_history=True, log_blank_skip_threshold=0.0, topk=1, spm_token="▁",
                  dtype=np.float64):
    """x [T,V] float32 log-probabilities of one utterance -> [(text, score, text_frames)], best first."""
    f, neg = dtype, dtype(-np.inf)
    spm = any(str(s).startswith(spm_token) for s in vocab)
    space = vocab.index(space_token) if (not spm and space_token in vocab) else -1

    def lae(a, b):
        return f(np.logaddexp(f(a), f(b)))

    beams = [_Beam("", "", -1, [], (-1, -1), f(0), f(0), neg)]
    for t in range(n_frames):
        row = x[t]
        if row[blank] > np.float32(log_blank_skip_threshold):
            continue
        toks = sorted(v for v in set(np.where(row > np.float32(token_prune_min_logp))[0]) | {int(row.argmax())}
                      if v < len(vocab))
        entered = list(beams)  # only the beams alive at the start of the frame are extended
        first = {}  # text -> the first beam of the list with that text
        for bm in beams:
            first.setdefault(bm.text, bm)
        for v in toks:  # tokens ascending, then the beams in list order
            lp = f(row[v])
            for bm in entered:
                if v == blank:
                    bm.n_b = lae(bm.n_b, bm.score + lp)
                    continue
                if v == bm.last:
                    bm.n_nb = lae(bm.n_nb, bm.p_nb + lp)
                tok = str(vocab[v])
                boundary = tok[:1] == spm_token if spm else v == space
                tgt = first.get(bm.text + tok)
                if tgt is None:
                    if boundary:  # the partial word is closed; a piece's text starts the next one
                        frames = bm.frames + [bm.pf] if bm.partial != "" else bm.frames
                        partial, pf = (tok[1:], (t, t + 1)) if spm else ("", (-1, -1))
                        tgt = _Beam(bm.text + " " + partial, partial, v, frames, pf, neg, neg, neg)
                    elif v == bm.last:  # a repeat lengthens the text, not the partial word
                        tgt = _Beam(bm.text + tok, bm.partial, v, bm.frames, (bm.pf[0], t + 1), neg, neg, neg)
                    else:
                        pf = (t, t + 1) if bm.pf[0] < 0 else (bm.pf[0], t + 1)
                        tgt = _Beam(bm.text + tok, bm.partial + tok, v, bm.frames, pf, neg, neg, neg)
                    beams.append(tgt)
                    first.setdefault(tgt.text, tgt)
                tgt.n_nb = lae(tgt.n_nb, (bm.p_b if v == bm.last else bm.score) + lp)
        for bm in beams:
            bm.p_b, bm.p_nb, bm.n_b, bm.n_nb = bm.n_b, bm.n_nb, neg, neg
            bm.score = lae(bm.p_b, bm.p_nb)
        cut = max(bm.score for bm in beams) + f(beam_prune_logp)
        beams = sorted((bm for bm in beams if bm.score >= cut), key=lambda bm: -bm.score)[:beam_size]  # (stable)
        if prune_history:
            seen, kept = set(), []
            for bm in beams:
                key = (tuple(bm.text.split()[-1:]), bm.partial, bm.last)
                if key not in seen:
                    seen.add(key)
                    kept.append(bm)
            beams = kept
    merged = {}  # the end: beams that agree on text + " " + partial word fold into the first, with the fields of the last
    for bm in beams:
        key = bm.text + " " + bm.partial if bm.partial != "" and bm.text != "" else bm.text + bm.partial
        frames = bm.frames + [bm.pf] if bm.partial != "" else bm.frames
        merged[key] = (lae(merged[key][0], bm.score) if key in merged else bm.score, bm.text, frames)
    cut = max(m[0] for m in merged.values()) + f(beam_prune_logp)
    out = sorted((m for m in merged.values() if m[0] >= cut), key=lambda m: -m[0])[:beam_size][:topk]
    return [(" ".join(text.split()), float(score), list(zip(text.split(), frames))) for score, text, frames in out]
