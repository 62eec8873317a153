"""Host restatement of the S2S attention beam search of csrc/search.hip over a MEMORYLESS source -- tests only.

With a zero seq_lin weight the logits of every hypothesis at every step are the seq_lin bias, so the search sees one fixed
log-prob row ``lp`` (fp32, taken from native.log_softmax: the step's own log_softmax_row_kernel).  Everything after that row is
IEEE fp32 arithmetic that csrc/internal.h writes out operation by operation (score_cand: add, then a true division;
beam_update: score * (step + 1)), so this numpy-float32 restatement of selection, bookkeeping and finalisation reproduces every
output of the search bit for bit.  No torch on the scoring path.

Every keyword that defaults to the right behaviour is a planted mistake (MUTATIONS) for ``test_cases_tell_mistakes_apart``.
One of them needs a word.  Selection emits a step's winners in descending order, so WITHIN a step "beam order" and "score order"
are the same order and a harvest sorted by score would be no mistake at all.  What first-come order decides is which hypotheses
a list holds once it is full: the earliest ``beam`` arrivals, although a later one may score better under length normalisation.
``harvest_best`` plants that mistake: the search goes on past a full list and a better-scoring arrival displaces its worst entry."""
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


@dataclass
class Result:
    tokens: np.ndarray   # [topk, L] int32 (topk = 1: last token stripped; else kept)
    lens: np.ndarray     # [topk] int32: token count - 1
    scores: np.ndarray   # [topk] fp32
    logp: np.ndarray     # [topk, L] fp32: keeps the stripped position
    longest: int         # longest final entry of the utterance, filled ones included
    harvested: list = field(default_factory=list)  # (length, score) of every hypothesis that ended through eos, in list order
    full_at: int = -1    # number of steps after which the finished list was full (-1: never)
    straddles: list = field(default_factory=list)  # per step with a tie group across the beam-th rank:
    #                      (step, tie value, size of the group, how many of it are taken, highest candidate index taken)


def select(flat, k, ties_to_higher_index=False):
    """Indices of the k best of ``flat`` in descending order; equal values: the lower index first."""
    if ties_to_higher_index:
        return np.lexsort((-np.arange(flat.size), -flat))[:k]
    return np.argsort(-flat, kind="stable")[:k]


def search(lp, beam, eos, min_steps, max_steps, bos=None, length_normalization=True, using_eos_threshold=True,
           eos_threshold=1.5, minus_inf=-1e20, topk=1, return_topk=False, pitch=None,
           ties_to_higher_index=False, threshold_inclusive=False, min_steps_shift=0, harvest_best=False, multiply_back=True,
           fill="beam order", final_ties_to_later=False, strip_last=True):
    """One utterance.  ``lp`` [V] fp32; ``min_steps`` / ``max_steps`` are this utterance's own limits (a grouped search freezes
    it when ``max_steps`` is reached, which for its outputs is the same as ending there); ``pitch`` = row length of the outputs
    (the call's largest max_steps).  ``bos`` only names the first input token: a memoryless source never reads it."""
    lp = np.ascontiguousarray(lp, dtype=F32)
    V = lp.size
    topk = topk if return_topk or topk == 1 else 1
    L = max(pitch if pitch is not None else max_steps, 1)
    minus_inf = F32(minus_inf)
    am_max = lp.max()
    seq = np.full(beam, NEG_INF, dtype=F32)
    seq[0] = F32(0.0)  # only beam 0 is alive
    hist_tok = np.zeros((beam, L), dtype=np.int32)
    hist_lp = np.zeros((beam, L), dtype=F32)
    fin = []  # [length, score, tokens, logp]
    res = Result(None, None, None, None, 0)
    cand_val, steps_done = None, 0
    for step in range(max_steps):
        if len(fin) == beam and not harvest_best:
            break  # a full list accepts nothing more
        row = lp.copy()
        v = row[eos]
        if step < min_steps + min_steps_shift:
            v = minus_inf
        if using_eos_threshold:
            bound = F32(eos_threshold) * am_max
            if not (v >= bound if threshold_inclusive else v > bound):
                v = minus_inf
        row[eos] = v
        flat = (seq[:, None] + row[None, :]).reshape(-1)  # candidate j * V + c
        if length_normalization:
            flat = flat / F32(step + 1)
        order = select(flat, min(beam + 1, flat.size), ties_to_higher_index)
        if order.size > beam and flat[order[beam]] == flat[order[beam - 1]]:
            tie = flat[order[beam - 1]]
            taken = order[:beam][flat[order[:beam]] == tie]
            res.straddles.append((step, float(tie), int((flat == tie).sum()), int(taken.size), int(taken.max())))
        cand_idx = order[:beam]
        cand_val = flat[cand_idx]
        pred, tok = cand_idx // V, (cand_idx % V).astype(np.int32)
        hist_tok, hist_lp = hist_tok[pred], hist_lp[pred]
        hist_tok[:, step], hist_lp[:, step] = tok, lp[tok]  # the log-prob BEFORE the eos rules
        for j in range(beam):  # first come in beam order, at most `beam`
            if tok[j] != eos:
                continue
            entry = [step + 1, cand_val[j], hist_tok[j].copy(), hist_lp[j].copy()]
            if len(fin) < beam:
                fin.append(entry)
                res.harvested.append((step + 1, float(cand_val[j])))
            elif harvest_best:
                worst = min(range(beam), key=lambda f: (fin[f][1], -f))
                if cand_val[j] > fin[worst][1]:
                    fin[worst] = entry
        back = cand_val * F32(step + 1) if length_normalization and multiply_back else cand_val
        seq = np.where(tok == eos, NEG_INF, back).astype(F32)
        steps_done = step + 1
        if len(fin) == beam and res.full_at < 0:
            res.full_at = steps_done
    # finalisation: fill from the alive hypotheses, select topk, strip
    entries = [(e[1], e[0], e[2], e[3]) for e in fin]
    longest = max([e[0] for e in fin], default=0)
    if steps_done > 0 and len(entries) < beam:
        longest = max(longest, steps_done)
        alive = range(beam) if fill == "beam order" else range(beam - 1, -1, -1) if fill == "reverse" else ()
        for j in alive:
            if len(entries) == beam:
                break
            entries.append((cand_val[j], steps_done, hist_tok[j], hist_lp[j]))
    res.longest = longest
    res.tokens, res.logp = np.zeros((topk, L), dtype=np.int32), np.zeros((topk, L), dtype=F32)
    res.lens, res.scores = np.zeros(topk, dtype=np.int32), np.zeros(topk, dtype=F32)
    scores = np.array([e[0] for e in entries], dtype=F32)
    rank = select(scores, topk, final_ties_to_later) if scores.size else []
    for r, e in enumerate(rank):
        score, ntok, toks, lps = entries[e]
        keep = ntok if (topk > 1 or not strip_last) else ntok - 1
        res.scores[r], res.lens[r] = score, max(ntok - 1, 0)
        res.tokens[r, :keep] = toks[:keep]
        res.logp[r, :ntok] = lps[:ntok]
    return res


MUTATIONS = {
    "selection ties resolved towards the higher index": dict(ties_to_higher_index=True),
    "eos threshold compared with >=": dict(threshold_inclusive=True),
    "min_steps off by one": dict(min_steps_shift=1),
    "harvest in score order instead of first come": dict(harvest_best=True),
    "seq not multiplied back after normalisation": dict(multiply_back=False),
    "fill-from-alive skipped": dict(fill="none"),
    "fill-from-alive in reverse order": dict(fill="reverse"),
    "final ties resolved towards the later entry": dict(final_ties_to_later=True),
    "last token not stripped": dict(strip_last=False),
}
