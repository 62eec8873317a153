"""Stand-in for the ``kenlm`` Python module, so that the reference's CTC search (decoders/ctc.py, kenlm_scorer.py) runs
unmodified where kenlm is not installed (tools/make_ctc_lm_golden.py).  Our own code: an ARPA text file held in Python
dictionaries and scored by standard ARPA back-off with fp32 accumulation (kenlm returns C floats).  It implements only
what KenlmScorer calls.  Agreement with the real library on a real model has not been checked; the known answers it is
pinned to are in tests/test_ctc_lm_loader.py."""
import numpy as np


class State:
    def __init__(self):
        self.words = ()


class Model:
    def __init__(self, path):
        self.ngrams = {}
        n = 0
        with open(path, encoding="utf-8") as f:
            for line in f:
                parts = line.split()
                if not parts:
                    continue
                if parts[0].startswith("\\"):
                    head = parts[0]
                    n = int(head[1:head.index("-")]) if head.endswith("-grams:") else 0
                    continue
                if n == 0:
                    continue
                key = tuple(parts[1:1 + n])
                backoff = np.float32(parts[1 + n]) if len(parts) > 1 + n else np.float32(0.0)
                self.ngrams[key] = (np.float32(parts[0]), backoff)
        self.order = max(len(k) for k in self.ngrams)
        if ("<unk>",) not in self.ngrams:
            raise ValueError("the ARPA file has no <unk>")

    def __contains__(self, word):
        return (word,) in self.ngrams and word != "<unk>"

    def BeginSentenceWrite(self, state):
        state.words = ("<s>",) if ("<s>",) in self.ngrams else ("<unk>",)

    def NullContextWrite(self, state):
        state.words = ()

    def BaseScore(self, in_state, word, out_state):
        w = word if (word,) in self.ngrams else "<unk>"
        keep = self.order - 1
        ctx = tuple(in_state.words[max(0, len(in_state.words) - keep):]) if keep > 0 else ()
        matched, acc = 0, None
        for length in range(len(ctx), -1, -1):
            hit = self.ngrams.get(ctx[len(ctx) - length:] + (w,))
            if hit is not None:
                matched, acc = length, hit[0]
                break
        for length in range(matched + 1, len(ctx) + 1):
            hit = self.ngrams.get(ctx[len(ctx) - length:])
            if hit is not None:
                acc = np.float32(acc + hit[1])
        out_state.words = (ctx + (w,))[-keep:] if keep > 0 else ()
        return float(acc)
