"""Synthetic ARPA files for fixtures, tests and tools/ctc_bench.py: seeded random n-gram models over a word list."""
import numpy as np


def arpa_text(words, order, seed, per_order=None, two_field=(), extra_unigram_backoff=True):
    """An ARPA model of ``order`` over ``words`` (plus <unk>, <s>, </s>).  Each n-gram of order n >= 2 extends an
    (n-1)-gram of the model; ``per_order`` n-grams are drawn per order (default 3 * len(words)).  1-grams carry a back-off
    field even at order 1 unless listed in ``two_field`` (load_unigram_set_from_arpa keeps three-field lines only)."""
    rng = np.random.RandomState(seed)
    vocab = ["<unk>", "<s>", "</s>"] + list(words)
    per_order = per_order or 3 * len(words)
    grams = {1: [(w,) for w in vocab]}
    for n in range(2, order + 1):
        prev = [g for g in grams[n - 1] if g[-1] != "</s>"]
        seen = set()
        for _ in range(per_order):
            g = prev[rng.randint(len(prev))] + (vocab[2 + rng.randint(len(vocab) - 2)],)
            seen.add(g)
        grams[n] = sorted(seen)
    out = ["\\data\\"] + [f"ngram {n}={len(grams[n])}" for n in range(1, order + 1)] + [""]
    for n in range(1, order + 1):
        out.append(f"\\{n}-grams:")
        for g in grams[n]:
            logp = -0.2 - 3.0 * rng.rand() if n > 1 else -1.0 - 3.0 * rng.rand()
            if g == ("<s>",):
                logp = -99.0
            line = f"{logp:.4f}\t{' '.join(g)}"
            if (n < order or (n == 1 and extra_unigram_backoff)) and not (n == 1 and g[0] in two_field):
                line += f"\t{-1.5 * rng.rand():.4f}"
            out.append(line)
        out.append("")
    out.append("\\end\\")
    return "\n".join(out) + "\n"
