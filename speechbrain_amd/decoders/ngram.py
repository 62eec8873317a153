"""Word n-gram language models for CTC shallow fusion: an ARPA text file parsed into the flat device tables that
sbk_ctc_beam_search_lm_f32 reads (include/sbk.h), with KenlmScorer's scoring rules
(integrations/decoders/kenlm_scorer.py) restated over those same tables on the host for the tests.

Only ARPA text files of order 1..5 are read; kenlm's binary formats are refused.  Scoring is standard ARPA back-off with
fp32 accumulation; agreement with the kenlm library itself on a real model has not been checked."""
import math
import re

import numpy as np

HASH_MOD = 2147483647  # 2^31 - 1 (decoders/ctc.py)
HASH_BASE1 = 1103515245 % HASH_MOD
HASH_BASE2 = 2654435761 % HASH_MOD
MAX_ORDER = 5
_M32 = np.uint64(0xFFFFFFFF)


def hash_strings(strings):
    """(h1, h2) uint32 arrays: decoders.ctc.string_hash of every string, computed column by column over equal lengths."""
    n = len(strings)
    h1, h2 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    if n == 0:
        return h1.astype(np.uint32), h2.astype(np.uint32)
    lens = np.fromiter(map(len, strings), dtype=np.int64, count=n)
    codes = np.frombuffer("".join(strings).encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.uint64) + np.uint64(1)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
    order = np.argsort(lens, kind="stable")
    sl = lens[order]
    starts = np.flatnonzero(np.concatenate([[True], sl[1:] != sl[:-1]]))
    for a, b in zip(starts, list(starts[1:]) + [n]):
        L = int(sl[a])
        rows = order[a:b]
        a1, a2 = np.zeros(len(rows), dtype=np.uint64), np.zeros(len(rows), dtype=np.uint64)
        for k in range(L):
            c = codes[offs[rows] + k]
            a1 = (a1 * np.uint64(HASH_BASE1) + c) % np.uint64(HASH_MOD)
            a2 = (a2 * np.uint64(HASH_BASE2) + c) % np.uint64(HASH_MOD)
        h1[rows], h2[rows] = a1, a2
    return h1.astype(np.uint32), h2.astype(np.uint32)


def _mix(x):
    x = x & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x2C1B3C6D)) & _M32
    return x ^ (x >> np.uint64(12))


def _string_slot(h1, h2, length):
    h1, h2, length = (np.asarray(v).astype(np.uint64) for v in (h1, h2, length))
    return _mix(h1 ^ ((h2 * np.uint64(0x9E3779B1)) & _M32) ^ ((length * np.uint64(0x85EBCA6B)) & _M32))


def _ngram_slot(rev_ids, n):
    """rev_ids [N, n]: the ids of each n-gram, the last word first."""
    x = np.full(rev_ids.shape[0], n, dtype=np.uint64)
    for i in range(n):
        x = _mix(((x ^ rev_ids[:, i].astype(np.uint64)) * np.uint64(0x9E3779B1)) & _M32)
    return x


def _table_size(n):
    size = 2
    while size < 2 * n:
        size *= 2
    return size


def _place(start, size):
    """Slots of an open-addressing table with linear probing for keys whose first slots are ``start``: round by round,
    the first key that asks for a free slot takes it and the others move on."""
    n = len(start)
    slot = np.full(n, -1, dtype=np.int64)
    used = np.zeros(size, dtype=bool)
    pending = np.arange(n)
    want = start.astype(np.int64) & (size - 1)
    while len(pending):
        free = ~used[want]
        _, first = np.unique(want, return_index=True)
        win = np.zeros(len(pending), dtype=bool)
        win[first] = True
        win &= free
        slot[pending[win]] = want[win]
        used[want[win]] = True
        pending, want = pending[~win], (want[~win] + 1) & (size - 1)
    return slot


class ArpaModel:
    """An ARPA file as flat arrays: words (id = position among the 1-grams), uni [W,2] fp32 (log10 p, back-off) and, per
    order n >= 2, (ids [N,n] int32, log10 p [N], back-off [N])."""

    def __init__(self, path):
        try:
            with open(path, encoding="utf-8") as f:
                text = f.read()
        except (OSError, UnicodeDecodeError) as e:
            raise NotImplementedError(f"kenlm_model_path {path!r} cannot be read as an ARPA text file ({e}); only ARPA "
                                      "text models are supported, kenlm's binary (probing / trie) formats are not") from e
        lines = text.splitlines()
        marks = [(i, int(m.group(1))) for i, ln in enumerate(lines) for m in [re.fullmatch(r"\\(\d+)-grams:", ln.strip())] if m]
        if not marks or not any(ln.strip() == "\\data\\" for ln in lines[:marks[0][0]]):
            raise NotImplementedError(f"kenlm_model_path {path!r} is not an ARPA text file (no \\data\\ header); only ARPA "
                                      "text models are supported, kenlm's binary (probing / trie) formats are not")
        self.order = max(n for _, n in marks)
        if [n for _, n in marks] != list(range(1, self.order + 1)):
            raise ValueError(f"ARPA file {path!r}: n-gram sections out of order")
        if self.order > MAX_ORDER:
            raise NotImplementedError(f"ARPA model of order {self.order}: orders above {MAX_ORDER} are not supported (the "
                                      "n-gram context a beam carries on the device holds 4 words)")
        self.three_field_unigrams = []
        self.ngrams = {}
        ends = [i for i, _ in marks[1:]] + [len(lines)]
        for (i0, n), i1 in zip(marks, ends):
            rows = [p for p in (ln.split() for ln in lines[i0 + 1:i1]) if p and p[0] != "\\end\\"]
            bad = [p for p in rows if len(p) not in (n + 1, n + 2)]
            if bad:
                raise ValueError(f"ARPA file {path!r}: {n}-gram line with {len(bad[0])} fields: {' '.join(bad[0])!r}")
            logp = np.array([p[0] for p in rows], dtype=np.float64).astype(np.float32)
            bo = np.array([p[n + 1] if len(p) == n + 2 else "0" for p in rows], dtype=np.float64).astype(np.float32)
            if n == 1:
                self.words = [p[1] for p in rows]
                self.word_id = {w: i for i, w in enumerate(self.words)}
                if len(self.word_id) != len(self.words):
                    raise ValueError(f"ARPA file {path!r}: a word is listed twice among the 1-grams")
                self.uni = np.stack([logp, bo], axis=1) if rows else np.zeros((0, 2), np.float32)
                self.three_field_unigrams = [p[1] for p in rows if len(p) == 3]
            else:
                try:
                    ids = np.fromiter((self.word_id[w] for p in rows for w in p[1:n + 1]), dtype=np.int32,
                                      count=n * len(rows)).reshape(-1, n)
                except KeyError as e:
                    raise ValueError(f"ARPA file {path!r}: {n}-gram with a word that is not among the 1-grams: {e}") from e
                self.ngrams[n] = (ids, logp, bo)
        if "<unk>" not in self.word_id:
            raise ValueError(f"ARPA file {path!r} has no <unk> 1-gram: out-of-vocabulary words are scored with <unk>'s "
                             "probability, so the model must define it")

    def __contains__(self, word):  # kenlm.Model.__contains__: the vocabulary index is not <unk>'s
        return word in self.word_id and word != "<unk>"


class NgramLM:
    """What ``CTCBaseSearcher.lm`` holds: KenlmScorer's parameters and the tables of include/sbk.h (numpy; device copies on
    demand).  The scoring methods walk the same tables with the same arithmetic as the kernel."""

    def __init__(self, path, unigrams=None, alpha=0.5, beta=1.5, unk_score_offset=-10.0, score_boundary=True,
                 hash_fn=hash_strings):
        m = ArpaModel(path)
        self.model, self.order = m, m.order
        self.alpha, self.beta, self.unk_score_offset = float(alpha), float(beta), float(unk_score_offset)
        self.score_boundary = bool(score_boundary)
        self.log10_e = math.log10(math.e)
        self.unk_id, self.bos_id = m.word_id["<unk>"], m.word_id.get("<s>", m.word_id["<unk>"])
        # CTCBaseSearcher.__init__: without explicit unigrams they are read from the file only when it is named *.arpa
        # (load_unigram_set_from_arpa keeps the 1-gram lines of exactly three fields); otherwise there is no unigram set
        if unigrams is None and str(path).endswith(".arpa"):
            unigrams = m.three_field_unigrams
            if len(unigrams) == 0:
                raise ValueError("No unigrams found in arpa file. Something is wrong with the file.")
        self.unigram_set = set() if unigrams is None else {w for w in set(unigrams) if w in m}  # _prepare_unigram_set
        # strings: every prefix of the unigram set (CharTrie.has_node) and every word of the model
        prefixes = {w[:k] for w in self.unigram_set for k in range(1, len(w) + 1)}
        strings = sorted(prefixes | set(m.words))
        h1, h2 = hash_fn(strings)
        lens = np.fromiter(map(len, strings), dtype=np.int64, count=len(strings))
        keys = np.stack([h1.astype(np.int64), h2.astype(np.int64), lens], axis=1)
        if len(np.unique(keys, axis=0)) != len(strings):
            _, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
            clash = [strings[i] for i in np.flatnonzero(cnt[inv.reshape(-1)] > 1)[:4]]
            raise ValueError(f"n-gram tables: two distinct strings share both character hashes and their length ({clash}); "
                             "the device search could not tell them apart")
        wid = np.fromiter((m.word_id.get(s, -1) for s in strings), dtype=np.int64, count=len(strings))
        in_model = np.fromiter((s in m for s in strings), dtype=bool, count=len(strings))
        in_set = np.fromiter((s in self.unigram_set for s in strings), dtype=bool, count=len(strings))
        known = in_model & (in_set if self.unigram_set else True)
        is_prefix = np.fromiter((s in prefixes for s in strings), dtype=bool, count=len(strings))
        val = ((wid + 1) << 2) | (known.astype(np.int64) << 1) | is_prefix.astype(np.int64)
        size = _table_size(len(strings))
        slot = _place(_string_slot(h1, h2, lens), size)
        self.strings = np.zeros((size, 4), dtype=np.int32)
        self.strings[:, 2] = -1
        self.strings[slot] = np.stack([keys[:, 0], keys[:, 1], lens, val], axis=1).astype(np.int32)
        self.unigrams = np.ascontiguousarray(m.uni, dtype=np.float32)
        # n-grams of order >= 2, ids with the last word first
        rows = []
        for n, (ids, logp, bo) in sorted(m.ngrams.items()):
            e = np.full((len(ids), 8), -1, dtype=np.int32)
            e[:, 0] = n
            e[:, 1:1 + n] = ids[:, ::-1]
            e[:, 6], e[:, 7] = logp.view(np.int32), bo.view(np.int32)
            rows.append((e, _ngram_slot(ids[:, ::-1], n)))
        total = sum(len(e) for e, _ in rows)
        size = _table_size(total)
        self.ngrams = np.zeros((size, 8), dtype=np.int32)
        if total:
            slot = _place(np.concatenate([s for _, s in rows]), size)
            self.ngrams[slot] = np.concatenate([e for e, _ in rows])
        self.n_ngrams = total
        self._device = {}

    # ---------------------------------------------------------------- device side
    def tables(self, device):
        """native.CTCLMTables over copies of the tables on ``device`` (made once per device and kept)."""
        import torch

        from speechbrain_amd import native

        key = str(device)
        if key not in self._device:
            t = [torch.from_numpy(a).to(device).contiguous() for a in (self.strings, self.unigrams, self.ngrams)]
            s = native.CTCLMTables(
                strings=t[0].data_ptr(), unigrams=t[1].data_ptr(), ngrams=t[2].data_ptr(), n_string_slots=len(self.strings),
                n_words=len(self.unigrams), n_ngram_slots=len(self.ngrams), order=self.order, unk_id=self.unk_id,
                bos_id=self.bos_id, score_boundary=int(self.score_boundary), alpha=self.alpha, beta=self.beta,
                unk_score_offset=self.unk_score_offset, log10_e=self.log10_e)
            self._device[key] = (t, s)
        return self._device[key][1]

    # ---------------------------------------------------------------- the same walk on the host
    def string_value(self, s):
        """The table's value for a string: (word id + 1) << 2 | known << 1 | prefix; 0 when absent."""
        from speechbrain_amd.decoders.ctc import string_hash

        h1, _, h2, _ = string_hash(s)
        size = len(self.strings)
        i = int(_string_slot(h1, h2, len(s))) & (size - 1)
        for _ in range(size):
            e = self.strings[i]
            if e[2] < 0:
                return 0
            if e[0] == h1 and e[1] == h2 and e[2] == len(s):
                return int(e[3])
            i = (i + 1) & (size - 1)
        return 0

    def ngram(self, rev_ids):
        """(log10 p, back-off) of the n-gram whose ids, the last word first, are ``rev_ids`` (n >= 2), or None."""
        n, size = len(rev_ids), len(self.ngrams)
        i = int(_ngram_slot(np.asarray([rev_ids], dtype=np.int64), n)[0]) & (size - 1)
        for _ in range(size):
            e = self.ngrams[i]
            if e[0] == 0:
                return None
            if e[0] == n and list(e[1:1 + n]) == list(rev_ids):
                return e[6:8].view(np.float32)
            i = (i + 1) & (size - 1)
        return None

    def word_logp(self, ctx, w):
        """log10 p(w | ctx), ctx = word ids with the most recent first: the longest n-gram in the model, plus the back-offs
        of the longer contexts from the shortest up, in fp32."""
        acc, matched = np.float32(self.unigrams[w, 0]), 0
        for L in range(len(ctx), 0, -1):
            hit = self.ngram([w] + list(ctx[:L]))
            if hit is not None:
                acc, matched = np.float32(hit[0]), L
                break
        for L in range(matched + 1, len(ctx) + 1):
            if L == 1:
                acc = np.float32(acc + self.unigrams[ctx[0], 1])
            else:
                hit = self.ngram(list(ctx[:L]))
                if hit is not None:
                    acc = np.float32(acc + hit[1])
        return acc

    def start_context(self):
        return (self.bos_id,) if self.score_boundary and self.order > 1 else ()

    def score(self, ctx, word):
        """KenlmScorer.score(state, word): (alpha * log10 p * ln 10 + beta with the OOV offset, the next context)."""
        v = self.string_value(word)
        w = (v >> 2) - 1 if (v >> 2) > 0 else self.unk_id
        s = float(self.word_logp(ctx, w))
        if not v & 2:
            s += self.unk_score_offset
        new_ctx = ((w,) + tuple(ctx))[:self.order - 1]
        return self.alpha * s * 1.0 / self.log10_e + self.beta, new_ctx

    def score_partial_token(self, partial):
        """KenlmScorer.score_partial_token."""
        u = self.unk_score_offset * (0 if self.string_value(partial) & 1 else 1)
        if len(partial) > 6:
            u = u * len(partial) / 6
        return u

