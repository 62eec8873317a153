"""speechbrain.decoders.ctc mirror: CTC output filtering, greedy decoding and CTCBeamSearcher (decoders/ctc.py:298-380,
505-1487) on the device kernels of csrc/ctc_decode.hip.

The frame loop of the beam search runs on the MI355X in one launch per batch (include/sbk.h, sbk_ctc_beam_search_f32); the
host only rebuilds each returned hypothesis' ``text`` and ``text_frames`` by replaying the token path the kernel reports
through the reference's string rules (O(T) per hypothesis).  With ``kenlm_model_path`` an ARPA n-gram model (order 1..5,
decoders/ngram.py) is fused into the same launch (sbk_ctc_beam_search_lm_f32).  CTCPrefixBeamSearcher and the streaming
``partial_decode_beams`` are not implemented."""
import dataclasses
import math
import warnings
from itertools import groupby
from typing import Any, List, Optional, Union

import numpy as np
import torch

# character hashes of the beam search's merge keys (include/sbk.h)
HASH_MOD = 2147483647  # 2^31 - 1
HASH_BASE1 = 1103515245 % HASH_MOD
HASH_BASE2 = 2654435761 % HASH_MOD


def filter_ctc_output(string_pred, blank_id=-1):
    """Collapse repetitions, then drop ``blank_id`` (decoders/ctc.py:298-333)."""
    if isinstance(string_pred, list):
        string_out = [i[0] for i in groupby(string_pred)]
        string_out = list(filter(lambda elem: elem != blank_id, string_out))
    else:
        raise ValueError("filter_ctc_out can only filter python lists")
    return string_out


def ctc_greedy_decode(probabilities, seq_lens, blank_id=-1):
    """decoders/ctc.py:335-380.  probabilities [B,T,V] (log-)probabilities, seq_lens [B] relative lengths -> list of token
    lists.  Device tensors run sbk_ctc_greedy_decode_f32 (one pass over the posteriors, one copy of the result to the
    host); CPU tensors take the reference's host path, as its recipes call this utility on whatever tensor they hold."""
    if isinstance(blank_id, int) and blank_id < 0:
        blank_id = probabilities.shape[-1] + blank_id
    if probabilities.is_cuda and isinstance(blank_id, int):
        from speechbrain_amd import native

        x = probabilities
        if x.dtype != torch.float32:
            x = x.float()
        tokens, count = native.ctc_greedy_decode(x, seq_lens, blank_id)
        tokens, count = tokens.cpu().tolist(), count.cpu().tolist()
        return [row[:n] for row, n in zip(tokens, count)]
    batch_max_len = probabilities.shape[1]
    batch_outputs = []
    for seq, seq_len in zip(probabilities, seq_lens):
        actual_size = int(torch.round(seq_len * batch_max_len))
        scores, predictions = torch.max(seq.narrow(0, 0, actual_size), dim=1)
        batch_outputs.append(filter_ctc_output(predictions.tolist(), blank_id=blank_id))
    return batch_outputs


@dataclasses.dataclass
class CTCHypothesis:
    """decoders/ctc.py:511-541."""

    text: str
    last_lm_state: None
    score: float
    lm_score: float
    text_frames: Optional[list] = None


def string_hash(s):
    """(h1, b1^n, h2, b2^n) of a string's code points: h_i = sum_k (c_k + 1) * b_i^(n-1-k) mod 2^31-1."""
    h1 = h2 = 0
    p1 = p2 = 1
    for ch in s:
        c = ord(ch) + 1
        h1, p1 = (h1 * HASH_BASE1 + c) % HASH_MOD, p1 * HASH_BASE1 % HASH_MOD
        h2, p2 = (h2 * HASH_BASE2 + c) % HASH_MOD, p2 * HASH_BASE2 % HASH_MOD
    return h1, p1, h2, p2


class CTCBaseSearcher(torch.nn.Module):
    """decoders/ctc.py:544-1153: same constructor arguments and defaults.  ``kenlm_model_path`` names an ARPA text file
    of order 1..5 (kenlm's binary formats raise NotImplementedError); ``unigrams``, ``alpha``, ``beta``,
    ``unk_score_offset`` and ``score_boundary`` mean what they mean to the reference's KenlmScorer.  ``self.lm`` is then a
    decoders.ngram.NgramLM (``.order``), whose tables are built once here and kept on the device."""

    def __init__(self, blank_index: int, vocab_list: List[str], space_token: str = " ",
                 kenlm_model_path: Union[None, str] = None, unigrams: Union[None, list, set] = None, alpha: float = 0.5,
                 beta: float = 1.5, unk_score_offset: float = -10.0, score_boundary: bool = True, beam_size: int = 100,
                 beam_prune_logp: float = -10.0, token_prune_min_logp: float = -5.0, prune_history: bool = True,
                 blank_skip_threshold: float = 1.0, topk: int = 1, spm_token: str = "▁"):
        super().__init__()
        self.blank_index = blank_index
        self.vocab_list = vocab_list
        self.space_token = space_token
        self.kenlm_model_path = kenlm_model_path
        self.unigrams = unigrams
        self.alpha, self.beta, self.unk_score_offset, self.score_boundary = alpha, beta, unk_score_offset, score_boundary
        self.beam_size = beam_size
        self.beam_prune_logp = beam_prune_logp
        self.token_prune_min_logp = token_prune_min_logp
        self.prune_history = prune_history
        self.blank_skip_threshold = math.log(blank_skip_threshold)
        self.topk = topk
        self.spm_token = spm_token
        self.is_spm = any([str(s).startswith(self.spm_token) for s in vocab_list])
        self.space_index = -1
        if not self.is_spm:
            try:
                self.space_index = vocab_list.index(space_token)
            except ValueError:
                self.space_index = -1
        self.kenlm_model = None
        self.lm = None  # (unigrams without a model are ignored, as in the reference)
        if kenlm_model_path is not None:
            from speechbrain_amd.decoders.ngram import NgramLM

            self.lm = NgramLM(kenlm_model_path, unigrams=unigrams, alpha=alpha, beta=beta,
                              unk_score_offset=unk_score_offset, score_boundary=score_boundary)
        self._table = None

    def normalize_whitespace(self, text: str) -> str:
        return " ".join(text.split())

    def merge_tokens(self, token_1: str, token_2: str) -> str:
        if len(token_2) == 0:
            return token_1
        if len(token_1) == 0:
            return token_2
        return token_1 + " " + token_2

    def partial_decoding(self, *args, **kwargs):
        raise NotImplementedError

    def partial_decode_beams(self, *args, **kwargs):
        raise NotImplementedError("partial_decode_beams (streaming chunk decoding of CTC beams) is not implemented: decode "
                                  "whole utterances with decode_beams")

    def token_table(self):
        """[len(vocab_list), 8] int32 of include/sbk.h: kind, string id, text length and its two hashes."""
        if self._table is None:
            sid, rows = {}, []
            for v, tok in enumerate(self.vocab_list):
                tok = str(tok)
                if tok in sid:
                    raise NotImplementedError(f"CTC beam search: vocabulary entry {v} ({tok!r}) repeats the string of entry "
                                              f"{sid[tok]}; vocabularies with duplicate strings are not supported")
                sid[tok] = v
                if v == self.blank_index:
                    kind, text = 1, ""
                elif self.is_spm and tok[:1] == self.spm_token:
                    kind, text = 2, tok[1:]
                elif not self.is_spm and v == self.space_index:
                    kind, text = 2, ""
                else:
                    kind, text = 0, tok
                h1, p1, h2, p2 = string_hash(text)
                rows.append([kind, v, len(text), h1, p1, h2, p2, 0])
            self._table = torch.tensor(rows, dtype=torch.int32).reshape(-1, 8)
        return self._table

    def replay(self, path, score, lm_score=None):
        """The hypothesis that follows ``path`` (the token expanded at each frame, -1 = none), through the rules of
        CTCBeamSearcher.partial_decoding / get_lm_beams / finalize_decoding / decode_log_probs.  ``score`` is the CTC score;
        ``lm_score`` the fused one (without a language model it is the CTC score)."""
        vocab, blank, spm = self.vocab_list, self.blank_index, self.spm_token
        text, partial, last, frames, pf = "", "", None, [], (-1, -1)
        for t, v in enumerate(path):
            if v < 0:
                continue
            tok = vocab[v]
            if v == blank or last == tok:
                if v != blank:
                    pf = (pf[0], t + 1)
            elif (self.is_spm and tok[:1] == spm) or (not self.is_spm and v == self.space_index):
                if partial != "":
                    frames = frames + [pf]
                text = self.merge_tokens(text, partial)
                partial, pf = (tok[1:], (t, t + 1)) if self.is_spm else ("", (-1, -1))
            else:
                pf = (t, t + 1) if pf[0] < 0 else (pf[0], t + 1)
                partial = partial + tok
            last = tok
        if partial != "":
            frames = frames + [pf]
        text = self.merge_tokens(text, partial)
        score = np.float32(score)
        return CTCHypothesis(text=self.normalize_whitespace(text), last_lm_state=None,
                             text_frames=list(zip(text.split(), frames)), score=score,
                             lm_score=score if lm_score is None else np.float32(lm_score))

    def decode_beams(self, log_probs: torch.Tensor, wav_lens: Optional[torch.Tensor] = None,
                     lm_start_state: Any = None) -> List[List[CTCHypothesis]]:
        raise NotImplementedError

    def __call__(self, log_probs, wav_lens=None, lm_start_state=None):
        return self.decode_beams(log_probs, wav_lens, lm_start_state)


class CTCBeamSearcher(CTCBaseSearcher):
    """decoders/ctc.py:1156-1487: the whole search of a batch is one device launch (sbk_ctc_beam_search_f32; with an
    n-gram model, sbk_ctc_beam_search_lm_f32).  Beam sizes up to 256 on both paths."""

    def config(self):
        from speechbrain_amd import native

        # a frame is skipped when logp[blank] > log(blank_skip_threshold): numpy compares the float32 entry with the
        # threshold cast to float32 (NEP 50); log(0) = -inf skips every frame whose blank is finite
        return native.CTCBeamConfig(
            blank=int(self.blank_index), beam_size=int(self.beam_size), topk=int(self.topk),
            prune_history=1 if self.prune_history else 0, beam_prune_logp=float(np.float32(self.beam_prune_logp)),
            token_prune_min_logp=float(np.float32(self.token_prune_min_logp)),
            log_blank_skip_threshold=float(np.float32(self.blank_skip_threshold)), char_base1=HASH_BASE1,
            char_base2=HASH_BASE2, space_code=ord(" ") + 1)

    def decode_beams(self, log_probs, wav_lens=None, lm_start_state=None):
        from speechbrain_amd import native

        if lm_start_state is not None:
            raise NotImplementedError("lm_start_state: the search starts from the model's begin-of-sentence or null "
                                      "context; resuming from a given language-model state is not implemented")
        if log_probs.size(2) != len(self.vocab_list):
            warnings.warn(f"Vocab size mismatch: log_probs vocab dim is {log_probs.size(2)} while vocab_list is "
                          f"{len(self.vocab_list)}. During decoding, going to truncate the log_probs vocab dim to match "
                          "vocab_list.")
        if log_probs.size(2) < len(self.vocab_list):
            raise NotImplementedError("CTC beam search: a vocabulary longer than the posteriors' last dimension")
        x = log_probs if log_probs.dtype == torch.float32 else log_probs.float()
        if self.lm is not None:
            paths, scores, count, fused = native.ctc_beam_search(x, wav_lens, self.token_table(), len(self.vocab_list),
                                                                 self.config(), lm=self.lm)
            paths, scores, fused, count = paths.cpu().numpy(), scores.cpu().numpy(), fused.cpu().numpy(), count.cpu().tolist()
            return [[self.replay(paths[b, k], scores[b, k], fused[b, k]) for k in range(count[b])]
                    for b in range(len(count))]
        paths, scores, count = native.ctc_beam_search(x, wav_lens, self.token_table(), len(self.vocab_list),
                                                      self.config())
        paths, scores, count = paths.cpu().numpy(), scores.cpu().numpy(), count.cpu().tolist()
        return [[self.replay(paths[b, k], scores[b, k]) for k in range(count[b])] for b in range(len(count))]


class CTCPrefixBeamSearcher(CTCBaseSearcher):
    """decoders/ctc.py:1490-: not implemented (the reference itself calls it unstable); use CTCBeamSearcher."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("CTCPrefixBeamSearcher is not implemented: use CTCBeamSearcher")
