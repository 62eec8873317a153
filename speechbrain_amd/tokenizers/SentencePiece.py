"""speechbrain.tokenizers.SentencePiece mirror: the streaming decode helpers (tokenizers/SentencePiece.py:519-570), host
code on the ``sentencepiece`` package."""
from dataclasses import dataclass
from typing import List


@dataclass
class SentencePieceDecoderStreamingContext:
    """Mutable streaming context for a single SentencePiece streaming session."""

    emitted_symbol_count: int = 0


def spm_decode_preserve_leading_space(tokenizer, hyps: List[int], context: SentencePieceDecoderStreamingContext) -> str:
    """Decodes one hypothesis without dropping the leading space of a piece that starts mid-transcription (SentencePiece
    decodes every call as a whole sentence, so the word boundary of a chunk's first piece would be lost)."""
    # (the reference reads text and pieces from the decoder's immutable proto, which newer sentencepiece releases no longer
    # offer; the proto's pieces are the hypothesis' ids as pieces and its text is the plain decode)
    hyps = [int(t) for t in hyps]
    text = tokenizer.decode(hyps)
    if len(hyps) >= 1:
        if context.emitted_symbol_count > 0 and tokenizer.id_to_piece(hyps[0]).startswith("\u2581"):
            text = " " + text
        context.emitted_symbol_count += len(hyps)
    return text
