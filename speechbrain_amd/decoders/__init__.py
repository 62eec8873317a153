"""speechbrain.decoders mirror (ASR searchers + CTC / TransformerLM scorers)."""
from speechbrain_amd.decoders.scorer import CTCScorer, ScorerBuilder, TransformerLMScorer  # noqa: F401
from speechbrain_amd.decoders.seq2seq import (S2SRNNBeamSearcher, S2SRNNGreedySearcher,  # noqa: F401
                                                S2STransformerBeamSearcher, S2STransformerGreedySearcher,
                                                S2SWhisperBeamSearcher, S2SWhisperGreedySearcher)
from speechbrain_amd.decoders.ctc import (CTCBaseSearcher, CTCBeamSearcher, CTCHypothesis,  # noqa: F401
                                           CTCPrefixBeamSearcher, ctc_greedy_decode, filter_ctc_output)
from speechbrain_amd.decoders.transducer import (TransducerBeamSearcher,  # noqa: F401
                                                  TransducerGreedySearcherStreamingContext)
