"""speechbrain.decoders.transducer mirror: TransducerBeamSearcher's greedy search and beam search (decoders/transducer.py:
25-476) on the device.

The whole search of a batch -- prediction network (PN) steps, joint, classifier, log-softmax and arg-max or top-k for every
frame -- is ONE launch of sbk_transducer_greedy_f32 (``beam_size <= 1``) or sbk_transducer_beam_search_f32 (``beam_size >
1``; csrc/transducer.hip), one workgroup per utterance.  Supported: the PN [Embedding (dense or one-hot), LSTM
(unidirectional, 1..4 layers), Linear], Transducer_joint(joint="sum") with GELU, LeakyReLU, Tanh or ReLU, and one classifier
Linear.  The beam search fuses an LM (``lm_module`` with ``lm_weight > 0``) when it is a lobes.models.RNNLM.RNNLM with a 1..4
layer unidirectional LSTM, 1..2 DNN blocks and LeakyReLU, ReLU, GELU or Tanh: sbk_transducer_beam_search_lm_f32, still one
launch.  Any other LM, LM fusion in the greedy search and other PN layers raise NotImplementedError when the searcher is
called; so does a beam above native.TRANSDUCER_MAX_BEAM.

The reference's beam search has no bound on the expansions of a frame (it never leaves a frame whose blank stays out of the
top ``beam_size``); here ``max_expansions`` (default ``4 * beam_size``) bounds them.  A search that reaches the bound ends,
warns and names the utterances; its tokens for those are unspecified."""
import warnings
from dataclasses import dataclass
from typing import Any, Optional

import torch

from speechbrain_amd import native


@dataclass
class TransducerGreedySearcherStreamingContext(torch.nn.Module):
    """The hidden state carried between the chunks of a stream (decoders/transducer.py:15-22)."""

    hidden: Optional[Any] = None


class TransducerBeamSearcher(torch.nn.Module):
    """decoders/transducer.py:25-145.  Constructs with any arguments (reference YAMLs define a beam searcher with an LM
    beside the greedy one); what is not built raises when the searcher is called."""

    def __init__(self, decode_network_lst, tjoint, classifier_network, blank_id, beam_size=4, nbest=5, lm_module=None,
                 lm_weight=0.0, state_beam=2.3, expand_beam=2.3):
        super().__init__()
        self.decode_network_lst = decode_network_lst
        self.tjoint = tjoint
        self.classifier_network = classifier_network
        self.blank_id = blank_id
        self.beam_size = beam_size
        self.nbest = nbest
        self.lm = lm_module
        self.lm_weight = lm_weight
        if lm_module is None and lm_weight > 0:
            raise ValueError("Language model is not provided.")
        self.state_beam = state_beam
        self.expand_beam = expand_beam
        if self.beam_size <= 1:
            self.searcher = self.transducer_greedy_decode
        else:
            self.searcher = self.transducer_beam_search_decode
        self._prepared, self._lm_prepared = native.Derived(), native.Derived()

    def forward(self, tn_output):
        return self.searcher(tn_output)

    def transducer_beam_search_decode(self, tn_output, max_expansions=None, return_status=False):
        """decoders/transducer.py:320-476.  Returns (best hypothesis per utterance, exp(best scores).mean(), nbest_batch,
        nbest_batch_score): token lists without the leading blank, and logp_score / len(prediction) (the leading blank counts)
        as Python floats.  ``max_expansions``: the bound on the expansions of one frame (default 4 * beam_size; the reference
        has none).  Utterances that reach it, or whose log-probabilities are not finite, are named in a warning and their
        result is unspecified.  ``return_status`` appends (status word, number of expansions) per utterance, as lists.  (No
        hypothesis is truncated: the kernel is given room for T * max_expansions tokens, which none can exceed.)"""
        fuse = self.lm is not None and self.lm_weight > 0  # (with lm_weight <= 0 the reference never touches the LM)
        if fuse:
            self._lm_networks()  # (refuses what is not built before anything runs)
        if self.beam_size > native.TRANSDUCER_MAX_BEAM:
            raise NotImplementedError(f"transducer beam search with beam_size={self.beam_size} is not implemented "
                                      f"(at most {native.TRANSDUCER_MAX_BEAM})")
        tn = tn_output.detach().float().contiguous()
        prep = self._prepare(tn.device, beam=True)
        lm = self._prepare_lm(tn.device) if fuse else None
        if lm is not None and lm.M.vocab < prep.W.vocab:
            raise ValueError(f"the LM has {lm.M.vocab} outputs, fewer than the {prep.W.vocab} of the classifier")
        if self.beam_size > prep.W.vocab:
            raise ValueError(f"beam_size={self.beam_size} is larger than the {prep.W.vocab} outputs of the classifier")
        if tn.shape[0] == 0:  # (the reference's mean over no utterances)
            ret = ([], torch.tensor(float("nan")), [], [])
            return ret + (([], []),) if return_status else ret
        if max_expansions is None:
            max_expansions = native.transducer_beam_max_expansions(self.beam_size)
        tokens, length, score, count, status, expansions = native.transducer_beam_search(
            prep, tn, self.blank_id, self.beam_size, self.nbest, state_beam=self.state_beam, expand_beam=self.expand_beam,
            max_expansions=max_expansions, act=self.tjoint.act_code, lm=lm, lm_weight=float(self.lm_weight) if fuse else 0.0)
        length, counts, status = length.cpu(), count.cpu().tolist(), status.cpu().tolist()
        rows = tokens[:, :, :max(1, int(length.max()))].cpu().tolist()
        length, scores = length.tolist(), score.cpu().tolist()
        capped = [b for b, st in enumerate(status) if st & native.TBEAM_CAPPED]
        if capped:
            warnings.warn(f"transducer beam search: utterances {capped} reached the bound on the expansions of one frame "
                          f"(max_expansions={max_expansions}); their hypotheses are unspecified")
        exhausted = [b for b, st in enumerate(status) if st & native.TBEAM_EXHAUSTED]
        if exhausted:
            warnings.warn(f"transducer beam search: utterances {exhausted} ran out of hypotheses to expand (log-probabilities "
                          "that are not finite); their hypotheses are unspecified")
        nbest_batch = [[rows[b][k][:length[b][k]] for k in range(counts[b])] for b in range(len(counts))]
        nbest_batch_score = [scores[b][:counts[b]] for b in range(len(counts))]
        best = torch.tensor([s[0] for s in nbest_batch_score], dtype=torch.float32)
        ret = ([n[0] for n in nbest_batch], best.exp().mean(), nbest_batch, nbest_batch_score)
        return ret + ((status, expansions.cpu().tolist()),) if return_status else ret

    # ------------------------------------------------------------------ the network, in the kernel's layout
    def _networks(self, beam=False):
        from speechbrain_amd.nnet.embedding import Embedding
        from speechbrain_amd.nnet.linear import Linear
        from speechbrain_amd.nnet.RNN import LSTM

        if self.lm is not None and self.lm_weight > 0 and not beam:
            raise NotImplementedError("transducer decoding with LM fusion is not implemented")
        layers = list(self.decode_network_lst)
        for layer in layers:
            if type(layer).__name__ in ("GRU", "RNN", "LiGRU", "LiGRU_Layer"):
                raise NotImplementedError(f"a {type(layer).__name__} prediction network is not implemented (LSTM only)")
        if not (len(layers) == 3 and isinstance(layers[0], Embedding) and isinstance(layers[1], LSTM)
                and isinstance(layers[2], Linear)):
            raise NotImplementedError("transducer prediction networks other than [Embedding, LSTM, Linear] are not "
                                      f"implemented (got {[type(x).__name__ for x in layers]})")
        cls = list(self.classifier_network)
        if not (len(cls) == 1 and isinstance(cls[0], Linear)):
            raise NotImplementedError("transducer classifiers other than one Linear are not implemented "
                                      f"(got {[type(x).__name__ for x in cls]})")
        return layers[0], layers[1], layers[2], cls[0]

    _LM_ACTS = {"LeakyReLU": native.ACT_LEAKY_RELU, "ReLU": native.ACT_RELU, "GELU": native.ACT_GELU, "Tanh": native.ACT_TANH}

    def _lm_networks(self):
        """(embedding, LSTM, [(Linear, LayerNorm)] per DNN block, out Linear, activation code) of an LM the kernel fuses."""
        from speechbrain_amd.lobes.models.RNNLM import RNNLM

        lm = self.lm
        refuse = lambda why: NotImplementedError(  # noqa: E731
            f"transducer beam search with LM fusion is not implemented for {type(lm).__name__}{why} (an RNNLM with a 1..4 layer "
            "unidirectional LSTM, 1..2 DNN blocks and LeakyReLU, ReLU, GELU or Tanh)")
        if not isinstance(lm, RNNLM):
            raise refuse("")
        rnn = lm.rnn.rnn
        if rnn.bidirectional or not 1 <= rnn.num_layers <= native.TRANSDUCER_MAX_LAYERS:
            raise refuse(f" with {rnn.num_layers} {'bidirectional ' if rnn.bidirectional else ''}LSTM layers")
        blocks = lm.blocks()
        if not 1 <= len(blocks) <= native.RNNLM_MAX_DNN:
            raise refuse(f" with {len(blocks)} DNN blocks")
        acts = {type(b[2]) for b in blocks}
        act = next(iter(acts))
        if len(acts) != 1 or act not in (torch.nn.LeakyReLU, torch.nn.ReLU, torch.nn.GELU, torch.nn.Tanh):
            raise refuse(f" with activation {sorted(a.__name__ for a in acts)}")
        mod = blocks[0][2]
        if (act is torch.nn.LeakyReLU and mod.negative_slope != 0.01) or (act is torch.nn.GELU and mod.approximate != "none"):
            raise refuse(f" with {mod}")
        return lm.embedding, lm.rnn, [(b[0], b[1]) for b in blocks], lm.out, self._LM_ACTS[act.__name__]

    def _prepare_lm(self, device):
        """The LM's weight layouts on ``device``, by the key rule of _prepare."""
        emb, lstm, blocks, out, act = self._lm_networks()
        d = lambda t: None if t is None else t.detach().to(device)  # noqa: E731

        def build():
            layers = [tuple(d(t) for t in layer) for layer in lstm.layer_weights()]
            dnn = [(d(lin.w.weight), d(lin.w.bias), d(ln.norm.weight), d(ln.norm.bias), ln.eps) for lin, ln in blocks]
            return native.RNNLMPrepared(d(emb.Embedding.weight), layers, dnn, d(out.w.weight), d(out.w.bias), act)

        return self._lm_prepared.get(list(self.lm.parameters()), build, device=device,
                                     extra=(device, act) + tuple(ln.eps for _, ln in blocks))

    def _prepare(self, device, beam=False):
        """The kernel's weight layouts on ``device``, rebuilt when a parameter changes (the PN and classifier modules are
        plain list members, as in the reference, so they are not moved with the searcher).  ``beam``: called by the beam
        search, which decodes with an LM; the greedy search refuses one."""
        emb, lstm, proj, lin = self._networks(beam)
        params = [emb.Embedding.weight] + [p for p in lstm.parameters()] + [p for p in proj.parameters()] + [
            p for p in lin.parameters()]
        d = lambda t: None if t is None else t.detach().to(device)  # noqa: E731

        def build():
            layers = [tuple(d(t) for t in layer) for layer in lstm.layer_weights()]
            return native.TransducerPrepared(d(emb.Embedding.weight), layers, d(proj.w.weight), d(proj.w.bias), d(lin.w.weight),
                                             d(lin.w.bias))

        return self._prepared.get(params, build, device=device, extra=(device,))

    # ------------------------------------------------------------------ greedy search
    def transducer_greedy_decode(self, tn_output, hidden_state=None, return_hidden=False, max_symbols_per_step=5,
                                 frame_block=0):
        """decoders/transducer.py:156-291.  Returns (hyps, exp(scores).mean(), None, None[, (out_PN, (h, c))]) with
        hyps a list of token lists.  The hidden state is a set of device tensors of the reference's shapes, out_PN
        [B,1,J] and h / c [L,B,H]; a given ``hidden_state`` is updated in place, as the reference does.  ``frame_block``:
        frames evaluated together by the kernel (0 = its default; the result does not depend on it)."""
        tn = tn_output.detach().float().contiguous()
        prep = self._prepare(tn.device)
        act = self.tjoint.act_code
        B, T, J = tn.shape
        L, H = prep.W.n_layers, prep.W.hidden
        if hidden_state is None:
            out_pn = torch.empty(B, 1, J, dtype=torch.float32, device=tn.device)
            h = torch.empty(L, B, H, dtype=torch.float32, device=tn.device)
            c = torch.empty(L, B, H, dtype=torch.float32, device=tn.device)
            start = True
        else:
            out_pn, (h, c) = hidden_state
            for t, shape in ((out_pn, (B, 1, J)), (h, (L, B, H)), (c, (L, B, H))):
                if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"hidden_state: expected contiguous fp32 tensors of shapes [B,1,J], [L,B,H], [L,B,H]; "
                                     f"got {tuple(t.shape)} {t.dtype}")
            start = False
        tokens, count, score = native.transducer_greedy(prep, tn, out_pn, h, c, self.blank_id, max_symbols_per_step,
                                                        start_from_blank=start, act=act, frame_block=frame_block)
        counts = count.cpu().tolist()
        rows = tokens.cpu().tolist()
        hyps = [row[:n] for row, n in zip(rows, counts)]
        scores = score.cpu()
        ret = (hyps, scores.exp().mean(), None, None)
        if return_hidden:
            ret += ((out_pn, (h, c)),)
        return ret

    def transducer_greedy_decode_streaming(self, x: torch.Tensor, context: TransducerGreedySearcherStreamingContext):
        """decoders/transducer.py:293-317: a `decoding_function` for StreamingASR."""
        hyp, _scores, _, _, hidden = self.transducer_greedy_decode(x, context.hidden, return_hidden=True)
        context.hidden = hidden
        return hyp
