"""Host restatement of the transducer beam search with RNNLM shallow fusion (TransducerBeamSearcher.
transducer_beam_search_decode with lm_weight > 0, as DESIGN.md section 5 lists its rules), written from that description in
plain fp32 numpy on the network of tests/transducer_host_ref.py and an RNNLM restated here.  The CPU suite pins it to
tests/golden/transducer_beam_lm.npz, which the reference itself wrote, so that the device search can be compared against it
at shapes the fixture does not cover, without the reference.  Besides the result it reports the number of expansions of every
frame, the LM steps taken and the smallest decision margin of the search (measured on the scores the hypotheses hold, so the
LM terms are part of it).  Test tooling only."""
import numpy as np
import torch

from transducer_beam_host_ref import ExpansionCap, _first_max, _key  # noqa: F401  (the same key and selection rules)
from transducer_host_ref import Network, _act, _sigmoid  # noqa: F401

f32 = np.float32


class LM:
    """An RNNLM by the reference's state_dict names under ``prefix`` (embedding.Embedding.weight, rnn.rnn.weight_ih_l0, ...,
    dnn.linear.w.weight, dnn.norm.norm.weight, dnn.linear_0..., out.w.weight) as float32 numpy arrays."""

    def __init__(self, sd, act, prefix="lm.", eps=1e-5):
        g = lambda k: None if prefix + k not in sd else np.asarray(sd[prefix + k], dtype=f32)  # noqa: E731
        self.emb = g("embedding.Embedding.weight")
        self.layers = []
        l = 0
        while g(f"rnn.rnn.weight_hh_l{l}") is not None:
            self.layers.append(tuple(g(f"rnn.rnn.{n}_l{l}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")))
            l += 1
        self.blocks = []
        for name in ["", "_0", "_1", "_2"]:
            if g(f"dnn.linear{name}.w.weight") is None:
                break
            self.blocks.append((g(f"dnn.linear{name}.w.weight"), g(f"dnn.linear{name}.w.bias"),
                                g(f"dnn.norm{name}.norm.weight"), g(f"dnn.norm{name}.norm.bias")))
        self.out_w, self.out_b = g("out.w.weight"), g("out.w.bias")
        self.act, self.eps = act, f32(eps)
        self.H = self.layers[0][1].shape[1]

    def zero(self):
        return np.zeros((len(self.layers), self.H), f32), np.zeros((len(self.layers), self.H), f32)

    def logits(self, tok, h, c):
        """One step -> (logits [V_lm], h, c)"""
        x = self.emb[tok]
        h, c = h.copy(), c.copy()
        H = self.H
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.layers):
            g = w_ih @ x + w_hh @ h[l]
            if b_ih is not None:
                g = g + b_ih + b_hh
            i, f, gg, o = _sigmoid(g[:H]), _sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sigmoid(g[3 * H:])
            c[l] = f * c[l] + i * gg
            h[l] = o * np.tanh(c[l])
            x = h[l]
        for w, b, ln_g, ln_b in self.blocks:
            y = (w @ x + b).astype(f32)
            mean = y.mean(dtype=f32)
            var = ((y - mean) ** 2).mean(dtype=f32)
            x = _act(((y - mean) / np.sqrt(var + self.eps) * ln_g + ln_b).astype(f32), self.act)
        out = self.out_w @ x
        if self.out_b is not None:
            out = out + self.out_b
        return out.astype(f32), h, c

    def step(self, tok, h, c):
        """-> (log-probabilities over the LM's whole output, h, c)"""
        out, h, c = self.logits(tok, h, c)
        m = out.max()
        return ((out - m) - np.log(np.exp(out - m).sum())).astype(f32), h, c


def beam_search(net, lm, lm_weight, tn, blank=0, beam_size=4, nbest=5, state_beam=2.3, expand_beam=2.3, max_expansions=None):
    """tn [B,T,J] -> dict(nbest, scores, mean, expansions [B][T], lm_steps [B], margin, gaps).  ``lm`` None or ``lm_weight``
    <= 0: the search without an LM.  Raises ExpansionCap when a frame asks for an expansion beyond ``max_expansions`` (default
    4 * beam_size)."""
    tn = np.asarray(tn, dtype=f32)
    B, T, _ = tn.shape
    L, H = len(net.layers), net.H
    fuse = lm is not None and lm_weight > 0
    lw = f32(lm_weight)
    cap = 4 * beam_size if max_expansions is None else max_expansions
    sb, eb = f32(state_beam), f32(expand_beam)
    gaps = dict(topk=float("inf"), expand=float("inf"), state=float("inf"), select=float("inf"), final=float("inf"))
    all_nbest, all_scores, expansions, lm_steps = [], [], np.zeros((B, T), np.int64), np.zeros(B, np.int64)
    for b in range(B):
        zero = (np.zeros((L, H), f32), np.zeros((L, H), f32))
        beam = [dict(pred=[blank], score=f32(0.0), state=None, lm=None, lm_out=None)]
        for t in range(T):
            A, beam = beam, []
            while True:
                if len(beam) >= beam_size:
                    break
                ai = _first_max(A)
                a = A[ai]
                if len(A) > 1:
                    keys = sorted((float(_key(h)) for h in A), reverse=True)
                    gaps["select"] = min(gaps["select"], keys[0] - keys[1])
                if beam:
                    bb = beam[_first_max(beam)]
                    rhs = f32(sb + a["score"])
                    gaps["state"] = min(gaps["state"], abs(float(bb["score"]) - float(rhs)))
                    if bb["score"] >= rhs:
                        break
                if expansions[b, t] >= cap:
                    raise ExpansionCap(f"utterance {b} frame {t}: more than {cap} expansions")
                A.pop(ai)
                h0, c0 = zero if a["state"] is None else a["state"]
                out, h1, c1 = net.pn_step(a["pred"][-1], h0, c0)
                lp = net.joint(tn[b, t], out)
                expansions[b, t] += 1
                lm_out = a["lm_out"]
                if fuse and lm_out is None:  # the LM takes the PN's input and moves with its state
                    lh, lc = lm.zero() if a["lm"] is None else a["lm"]
                    lm_lp, lh1, lc1 = lm.step(a["pred"][-1], lh, lc)
                    lm_out = (lm_lp, (lh1, lc1))
                    lm_steps[b] += 1
                vals, pos = torch.topk(torch.from_numpy(lp), beam_size)
                vals, pos = vals.numpy(), pos.numpy().tolist()
                if len(lp) > beam_size:
                    rest = np.delete(lp, pos)
                    gaps["topk"] = min(gaps["topk"], float(vals[-1]) - float(rest.max()))
                best = vals[0] if pos[0] != blank else vals[1]
                thr = f32(best - eb)
                for j in range(beam_size):
                    if pos[j] == blank:  # the old PN and LM state, no LM term; (lm_out: the step of this (token, state) pair
                        # is deterministic, so a hypothesis expanded again at the next frame keeps what it gave)
                        beam.append(dict(pred=a["pred"], score=f32(a["score"] + vals[j]), state=a["state"], lm=a["lm"],
                                         lm_out=lm_out))
                        continue
                    gaps["expand"] = min(gaps["expand"], abs(float(vals[j]) - float(thr)))
                    if vals[j] >= thr:
                        score = f32(a["score"] + vals[j])
                        if fuse:
                            score = f32(score + f32(lw * lm_out[0][pos[j]]))  # the product is rounded before the add
                        A.append(dict(pred=a["pred"] + [pos[j]], score=score, state=(h1, c1),
                                      lm=lm_out[1] if fuse else None, lm_out=None))
        order = sorted(range(len(beam)), key=lambda i: -_key(beam[i]))  # (stable: list order among equal keys)
        keys = [float(_key(beam[i])) for i in order]
        for x, y in zip(keys, keys[1:]):
            gaps["final"] = min(gaps["final"], x - y)
        all_nbest.append([beam[i]["pred"][1:] for i in order[:nbest]])
        all_scores.append(keys[:nbest])
    mean = float(np.exp(np.array([s[0] for s in all_scores], dtype=f32)).mean())
    return dict(nbest=all_nbest, scores=all_scores, mean=mean, expansions=expansions, lm_steps=lm_steps,
                margin=min(gaps.values()), gaps=gaps)
