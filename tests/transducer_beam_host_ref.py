"""Host restatement of the transducer beam search (TransducerBeamSearcher.transducer_beam_search_decode as DESIGN.md section 5
lists its rules, steps 1-7), written from that description in plain fp32 on the network of tests/transducer_host_ref.py.
The CPU suite pins it to tests/golden/transducer_beam.npz, which the reference itself wrote, so that the device search can be
compared against it at shapes the fixture does not cover, without the reference.  Besides the result it reports the number of
expansions of every frame and the smallest decision margin of the search.  Test tooling only."""
import numpy as np
import torch

from transducer_host_ref import Network  # noqa: F401  (re-exported: the callers build the network from here)

f32 = np.float32


class ExpansionCap(RuntimeError):
    """A frame wanted more than ``max_expansions`` expansions (the reference would go on)."""


def _key(h):
    return f32(h["score"]) / f32(len(h["pred"]))  # an fp32 division by the length


def _first_max(hyps):
    best = 0
    for i in range(1, len(hyps)):
        if _key(hyps[i]) > _key(hyps[best]):
            best = i
    return best


def beam_search(net, tn, blank=0, beam_size=4, nbest=5, state_beam=2.3, expand_beam=2.3, max_expansions=None):
    """tn [B,T,J] -> dict(nbest [[tokens]] per utterance, scores [[float]], mean, expansions [B][T], margin, gaps: the margin by the
    kind of decision).  Raises
    ExpansionCap when a frame asks for an expansion beyond ``max_expansions`` (default 4 * beam_size)."""
    tn = np.asarray(tn, dtype=f32)
    B, T, _ = tn.shape
    L, H = len(net.layers), net.H
    cap = 4 * beam_size if max_expansions is None else max_expansions
    sb, eb = f32(state_beam), f32(expand_beam)
    gaps = dict(topk=float("inf"), expand=float("inf"), state=float("inf"), select=float("inf"), final=float("inf"))
    all_nbest, all_scores, expansions = [], [], np.zeros((B, T), np.int64)
    for b in range(B):
        zero = (np.zeros((L, H), f32), np.zeros((L, H), f32))
        beam = [dict(pred=[blank], score=f32(0.0), state=None)]
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
                vals, pos = torch.topk(torch.from_numpy(lp), beam_size)
                vals, pos = vals.numpy(), pos.numpy().tolist()
                if len(lp) > beam_size:
                    rest = np.delete(lp, pos)
                    gaps["topk"] = min(gaps["topk"], float(vals[-1]) - float(rest.max()))
                best = vals[0] if pos[0] != blank else vals[1]
                thr = f32(best - eb)
                for j in range(beam_size):
                    if pos[j] == blank:
                        beam.append(dict(pred=a["pred"], score=f32(a["score"] + vals[j]), state=a["state"]))
                        continue
                    gaps["expand"] = min(gaps["expand"], abs(float(vals[j]) - float(thr)))
                    if vals[j] >= thr:
                        A.append(dict(pred=a["pred"] + [pos[j]], score=f32(a["score"] + vals[j]), state=(h1, c1)))
        order = sorted(range(len(beam)), key=lambda i: -_key(beam[i]))  # (stable: list order among equal keys)
        keys = [float(_key(beam[i])) for i in order]
        for x, y in zip(keys, keys[1:]):
            gaps["final"] = min(gaps["final"], x - y)
        all_nbest.append([beam[i]["pred"][1:] for i in order[:nbest]])
        all_scores.append(keys[:nbest])
    mean = float(np.exp(np.array([s[0] for s in all_scores], dtype=f32)).mean())
    return dict(nbest=all_nbest, scores=all_scores, mean=mean, expansions=expansions, margin=min(gaps.values()), gaps=gaps)
