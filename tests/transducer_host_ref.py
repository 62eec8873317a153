"""Host restatement of the transducer greedy search (TransducerBeamSearcher.transducer_greedy_decode as DESIGN.md section 5
lists its rules), written from that description in plain numpy.  The CPU suite pins it to tests/golden/transducer_decode.npz,
which the reference itself wrote, so that GPU tests can compare the device search against it at shapes the fixtures do not
cover, without the reference.  Test tooling only."""
import math

import numpy as np

_SQRT1_2 = np.float32(1.0 / math.sqrt(2.0))


def _act(x, name):
    if name == "gelu":
        erf = np.vectorize(math.erf, otypes=[np.float64])
        return (0.5 * x * (1.0 + erf(x.astype(np.float64) * float(_SQRT1_2)))).astype(np.float32)
    if name == "leaky_relu":
        return np.where(x > 0, x, x * np.float32(0.01)).astype(np.float32)
    if name == "relu":
        return np.maximum(x, np.float32(0.0))
    return np.tanh(x).astype(np.float32)


def _sigmoid(x):
    return (1.0 / (1.0 + np.exp(-x))).astype(np.float32)


class Network:
    """The weights of one transducer by the reference's state_dict names (emb.Embedding.weight, dec.rnn.weight_ih_l0, ...,
    proj_dec.w.weight, transducer_lin.w.weight) as float32 numpy arrays."""

    def __init__(self, sd, act):
        g = lambda k: None if k not in sd else np.asarray(sd[k], dtype=np.float32)  # noqa: E731
        self.emb = g("emb.Embedding.weight")
        self.layers = []
        l = 0
        while f"dec.rnn.weight_hh_l{l}" in sd:
            self.layers.append((g(f"dec.rnn.weight_ih_l{l}"), g(f"dec.rnn.weight_hh_l{l}"), g(f"dec.rnn.bias_ih_l{l}"),
                                g(f"dec.rnn.bias_hh_l{l}")))
            l += 1
        self.proj_w, self.proj_b = g("proj_dec.w.weight"), g("proj_dec.w.bias")
        self.out_w, self.out_b = g("transducer_lin.w.weight"), g("transducer_lin.w.bias")
        self.act = act
        self.H = self.layers[0][1].shape[1]

    def pn_step(self, tok, h, c):
        x = self.emb[tok]
        h, c = h.copy(), c.copy()
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.layers):
            g = w_ih @ x + w_hh @ h[l]
            if b_ih is not None:
                g = g + b_ih + b_hh
            H = self.H
            i, f, gg, o = _sigmoid(g[:H]), _sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), _sigmoid(g[3 * H:])
            c[l] = f * c[l] + i * gg
            h[l] = o * np.tanh(c[l])
            x = h[l]
        out = self.proj_w @ x
        if self.proj_b is not None:
            out = out + self.proj_b
        return out.astype(np.float32), h, c

    def joint(self, tn_t, out_pn):
        z = _act((tn_t + out_pn).astype(np.float32), self.act)
        logits = self.out_w @ z
        if self.out_b is not None:
            logits = logits + self.out_b
        m = logits.max()
        return ((logits - m) - np.log(np.exp(logits - m).sum())).astype(np.float32)


def greedy(net, tn, blank=0, max_symbols_per_step=5, state=None):
    """tn [B,T,J] -> (tokens [[int]] * B, score [B], out_pn [B,J], h [L,B,H], c [L,B,H], gaps [[float]] * B): every frame
    of every utterance, at most max_symbols_per_step + 1 emissions per frame, arg-max ties to the first index."""
    tn = np.asarray(tn, dtype=np.float32)
    B, T, _ = tn.shape
    L, H = len(net.layers), net.H
    toks, scores, gaps = [], np.zeros(B, np.float32), []
    outs, hs, cs = [], np.zeros((L, B, H), np.float32), np.zeros((L, B, H), np.float32)
    for b in range(B):
        if state is None:
            out, h, c = net.pn_step(blank, np.zeros((L, H), np.float32), np.zeros((L, H), np.float32))
        else:
            out, h, c = (np.asarray(state[0][b], np.float32).reshape(-1), np.asarray(state[1][:, b], np.float32),
                         np.asarray(state[2][:, b], np.float32))
        seq, gp, score = [], [], np.float32(0.0)
        for t in range(T):
            for _ in range(max_symbols_per_step + 1):
                lp = net.joint(tn[b, t], out)
                k = int(np.argmax(lp))
                top2 = np.sort(lp)[-2:]
                gp.append(float(top2[1] - top2[0]))
                if k == blank:
                    break
                seq.append(k)
                score = np.float32(score + lp[k])
                out, h, c = net.pn_step(k, h, c)
        toks.append(seq)
        scores[b] = score
        gaps.append(gp)
        outs.append(out)
        hs[:, b], cs[:, b] = h, c
    return toks, scores, np.stack(outs), hs, cs, gaps
