"""Host restatement of the CTC prefix scorer (the reference's decoders/ctc.py:26-295, CTCPrefixScore.forward_step and
permute_mem in full-vocabulary mode, with and without ctc_window_size), written from that description in plain numpy:
float64, log domain, true -inf inside.  The CPU suite pins it to oracle.sb_oracle.CTCPrefixScorer (float32) and to
tests/golden/ctc_prefix.npz, which the reference itself wrote, so that the kernels of csrc/ctc_prefix.hip can be compared
against it at shapes neither covers.  Test tooling only.

psi needs no recurrence (it is a log-sum over frames of the PARENT's variables), so only the forward variables of the
(parent, token) pairs the driver selects are evaluated: O(T * n_bh) per step instead of the reference's [T,2,n_bh,V]."""
import numpy as np

NEG = -1e20  # the reference's finite "minus infinity" (ctc.py:53)


def _lse(a, axis):
    """log-sum-exp along `axis`; an all -inf (or empty) slice gives -inf."""
    if a.shape[axis] == 0:
        return np.full(a.shape[:axis] + a.shape[axis + 1:], -np.inf)
    m = a.max(axis=axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return np.squeeze(ms, axis) + np.log(np.exp(a - ms).sum(axis=axis))


def sentinel(a):
    """-inf -> the reference's -1e20."""
    return np.maximum(a, NEG)


class CTCPrefixRef:
    """log_probs [B,T,V] = log_softmax(ctc_fc(enc)), enc_len [B] absolute lengths.  ``score(last_tok, step)`` returns
    psi - psi_prev [B*beam, V] with both terms mapped to the -1e20 sentinel first (a dead entry of a dead hypothesis is 0,
    as in the reference); ``permute(parent, token)`` moves the state to hypotheses (parent row in [0, B*beam), token)."""

    def __init__(self, log_probs, enc_len, blank, eos, ctc_window_size=0):
        x = np.array(log_probs, dtype=np.float64)
        self.B, self.T, self.V = x.shape
        self.len = np.asarray(enc_len, dtype=np.int64)
        pad = np.arange(self.T)[None, :] >= self.len[:, None]  # frames >= len (ctc.py:58-62)
        x[pad] = -np.inf
        x[:, :, 0][pad] = 0.0  # column 0 whatever the blank index is, as the reference does
        self.x, self.blank, self.eos, self.window = x, int(blank), int(eos), int(ctc_window_size)
        self.r_nb = self.r_b = self.psi_prev = self.psi = None

    def frame_range(self, step, attn_window=None):
        start, end = max(1, step), self.T
        if self.window > 0 and attn_window is not None:  # ctc.py:189-200, attn_window = (min, max) of the attention peaks
            start = max(start, int(attn_window[0]) - self.window)
            end = min(self.T, int(attn_window[1]) + self.window)
        return start, end

    def score(self, last_tok, step, attn_window=None):
        last_tok = np.asarray(last_tok, dtype=np.int64)
        n_bh = last_tok.shape[0]
        beam = n_bh // self.B
        B, T, V = self.B, self.T, self.V
        if self.r_nb is None:  # ctc.py:108-123
            self.r_nb = np.full((n_bh, T), -np.inf)
            self.r_b = np.repeat(np.cumsum(self.x[:, :, self.blank], axis=1), beam, axis=0)
            self.psi_prev = np.zeros(n_bh)
        start, end = self.frame_range(step, attn_window)
        r_sum = np.logaddexp(self.r_nb, self.r_b)
        psi = np.empty((n_bh, V))
        rows = slice(max(start - 1, 0), max(end - 1, start - 1))  # phi[t-1] of the scored frames t in [start, end)
        frames = slice(start, max(end, start))
        for b in range(B):
            hyp = slice(b * beam, (b + 1) * beam)
            psi[hyp] = _lse(r_sum[hyp, rows, None] + self.x[b, None, frames, :], axis=1)
        for n in range(n_bh):  # the token that repeats the prefix' last one continues from the blank variable only
            c = int(last_tok[n])
            if 0 <= c < V:
                psi[n, c] = _lse(self.r_b[n, rows] + self.x[n // beam, frames, c], axis=0)
        if step == 0 and start == 1:  # psi_init = r[start-1][nb] (ctc.py:172-173,212)
            psi = np.logaddexp(psi, np.repeat(self.x[:, 0, :], beam, axis=0))
        idx = np.arange(n_bh)
        psi[idx, self.eos] = r_sum[idx, np.repeat(self.len - 1, beam)]
        if self.eos != self.blank:
            psi[:, self.blank] = -np.inf
        self.psi, self.last_tok, self.step, self.range = psi, last_tok, step, (start, end)
        return sentinel(psi) - sentinel(self.psi_prev)[:, None]

    def permute(self, parent, token):
        """The forward variables of hypothesis n = (parent[n], token[n]) over the frames of the last score() call."""
        parent, token = np.asarray(parent, dtype=np.int64), np.asarray(token, dtype=np.int64)
        n_bh = parent.shape[0]
        beam = n_bh // self.B
        utt = np.arange(n_bh) // beam
        assert np.array_equal(parent // beam, utt)
        start, end = self.range
        same = self.last_tok[parent] == token
        phi = np.where(same[:, None], self.r_b[parent], np.logaddexp(self.r_nb[parent], self.r_b[parent]))
        xc = self.x[utt, :, token]  # [n_bh, T]
        xb = self.x[utt, :, self.blank]
        nb = np.full((n_bh, self.T), -np.inf)
        bl = np.full((n_bh, self.T), -np.inf)
        if self.step == 0:
            nb[:, 0] = xc[:, 0]
        for t in range(start, end):
            nb[:, t] = np.logaddexp(nb[:, t - 1], phi[:, t - 1]) + xc[:, t]
            bl[:, t] = np.logaddexp(nb[:, t - 1], bl[:, t - 1]) + xb[:, t]
        self.psi_prev = self.psi[parent, token]
        self.r_nb, self.r_b = nb, bl
