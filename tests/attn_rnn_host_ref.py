"""Host restatement of the GRU attention decoder (csrc/attn_rnn.hip) in plain torch, in fp32 or fp64 -- tests only.

Written from the definitions (Bahdanau / Chorowski attention, the GRU cell, the decoder step, greedy decoding), not from
the kernels: content-based and location-aware attention, the GRU cell, one decoder step, teacher forcing and the greedy
loop.  ``mistakes`` plants one of the errors named in MISTAKES, so that the tests can show that their cases would see it.
"""
import torch
import torch.nn.functional as F

MISTAKES = (
    "conv_flipped",         # convolution instead of cross-correlation (taps reversed)
    "mask_ignored",         # frames past enc_len take part in the softmax
    "scale_after_softmax",  # scaling multiplies the softmax instead of the energies
    "ctx_from_enc_h",       # the context is taken from mlp_enc(enc) instead of enc (needs A == E)
    "init_uniform_T",       # the first prev_attn is 1 / T on every frame instead of 1 / enc_len on the valid ones
    "prev_not_updated",     # every step sees the first prev_attn
    "gate_order_zrn",       # the GRU's chunks read as z, r, n
    "b_hn_outside",         # n = tanh(gi_n + b_in + r * gh_n + b_hn)
    "cell_input_c_emb",     # the cell's input is [c | emb]
    "dec_out_cell_c",       # proj takes [cell_out | c]
    "loc_bias_dropped",     # mlp_loc without its bias
)


def attn_init(enc_len, T, dtype, row_utt=None, mistakes=()):
    """The first prev_attn [n,T]: 1 / enc_len on the valid frames of each row's utterance, 0 behind them."""
    lens = enc_len if row_utt is None else enc_len[row_utt.long()]
    if "init_uniform_T" in mistakes:
        return torch.full((lens.shape[0], T), 1.0 / T, dtype=dtype)
    mask = (torch.arange(T)[None, :] < lens[:, None]).to(dtype)
    return mask * (1.0 / lens.to(dtype))[:, None]


def attend(enc, enc_h, enc_len, dec_h, v, prev=None, conv_w=None, loc_w=None, loc_b=None, scaling=1.0, row_utt=None,
           mistakes=()):
    """One attention step for n rows -> (attn [n,T], ctx [n,E]).  enc [B,T,E], enc_h [B,T,A], enc_len [B] (integers),
    dec_h [n,A], v [A]; location-aware when conv_w [C,2k+1], loc_w [A,C], loc_b [A] and prev [n,T] are given."""
    n, T = dec_h.shape[0], enc.shape[1]
    u = torch.arange(n) if row_utt is None else row_utt.long()
    x = enc_h[u] + dec_h[:, None, :]
    if conv_w is not None:
        taps = conv_w.shape[1]
        k = (taps - 1) // 2
        w = conv_w.flip(-1) if "conv_flipped" in mistakes else conv_w
        windows = F.pad(prev, (k, k)).unfold(1, taps, 1)  # [n,T,taps]: window t holds prev[t-k .. t+k]
        loc = torch.einsum("ntj,cj->ntc", windows, w)
        x = x + loc @ loc_w.T
        if "loc_bias_dropped" not in mistakes:
            x = x + loc_b
    e = torch.tanh(x) @ v
    if "mask_ignored" not in mistakes:
        valid = torch.arange(T)[None, :] < enc_len[u][:, None]
        e = e.masked_fill(~valid, float("-inf"))
    attn = torch.softmax(e, dim=-1) * scaling if "scale_after_softmax" in mistakes else torch.softmax(e * scaling, dim=-1)
    src = enc_h if "ctx_from_enc_h" in mistakes else enc
    return attn, torch.einsum("nt,nte->ne", attn, src[u])


def gru_cell(gi, gh, b_ih, b_hh, h, mistakes=()):
    """torch.nn.GRUCell's update from gi = x . W_ih^T and gh = h . W_hh^T (no biases inside); h None = zeros."""
    H = gi.shape[1] // 3
    if b_ih is not None:
        gi, gh = gi + b_ih, gh + b_hh
    b_hn = b_hh[2 * H:] if b_hh is not None else torch.zeros(H, dtype=gi.dtype)
    i0, i1, i_n = gi[:, :H], gi[:, H:2 * H], gi[:, 2 * H:]
    h0, h1, h_n = gh[:, :H], gh[:, H:2 * H], gh[:, 2 * H:]
    if "gate_order_zrn" in mistakes:
        z, r = torch.sigmoid(i0 + h0), torch.sigmoid(i1 + h1)
    else:
        r, z = torch.sigmoid(i0 + h0), torch.sigmoid(i1 + h1)
    if "b_hn_outside" in mistakes:
        cand = torch.tanh(i_n + r * (h_n - b_hn) + b_hn)
    else:
        cand = torch.tanh(i_n + r * h_n)
    hp = h if h is not None else torch.zeros_like(cand)
    return (1.0 - z) * cand + z * hp


class HostDecoder:
    """AttentionalRNNDecoder with GRU cells on the host.  ``sd``: the decoder's state dict under the reference's keys
    (proj.*, attn.mlp_enc.*, attn.mlp_dec.*, attn.mlp_attn.weight, attn.conv_loc.weight, attn.mlp_loc.*, attn.mlp_out.*,
    rnn.rnn_cells.{i}.*); content-based when it has no attn.conv_loc.weight."""

    def __init__(self, sd, scaling=1.0, dtype=torch.float64, mistakes=()):
        self.p = {k: v.detach().to(dtype) for k, v in sd.items()}
        self.dtype, self.scaling, self.mistakes = dtype, scaling, tuple(mistakes)
        self.layers = len([k for k in self.p if k.endswith("weight_ih")])
        self.location = "attn.conv_loc.weight" in self.p
        self.reset()

    def reset(self):
        self.enc_h = self.prev = None

    def step(self, inp, hs, c, enc, enc_len):
        """inp [B,in], hs [L,B,H] or None, c [B,A] -> (dec_out [B,H], hs [L,B,H], c [B,A], attn [B,T])."""
        p, m = self.p, self.mistakes
        x = torch.cat([c, inp], dim=-1) if "cell_input_c_emb" in m else torch.cat([inp, c], dim=-1)
        new_hs = []
        for l in range(self.layers):
            cell = f"rnn.rnn_cells.{l}."
            h = hs[l] if hs is not None else None
            gi = x @ p[cell + "weight_ih"].T
            gh = h @ p[cell + "weight_hh"].T if h is not None else torch.zeros_like(gi)
            x = gru_cell(gi, gh, p.get(cell + "bias_ih"), p.get(cell + "bias_hh"), h, m)
            new_hs.append(x)
        cell_out = x
        if self.enc_h is None:
            self.enc_h = enc @ p["attn.mlp_enc.weight"].T + p["attn.mlp_enc.bias"]
            if self.location:
                self.prev = attn_init(enc_len, enc.shape[1], self.dtype, mistakes=m)
        dec_h = cell_out @ p["attn.mlp_dec.weight"].T + p["attn.mlp_dec.bias"]
        loc = {}
        if self.location:
            w = p["attn.conv_loc.weight"]
            loc = dict(prev=self.prev, conv_w=w.reshape(w.shape[0], w.shape[-1]), loc_w=p["attn.mlp_loc.weight"],
                       loc_b=p["attn.mlp_loc.bias"])
        attn, ctx = attend(enc, self.enc_h, enc_len, dec_h, p["attn.mlp_attn.weight"].reshape(-1), scaling=self.scaling,
                           mistakes=m, **loc)
        if self.location and "prev_not_updated" not in m:
            self.prev = attn
        c = ctx @ p["attn.mlp_out.weight"].T + p["attn.mlp_out.bias"]
        cat = torch.cat([cell_out, c], dim=1) if "dec_out_cell_c" in m else torch.cat([c, cell_out], dim=1)
        return cat @ p["proj.weight"].T + p["proj.bias"], torch.stack(new_hs), c, attn

    def forward(self, inp_tensor, enc, enc_len):
        """Teacher forcing: inp_tensor [B,L,in] -> (outputs [B,L,H], attn [B,L,T], hs [L,B,H], c [B,A])."""
        enc, inp_tensor = enc.to(self.dtype), inp_tensor.to(self.dtype)
        self.reset()
        c = torch.zeros(enc.shape[0], self.p["attn.mlp_out.weight"].shape[0], dtype=self.dtype)
        hs, outs, attns = None, [], []
        for t in range(inp_tensor.shape[1]):
            out, hs, c, w = self.step(inp_tensor[:, t], hs, c, enc, enc_len)
            outs.append(out)
            attns.append(w)
        return torch.stack(outs, 1), torch.stack(attns, 1), hs, c


def greedy(dec, emb, fc_w, fc_b, enc, enc_len, n_steps, bos, eos):
    """Greedy decoding for at most n_steps steps, stopping after the step at which every row has ended.  Returns (tokens [B,L],
    scores [B,L], logits [B,L,V]): a row that has emitted eos, at that step or before, records (eos, 0)."""
    dt = dec.dtype
    emb, fc_w, enc = emb.to(dt), fc_w.to(dt), enc.to(dt)
    fc_b = fc_b.to(dt) if fc_b is not None else torch.zeros(fc_w.shape[0], dtype=dt)
    B = enc.shape[0]
    dec.reset()
    c = torch.zeros(B, dec.p["attn.mlp_out.weight"].shape[0], dtype=dt)
    hs, tok, ended = None, torch.full((B,), bos, dtype=torch.long), torch.zeros(B, dtype=torch.bool)
    toks, scores, logits = [], [], []
    for _ in range(n_steps):
        out, hs, c, _ = dec.step(emb[tok], hs, c, enc, enc_len)
        lg = out @ fc_w.T + fc_b
        tok = lg.argmax(dim=-1)
        sc = torch.log_softmax(lg, dim=-1).gather(1, tok[:, None])[:, 0]
        ended = ended | (tok == eos)
        tok = torch.where(ended, torch.full_like(tok, eos), tok)
        toks.append(tok)
        scores.append(torch.where(ended, torch.zeros_like(sc), sc))
        logits.append(lg)
        if bool(ended.all()):
            break
    return torch.stack(toks, 1), torch.stack(scores, 1), torch.stack(logits, 1)


def hyps_of(tokens, eos):
    """(token lists up to the first eos, relative lengths) of eos-latched tokens [B,L], as S2SGreedySearcher returns them."""
    hyps, rel = [], []
    L = tokens.shape[1]
    for row in tokens.tolist():
        n = row.index(eos) if eos in row else L
        hyps.append(row[:n])
        rel.append(n / L)
    return hyps, rel


def bound(ref32, ref64, floor=1e-5):
    """The project's rule: max(4 x the fp32 restatement's own error against fp64 on the same inputs, floor)."""
    return max(4.0 * float((ref32.double() - ref64).abs().max()), floor)
