"""Host restatement of one RNNLM scorer step (RNNLMScorer.score after permute_mem): embedding, LSTMCell arithmetic per layer on the
state rows index_select'ed by ``parent``, the DNN blocks, the output layer and weight * log_softmax(logits / temperature).  Plain
torch in the dtype of the weights it is given."""
import torch

MISTAKES = (
    "state_by_row",     # h and c are read by row instead of through parent
    "gate_order_ifog",  # the gate chunks read as i, f, o, g
    "parent_mod_128",   # the parent index taken modulo 128 (a map kept per 128-row group)
    "rows_past_128_from_zero",  # rows >= 128 read the state that row r - 128 reads (a second row group that starts at row 0 again)
    "ln_first_256",     # LayerNorm statistics over the first 256 columns only (a strided loop that makes one trip)
    "bias_once",        # only b_ih is added
    "token_clamped_to_vocab",  # a token >= V embeds as V - 1 (clamped to the output size, not to the embedding table's)
)
ACTS = {"leaky_relu": torch.nn.functional.leaky_relu, "relu": torch.relu, "gelu": torch.nn.functional.gelu, "tanh": torch.tanh}


def random_lm(gen, V, E, H, layers, blocks, D, dtype=torch.float32, n_emb=None, lstm_bias=True, dnn_bias=True, out_bias=True):
    """Weights of an RNNLM by plain names: emb [n_emb,E] (n_emb None: V); lstm [(w_ih, w_hh, b_ih, b_hh)]; dnn [(w, b, ln_g, ln_b,
    eps)]; out_w, out_b.  ``lstm_bias`` / ``dnn_bias`` / ``out_bias`` False: those biases are None (drawn all the same, so that
    the other weights do not depend on the switch)."""
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=dtype)  # noqa: E731
    lstm = [(rn(4 * H, E if l == 0 else H) / (E if l == 0 else H) ** 0.5, rn(4 * H, H) / H ** 0.5, rn(4 * H) * 0.3, rn(4 * H) * 0.3)
            for l in range(layers)]
    dnn = [(rn(D, H if i == 0 else D) / (H if i == 0 else D) ** 0.5, rn(D) * 0.3, 1.0 + 0.2 * rn(D), rn(D) * 0.3, 1e-5)
           for i in range(blocks)]
    lm = dict(emb=rn(V if n_emb is None else n_emb, E), lstm=lstm, dnn=dnn, out_w=rn(V, D) / D ** 0.5, out_b=rn(V) * 0.3)
    if not lstm_bias:
        lm["lstm"] = [(w_ih, w_hh, None, None) for w_ih, w_hh, _, _ in lstm]
    if not dnn_bias:
        lm["dnn"] = [(w, None, g, beta, eps) for w, _, g, beta, eps in dnn]
    if not out_bias:
        lm["out_b"] = None
    return lm


def cast(lm, dtype):
    c = lambda t: t.to(dtype) if torch.is_tensor(t) else t  # noqa: E731
    return dict(emb=c(lm["emb"]), lstm=[tuple(c(t) for t in l) for l in lm["lstm"]], dnn=[tuple(c(t) for t in b) for b in lm["dnn"]],
                out_w=c(lm["out_w"]), out_b=c(lm["out_b"]))


def _layer_norm(y, g, beta, eps, first=None):
    """LayerNorm whose mean and variance come from the first ``first`` columns only (None: torch's own)."""
    if first is None or first >= y.shape[1]:
        return torch.nn.functional.layer_norm(y, (y.shape[1],), g, beta, eps)
    mean = y[:, :first].mean(1, keepdim=True)
    var = ((y[:, :first] - mean) ** 2).mean(1, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * g + beta


def step(lm, act, tokens, parent, state, weight=1.0, temperature=1.0, mistakes=()):
    """state [layers, 2, n, H] or None -> (out [n,V], new state).  Biases that are None are left out."""
    tokens = tokens.long()
    if "token_clamped_to_vocab" in mistakes:
        tokens = tokens.clamp(max=lm["out_w"].shape[0] - 1)
    x = lm["emb"][tokens]
    n, H = x.shape[0], lm["lstm"][0][1].shape[1]
    rows = None if parent is None or "state_by_row" in mistakes else parent.long()  # the row of the old state every row reads
    if rows is not None and "parent_mod_128" in mistakes:
        rows = rows % 128
    if "rows_past_128_from_zero" in mistakes and n > 128:
        rows = torch.arange(n) if rows is None else rows.clone()
        rows[128:] = rows[:n - 128].clone()
    new = []
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(lm["lstm"]):
        if state is None:
            h = c = torch.zeros(n, H, dtype=x.dtype)
        else:
            h, c = state[l, 0], state[l, 1]
            if rows is not None:
                h, c = h.index_select(0, rows), c.index_select(0, rows)
        g = x @ w_ih.T
        if b_ih is not None:
            g = g + b_ih
        g = g + h @ w_hh.T
        if b_hh is not None and "bias_once" not in mistakes:
            g = g + b_hh
        i, f, gg, o = g.chunk(4, dim=1)
        if "gate_order_ifog" in mistakes:
            gg, o = o, gg
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        x = torch.sigmoid(o) * torch.tanh(c)
        new.append(torch.stack([x, c]))
    for w, b, g, beta, eps in lm["dnn"]:
        y = x @ w.T if b is None else x @ w.T + b
        x = ACTS[act](_layer_norm(y, g, beta, eps, 256 if "ln_first_256" in mistakes else None))
    logits = x @ lm["out_w"].T if lm["out_b"] is None else x @ lm["out_w"].T + lm["out_b"]
    return weight * torch.log_softmax(logits / temperature, dim=-1), torch.stack(new)


def bound(ref32, ref64, floor=1e-5):
    """The project's rule: max(4 x the fp32 restatement's own error against fp64 on the same inputs, floor)."""
    return max(4.0 * float((ref32.double() - ref64).abs().max()), floor)
