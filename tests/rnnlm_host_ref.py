"""Host restatement of one RNNLM scorer step (RNNLMScorer.score after permute_mem): embedding, LSTMCell arithmetic per layer on the
state rows index_select'ed by ``parent``, the DNN blocks, the output layer and weight * log_softmax(logits / temperature).  Plain
torch in the dtype of the weights it is given."""
import torch

MISTAKES = (
    "state_by_row",     # h and c are read by row instead of through parent
    "gate_order_ifog",  # the gate chunks read as i, f, o, g
)
ACTS = {"leaky_relu": torch.nn.functional.leaky_relu, "relu": torch.relu, "gelu": torch.nn.functional.gelu, "tanh": torch.tanh}


def random_lm(gen, V, E, H, layers, blocks, D, dtype=torch.float32):
    """Weights of an RNNLM by plain names: emb [V,E]; lstm [(w_ih, w_hh, b_ih, b_hh)]; dnn [(w, b, ln_g, ln_b, eps)]; out_w, out_b."""
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=dtype)  # noqa: E731
    lstm = [(rn(4 * H, E if l == 0 else H) / (E if l == 0 else H) ** 0.5, rn(4 * H, H) / H ** 0.5, rn(4 * H) * 0.3, rn(4 * H) * 0.3)
            for l in range(layers)]
    dnn = [(rn(D, H if i == 0 else D) / (H if i == 0 else D) ** 0.5, rn(D) * 0.3, 1.0 + 0.2 * rn(D), rn(D) * 0.3, 1e-5)
           for i in range(blocks)]
    return dict(emb=rn(V, E), lstm=lstm, dnn=dnn, out_w=rn(V, D) / D ** 0.5, out_b=rn(V) * 0.3)


def cast(lm, dtype):
    c = lambda t: t.to(dtype) if torch.is_tensor(t) else t  # noqa: E731
    return dict(emb=c(lm["emb"]), lstm=[tuple(c(t) for t in l) for l in lm["lstm"]], dnn=[tuple(c(t) for t in b) for b in lm["dnn"]],
                out_w=c(lm["out_w"]), out_b=c(lm["out_b"]))


def step(lm, act, tokens, parent, state, weight=1.0, temperature=1.0, mistakes=()):
    """state [layers, 2, n, H] or None -> (out [n,V], new state)."""
    x = lm["emb"][tokens.long()]
    n, H = x.shape[0], lm["lstm"][0][1].shape[1]
    new = []
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(lm["lstm"]):
        if state is None:
            h = c = torch.zeros(n, H, dtype=x.dtype)
        else:
            h, c = state[l, 0], state[l, 1]
            if parent is not None and "state_by_row" not in mistakes:
                h, c = h.index_select(0, parent.long()), c.index_select(0, parent.long())
        g = x @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i, f, gg, o = g.chunk(4, dim=1)
        if "gate_order_ifog" in mistakes:
            gg, o = o, gg
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        x = torch.sigmoid(o) * torch.tanh(c)
        new.append(torch.stack([x, c]))
    for w, b, g, beta, eps in lm["dnn"]:
        x = ACTS[act](torch.nn.functional.layer_norm(x @ w.T + b, (w.shape[0],), g, beta, eps))
    logits = x @ lm["out_w"].T + lm["out_b"]
    return weight * torch.log_softmax(logits / temperature, dim=-1), torch.stack(new)


def bound(ref32, ref64, floor=1e-5):
    """The project's rule: max(4 x the fp32 restatement's own error against fp64 on the same inputs, floor)."""
    return max(4.0 * float((ref32.double() - ref64).abs().max()), floor)
