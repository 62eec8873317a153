"""speechbrain.nnet.RNN mirror: the LSTM of a transducer's prediction network (nnet/RNN.py:187-302).

The LSTM's parameters live in ``self.rnn`` (a ``torch.nn.LSTM`` used as a parameter holder), so checkpoints keep the
reference's state_dict keys (``rnn.weight_ih_l0``, ...).  ``forward`` runs on the device (sbk_lstm_f32) for unidirectional
layers; as a prediction network it runs inside sbk_transducer_greedy_f32 (decoders/transducer.py).  A bidirectional stack is
the recurrent part of a CRDNN encoder: there this class holds the parameters and lobes.models.CRDNN.CRDNN runs the layers
(sbk_rnn_layer_f32 through ``direction_weights``); called on its own it raises.  ``GRU``, ``RNN`` and ``LiGRU`` are not
implemented.

``GRUCell`` and ``AttentionalRNNDecoder`` (nnet/RNN.py:539-648, :755-1013) are the decoder of the CRDNN seq2seq recipes: GRU
cells with location-aware or content-based attention (csrc/attn_rnn.hip)."""
import torch

from speechbrain_amd import native


class LSTM(torch.nn.Module):
    def __init__(self, hidden_size, input_shape=None, input_size=None, num_layers=1, bias=True, dropout=0.0, re_init=True,
                 bidirectional=False):
        super().__init__()
        self.reshape = False
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = int(torch.prod(torch.tensor(input_shape[2:])).item())
        self.rnn = torch.nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, dropout=dropout,
                                 bidirectional=bidirectional, bias=bias, batch_first=True)
        if re_init:
            _rnn_init(self.rnn)

    def layer_weights(self):
        """[(w_ih [4H, in], w_hh [4H, H], b_ih or None, b_hh or None)] per layer."""
        if self.rnn.bidirectional:
            raise NotImplementedError("a bidirectional LSTM is not implemented on its own: CRDNN drives it "
                                      "(lobes.models.CRDNN.CRDNN, through direction_weights())")
        out = []
        for l in range(self.rnn.num_layers):
            g = lambda n: getattr(self.rnn, f"{n}_l{l}", None)  # noqa: E731
            out.append((g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh")))
        return out

    def direction_weights(self):
        """[[(w_ih [4H, in], w_hh [4H, H], b_ih or None, b_hh or None) per direction (forward, then ``_reverse``)] per layer]."""
        out = []
        for l in range(self.rnn.num_layers):
            dirs = []
            for sfx in ("", "_reverse")[:2 if self.rnn.bidirectional else 1]:
                g = lambda n: getattr(self.rnn, f"{n}_l{l}{sfx}", None)  # noqa: E731
                dirs.append((g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh")))
            out.append(dirs)
        return out

    def forward(self, x, hx=None, lengths=None):
        """x [B,T,in] -> (output [B,T,H], (h [L,B,H], c [L,B,H]))."""
        if lengths is not None:
            raise NotImplementedError("packed LSTM sequences (lengths) are not implemented")
        if self.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        return native.lstm(x, self.layer_weights(), hx)


def _rnn_init(module):
    """nnet/RNN.py rnn_init: orthogonal recurrent weights (the values are overwritten by any checkpoint)."""
    for name, param in module.named_parameters():
        if "weight_hh" in name or ".u.weight" in name:
            torch.nn.init.orthogonal_(param)


class _NotImplementedRNN(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} is not implemented (transducer prediction networks use LSTM)")


class GRU(_NotImplementedRNN):
    pass


class RNN(_NotImplementedRNN):
    pass


class LiGRU(_NotImplementedRNN):
    pass


class GRUCell(torch.nn.Module):
    """nnet/RNN.py:539-648: a stack of torch.nn.GRUCell parameter holders (keys ``rnn_cells.{i}.weight_ih`` ...), one time step
    per call.  A layer is two contractions (x . W_ih^T, h . W_hh^T) and the cell update sbk_gru_cell_f32; dropout between the
    layers is a training feature and is not applied."""

    def __init__(self, hidden_size, input_shape=None, input_size=None, num_layers=1, bias=True, dropout=0.0, re_init=True):
        super().__init__()
        self.hidden_size, self.num_layers = hidden_size, num_layers
        if input_shape is None and input_size is None:
            raise ValueError("Expected one of input_shape or input_size.")
        if input_size is None:
            if len(input_shape) > 3:
                self.reshape = True
            input_size = int(torch.prod(torch.tensor(input_shape[1:])).item())
        cells = [torch.nn.GRUCell(input_size=input_size, hidden_size=hidden_size, bias=bias)]
        cells += [torch.nn.GRUCell(input_size=hidden_size, hidden_size=hidden_size, bias=bias) for _ in range(num_layers - 1)]
        self.rnn_cells = torch.nn.ModuleList(cells)
        self.dropout_layers = torch.nn.ModuleList([torch.nn.Dropout(p=dropout) for _ in range(num_layers - 1)])
        if re_init:
            _rnn_init(self.rnn_cells)

    def layer_weights(self):
        """[(w_ih [3H, in], w_hh [3H, H], b_ih or None, b_hh or None)] per layer."""
        return [(c.weight_ih, c.weight_hh, getattr(c, "bias_ih", None), getattr(c, "bias_hh", None)) for c in self.rnn_cells]

    @torch.no_grad()
    def forward(self, x, hx=None):
        """x [B,in], hx [L,B,H] or None (zeros) -> (h of the top layer [B,H], hidden [L,B,H])."""
        h, hidden = x.contiguous(), []
        with native.precision_scope("fp32"):
            for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self.layer_weights()):
                gi = native.gemm_nt(h, w_ih)
                gh = native.gemm_nt(hx[l].contiguous(), w_hh) if hx is not None else torch.zeros_like(gi)
                h = native.gru_cell(gi, gh, b_ih, b_hh, hx[l].contiguous() if hx is not None else None)
                hidden.append(h)
        return h, torch.stack(hidden, dim=0)


class AttentionalRNNDecoder(torch.nn.Module):
    """nnet/RNN.py:755-1013 for ``rnn_type="gru"`` with location-aware or content-based attention: the decoder of the CRDNN
    seq2seq recipes.  Constructor, state-dict keys (``proj``, ``attn.*``, ``rnn.*``), ``forward_step`` and ``forward`` as the
    reference; ``forward`` (teacher forcing) is one sbk_attn_rnn_decode_f32 call, S2SRNNGreedySearcher runs the same step inside
    sbk_attn_rnn_greedy_f32.  Dropout is a training feature and is not applied."""

    def __init__(self, rnn_type, attn_type, hidden_size, attn_dim, num_layers, enc_dim, input_size, nonlinearity="relu",
                 re_init=True, normalization="batchnorm", scaling=1.0, channels=None, kernel_size=None, bias=True, dropout=0.0):
        super().__init__()
        from speechbrain_amd.nnet.attention import ContentBasedAttention, KeyValueAttention, LocationAwareAttention

        self.rnn_type, self.attn_type = rnn_type.lower(), attn_type.lower()
        self.hidden_size, self.attn_dim, self.num_layers = hidden_size, attn_dim, num_layers
        self.scaling, self.bias, self.dropout = scaling, bias, dropout
        self.normalization, self.re_init, self.nonlinearity = normalization, re_init, nonlinearity
        self.channels, self.kernel_size = channels, kernel_size
        self.proj = torch.nn.Linear(hidden_size + attn_dim, hidden_size)
        if self.attn_type == "content":
            self.attn = ContentBasedAttention(enc_dim=enc_dim, dec_dim=hidden_size, attn_dim=attn_dim, output_dim=attn_dim,
                                              scaling=scaling)
        elif self.attn_type == "location":
            self.attn = LocationAwareAttention(enc_dim=enc_dim, dec_dim=hidden_size, attn_dim=attn_dim, output_dim=attn_dim,
                                               conv_channels=channels, kernel_size=kernel_size, scaling=scaling)
        elif self.attn_type == "keyvalue":
            self.attn = KeyValueAttention(enc_dim=enc_dim, dec_dim=hidden_size, attn_dim=attn_dim, output_dim=attn_dim)
        else:
            raise ValueError(f"{self.attn_type} is not implemented.")
        self.drop = torch.nn.Dropout(p=dropout)
        if self.rnn_type in ("lstm", "rnn"):
            raise NotImplementedError(f"AttentionalRNNDecoder: rnn_type {self.rnn_type!r} is not implemented (the CRDNN seq2seq "
                                      "recipes decode with 'gru')")
        if self.rnn_type != "gru":
            raise ValueError(f"{self.rnn_type} not implemented.")
        self.rnn = GRUCell(input_size=input_size + attn_dim, hidden_size=hidden_size, num_layers=num_layers, bias=bias,
                           dropout=0 if num_layers == 1 else dropout, re_init=re_init)
        self._prepared = native.Derived()

    def prepared(self, device, emb=None, fc=None, derived=None):
        """The kernel's weight table on ``device`` (native.AttnRNNPrepared), rebuilt when a parameter moves or is updated in
        place; ``emb`` / ``fc``: the searcher's embedding table and output (weight, bias), held in the searcher's ``derived``."""
        params = list(self.parameters()) + [t for t in ((emb,) + tuple(fc or ())) if t is not None]
        d = lambda t: None if t is None else t.detach().to(device)  # noqa: E731

        def build():
            layers = [tuple(d(t) for t in layer) for layer in self.rnn.layer_weights()]
            attn = {k: d(v) for k, v in self.attn.kernel_weights().items()}
            return native.AttnRNNPrepared(layers, attn, d(self.proj.weight), d(self.proj.bias), self.scaling, emb=d(emb),
                                          fc_w=d(fc[0]) if fc else None, fc_b=d(fc[1]) if fc else None)

        return (derived or self._prepared).get(params, build, device=device, extra=(device, float(self.scaling)))

    @torch.no_grad()
    def forward_step(self, inp, hs, c, enc_states, enc_len):
        """inp [B,in], hs [L,B,H] or None, c [B,attn_dim] -> (dec_out [B,H], hs, c, attn [B,T]); the attention's memory
        (``self.attn``) is the reference's."""
        cell_out, hs = self.rnn(torch.cat([inp, c], dim=-1), hs)
        c, w = self.attn(enc_states, enc_len, cell_out)
        with native.precision_scope("fp32"):
            dec_out = native.gemm_nt(torch.cat([c, cell_out], dim=1), self.proj.weight, self.proj.bias)
        return dec_out, hs, c, w

    @torch.no_grad()
    def forward(self, inp_tensor, enc_states, wav_len):
        """inp_tensor [B,L,in] (embedded tokens), enc_states [B,T,E], wav_len [B] relative -> (outputs [B,L,H], attn [B,L,T])."""
        enc = enc_states.detach().float().contiguous()
        enc_len = torch.round(enc.shape[1] * wav_len).to(device=enc.device, dtype=torch.int32).contiguous()
        self.attn.reset()
        with native.precision_scope("fp32"):
            outputs, attn, _, _ = native.attn_rnn_decode(self.prepared(enc.device), inp_tensor.detach().float().contiguous(), enc,
                                                         enc_len)
        return outputs, attn
