"""The GRU attention decoder at the recipe's shape (train_BPE_1000.yaml: embedding 128, hidden 1024, attention 1024 with 10 channels
and kernel 100, encoder 512, 1000 tokens; seeded random weights) on the MI355X against the fp64 host restatement
(tests/attn_rnn_host_ref.py): B 2, T 64, 16 teacher-forced steps and 16 greedy steps.

Bound (the project's rule): max(4 x the fp32 host restatement's error against fp64 on the same inputs, 1e-5) for dec_out, the
attention and the logits.  Greedy ids follow the margin rule of tests/test_full_size_gpu.py: the fp64 restatement, teacher forced on
the device's own tokens, gives every step's logits; wherever its margin between the best two exceeds the measured logit error of
that row and step, the device's token must be its arg-max.  SEED is chosen so that every step of both utterances passes the margin
on the CPU emulator (the share asserted is 90 %)."""
import pytest
import torch

import attn_rnn_host_ref as R
from speechbrain_amd import native
from speechbrain_amd.decoders import S2SRNNGreedySearcher
from speechbrain_amd.nnet.embedding import Embedding
from speechbrain_amd.nnet.linear import Linear
from speechbrain_amd.nnet.RNN import AttentionalRNNDecoder

SEED = 5
EMB, HID, ATT, ENC, VOCAB, CH, KS = 128, 1024, 1024, 512, 1000, 10, 100
B, T, STEPS = 2, 64, 16
EOS = 7


def build():
    torch.manual_seed(SEED)
    emb = Embedding(num_embeddings=VOCAB, embedding_dim=EMB)
    dec = AttentionalRNNDecoder(rnn_type="gru", attn_type="location", hidden_size=HID, attn_dim=ATT, num_layers=1, enc_dim=ENC,
                                input_size=EMB, scaling=1.0, channels=CH, kernel_size=KS, re_init=True, dropout=0.15)
    lin = Linear(input_size=HID, n_neurons=VOCAB)
    with torch.no_grad():
        dec.attn.mlp_attn.weight.mul_(8.0)  # an attention that looks somewhere, an output layer that decides
        dec.attn.conv_loc.weight.mul_(8.0)
        lin.w.weight.mul_(8.0)
        lin.w.bias[EOS] -= 50.0  # (no utterance ends inside the 16 steps)
    gen = torch.Generator().manual_seed(SEED + 1)
    enc = torch.randn(B, T, ENC, generator=gen)
    wav_len = torch.tensor([1.0, 0.75])
    tokens = torch.randint(0, VOCAB, (B, STEPS), generator=gen)
    searcher = S2SRNNGreedySearcher(embedding=emb, decoder=dec, linear=lin, bos_index=0, eos_index=EOS, min_decode_ratio=0.0,
                                    max_decode_ratio=STEPS / T).eval()
    return emb, dec, lin, searcher, enc, wav_len, tokens


def host(dec, emb, lin, tokens, enc, enc_len, dtype):
    """(dec_out, attn, logits) of the host restatement, teacher forced on ``tokens`` [B,L] (the inputs: bos, then tokens[:, :-1])."""
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    inp = torch.cat([torch.zeros(B, 1, dtype=torch.long), tokens[:, :-1]], dim=1)
    out, attn, _, _ = R.HostDecoder(sd, 1.0, dtype).forward(emb.Embedding.weight.detach().cpu()[inp], enc, enc_len)
    return out, attn, out @ lin.w.weight.detach().cpu().to(dtype).T + lin.w.bias.detach().cpu().to(dtype)


def run(nat, dev):
    emb, dec, lin, searcher, enc, wav_len, tokens = build()
    enc_len = torch.round(T * wav_len).int()
    r32, r64 = host(dec, emb, lin, tokens, enc, enc_len, torch.float32), host(dec, emb, lin, tokens, enc, enc_len, torch.float64)
    searcher.to(dev)

    def device_forward(toks):
        inp = torch.cat([torch.zeros(B, 1, dtype=torch.long), toks[:, :-1]], dim=1).to(dev)
        out, attn = dec(emb.Embedding.weight.detach()[inp], enc.to(dev), wav_len.to(dev))
        with nat.precision_scope("fp32"):
            return out.cpu(), attn.cpu(), nat.gemm_nt(out.contiguous(), lin.w.weight, lin.w.bias).cpu()

    # 16 teacher-forced steps
    for what, g, a32, a64 in zip(("dec_out", "attn", "logits"), device_forward(tokens), r32, r64):
        err, bound = float((g.double() - a64).abs().max()), R.bound(a32, a64)
        print(f"s2srnn full size {what}: max|d| {err:.3e} (bound {bound:.1e}, fp32 host {float((a32.double() - a64).abs().max()):.3e})")
        assert g.shape == a64.shape and err <= bound, what
    # 16 greedy steps
    hyps, lengths, scores, _ = searcher(enc.to(dev), wav_len.to(dev))
    got = torch.tensor(hyps)
    assert got.shape == (B, STEPS) and bool((lengths == 1.0).all())
    _, _, lg64 = host(dec, emb, lin, got, enc, enc_len, torch.float64)
    _, _, lg_dev = device_forward(got)
    logit_err = (lg_dev.double() - lg64).abs().amax(dim=-1)  # [B,STEPS]
    top2 = lg64.topk(2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > logit_err
    share = float(decided.float().mean())
    print(f"s2srnn full size greedy: {int(decided.sum())} of {decided.numel()} steps pass the margin (smallest margin "
          f"{float((top2[..., 0] - top2[..., 1]).min()):.3e}, largest logit error {float(logit_err.max()):.3e})")
    assert share >= 0.9
    assert torch.equal(got[decided], lg64.argmax(dim=-1)[decided])
    sc64 = torch.log_softmax(lg64, dim=-1).gather(2, got[..., None])[..., 0]
    assert float((scores[:, 0].double() - sc64).abs().max()) <= max(4.0 * float(logit_err.max()), 1e-5)


@pytest.mark.gpu
def test_recipe_shape_teacher_forced_and_greedy_against_fp64():
    native.load()
    run(native, torch.device("cuda:0"))
