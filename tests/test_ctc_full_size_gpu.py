"""EncoderASR at the LibriSpeech CTC recipe's shape (conformer_large.yaml: d 256, 4 heads, d_ffn 1 024, 18 layers, GELU,
31 characters) on the MI355X, 32 x 10 s, seeded weights: the encoder + CTC head against the oracle, the device greedy
decode against a host arg-max collapse, and the device beam search (beam 100 at the recipe's test settings) against the
host restatement of CTCBeamSearcher (tests/ctc_host_ref.py) on the same log-probabilities."""
import pytest
import torch

import ctc_host_ref
from oracle import sb_oracle as O

pytestmark = pytest.mark.gpu

CFG = dict(d_model=256, nhead=4, d_ffn=1024, n_enc=18, n_dec=0, n_fft=512, win_length=32)
CHARS = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "-", "."]
MARGIN = 1e-4


def _asr(decoding, scale=8.0, **beam):
    import functools

    from speechbrain_amd import native
    from speechbrain_amd.dataio.encoder import CTCTextEncoder
    from speechbrain_amd.decoders.ctc import CTCBeamSearcher, ctc_greedy_decode
    from speechbrain_amd.inference.ASR import EncoderASR
    from speechbrain_amd.inference.builders import build_modules
    from speechbrain_amd.lobes.models.transformer.TransformerASR import EncoderWrapper
    from speechbrain_amd.nnet.containers import LengthsCapableSequential

    import emu_utils

    emu_utils.detach()
    native.load()
    m = build_modules(CFG, vocab=len(CHARS), seed=21)
    with torch.no_grad():
        m["ctc_lin"].w.weight.mul_(scale)
    encoder = LengthsCapableSequential(compute_features=m["compute_features"], normalize=m["normalize"], CNN=m["CNN"],
                                       transformer_encoder=EncoderWrapper(m["Transformer"]), ctc_lin=m["ctc_lin"],
                                       log_softmax=torch.nn.LogSoftmax(dim=-1))
    tok = CTCTextEncoder()
    tok.lab2ind, tok.ind2lab, tok.blank_label = {c: i for i, c in enumerate(CHARS)}, dict(enumerate(CHARS)), "<blank>"
    fn = functools.partial(ctc_greedy_decode, blank_id=0) if decoding == "greedy" else CTCBeamSearcher
    hp = {"tokenizer": tok, "decoding_function": fn, "test_beam_search": dict(blank_index=0, **beam)}
    return EncoderASR(modules={"encoder": encoder}, hparams=hp, run_opts={"device": "cuda:0"}), m


def _batch(B=32, sec=10.0):
    n = int(sec * 16000)
    wav = 0.1 * torch.randn(B, n, generator=torch.Generator().manual_seed(77))
    lens = torch.linspace(0.6, 1.0, B)
    for i in range(B):
        wav[i, int(lens[i] * n):] = 0
    return wav, lens


def test_ctc_large_encoder_head_vs_oracle_and_greedy_exact():
    asr, m = _asr("greedy")
    wav, lens = _batch()
    logp = asr.encode_batch(wav, lens)
    assert logp.shape[-1] == 31
    # encoder + head against the oracle on full-length utterances (EncoderWrapper runs the encoder unmasked, as the
    # reference's does inside a LengthsCapableSequential)
    sd = {}
    for pfx, mod in (("CNN.", m["CNN"]), ("Transformer.", m["Transformer"])):
        sd.update({pfx + k: v.detach().cpu() for k, v in mod.state_dict().items()})
    fc = O.FbankCfg(n_fft=CFG["n_fft"], n_mels=80, win_length_ms=CFG["win_length"])
    mc = O.ModelCfg(d_model=256, nhead=4, num_encoder_layers=18, num_decoder_layers=0, d_ffn=1024, vocab=31)
    full = torch.ones(2)
    enc = O.encode_batch(wav[-2:], full, sd, fc, mc, torch.zeros(80), torch.ones(80))
    w, b = m["ctc_lin"].w.weight.detach().cpu(), m["ctc_lin"].w.bias.detach().cpu()
    ref = torch.log_softmax(enc @ w.T + b, dim=-1)
    got = asr.encode_batch(wav[-2:], full).cpu()
    assert float((got - ref).abs().max()) <= 2e-4
    # greedy: bit-exact against a host arg-max collapse of the same device log-probabilities
    words, tokens = asr.transcribe_batch(wav, lens)
    x, T = logp.cpu(), logp.shape[1]
    for i in range(len(tokens)):
        path = x[i, :int(torch.round(lens[i] * T))].argmax(-1).tolist()
        assert tokens[i] == [t for j, t in enumerate(path) if t != 0 and (j == 0 or path[j - 1] != t)], i
    assert sum(len(t) for t in tokens) > 0


@pytest.mark.parametrize("scale,prune_history", [(8.0, False), (1.0, True)])
def test_ctc_large_beam100_vs_host_restatement(scale, prune_history):
    beam = dict(beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2, prune_history=prune_history, topk=1)
    asr, _ = _asr("beam", scale=scale, **beam)
    wav, lens = _batch()
    logp = asr.encode_batch(wav, lens)
    words, hyps = asr.transcribe_batch(wav, lens)
    ref = ctc_host_ref.beam_search(logp.cpu(), lens, blank=0, vocab=CHARS, **beam)
    checked = 0
    for i, (h, r) in enumerate(zip(hyps, ref)):
        assert abs(float(h[0].score) - float(r[0].score)) <= MARGIN, i
        if h[0].text == r[0].text:
            checked += 1
            assert words[i] == r[0].text
        else:  # a different best hypothesis is only allowed on a tie within the margin
            assert abs(float(h[0].score) - float(r[0].score)) <= MARGIN, (i, h[0].text, r[0].text)
    assert checked >= 0.8 * len(hyps)
