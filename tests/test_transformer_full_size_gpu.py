"""The transformer.yaml recipe at full size on the MI355X: 12 + 6 layers, d_model 512, 4 heads (head dim 128), d_ffn 2048, vocab
5000, the three-block convolution front end (64 channels); random weights, 2 x 3 s of PCM.

enc_out is compared with the fp32 host restatement (tests/transformer_host_ref.py) on the CPU.  The bound is measured in the test,
not guessed: the fp32 restatement's own error against its fp64 run at this shape, times 4 (another, equally legitimate,
summation order in every contraction, LayerNorm and softmax of 3 conv blocks and 12 layers).  DESIGN.md section 5 records the
figures of the first GPU run."""
import pytest
import torch

import transformer_host_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def asr():
    from speechbrain_amd.inference.builders import build_asr, build_transformer_modules

    mods = build_transformer_modules(vocab=5000, seed=31)
    a = build_asr(modules=mods, beam_size=4, ctc_weight=0.4, device="cuda:0")
    with torch.no_grad():  # peaked heads: EOS appears, the beams are decided by clear margins
        a.mods.seq_lin.w.weight.mul_(6.0)
        a.mods.ctc_lin.w.weight.mul_(6.0)
    return a


@pytest.fixture(scope="module")
def audio():
    from speechbrain_amd import native

    g = torch.Generator().manual_seed(5)
    pcm = (0.1 * torch.randn(2, 48000, generator=g) * 32767).round().clamp(-32768, 32767).to(torch.int16)
    lens = torch.tensor([1.0, 0.7])
    pcm[1, int(0.7 * 48000):] = 0
    return native.pcm16_to_f32(pcm.cuda()), lens.cuda()


def test_full_size_encoder_vs_host_restatement(asr, audio):
    from speechbrain_amd.inference.builders import flat_state_dict

    wav, lens = audio
    enc_mod = asr.mods.encoder
    with torch.no_grad():
        feats = enc_mod["normalize"](enc_mod["compute_features"](wav), lens)
        cnn_out = enc_mod["model"](feats)
        enc = asr.mods.transformer.encode(cnn_out, lens)
        assert torch.equal(enc, asr.encode_batch(wav, lens))
    assert cnn_out.shape[1:] == (76, 20, 64) and enc.shape == (2, 76, 512)  # 301 feature frames -> 151 -> 76
    sd = flat_state_dict(asr)
    f32, wl = feats.cpu(), lens.cpu()
    with torch.no_grad():
        ref32 = R.encode(R.conv_frontend(f32, sd, "CNN."), wl, sd, "Transformer.", 4, 12)
        sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
        ref64 = R.encode(R.conv_frontend(f32.double(), sd64, "CNN."), wl, sd64, "Transformer.", 4, 12)
        cnn32 = R.conv_frontend(f32, sd, "CNN.")
    err32 = float((ref32.double() - ref64).abs().max())
    bound = 4.0 * err32
    err = float((enc.cpu() - ref32).abs().max())
    err64 = float((enc.cpu().double() - ref64).abs().max())
    err_cnn = float((cnn_out.cpu() - cnn32).abs().max())
    print(f"transformer full size: enc_out vs fp32 restatement {err:.3e} (vs fp64 {err64:.3e}); fp32 restatement vs fp64 {err32:.3e}, "
          f"bound {bound:.3e}; front end vs fp32 restatement {err_cnn:.3e}")
    assert err <= bound


def test_full_size_beam_search_runs_and_matches_utterance_by_utterance(asr, audio):
    """Beam 4 + CTC 0.4 to completion; the batch's ids equal transcribe_batch utterance by utterance; the decoder steps are the
    head-dim-128 kernels."""
    from speechbrain_amd import native

    wav, lens = audio
    native.prof_reset()
    native.prof_enable(True)
    try:
        _, toks = asr.transcribe_batch(wav, lens)
    finally:
        native.prof_enable(False)
    rep = native.prof_report()
    assert "cross_attn_step" in rep and "self_attn_step" in rep and "rope_attention" in rep, sorted(rep)
    assert "conv_block5_mfma" in rep and "conv_block_res1x1" in rep and "conv_block5_cin1" in rep, sorted(rep)
    assert len(toks) == 2 and all(len(t) > 0 for t in toks)
    for i in range(2):  # (a single utterance's beam: 4 rows -- the plain launches, not the head-dim-64 cooperative decoder)
        _, one = asr.transcribe_batch(wav[i:i + 1], lens[i:i + 1])
        assert one[0] == toks[i], i
