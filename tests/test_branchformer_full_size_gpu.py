"""Branchformer encoder at the recipe's widths on the MI355X (gpu only): d 512, 8 heads, csgu_linear_units 3072, kernel 31 --
branchformer_large.yaml's layer -- at a small extent (2 layers, B = 2, T' = 70, one utterance at 0.6 of the length), random
weights, against tests/branchformer_host_ref.py in fp64 (test_branchformer_model.py pins that restatement to the reference's
own outputs).  Bound: 2e-4 absolute, DESIGN section 3's full-size encoder bound (test_encoder_vs_oracle)."""
import pytest
import torch

import branchformer_host_ref as R

pytestmark = pytest.mark.gpu

D, H, LAYERS, CSGU, KSIZE, FEAT = 512, 8, 2, 3072, 31, 640
_REF = {}


def _model_and_reference():
    """The model (CPU), its inputs and the fp64 encoder outputs -- computed once, shared by the two tests, never modified."""
    if not _REF:
        from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR

        torch.manual_seed(31)
        tr = TransformerASR(input_size=FEAT, tgt_vocab=100, d_model=D, nhead=H, num_encoder_layers=LAYERS, num_decoder_layers=0,
                            dropout=0.1, activation=torch.nn.GELU, branchformer_activation=torch.nn.GELU,
                            encoder_module="branchformer", csgu_linear_units=CSGU, kernel_size=KSIZE,
                            attention_type="RelPosMHAXL", normalize_before=True, causal=False).eval()
        g = torch.Generator().manual_seed(32)
        with torch.no_grad():
            for n, p in tr.named_parameters():
                if n.endswith("csgu.conv.conv.weight"):  # (drawn with std 1e-6 by the constructor: it would not filter)
                    p.copy_(0.15 * torch.randn(p.shape, generator=g))
                elif p.dim() == 1 or "norm" in n:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        sd64 = {"Transformer." + k: (v.double() if v.is_floating_point() else v) for k, v in tr.state_dict().items()}
        feats = [torch.randn(2, 70, FEAT, generator=g), torch.randn(1, 33, FEAT, generator=g)]
        lens = [torch.tensor([1.0, 0.6]), torch.tensor([1.0])]
        refs = [R.encode(f.double(), l, sd64, D, H, LAYERS, "Transformer.") for f, l in zip(feats, lens)]
        _REF.update(tr=tr, feats=feats, lens=lens, refs=refs)
    return _REF["tr"], _REF["feats"], _REF["lens"], _REF["refs"]


def _cuda(tr):
    from speechbrain_amd import native

    import emu_utils

    emu_utils.detach()
    native.load()
    return tr.to("cuda:0")


def test_branchformer_encode_vs_fp64_restatement():
    tr, feats, lens, refs = _model_and_reference()
    tr = _cuda(tr)
    with torch.no_grad():
        enc = tr.encode(feats[0].cuda(), lens[0].cuda())
    assert enc.shape == refs[0].shape
    err = float((enc.cpu().double() - refs[0]).abs().max())
    print(f"branchformer encode, d {D} csgu {CSGU} k {KSIZE}: max|d| vs fp64 = {err:.3e}")
    assert err <= 2e-4


def test_branchformer_encode_group_vs_fp64_restatement():
    """Two differently padded batches through the grouped pass: the row-wise launches once over all 173 rows, attention and the
    CSGU per batch (T' = 70 and T' = 33, which is 17 frames more than the halo)."""
    tr, feats, lens, refs = _model_and_reference()
    tr = _cuda(tr)
    with torch.no_grad():
        encs = tr.encode_group([f.cuda() for f in feats], [l.cuda() for l in lens])
    for enc, ref in zip(encs, refs):
        assert enc.shape == ref.shape
        err = float((enc.cpu().double() - ref).abs().max())
        print(f"branchformer encode_group, T' {ref.shape[1]}: max|d| vs fp64 = {err:.3e}")
        assert err <= 2e-4
