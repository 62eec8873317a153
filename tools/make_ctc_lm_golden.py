"""Write tests/golden/ctc_decode_lm.npz and the model directory tests/golden/pretrained_ctc_lm_tiny/ with the REFERENCE's own
CTCBeamSearcher and KenlmScorer (decoders/ctc.py, integrations/decoders/kenlm_scorer.py, both unmodified).

Runs only where the reference checkout is available (SB_REFERENCE, default /root/reference).  ``kenlm`` and ``pygtrie`` are
served by the stand-ins of tools/ref_standins/ (our own ARPA back-off scorer and prefix set; the known answers they are
pinned to are in tests/test_ctc_lm_loader.py) -- agreement with the real kenlm library has not been checked.

    python tools/make_ctc_lm_golden.py

Random posteriors spell no words, so each case's posteriors follow a target sentence of lexicon and non-lexicon words (a
peaked path with repeats and blanks, plus noise): beams hold in-vocabulary words, out-of-vocabulary words and partial words
longer than six characters.  Every case stores its log-probabilities, lengths, the ARPA text (data) and the reference's
hypotheses: text, score (CTC), lm_score (fused), text_frames and the adjacent lm_score gaps.

The model directory re-uses the checkpoints of tests/golden/pretrained_ctc_tiny (copied) under a hyperparams.yaml whose
test_beam_search names an ARPA file; the expected words are the reference searcher's on the reference encoder's recorded
log-probabilities (pretrained_ctc_tiny_expected.npz), which is what its EncoderASR.transcribe_batch returns.
"""
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("SB_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_stubs"))
sys.path.insert(0, os.path.join(HERE, "ref_standins"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.arpa_synth import arpa_text  # noqa: E402
from tools.make_ctc_golden import CHARS, CTC_YAML, SPM  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-4

CHAR_LEXICON = ["the", "cat", "sat", "on", "a", "mat", "dog", "ran", "to", "cab", "bad", "abandonment"]
CHAR_SENTENCES = ["the cat sat on mat", "a zzq dog  ran to", "abandonment xylophones"]  # (two spaces: an empty next word)
SPM_LEXICON = ["a", "ab", "abc", "b", "c", "cab", "bad", "dab", "cad", "abba", "bcd", "abcabcabc"]
SPM_SENTENCES = [["▁a", "▁ab", "▁c", "ab", "▁b", "a", "d", "▁abc", "ab", "c", "ab", "c"],
                 ["▁", "d", "d", "▁c", "a", "d", "▁abc", "d", "▁b", "c", "d"],
                 ["▁abc", "ab", "ca", "bc", "ab", "▁a", "▁b", "a", "b"]]


def spelled_posteriors(vocab, sentences, T, V, seed, peak, noise):
    """[B,T,V] log-probabilities whose best path spells ``sentences`` (strings of characters or lists of pieces)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(len(sentences), T, V, generator=g) * noise
    for b, sent in enumerate(sentences):
        frames, prev = [], None
        for tok in sent:
            v = vocab.index(tok)
            if v == prev:
                frames.append(0)
            frames += [v] * (1 + int(torch.randint(0, 2, (1,), generator=g)))
            if int(torch.randint(0, 3, (1,), generator=g)) == 0:
                frames.append(0)
            prev = v
        frames = (frames + [0] * T)[:T]
        z[b, torch.arange(T), torch.tensor(frames)] += peak
    return torch.log_softmax(z, dim=-1)


def cases():
    """(name, vocab, log_probs, wav_lens, arpa key, searcher kwargs)"""
    lens3 = torch.tensor([1.0, 0.8, 0.55])
    out = []

    def char(name, order, seed, V=31, lens=lens3, **kw):
        x = spelled_posteriors(CHARS, CHAR_SENTENCES, 40, V, seed, peak=5.0, noise=1.2)
        out.append((name, CHARS, x, lens, f"char{order}", kw))

    def spm(name, order, seed, **kw):
        x = spelled_posteriors(SPM, SPM_SENTENCES, 40, len(SPM), seed, peak=4.0, noise=1.2)
        out.append((name, SPM, x, lens3, f"spm{order}", kw))

    char("char_o1_b10_k3", 1, 11, beam_size=10, topk=3, prune_history=False)
    char("char_o2_b100_k3", 2, 12, beam_size=100, topk=3, prune_history=False, token_prune_min_logp=-3.0)
    char("char_o3_b10_ph1_k3", 3, 13, beam_size=10, topk=3, prune_history=True)
    char("char_o3_b10_ph0_k3", 3, 13, beam_size=10, topk=3, prune_history=False)
    char("char_o5_b100_defaults", 5, 14, token_prune_min_logp=-3.0)
    char("char_o3_b1", 3, 15, beam_size=1)
    char("char_o2_no_boundary", 2, 16, beam_size=10, topk=3, prune_history=False, score_boundary=False)
    char("char_o3_unigrams", 3, 17, beam_size=10, topk=3, prune_history=False, unigrams=["the", "cat", "dog", "xylophones"])
    char("char_o3_alpha0", 3, 18, beam_size=10, topk=3, prune_history=False, alpha=0.0, beta=0.7)
    char("char_o2_wide_v", 2, 19, V=34, beam_size=10, topk=3, prune_history=False)
    char("char_o3_len0", 3, 20, lens=torch.tensor([1.0, 0.0, 0.55]), beam_size=10, topk=3, prune_history=False)
    char("char_o5_b10_ph1_k3", 5, 21, beam_size=10, topk=3, prune_history=True, unk_score_offset=-4.0)
    spm("spm_o2_b10_k3", 2, 31, beam_size=10, topk=3, prune_history=False)
    spm("spm_o3_b100_ph1_k3", 3, 32, beam_size=100, topk=3, prune_history=True, token_prune_min_logp=-3.0)
    spm("spm_o5_b10_k3", 5, 33, beam_size=10, topk=3, prune_history=False, beam_prune_logp=-14.0)
    spm("spm_o1_b1", 1, 34, beam_size=1)
    return out


def arpas():
    texts = {}
    for order in (1, 2, 3, 5):
        texts[f"char{order}"] = arpa_text(CHAR_LEXICON, order, seed=100 + order, two_field=("on",))
        texts[f"spm{order}"] = arpa_text(SPM_LEXICON, order, seed=200 + order, two_field=("cad",))
    return texts


def record(hyps):
    res = []
    for hl in hyps:
        fused = [float(h.lm_score) for h in hl]
        res.append(dict(text=[h.text for h in hl], score=[float(h.score) for h in hl], lm_score=fused,
                        text_frames=[[[w, list(f)] for w, f in h.text_frames] for h in hl],
                        gaps=[fused[k] - fused[k + 1] for k in range(len(fused) - 1)]))
        assert all(h.last_lm_state is None for h in hl)
    return res


def main():
    from speechbrain.decoders.ctc import CTCBeamSearcher

    texts = arpas()
    tmp = tempfile.mkdtemp()
    paths = {}
    for key, text in texts.items():
        paths[key] = os.path.join(tmp, key + ".arpa")
        with open(paths[key], "w", encoding="utf-8") as f:
            f.write(text)
    out, meta = {}, []
    total = decided = 0
    for i, (name, vocab, x, lens, key, kw) in enumerate(cases()):
        s = CTCBeamSearcher(blank_index=0, vocab_list=vocab, space_token=" ", kenlm_model_path=paths[key], **kw)
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = record(s(x, lens))
        for r in res:
            n = len(r["text"])
            total += n
            decided += next((k for k, gap in enumerate(r["gaps"]) if gap <= MARGIN), n)
        out[f"case{i}_x"] = x.numpy()
        out[f"case{i}_lens"] = lens.numpy()
        meta.append(dict(name=name, vocab=vocab, arpa=key, kwargs=kw, result=res))
        print(f"  {name:26s} {[(r['text'] or ['-'])[0][:28] for r in res]}")
    assert decided >= 0.8 * total, (decided, total)
    print(f"  {decided} of {total} hypotheses ranked by more than {MARGIN}")
    interface = model_directory()
    out["meta"] = np.array(json.dumps(dict(cases=meta, arpa=texts, interface=interface)))
    np.savez_compressed(os.path.join(OUT, "ctc_decode_lm.npz"), **out)
    print("wrote", os.path.join(OUT, "ctc_decode_lm.npz"))
    shutil.rmtree(tmp)


LM_DECODING = """kenlm_model_path: tests/golden/pretrained_ctc_lm_tiny/lm.arpa

test_beam_search:
    blank_index: !ref <blank_index>
    beam_size: 100
    beam_prune_logp: -12.0
    token_prune_min_logp: -1.2
    prune_history: True
    kenlm_model_path: !ref <kenlm_model_path>
    alpha: 0.5
    beta: 1.5

decoding_function: !name:speechbrain.decoders.ctc.CTCBeamSearcher"""
LM_SETTINGS = dict(beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2, prune_history=True, alpha=0.5, beta=1.5)


def model_directory():
    from speechbrain.decoders.ctc import CTCBeamSearcher

    src, dst = os.path.join(OUT, "pretrained_ctc_tiny"), os.path.join(OUT, "pretrained_ctc_lm_tiny")
    os.makedirs(dst, exist_ok=True)
    for name in ("model.ckpt", "normalize.ckpt", "tokenizer.ckpt"):
        shutil.copyfile(os.path.join(src, name), os.path.join(dst, name))
    with open(os.path.join(dst, "hyperparams.yaml"), "w", encoding="utf-8") as f:
        f.write(CTC_YAML.replace("tools/make_ctc_golden.py", "tools/make_ctc_lm_golden.py").replace("%DECODING%", LM_DECODING))
    exp = np.load(os.path.join(OUT, "pretrained_ctc_tiny_expected.npz"))
    # a lexicon that knows half of what the model says without a language model, so that fusion has something to prefer
    said = sorted({w for words in exp["beam_words"] for w in str(words).split()})
    lexicon = said[::2] + ["the", "a", "to"]
    arpa = os.path.join(dst, "lm.arpa")
    with open(arpa, "w", encoding="utf-8") as f:
        f.write(arpa_text(lexicon, 3, seed=300))
    from speechbrain.dataio.encoder import CTCTextEncoder

    tok = CTCTextEncoder()  # the label order of tokenizer.ckpt
    tok.load(os.path.join(dst, "tokenizer.ckpt"))
    vocab = [tok.ind2lab[i] for i in range(len(tok.ind2lab))]
    s = CTCBeamSearcher(blank_index=0, vocab_list=vocab, kenlm_model_path=arpa, **LM_SETTINGS)
    hyps = s(torch.from_numpy(exp["logp"]), torch.from_numpy(exp["lens"]))
    words = [h[0].text for h in hyps]
    print("  interface:", words, "without the model:", [str(w) for w in exp["beam_words"]])
    return dict(words=words, lm_score=[float(h[0].lm_score) for h in hyps], score=[float(h[0].score) for h in hyps])


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
