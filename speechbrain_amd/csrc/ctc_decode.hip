// CTC decoding on the device: ctc_greedy_decode (decoders/ctc.py:335-380) and CTCBeamSearcher, without a language model
// and with an ARPA n-gram model fused in (decoders/ctc.py:782-935,1070-1153,1203-1296,1298-1487).  One workgroup per
// utterance; the beam search runs every frame of an utterance in ONE launch with its beam in LDS.  The semantics
// reproduced here are listed in DESIGN.md section 5.
#include <math.h>

#include "argmax.h"
#include "common.h"
#include "device.h"

namespace sbk {

namespace {

constexpr int kCtcThreads = 256;       // one thread per beam slot / candidate
constexpr int kCtcBeamMax = kCtcThreads;
constexpr uint32_t kHashMod = 2147483647u;  // 2^31 - 1: two polynomial hashes of a string's characters

__device__ __forceinline__ uint32_t hmul(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) % kHashMod); }
__device__ __forceinline__ uint32_t hadd(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;  // (a, b < 2^31: no wrap)
  return s >= kHashMod ? s - kHashMod : s;
}

// ---------------------------------------------------------------------------------------------------------- greedy
// x [B,T,V]; len_b = int(round(fp32(rel[b] * T))) (half to even, as torch.round); tokens [B,T] (compacted), count [B].
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ x, const float* __restrict__ rel,
                                                         int32_t* tokens, int32_t* count, int T, int V, int blank) {
  __shared__ int s_scan[kCtcThreads];
  __shared__ int s_carry[2];  // running output count, arg-max of the previous chunk's last frame
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float lf = rel ? rel[b] * (float)T : (float)T;
  lf = rintf(lf);
  const int len = isnan(lf) ? 0 : (int)fminf(fmaxf(lf, 0.0f), (float)T);
  const float* xb = x + (size_t)b * T * V;
  int32_t* ob = tokens + (size_t)b * T;
  // phase 1: the arg-max of every frame (one wave per frame) into the output row
  for (int t = wave; t < len; t += kCtcThreads / 64) {
    const float* row = xb + (size_t)t * V;
    float bv = NAN;
    int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float w = row[v];
      if (bi == 0x7fffffff || arg_better(w, v, bv, bi)) bv = w, bi = v;
    }
    for (int m = 32; m >= 1; m >>= 1) {
      const float w = shfl_xor(bv, m);
      const int j = shfl_xor(bi, m);
      if (j != 0x7fffffff && (bi == 0x7fffffff || arg_better(w, j, bv, bi))) bv = w, bi = j;
    }
    if (lane == 0) ob[t] = bi;
  }
  if (tid == 0) s_carry[0] = 0, s_carry[1] = -1;
  __syncthreads();
  // phase 2: collapse repeats, drop blanks, compact in place (a write lands at or before the frame it came from)
  for (int t0 = 0; t0 < len; t0 += kCtcThreads) {
    const int t = t0 + tid;
    const int a = t < len ? ob[t] : -1;
    const int prev = t == t0 ? s_carry[1] : (t - 1 < len ? ob[t - 1] : -1);
    const int keep = (t < len && a != blank && a != prev) ? 1 : 0;
    s_scan[tid] = keep;
    __syncthreads();
    for (int off = 1; off < kCtcThreads; off <<= 1) {  // inclusive scan
      const int add = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    const int base = s_carry[0];
    const int last = min(len, t0 + kCtcThreads) - 1 - t0;
    const int last_tok = ob[t0 + last];
    __syncthreads();  // every read of this chunk precedes every write
    if (keep) ob[base + s_scan[tid] - 1] = a;
    __syncthreads();
    if (tid == 0) s_carry[0] = base + s_scan[kCtcThreads - 1], s_carry[1] = last_tok;
    __syncthreads();
  }
  if (tid == 0) count[b] = s_carry[0];
}

// ---------------------------------------------------------------------------------------------------------- beam search
// One hypothesis: its score, its (merged) text, partial word and last word as character hashes with lengths, the string id
// of its last token (-1 = None), its pre-sort order and its backpointer record (parent slot << 16 | token).
struct CtcBeam {
  float score;
  int order, rec, sid;
  uint32_t th1, th2;
  int tlen;
  uint32_t ph1, ph2, pp1, pp2;
  int plen;
  uint32_t wh1, wh2;
  int wlen;
};

// n-gram fusion (get_lm_beams with self.lm set): what a beam carries on top of CtcBeam.  Every field is a function of the
// beam's merge key (text, partial word), so merged beams agree on them.
constexpr int kLmMaxOrder = 5;
constexpr int kLmCtx = kLmMaxOrder - 1;
constexpr uint32_t kNoWord = 0xffffffffu;  // (hashes are < 2^31 - 1)
struct CtcBeamLm : CtcBeam {
  double raw;            // the accumulated raw LM score of the text (the reference adds Python floats)
  float lmf, lm_score;   // fp32(raw + partial-word score); score + lmf: the key of ranking and pruning
  int nctx, ctx[kLmCtx]; // the n-gram context: word ids, the most recent first
  int poov;              // 1: the partial word is not a prefix of any unigram
  uint32_t hh1[kLmCtx - 1], hh2[kLmCtx - 1];  // the words before the last word (wh1/wh2), the most recent first
};
static_assert(sizeof(CtcBeamLm) == 128, "4 * 256 beam records must fit the 160 KiB of LDS beside the static arrays");

struct CtcLmArgs {
  const int32_t* strtab;  // [str_mask + 1][4]: h1, h2, length (-1 = empty slot), (word id + 1) << 2 | known << 1 | prefix
  const float* uni;       // [words][2]: log10 p, back-off
  const int32_t* ngtab;   // [ng_mask + 1][8]: n (0 = empty slot), ids last word first (5), log10 p, back-off (float bits)
  float* out_lm_score;    // [B][topk]
  uint32_t str_mask, ng_mask;
  int order, unk_id, bos_id, nhist;
  double alpha, beta, unk_offset, log10e;
};

__device__ __forceinline__ float rank_score(const CtcBeam& b) { return b.score; }
__device__ __forceinline__ float rank_score(const CtcBeamLm& b) { return b.lm_score; }

__device__ __forceinline__ bool same_key(const CtcBeam& a, const CtcBeam& b) {  // (text, partial_word, last_token)
  return a.th1 == b.th1 && a.tlen == b.tlen && a.ph1 == b.ph1 && a.sid == b.sid && a.plen == b.plen && a.th2 == b.th2 &&
         a.ph2 == b.ph2;
}
__device__ __forceinline__ bool same_history(const CtcBeam& a, const CtcBeam& b) {  // (last word of text, partial, last)
  return a.wh1 == b.wh1 && a.wlen == b.wlen && a.ph1 == b.ph1 && a.sid == b.sid && a.plen == b.plen && a.wh2 == b.wh2 &&
         a.ph2 == b.ph2;
}
// with an LM of order n the history key holds the last max(1, n - 1) words of the text
__device__ __forceinline__ bool same_history_lm(const CtcBeamLm& a, const CtcBeamLm& b, int nhist) {
  if (!same_history(a, b)) return false;
  for (int i = 0; i < kLmCtx - 1; ++i)
    if (i + 1 < nhist && (a.hh1[i] != b.hh1[i] || a.hh2[i] != b.hh2[i])) return false;
  return true;
}
// sort order: score descending (NaN ranks with -inf), then the pre-sort order ascending -- a total order
template <class Beam>
__device__ __forceinline__ bool beam_before(const Beam& a, const Beam& b) {
  const float sa = rank_score(a), sb = rank_score(b);
  const float ka = isnan(sa) ? -INFINITY : sa, kb = isnan(sb) ? -INFINITY : sb;
  return ka > kb || (ka == kb && a.order < b.order);
}
// numpy's npy_logaddexpf
__device__ __forceinline__ float logaddexp_f32(float x, float y) {
  if (x == y) return x + 0.693147180559945309f;
  const float d = x - y;
  if (d > 0.0f) return x + log1pf(expf(-d));
  if (d <= 0.0f) return y + log1pf(expf(d));
  return d;  // NaN
}
// merge_tokens(text, w) with w = the beam's partial word: text + " " + w (either side empty: the other)
__device__ __forceinline__ void fold_partial(CtcBeam& c, uint32_t sp1, uint32_t sp2, uint32_t space_code) {
  if (c.plen == 0) return;
  if (c.tlen == 0) {
    c.th1 = c.ph1, c.th2 = c.ph2, c.tlen = c.plen;
  } else {
    c.th1 = hadd(hmul(hadd(hmul(c.th1, sp1), space_code), c.pp1), c.ph1);
    c.th2 = hadd(hmul(hadd(hmul(c.th2, sp2), space_code), c.pp2), c.ph2);
    c.tlen += 1 + c.plen;
  }
  c.wh1 = c.ph1, c.wh2 = c.ph2, c.wlen = c.plen;
}

// ---- n-gram tables (speechbrain_amd/decoders/ngram.py builds them)
__device__ __forceinline__ uint32_t lm_mix(uint32_t x) {
  x ^= x >> 15;
  x *= 0x2c1b3c6du;
  x ^= x >> 12;
  return x;
}
// the value of a string (a word or a prefix of one) by its two hashes and length; 0 = not in the table
__device__ __forceinline__ int lm_string(const CtcLmArgs& lm, uint32_t h1, uint32_t h2, int len) {
  uint32_t s = lm_mix(h1 ^ (h2 * 0x9e3779b1u) ^ ((uint32_t)len * 0x85ebca6bu)) & lm.str_mask;
  for (uint32_t i = 0; i <= lm.str_mask; ++i, s = (s + 1) & lm.str_mask) {
    const int32_t* e = lm.strtab + (size_t)s * 4;
    const int l = e[2];
    if (l < 0) return 0;
    if (l == len && (uint32_t)e[0] == h1 && (uint32_t)e[1] == h2) return e[3];
  }
  return 0;
}
// the n-gram r[0..n) (ids, the LAST word first), n >= 2: its log10 p and back-off
__device__ __forceinline__ bool lm_ngram(const CtcLmArgs& lm, const int (&r)[kLmMaxOrder], int n, float& p, float& bo) {
  uint32_t x = (uint32_t)n;
  for (int i = 0; i < kLmMaxOrder; ++i)
    if (i < n) x = lm_mix((x ^ (uint32_t)r[i]) * 0x9e3779b1u);
  uint32_t s = x & lm.ng_mask;
  for (uint32_t k = 0; k <= lm.ng_mask; ++k, s = (s + 1) & lm.ng_mask) {
    const int32_t* e = lm.ngtab + (size_t)s * 8;
    const int en = e[0];
    if (en == 0) return false;
    if (en != n) continue;
    bool eq = true;
    for (int i = 0; i < kLmMaxOrder; ++i)
      if (i < n && e[1 + i] != r[i]) eq = false;
    if (eq) {
      p = __uint_as_float((unsigned)e[6]), bo = __uint_as_float((unsigned)e[7]);
      return true;
    }
  }
  return false;
}
// ARPA back-off: log10 p(w | ctx) = the longest n-gram (ctx[L-1..0], w) in the model, plus the back-offs of the longer
// contexts (the shortest first), accumulated in fp32 as kenlm's float does
__device__ __forceinline__ float lm_word_logp(const CtcLmArgs& lm, const CtcBeamLm& c, int w) {
  int r[kLmMaxOrder];
  r[0] = w;
  for (int i = 0; i < kLmCtx; ++i) r[1 + i] = c.ctx[i];
  float acc = lm.uni[2 * (size_t)w], p = 0.0f, bo = 0.0f;
  int matched = 0;
  for (int L = kLmCtx; L >= 1; --L)
    if (matched == 0 && L <= c.nctx && lm_ngram(lm, r, L + 1, p, bo)) acc = p, matched = L;
  for (int i = 0; i < kLmCtx; ++i) r[i] = c.ctx[i];
  r[kLmCtx] = 0;
  for (int L = 1; L <= kLmCtx; ++L) {
    if (L <= matched || L > c.nctx) continue;
    if (L == 1)
      acc += lm.uni[2 * (size_t)c.ctx[0] + 1];
    else if (lm_ngram(lm, r, L, p, bo))
      acc += bo;
  }
  return acc;
}
// KenlmScorer.score for next_word = the beam's partial word (not empty), before fold_partial moves it into the text
__device__ __forceinline__ void lm_fold_word(CtcBeamLm& c, const CtcLmArgs& lm) {
  if (c.plen == 0) return;
  const int v = lm_string(lm, c.ph1, c.ph2, c.plen);
  const int w = (v >> 2) > 0 ? (v >> 2) - 1 : lm.unk_id;
  double s = (double)lm_word_logp(lm, c, w);
  if (!(v & 2)) s += lm.unk_offset;  // outside the unigram set, or outside the model
  c.raw = c.raw + (lm.alpha * s * 1.0 / lm.log10e + lm.beta);
  for (int i = kLmCtx - 1; i >= 1; --i) c.ctx[i] = c.ctx[i - 1];
  c.ctx[0] = w;
  c.nctx = min(c.nctx + 1, lm.order - 1);
  for (int i = kLmCtx - 2; i >= 1; --i) c.hh1[i] = c.hh1[i - 1], c.hh2[i] = c.hh2[i - 1];
  c.hh1[0] = c.wlen > 0 ? c.wh1 : kNoWord, c.hh2[0] = c.wlen > 0 ? c.wh2 : kNoWord;
}
// score_partial_token of the beam's partial word, and the fp32 the reference adds to the CTC score
__device__ __forceinline__ void lm_partial(CtcBeamLm& c, const CtcLmArgs& lm, bool lookup) {
  double tot = c.raw;
  if (c.plen > 0) {
    if (lookup) c.poov = (lm_string(lm, c.ph1, c.ph2, c.plen) & 1) ? 0 : 1;
    double u = lm.unk_offset * (double)c.poov;
    if (c.plen > 6) u = u * (double)c.plen / 6.0;
    tot += u;
  } else {
    c.poov = 0;
  }
  c.lmf = (float)tot;
}

struct CtcBeamArgs {
  const float* x;
  const float* rel;
  const int32_t* table;  // [Vl][8]: kind (0 regular, 1 blank, 2 word boundary), string id, length, h1, p1, h2, p2, -
  int32_t* bp;           // workspace: [B][T][beam] records
  int32_t* fproc;        // workspace: [B][T] 1 = the frame was expanded
  int32_t* out_tokens;   // [B][topk][T]: the token of each expanded frame along the hypothesis' path, -1 elsewhere
  float* out_score;      // [B][topk]
  int32_t* out_count;    // [B]
  int T, V, Vl, blank, beam, topk, prune_history;
  float beam_prune_logp, token_min_logp, blank_skip_logp;
  uint32_t sp1, sp2, space_code;  // base powers of one character, the hash of " "
};

// Stable compaction of the first n entries of buf (kept where keep != 0) into dst; returns the kept count.
template <class Beam>
__device__ __forceinline__ int compact(const Beam* src, Beam* dst, int n, int keep, int* s_scan) {
  const int tid = threadIdx.x;
  s_scan[tid] = (tid < n && keep) ? 1 : 0;
  __syncthreads();
  for (int off = 1; off < kCtcThreads; off <<= 1) {
    const int add = tid >= off ? s_scan[tid - off] : 0;
    __syncthreads();
    s_scan[tid] += add;
    __syncthreads();
  }
  if (tid < n && keep) dst[s_scan[tid] - 1] = src[tid];
  const int total = s_scan[kCtcThreads - 1];
  __syncthreads();
  return total;
}

template <bool kLm>
struct BeamOf {
  using type = CtcBeam;
};
template <>
struct BeamOf<true> {
  using type = CtcBeamLm;
};

// The search of one utterance by one workgroup.  kLm = false is CTCBeamSearcher without a language model (lm unused);
// kLm = true fuses the n-gram model: every candidate carries its LM score, and ranking and pruning read lm_score.
template <bool kLm>
__device__ __forceinline__ void ctc_beam_body(const CtcBeamArgs& a, const CtcLmArgs& lm) {
  using Beam = typename BeamOf<kLm>::type;
  SBK_DYN_LDS(unsigned char, lds_bytes);
  Beam* lds = reinterpret_cast<Beam*>(lds_bytes);
  Beam* cur = lds;                    // beams entering the frame (sorted)
  Beam* cand = lds + a.beam;          // candidates of one token, then merged
  Beam* run0 = lds + 2 * a.beam;      // running top-`beam` of the frame (double buffer)
  Beam* run1 = lds + 3 * a.beam;
  __shared__ int s_scan[kCtcThreads];
  __shared__ int s_lead[kCtcThreads];
  __shared__ int s_tok[kCtcThreads];
  __shared__ int s_misc[4];  // 0: arg-max token of the frame, 1: kept tokens of the chunk, 2: candidates merged
  const int b = blockIdx.x, tid = threadIdx.x;
  float lf = a.rel ? (float)a.T * a.rel[b] : (float)a.T;
  const int len = isnan(lf) ? 0 : (int)fminf(fmaxf(lf, 0.0f), (float)a.T);  // .astype(int): truncation
  const float* xb = a.x + (size_t)b * a.T * a.V;
  int32_t* bpb = a.bp + (size_t)b * a.T * a.beam;
  int32_t* fpb = a.fproc + (size_t)b * a.T;
  if (tid == 0) {
    Beam z;
    z.score = 0.0f, z.order = 0, z.rec = -1, z.sid = -1;
    z.th1 = z.th2 = 0, z.tlen = 0, z.ph1 = z.ph2 = 0, z.pp1 = z.pp2 = 1, z.plen = 0, z.wh1 = z.wh2 = 0, z.wlen = 0;
    if constexpr (kLm) {  // get_start_state: begin-of-sentence (score_boundary) or the null context
      z.raw = 0.0, z.lmf = 0.0f, z.lm_score = 0.0f, z.poov = 0;
      for (int i = 0; i < kLmCtx; ++i) z.ctx[i] = 0;
      for (int i = 0; i < kLmCtx - 1; ++i) z.hh1[i] = z.hh2[i] = kNoWord;
      z.nctx = (lm.bos_id >= 0 && lm.order > 1) ? 1 : 0;
      if (z.nctx) z.ctx[0] = lm.bos_id;
    }
    cur[0] = z;
  }
  int nb = 1;
  for (int t = tid; t < a.T; t += kCtcThreads) fpb[t] = 0;
  __syncthreads();
  for (int t = 0; t < len; ++t) {
    const float* row = xb + (size_t)t * a.V;
    if (row[a.blank] > a.blank_skip_logp) continue;  // (uniform)
    // arg-max of the frame (numpy: the first maximum; NaN counts as the maximum)
    {
      float bv = NAN;
      int bi = 0x7fffffff;
      for (int v = tid; v < a.V; v += kCtcThreads) {
        const float w = row[v];
        if (bi == 0x7fffffff || arg_better(w, v, bv, bi)) bv = w, bi = v;
      }
      for (int m = 32; m >= 1; m >>= 1) {
        const float w = shfl_xor(bv, m);
        const int j = shfl_xor(bi, m);
        if (j != 0x7fffffff && (bi == 0x7fffffff || arg_better(w, j, bv, bi))) bv = w, bi = j;
      }
      if ((tid & 63) == 0) s_tok[tid >> 6] = bi, s_scan[tid >> 6] = __float_as_uint(bv);
      __syncthreads();
      if (tid == 0) {
        int best = s_tok[0];
        float bestv = __uint_as_float((unsigned)s_scan[0]);
        for (int w = 1; w < kCtcThreads / 64; ++w) {
          const int j = s_tok[w];
          const float wv = __uint_as_float((unsigned)s_scan[w]);
          if (j != 0x7fffffff && (best == 0x7fffffff || arg_better(wv, j, bestv, best))) best = j, bestv = wv;
        }
        s_misc[0] = best;
      }
      __syncthreads();
    }
    const int amax = s_misc[0];
    int nrun = 0;
    Beam* run = run0;
    Beam* nxt = run1;
    // (kLm) the beam of this thread with its partial word scored and folded into the text: the same for every word-boundary
    // token of the frame, so the n-gram lookups run once per beam and frame, at the first such token
    Beam folded;
    bool have_folded = false;
    for (int c0 = 0; c0 < a.Vl; c0 += kCtcThreads) {
      // the kept tokens of this chunk, in index order
      const int v = c0 + tid;
      const int keep = v < a.Vl && (row[v] > a.token_min_logp || v == amax);
      s_scan[tid] = keep;
      __syncthreads();
      for (int off = 1; off < kCtcThreads; off <<= 1) {
        const int add = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
      }
      if (keep) s_tok[s_scan[tid] - 1] = v;
      const int nk = s_scan[kCtcThreads - 1];
      __syncthreads();
      for (int k = 0; k < nk; ++k) {
        const int tv = s_tok[k];
        const int32_t* e = a.table + (size_t)tv * 8;
        const int kind = e[0], sid = e[1];
        const float lp = row[tv];
        // 1. expand every beam by token tv (partial_decoding's four branches, then get_lm_beams' text merge)
        if (tid < nb) {
          Beam c = cur[tid];
          c.score = c.score + lp;
          if (!(kind == 1 || c.sid == sid)) {
            const int tl = e[2];
            const uint32_t h1 = (uint32_t)e[3], p1 = (uint32_t)e[4], h2 = (uint32_t)e[5], p2 = (uint32_t)e[6];
            if (kind == 2) {  // word boundary: the partial word becomes the next word, the token's text starts a new one
              if constexpr (kLm) {
                if (!have_folded) {
                  folded = c;
                  lm_fold_word(folded, lm);
                  fold_partial(folded, a.sp1, a.sp2, a.space_code);
                  have_folded = true;
                }
                const float sc = c.score;
                c = folded;
                c.score = sc;
              } else {
                fold_partial(c, a.sp1, a.sp2, a.space_code);
              }
              c.ph1 = h1, c.ph2 = h2, c.pp1 = p1, c.pp2 = p2, c.plen = tl;
              if constexpr (kLm) lm_partial(c, lm, true);
            } else if (tl > 0) {  // the partial word grows by the token's text
              c.ph1 = hadd(hmul(c.ph1, p1), h1), c.ph2 = hadd(hmul(c.ph2, p2), h2);
              c.pp1 = hmul(c.pp1, p1), c.pp2 = hmul(c.pp2, p2), c.plen += tl;
              // (a word that is no prefix of a unigram stays none however it grows: no lookup)
              if constexpr (kLm) lm_partial(c, lm, c.poov == 0 || c.plen == tl);
            }
          }
          c.sid = sid;
          c.order = tv * kCtcBeamMax + tid;
          c.rec = (tid << 16) | tv;
          cand[tid] = c;
        }
        __syncthreads();
        // 2. merge_beams: equal keys fold into the first position, with the last member's fields and the scores added
        //    (logaddexp) in parent order
        if (tid < nb) {
          int lead = tid;
          for (int q = 0; q < tid; ++q)
            if (same_key(cand[q], cand[tid])) {
              lead = q;
              break;
            }
          s_lead[tid] = lead;
        }
        __syncthreads();
        Beam m;
        const bool is_lead = tid < nb && s_lead[tid] == tid;
        if (is_lead) {
          m = cand[tid];
          int last = tid;
          for (int j = tid + 1; j < nb; ++j)
            if (s_lead[j] == tid) m.score = logaddexp_f32(m.score, cand[j].score), last = j;
          m.rec = cand[last].rec;
          if constexpr (kLm) m.lm_score = m.score + m.lmf;
        }
        __syncthreads();
        if (is_lead) cand[tid] = m;
        __syncthreads();
        // 3. merge the token's candidates into the running top-`beam` (sorted, ties to the earlier order)
        int rank = -1;
        if (is_lead) {
          rank = 0;
          for (int j = 0; j < nb; ++j)
            if (j != tid && s_lead[j] == j && beam_before(cand[j], m)) ++rank;
          for (int j = 0; j < nrun; ++j)
            if (beam_before(run[j], m)) ++rank;
        }
        int rrank = -1;
        Beam r;
        if (tid < nrun) {
          r = run[tid];
          rrank = tid;
          for (int j = 0; j < nb; ++j)
            if (s_lead[j] == j && beam_before(cand[j], r)) ++rrank;
        }
        if (tid == 0) {
          int nl = 0;
          for (int j = 0; j < nb; ++j) nl += s_lead[j] == j;
          s_misc[2] = nl;
        }
        __syncthreads();
        if (rank >= 0 && rank < a.beam) nxt[rank] = m;
        if (rrank >= 0 && rrank < a.beam) nxt[rrank] = r;
        nrun = min(a.beam, nrun + s_misc[2]);
        Beam* sw = run;
        run = nxt, nxt = sw;
        __syncthreads();
      }
    }
    // 4. beam pruning: score >= fp32(best + beam_prune_logp); the list is already the best `beam_size` in order
    const float thr = nrun > 0 ? rank_score(run[0]) + a.beam_prune_logp : 0.0f;
    int keep = tid < nrun && rank_score(run[tid]) >= thr;
    int n2 = compact(run, nxt, nrun, keep, s_scan);
    Beam* sorted = nxt;
    // 5. prune_history: the first beam of each (last word(s), partial word, last token) survives
    if (a.prune_history) {
      keep = 0;
      if (tid < n2) {
        keep = 1;
        for (int j = 0; j < tid; ++j) {
          bool same;
          if constexpr (kLm)
            same = same_history_lm(sorted[j], sorted[tid], lm.nhist);
          else
            same = same_history(sorted[j], sorted[tid]);
          if (same) {
            keep = 0;
            break;
          }
        }
      }
      n2 = compact(sorted, cur, n2, keep, s_scan);
    } else {
      if (tid < n2) cur[tid] = sorted[tid];
      __syncthreads();
    }
    if (tid < n2) bpb[(size_t)t * a.beam + tid] = cur[tid].rec;
    if (tid == 0) fpb[t] = 1;
    nb = n2;
    __syncthreads();
  }
  // finalize_decoding(force_next_word=True): fold the partial word, last_token = None, merge on the text, prune, sort
  if (tid < nb) {
    Beam c = cur[tid];
    if constexpr (kLm) lm_fold_word(c, lm);
    fold_partial(c, a.sp1, a.sp2, a.space_code);
    c.ph1 = c.ph2 = 0, c.pp1 = c.pp2 = 1, c.plen = 0, c.sid = -1;
    if constexpr (kLm) lm_partial(c, lm, false);
    c.order = tid, c.rec = tid;
    cand[tid] = c;
  }
  __syncthreads();
  if (tid < nb) {
    int lead = tid;
    for (int q = 0; q < tid; ++q)
      if (same_key(cand[q], cand[tid])) {
        lead = q;
        break;
      }
    s_lead[tid] = lead;
  }
  __syncthreads();
  Beam m;
  const bool is_lead = tid < nb && s_lead[tid] == tid;
  if (is_lead) {
    m = cand[tid];
    for (int j = tid + 1; j < nb; ++j)
      if (s_lead[j] == tid) m.score = logaddexp_f32(m.score, cand[j].score), m.rec = cand[j].rec;
    if constexpr (kLm) m.lm_score = m.score + m.lmf;
  }
  __syncthreads();
  if (is_lead) cand[tid] = m;  // the leaders are ranked on their MERGED scores: ranks form a permutation of 0..nl-1
  __syncthreads();
  int rank = -1;
  if (is_lead) {
    rank = 0;
    for (int j = 0; j < nb; ++j)
      if (j != tid && s_lead[j] == j && beam_before(cand[j], m)) ++rank;
  }
  __syncthreads();
  if (rank >= 0) run0[rank] = m;  // (all leaders: <= nb <= beam)
  if (tid == 0) {
    int nl = 0;
    for (int j = 0; j < nb; ++j) nl += s_lead[j] == j;
    s_misc[2] = nl;
  }
  __syncthreads();
  const int nl = s_misc[2];
  const float thr = nl > 0 ? rank_score(run0[0]) + a.beam_prune_logp : 0.0f;
  const int keep = tid < nl && rank_score(run0[tid]) >= thr;
  const int nout = min(a.topk, compact(run0, run1, nl, keep, s_scan));
  // backtrack: thread k walks the records of hypothesis k from the last frame to the first
  if (tid < nout) {
    int32_t* path = a.out_tokens + ((size_t)b * a.topk + tid) * a.T;
    int slot = run1[tid].rec;
    for (int t = a.T - 1; t >= 0; --t) {
      if (t < len && fpb[t] && slot >= 0 && slot < a.beam) {  // (a record's parent is always a live slot)
        const int rec = bpb[(size_t)t * a.beam + slot];
        path[t] = rec & 0xffff;
        slot = rec >> 16;
      } else {
        path[t] = -1;
      }
    }
    a.out_score[(size_t)b * a.topk + tid] = run1[tid].score;
    if constexpr (kLm) lm.out_lm_score[(size_t)b * a.topk + tid] = run1[tid].lm_score;
  }
  if (tid == 0) a.out_count[b] = nout;
}

__global__ __launch_bounds__(256) void ctc_beam_kernel(CtcBeamArgs a) { ctc_beam_body<false>(a, CtcLmArgs{}); }
__global__ __launch_bounds__(256) void ctc_beam_lm_kernel(CtcBeamArgs a, CtcLmArgs lm) { ctc_beam_body<true>(a, lm); }

}  // namespace

}  // namespace sbk

using namespace sbk;

extern "C" int sbk_ctc_greedy_decode_f32(const float* x, const float* rel_len, int32_t* tokens, int32_t* count, int B,
                                         int T, int V, int blank, sbk_stream_t stream) {
  if (B == 0) return 0;
  SBK_REQUIRE(x && tokens && count && B > 0 && T > 0 && V > 0, "ctc_greedy_decode: bad arguments (B=%d T=%d V=%d)", B, T, V);
  SBK_REQUIRE(blank >= 0 && blank < V, "ctc_greedy_decode: blank %d outside [0, %d)", blank, V);
  hipStream_t st = as_stream(stream);
  ProfScope prof("ctc_greedy_decode", 1.0 * B * T * V, 4.0 * B * T * V + 8.0 * B * T, st);
  SBK_LAUNCH(ctc_greedy_kernel, dim3(B), dim3(kCtcThreads), 0, st, x, rel_len, tokens, count, T, V, blank);
  return launch_status("ctc_greedy_decode");
}

extern "C" size_t sbk_ctc_beam_search_workspace_bytes(int B, int T, int V, int beam, int topk) {
  (void)V, (void)topk;
  if (B <= 0 || T <= 0 || beam <= 0) return 0;
  return ((size_t)B * T * beam + (size_t)B * T) * sizeof(int32_t);
}

// The checks and the kernel arguments that the plain and the fused search share.
static int ctc_beam_prepare(const float* x, const float* rel_len, const int32_t* token_table, int Vl,
                            const sbk_ctc_beam_config* cfg, void* workspace, size_t workspace_bytes, int32_t* out_tokens,
                            float* out_score, int32_t* out_count, int B, int T, int V, CtcBeamArgs& a) {
  SBK_REQUIRE(cfg, "ctc_beam_search: cfg is NULL");
  SBK_REQUIRE(x && token_table && workspace && out_tokens && out_score && out_count && B > 0 && T > 0 && V > 0,
              "ctc_beam_search: bad arguments (B=%d T=%d V=%d)", B, T, V);
  SBK_REQUIRE(Vl > 0 && Vl <= V && V <= 65535, "ctc_beam_search: vocabulary of %d tokens for V=%d (1 <= len <= V <= 65535)",
              Vl, V);
  SBK_REQUIRE(cfg->blank >= 0 && cfg->blank < V, "ctc_beam_search: blank %d outside [0, %d)", cfg->blank, V);
  SBK_REQUIRE(cfg->beam_size >= 1 && cfg->beam_size <= kCtcBeamMax,
              "ctc_beam_search: beam_size %d is not supported (1..%d: the beam lives in one workgroup's LDS)",
              cfg->beam_size, kCtcBeamMax);
  SBK_REQUIRE(cfg->topk >= 1 && cfg->topk <= cfg->beam_size, "ctc_beam_search: topk %d outside [1, beam_size]", cfg->topk);
  SBK_REQUIRE(workspace_bytes >= sbk_ctc_beam_search_workspace_bytes(B, T, V, cfg->beam_size, cfg->topk),
              "ctc_beam_search: workspace of %zu bytes, %zu needed", workspace_bytes,
              sbk_ctc_beam_search_workspace_bytes(B, T, V, cfg->beam_size, cfg->topk));
  SBK_REQUIRE(aligned16(workspace), "ctc_beam_search: workspace must be 16-byte aligned");
  a.x = x, a.rel = rel_len, a.table = token_table;
  a.bp = static_cast<int32_t*>(workspace);
  a.fproc = a.bp + (size_t)B * T * cfg->beam_size;
  a.out_tokens = out_tokens, a.out_score = out_score, a.out_count = out_count;
  a.T = T, a.V = V, a.Vl = Vl, a.blank = cfg->blank, a.beam = cfg->beam_size, a.topk = cfg->topk;
  a.prune_history = cfg->prune_history;
  a.beam_prune_logp = cfg->beam_prune_logp, a.token_min_logp = cfg->token_prune_min_logp;
  a.blank_skip_logp = cfg->log_blank_skip_threshold;
  a.sp1 = cfg->char_base1, a.sp2 = cfg->char_base2, a.space_code = cfg->space_code;
  SBK_REQUIRE(a.sp1 < kHashMod && a.sp2 < kHashMod && a.space_code < kHashMod, "ctc_beam_search: hash constants >= 2^31-1");
  return 0;
}

extern "C" int sbk_ctc_beam_search_f32(const float* x, const float* rel_len, const int32_t* token_table, int Vl,
                                       const sbk_ctc_beam_config* cfg, void* workspace, size_t workspace_bytes,
                                       int32_t* out_tokens, float* out_score, int32_t* out_count, int B, int T, int V,
                                       sbk_stream_t stream) {
  if (B == 0) return 0;
  CtcBeamArgs a;
  if (const int rc = ctc_beam_prepare(x, rel_len, token_table, Vl, cfg, workspace, workspace_bytes, out_tokens, out_score,
                                      out_count, B, T, V, a))
    return rc;
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)4 * cfg->beam_size * sizeof(CtcBeam);
  if (allow_dyn_lds(ctc_beam_kernel, lds) != hipSuccess)
    return fail(SBK_EINVAL, "ctc_beam_search: %zu bytes of LDS for beam_size %d not available", lds, cfg->beam_size);
  ProfScope prof("ctc_beam_search", 0.0, 4.0 * B * T * V + 4.0 * B * T * cfg->beam_size, st);
  SBK_LAUNCH(ctc_beam_kernel, dim3(B), dim3(kCtcThreads), lds, st, a);
  return launch_status("ctc_beam_search");
}

extern "C" int sbk_ctc_beam_search_lm_f32(const float* x, const float* rel_len, const int32_t* token_table, int Vl,
                                          const sbk_ctc_beam_config* cfg, const sbk_ctc_lm_tables* lm, void* workspace,
                                          size_t workspace_bytes, int32_t* out_tokens, float* out_score,
                                          float* out_lm_score, int32_t* out_count, int B, int T, int V,
                                          sbk_stream_t stream) {
  if (B == 0) return 0;
  CtcBeamArgs a;
  if (const int rc = ctc_beam_prepare(x, rel_len, token_table, Vl, cfg, workspace, workspace_bytes, out_tokens, out_score,
                                      out_count, B, T, V, a))
    return rc;
  SBK_REQUIRE(lm && out_lm_score, "ctc_beam_search_lm: lm tables or out_lm_score is NULL");
  SBK_REQUIRE(lm->order >= 1 && lm->order <= kLmMaxOrder,
              "ctc_beam_search_lm: an n-gram model of order %d is not supported (1..%d: the context a beam carries)",
              lm->order, kLmMaxOrder);
  SBK_REQUIRE(lm->strings && lm->unigrams && lm->ngrams, "ctc_beam_search_lm: a table pointer is NULL");
  SBK_REQUIRE(lm->n_string_slots >= 2 && (lm->n_string_slots & (lm->n_string_slots - 1)) == 0 && lm->n_ngram_slots >= 2 &&
                  (lm->n_ngram_slots & (lm->n_ngram_slots - 1)) == 0,
              "ctc_beam_search_lm: table sizes %d / %d are not powers of two >= 2", lm->n_string_slots, lm->n_ngram_slots);
  SBK_REQUIRE(lm->n_words >= 1 && lm->unk_id >= 0 && lm->unk_id < lm->n_words && lm->bos_id < lm->n_words,
              "ctc_beam_search_lm: word ids unk %d / bos %d outside the %d unigrams", lm->unk_id, lm->bos_id, lm->n_words);
  CtcLmArgs l;
  l.strtab = lm->strings, l.uni = lm->unigrams, l.ngtab = lm->ngrams, l.out_lm_score = out_lm_score;
  l.str_mask = (uint32_t)lm->n_string_slots - 1, l.ng_mask = (uint32_t)lm->n_ngram_slots - 1;
  l.order = lm->order, l.unk_id = lm->unk_id, l.bos_id = lm->score_boundary ? lm->bos_id : -1;
  l.nhist = lm->order - 1 > 1 ? lm->order - 1 : 1;
  l.alpha = lm->alpha, l.beta = lm->beta, l.unk_offset = lm->unk_score_offset, l.log10e = lm->log10_e;
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)4 * cfg->beam_size * sizeof(CtcBeamLm);
  if (allow_dyn_lds(ctc_beam_lm_kernel, lds) != hipSuccess)
    return fail(SBK_EINVAL, "ctc_beam_search_lm: %zu bytes of LDS for beam_size %d not available", lds, cfg->beam_size);
  ProfScope prof("ctc_beam_search_lm", 0.0, 4.0 * B * T * V + 4.0 * B * T * cfg->beam_size, st);
  SBK_LAUNCH(ctc_beam_lm_kernel, dim3(B), dim3(kCtcThreads), lds, st, a, l);
  return launch_status("ctc_beam_search_lm");
}
