// CTCPrefixBeamSearcher without a language model on the device (decoders/ctc.py:382-509 CTCBeam, 1488-1905 the searcher,
// 868-934 finalize_decoding).  One workgroup per utterance runs every frame of it in ONE launch; nothing is read back per
// frame.  DESIGN.md section 5, "CTC prefix beam search", lists the semantics reproduced here.
//
// A beam is a prefix text with the probabilities of ending in blank (p_b) and not in blank (p_nb).  The beams of a frame
// live in LDS as a list in the reference's list order; what identifies a text is a 64-bit key, the pair of polynomial
// hashes of csrc/ctc_text.h extended token by token, so that one text reached over two token paths has one key.
//
// One frame:
//   1. the token set {v < Vl : x[v] > token_prune_min_logp or v = argmax} without the blank, compacted by wave scans in
//      ascending token order;
//   2. the items of the frame: the nb current beams, then the nb * ntok extensions e = k * nb + beam (token-major: tokens
//      ascending, then the beams in list order -- the loop nest of the reference, on which the creator of a text
//      depends).  Every item has the key of the text it stands for; an open-addressed index over the keys holds, per
//      key, the LOWEST item that has it (atomicMin: the result does not depend on the order of arrival).  The target of an
//      extension is that lowest item: a current beam with the text, else the first extension that spells it, which
//      thereby creates the beam.  (A SentencePiece boundary piece is looked up by the reference under a text no beam has:
//      it always creates, and only later extensions find it.)
//   3. merge = group, then reduce: every extension links itself into its target's list (the order of a list is the order
//      of arrival and is never used); the owner of a target then takes the members in ASCENDING extension order, by
//      repeated minimum extraction, and folds logaddexp over them in exactly that order, with the beam's own
//      repeated-token term at its place in the order.  No sum is ever formed in the order atomics arrive: two runs,
//      and runs on two streams, give the same bits.  The extraction costs the square of a list's length in one thread.
//      A list holds the beams that reach one text with one token: one for one-character vocabularies, a few with
//      word pieces ("a" + "bc", "ab" + "c"), at most nb if every beam converged on one text, which would serialise
//      nb * nb / 2 steps on one lane (32 768 at beam 256) -- bounded, and not met with posteriors we have seen; a list
//      sorted once would be the remedy;
//   4. step(): p_b, p_nb <- n_p_b, n_p_nb and score = logaddexp(p_b, p_nb); the cut at max + beam_prune_logp; the
//      beam_size best by (score descending, list position ascending) through an exact radix selection over the 64-bit
//      order key (order_key(score) << 32 | ~position: unique, so ties go to the lower position); prune_history.
// The items of a frame (keys, index, lists, scores, tokens) live in LDS while nb * (ntok + 1) fits the LDS region, and in
// the caller's workspace otherwise, which the workspace query sizes for beam_size * (min(V, Vl) + 1) items: no frame can
// exceed it and nothing is capped.  Scores are fp32; -inf is a real -INFINITY and logaddexp(-inf, -inf) = -inf.
#include <math.h>

#include "argmax.h"
#include "common.h"
#include "ctc_text.h"
#include "device.h"
#include "kernel_util.h"

namespace sbk {

namespace {

constexpr int kPfxThreads = 256;
constexpr int kPfxBeamMax = kPfxThreads;  // a surviving beam per thread
constexpr int kPfxLdsItems = 2048;        // items of a frame that LDS holds (a power of two)
constexpr int kNoToken = 0xffff;          // record: the beam was carried over the frame, not created in it
constexpr int kNone = 0x7fffffff;

// One prefix: the key of its text, the last word of the text and the partial word as hashes with lengths (prune_history
// and the final merge read them), the last token, the probabilities, and the record (parent slot << 16 | token) the host
// rebuilds the text and its frames from.
struct PfxBeam {
  uint32_t th1, th2;
  uint32_t wh1, wh2;
  int wlen, wopen;  // wopen: the text ends inside the word (no space after it)
  uint32_t ph1, ph2;
  int plen;
  int last;  // token index, -1 = none
  float p_b, p_nb, score;
  int rec;
  int pad[2];
};
static_assert(sizeof(PfxBeam) == 64, "two lists of 256 beams take 32 KiB of LDS");

struct PfxArgs {
  const float* x;
  const float* rel;
  const int32_t* table;  // [Vl][8]: kind, string id, length, h1, p1, h2, p2, never-found (include/sbk.h)
  int32_t* bp;           // workspace [B][T][beam]: records
  int32_t* fproc;        // workspace [B][T]: 1 = the frame was expanded
  int32_t* stats;        // workspace [B][4]: frames expanded, frames skipped, extensions, frames held in the workspace
  unsigned char* items;  // workspace [B][item_bytes]
  size_t item_bytes;
  int32_t* out_tokens;
  float* out_score;
  int32_t* out_count;
  int T, V, Vl, blank, beam, topk, prune_history;
  int lds_cap, ws_cap;
  float beam_prune_logp, token_min_logp, blank_skip_logp;
  uint32_t sp1, sp2, space_code;
};

// The arrays of one frame over `cap` items, in LDS or in the workspace.
struct PfxFrame {
  unsigned long long* key;  // [cap] per item
  int* slot;                // [nslot_cap] the index: lowest item of the key in the slot, -1 = empty
  int* next;                // [cap] per extension: the next member of its target's list
  int* head;                // [cap] per item: its list
  int* target;              // [cap] per extension
  float* score;             // [cap] per item
  int* tok;                 // [cap] the token set
};
__host__ __device__ inline int pow2_ceil(long n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}
__host__ __device__ inline size_t pfx_frame_bytes(long cap) { return (size_t)cap * 28 + (size_t)pow2_ceil(2 * cap) * 4; }
__device__ __forceinline__ PfxFrame pfx_frame(unsigned char* base, long cap) {
  PfxFrame f;
  f.key = reinterpret_cast<unsigned long long*>(base);
  f.slot = reinterpret_cast<int*>(base + (size_t)cap * 8);
  f.next = f.slot + pow2_ceil(2 * cap);
  f.head = f.next + cap;
  f.target = f.head + cap;
  f.score = reinterpret_cast<float*>(f.target + cap);
  f.tok = reinterpret_cast<int*>(f.score + cap);
  return f;
}

__device__ __forceinline__ unsigned long long text_key(uint32_t h1, uint32_t h2) { return ((unsigned long long)h1 << 32) | h2; }
__device__ __forceinline__ uint32_t key_slot(unsigned long long k) { return (uint32_t)((k * 0x9e3779b97f4a7c15ull) >> 32); }

// the text of beam `c` extended by the token of table row e: its hashes (what _get_new_beam makes the new text)
__device__ __forceinline__ void extend_text(const PfxBeam& c, const int32_t* e, const PfxArgs& a, uint32_t& h1, uint32_t& h2) {
  const uint32_t th1 = (uint32_t)e[3], tp1 = (uint32_t)e[4], th2 = (uint32_t)e[5], tp2 = (uint32_t)e[6];
  h1 = c.th1, h2 = c.th2;
  if (e[0] == 2) h1 = hadd(hmul(h1, a.sp1), a.space_code), h2 = hadd(hmul(h2, a.sp2), a.space_code);
  if (e[2] > 0) h1 = hadd(hmul(h1, tp1), th1), h2 = hadd(hmul(h2, tp2), th2);
}
// the beam _get_new_beam creates from `c` and token v (its probabilities are the caller's)
__device__ __forceinline__ PfxBeam create_beam(const PfxBeam& c, int v, const int32_t* e, const PfxArgs& a) {
  PfxBeam n = c;
  const uint32_t th1 = (uint32_t)e[3], tp1 = (uint32_t)e[4], th2 = (uint32_t)e[5], tp2 = (uint32_t)e[6];
  const int tl = e[2];
  extend_text(c, e, a, n.th1, n.th2);
  if (e[0] == 2) {  // a word boundary: the token's text starts the next word
    n.ph1 = th1, n.ph2 = th2, n.plen = tl;
    n.wopen = 0;
    if (tl > 0) n.wh1 = th1, n.wh2 = th2, n.wlen = tl, n.wopen = 1;
  } else {
    if (c.wopen)
      n.wh1 = hadd(hmul(c.wh1, tp1), th1), n.wh2 = hadd(hmul(c.wh2, tp2), th2), n.wlen = c.wlen + tl;
    else
      n.wh1 = th1, n.wh2 = th2, n.wlen = tl;
    n.wopen = 1;
    if (v != c.last)  // (a repeated token lengthens the text, not the partial word)
      n.ph1 = hadd(hmul(c.ph1, tp1), th1), n.ph2 = hadd(hmul(c.ph2, tp2), th2), n.plen = c.plen + tl;
  }
  n.last = v;
  return n;
}
__device__ __forceinline__ uint32_t hpow(uint32_t b, int n) {
  uint32_t r = 1;
  for (; n > 0; n >>= 1, b = hmul(b, b))
    if (n & 1) r = hmul(r, b);
  return r;
}

// sum / max over the workgroup, in every thread (red: 4 words; order-free operations only)
__device__ __forceinline__ int block_sum_int(int v, int* red) {
  for (int m = 32; m >= 1; m >>= 1) v += shfl_xor(v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max(float v, int* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (int)__float_as_uint(v);
  __syncthreads();
  return fmaxf(fmaxf(__uint_as_float((unsigned)red[0]), __uint_as_float((unsigned)red[1])),
               fmaxf(__uint_as_float((unsigned)red[2]), __uint_as_float((unsigned)red[3])));
}

__global__ __launch_bounds__(256) void ctc_prefix_kernel(PfxArgs a) {
  SBK_DYN_LDS(unsigned char, lds_bytes);
  PfxBeam* cur = reinterpret_cast<PfxBeam*>(lds_bytes);
  PfxBeam* nxt = cur + a.beam;
  unsigned char* lds_items = lds_bytes + (size_t)2 * a.beam * sizeof(PfxBeam);
  __shared__ int s_scan[kPfxThreads];
  __shared__ int s_hist[256];
  __shared__ unsigned long long s_sel[kPfxThreads];
  __shared__ int s_red[4];
  __shared__ int s_misc[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float lf = a.rel ? (float)a.T * a.rel[b] : (float)a.T;
  // (.astype(int): truncation.)  A length that is no number, negative or past T is reported through out_count = -1.
  const bool bad_len = isnan(lf) || lf < 0.0f || lf >= (float)a.T + 1.0f;
  const int len = bad_len ? 0 : min((int)lf, a.T);
  const float* xb = a.x + (size_t)b * a.T * a.V;
  int32_t* bpb = a.bp + (size_t)b * a.T * a.beam;
  int32_t* fpb = a.fproc + (size_t)b * a.T;
  unsigned char* ws_items = a.items + (size_t)b * a.item_bytes;
  if (tid == 0) {
    PfxBeam z;
    z.th1 = z.th2 = 0, z.wh1 = z.wh2 = 0, z.wlen = 0, z.wopen = 0, z.ph1 = z.ph2 = 0, z.plen = 0, z.last = -1;
    z.p_b = 0.0f, z.p_nb = -INFINITY, z.score = 0.0f, z.rec = -1, z.pad[0] = z.pad[1] = 0;
    cur[0] = z;
  }
  int nb = 1;
  int st_done = 0, st_skip = 0, st_ext = 0, st_ws = 0;
  for (int t = tid; t < a.T; t += kPfxThreads) fpb[t] = 0;
  __syncthreads();
  for (int t = 0; t < len && nb > 0; ++t) {
    const float* row = xb + (size_t)t * a.V;
    if (row[a.blank] > a.blank_skip_logp) {  // (uniform)
      ++st_skip;
      continue;
    }
    // ---- the arg-max of the frame over all V columns (numpy: the first maximum, NaN above everything)
    {
      float bv = NAN;
      int bi = kNone;
      for (int v = tid; v < a.V; v += kPfxThreads) {
        const float w = row[v];
        if (bi == kNone || arg_better(w, v, bv, bi)) bv = w, bi = v;
      }
      for (int m = 32; m >= 1; m >>= 1) {
        const float w = shfl_xor(bv, m);
        const int j = shfl_xor(bi, m);
        if (j != kNone && (bi == kNone || arg_better(w, j, bv, bi))) bv = w, bi = j;
      }
      __syncthreads();
      if (lane == 0) s_scan[wave] = bi, s_scan[4 + wave] = (int)__float_as_uint(bv);
      __syncthreads();
      if (tid == 0) {
        int best = s_scan[0];
        float bestv = __uint_as_float((unsigned)s_scan[4]);
        for (int w = 1; w < kPfxThreads / 64; ++w) {
          const int j = s_scan[w];
          const float wv = __uint_as_float((unsigned)s_scan[4 + w]);
          if (j != kNone && (best == kNone || arg_better(wv, j, bestv, best))) best = j, bestv = wv;
        }
        s_misc[0] = best;
      }
      __syncthreads();
    }
    const int amax = s_misc[0];
    const bool has_blank = a.blank < a.Vl && (row[a.blank] > a.token_min_logp || a.blank == amax);
    // ---- the token set: counted, then compacted in ascending order by wave scans
    int cnt = 0;
    for (int v = tid; v < a.Vl; v += kPfxThreads) cnt += v != a.blank && (row[v] > a.token_min_logp || v == amax);
    const int ntok = block_sum_int(cnt, s_red);
    const long nitems = (long)nb * (ntok + 1);
    const int next_items = nb * ntok;  // (<= beam * Vl <= 256 * 65535)
    const bool in_lds = nitems <= a.lds_cap;
    const PfxFrame f = in_lds ? pfx_frame(lds_items, a.lds_cap) : pfx_frame(ws_items, a.ws_cap);
    const int nslot = pow2_ceil(2 * nitems);
    ++st_done, st_ext += next_items, st_ws += in_lds ? 0 : 1;
    for (int c0 = 0, base = 0; c0 < a.Vl; c0 += kPfxThreads) {
      const int v = c0 + tid;
      const int keep = v < a.Vl && v != a.blank && (row[v] > a.token_min_logp || v == amax);
      int incl = keep;
      for (int off = 1; off < 64; off <<= 1) {
        const int up = shfl(incl, lane >= off ? lane - off : lane);
        if (lane >= off) incl += up;
      }
      __syncthreads();
      if (lane == 63) s_red[wave] = incl;
      __syncthreads();
      int pos = base + incl - 1;
      for (int w = 0; w < wave; ++w) pos += s_red[w];
      if (keep) f.tok[pos] = v;
      base += s_red[0] + s_red[1] + s_red[2] + s_red[3];
    }
    for (int s = tid; s < nslot; s += kPfxThreads) f.slot[s] = -1;
    for (long j = tid; j < nitems; j += kPfxThreads) f.head[j] = -1;
    __syncthreads();
    // ---- the key of every item
    for (long j = tid; j < nitems; j += kPfxThreads) {
      if (j < nb) {
        f.key[j] = text_key(cur[j].th1, cur[j].th2);
      } else {
        const int e = (int)(j - nb), k = e / nb, i = e - k * nb, v = f.tok[k];
        uint32_t h1, h2;
        extend_text(cur[i], a.table + (size_t)v * 8, a, h1, h2);
        f.key[j] = text_key(h1, h2);
      }
    }
    __syncthreads();
    // ---- the index: per key the lowest item (f.target holds the item's slot until the targets are read)
    for (long j = tid; j < nitems; j += kPfxThreads) {
      const unsigned long long k = f.key[j];
      uint32_t s = key_slot(k) & (uint32_t)(nslot - 1);
      for (;;) {
        const int old = atomicCAS(&f.slot[s], -1, (int)j);
        if (old == -1) break;
        if (f.key[old] == k) {
          atomicMin(&f.slot[s], (int)j);
          break;
        }
        s = (s + 1) & (uint32_t)(nslot - 1);
      }
      if (j >= nb) f.target[j - nb] = (int)s;
    }
    __syncthreads();
    for (int e = tid; e < next_items; e += kPfxThreads) {
      const int v = f.tok[e / nb];
      // a token the reference looks up under a text no beam has (column 7) creates its own beam whatever the index holds
      const int tg = a.table[(size_t)v * 8 + 7] ? nb + e : f.slot[f.target[e]];
      f.target[e] = tg;
      f.next[e] = atomicExch(&f.head[tg], e);
    }
    __syncthreads();
    // ---- reduce: the owner of a target folds its members in ascending extension order
    float my_pb = -INFINITY, my_pnb = -INFINITY;
    for (long j = tid; j < nitems; j += kPfxThreads) {
      if (j >= nb && f.target[j - nb] != (int)j) continue;  // (not a beam)
      int eself = kNone;  // the place of the beam's own repeated-token term
      float cself = 0.0f;
      if (j < nb && cur[j].last >= 0) {
        int lo = 0, hi = ntok;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (f.tok[mid] < cur[j].last) lo = mid + 1; else hi = mid;
        }
        if (lo < ntok && f.tok[lo] == cur[j].last) eself = lo * nb + (int)j, cself = cur[j].p_nb + row[cur[j].last];
      }
      float acc = -INFINITY;
      int prev = -1;
      for (;;) {
        int m = kNone;
        for (int e = f.head[j]; e >= 0; e = f.next[e])
          if (e > prev && e < m) m = e;
        if (eself != kNone && eself <= m) acc = logaddexp_f32(acc, cself), eself = kNone;
        if (m == kNone) break;
        const int k = m / nb, i = m - k * nb, v = f.tok[k];
        const float lp = row[v];
        acc = logaddexp_f32(acc, (v == cur[i].last ? cur[i].p_b : cur[i].score) + lp);
        prev = m;
      }
      if (j < nb) {
        my_pb = has_blank ? cur[j].score + row[a.blank] : -INFINITY;
        my_pnb = acc;
      } else {
        f.score[j] = isnan(acc) ? -INFINITY : acc;
      }
    }
    __syncthreads();
    if (tid < nb) {  // step() of the beams that entered the frame
      const float sc = logaddexp_f32(my_pb, my_pnb);
      cur[tid].p_b = my_pb, cur[tid].p_nb = my_pnb, cur[tid].score = isnan(sc) ? -INFINITY : sc;
      f.score[tid] = cur[tid].score;
    }
    __syncthreads();
    // ---- the cut at max + beam_prune_logp, then the beam_size best: (score descending, list position ascending)
    float mx = -INFINITY;
    for (long j = tid; j < nitems; j += kPfxThreads)
      if (j < nb || f.target[j - nb] == (int)j) mx = fmaxf(mx, f.score[j]);
    mx = block_max(mx, s_red);
    const float thr = mx + a.beam_prune_logp;
    int alive = 0;
    for (long j = tid; j < nitems; j += kPfxThreads)
      alive += (j < nb || f.target[j - nb] == (int)j) && f.score[j] >= thr;
    alive = block_sum_int(alive, s_red);
    unsigned long long kth = 0;
    if (alive > a.beam) {  // radix selection of the beam-th largest order key, most significant byte first
      unsigned long long pmask = 0;
      int k = a.beam;
      for (int d = 7; d >= 0; --d) {
        s_hist[tid] = 0;
        __syncthreads();
        for (long j = tid; j < nitems; j += kPfxThreads) {
          if (!((j < nb || f.target[j - nb] == (int)j) && f.score[j] >= thr)) continue;
          const unsigned long long key = ((unsigned long long)order_key(f.score[j]) << 32) | (0xffffffffu - (uint32_t)j);
          if ((key & pmask) == kth) atomicAdd(&s_hist[(int)((key >> (8 * d)) & 255)], 1);
        }
        __syncthreads();
        if (tid == 0) {
          int digit = 255;
          for (; digit > 0 && k > s_hist[digit]; --digit) k -= s_hist[digit];
          s_misc[1] = digit, s_misc[2] = k;
        }
        __syncthreads();
        kth |= (unsigned long long)s_misc[1] << (8 * d), pmask |= 0xffull << (8 * d), k = s_misc[2];
      }
    }
    if (tid == 0) s_misc[3] = 0;
    __syncthreads();
    for (long j = tid; j < nitems; j += kPfxThreads) {
      if (!((j < nb || f.target[j - nb] == (int)j) && f.score[j] >= thr)) continue;
      const unsigned long long key = ((unsigned long long)order_key(f.score[j]) << 32) | (0xffffffffu - (uint32_t)j);
      if (key >= kth) s_sel[atomicAdd(&s_misc[3], 1)] = key;  // (at most beam_size of them; ranked below: any order)
    }
    __syncthreads();
    const int nsel = s_misc[3];
    PfxBeam mine;
    int rank = -1;
    if (tid < nsel) {
      const unsigned long long key = s_sel[tid];
      rank = 0;
      for (int q = 0; q < nsel; ++q) rank += s_sel[q] > key;
      const int j = (int)(0xffffffffu - (uint32_t)key);
      if (j < nb) {
        mine = cur[j];
        mine.rec = (j << 16) | kNoToken;
      } else {
        const int e = j - nb, k = e / nb, i = e - k * nb, v = f.tok[k];
        mine = create_beam(cur[i], v, a.table + (size_t)v * 8, a);
        mine.p_b = -INFINITY, mine.p_nb = mine.score = f.score[j];
        mine.rec = (i << 16) | v;
      }
      nxt[rank] = mine;
    }
    __syncthreads();
    // ---- prune_history: the first beam of each (last word of the text, partial word, last token) survives
    int keep = tid < nsel;
    if (a.prune_history && tid < nsel) {
      const PfxBeam& me = nxt[tid];
      for (int q = 0; q < tid; ++q) {
        const PfxBeam& o = nxt[q];
        if (o.wh1 == me.wh1 && o.wh2 == me.wh2 && o.wlen == me.wlen && o.ph1 == me.ph1 && o.ph2 == me.ph2 &&
            o.plen == me.plen && o.last == me.last) {
          keep = 0;
          break;
        }
      }
    }
    s_scan[tid] = keep;
    __syncthreads();
    for (int off = 1; off < kPfxThreads; off <<= 1) {
      const int add = tid >= off ? s_scan[tid - off] : 0;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    if (keep) {
      const PfxBeam kept = nxt[tid];
      cur[s_scan[tid] - 1] = kept;
      bpb[(size_t)t * a.beam + s_scan[tid] - 1] = kept.rec;
    }
    if (tid == 0) fpb[t] = 1;
    nb = s_scan[kPfxThreads - 1];
    __syncthreads();
  }
  // ---- finalize_decoding(force_next_word=True): beams whose merge_tokens(text, partial word) agree fold into the first
  // of them (scores added in list order, the fields of the last), then the cut, the order and the topk
  uint32_t* fk1 = reinterpret_cast<uint32_t*>(s_hist);
  uint32_t* fk2 = reinterpret_cast<uint32_t*>(s_sel);
  if (tid < nb) {
    const PfxBeam c = cur[tid];
    uint32_t h1 = c.th1, h2 = c.th2;
    if (c.plen > 0) {
      h1 = hadd(hmul(hadd(hmul(h1, a.sp1), a.space_code), hpow(a.sp1, c.plen)), c.ph1);
      h2 = hadd(hmul(hadd(hmul(h2, a.sp2), a.space_code), hpow(a.sp2, c.plen)), c.ph2);
    }
    fk1[tid] = h1, fk2[tid] = h2;
  }
  __syncthreads();
  int lead = -1;
  if (tid < nb) {
    lead = tid;
    for (int q = 0; q < tid; ++q)
      if (fk1[q] == fk1[tid] && fk2[q] == fk2[tid]) {
        lead = q;
        break;
      }
    s_scan[tid] = lead;
  }
  __syncthreads();
  const bool is_lead = tid < nb && lead == tid;
  if (is_lead) {
    PfxBeam m = cur[tid];
    m.rec = tid;  // from here on: the slot of the last expanded frame's list whose records spell the hypothesis
    for (int j = tid + 1; j < nb; ++j)
      if (s_scan[j] == tid) m.score = logaddexp_f32(m.score, cur[j].score), m.rec = j;
    nxt[tid] = m;
  }
  __syncthreads();
  float mx = -INFINITY;
  if (is_lead) mx = nxt[tid].score;
  mx = block_max(mx, s_red);
  const float thr = mx + a.beam_prune_logp;
  const bool out = is_lead && nxt[tid].score >= thr;
  int rank = -1;
  if (out) {
    rank = 0;
    for (int j = 0; j < nb; ++j)
      if (j != tid && s_scan[j] == j && nxt[j].score >= thr && better(nxt[j].score, j, nxt[tid].score, tid)) ++rank;
  }
  const int nout = min(a.topk, block_sum_int(out ? 1 : 0, s_red));
  if (rank >= 0 && rank < a.topk) {
    int32_t* path = a.out_tokens + ((size_t)b * a.topk + rank) * a.T;
    int slot = nxt[tid].rec;
    for (int t = a.T - 1; t >= 0; --t) {
      if (t < len && fpb[t] && slot >= 0 && slot < a.beam) {  // (a record's parent is always a live slot)
        const int rec = bpb[(size_t)t * a.beam + slot];
        path[t] = (rec & 0xffff) == kNoToken ? -1 : (rec & 0xffff);
        slot = rec >> 16;
      } else {
        path[t] = -1;
      }
    }
    a.out_score[(size_t)b * a.topk + rank] = nxt[tid].score;
  }
  if (tid == 0) {
    a.out_count[b] = bad_len ? -1 : nout;
    int32_t* st = a.stats + (size_t)b * 4;
    st[0] = st_done, st[1] = st_skip, st[2] = st_ext, st[3] = st_ws;
  }
}

}  // namespace

}  // namespace sbk

using namespace sbk;

static long pfx_ws_cap(int V, int Vl, int beam) { return (long)beam * ((V < Vl ? V : Vl) + 1); }

extern "C" size_t sbk_ctc_prefix_beam_search_workspace_bytes(int B, int T, int V, int Vl, int beam, int topk) {
  (void)topk;
  if (B <= 0 || T <= 0 || V <= 0 || Vl <= 0 || beam <= 0) return 0;
  const size_t per_utt = ((size_t)T * beam + T + 4) * sizeof(int32_t);
  const size_t items = (pfx_frame_bytes(pfx_ws_cap(V, Vl, beam)) + 15) / 16 * 16;
  return ((size_t)B * per_utt + 15) / 16 * 16 + (size_t)B * items;
}

extern "C" int sbk_ctc_prefix_beam_search_f32(const float* x, const float* rel_len, const int32_t* token_table, int Vl,
                                              const sbk_ctc_beam_config* cfg, void* workspace, size_t workspace_bytes,
                                              int32_t* out_tokens, float* out_score, int32_t* out_count, int B, int T,
                                              int V, sbk_stream_t stream) {
  if (B == 0) return 0;
  SBK_REQUIRE(cfg, "ctc_prefix_beam_search: cfg is NULL");
  SBK_REQUIRE(x && token_table && workspace && out_tokens && out_score && out_count && B > 0 && T > 0 && V > 0,
              "ctc_prefix_beam_search: bad arguments (B=%d T=%d V=%d)", B, T, V);
  SBK_REQUIRE(Vl > 0 && Vl <= V && V <= 65535,
              "ctc_prefix_beam_search: vocabulary of %d tokens for V=%d (1 <= len <= V <= 65535)", Vl, V);
  SBK_REQUIRE(cfg->blank >= 0 && cfg->blank < V, "ctc_prefix_beam_search: blank %d outside [0, %d)", cfg->blank, V);
  SBK_REQUIRE(cfg->beam_size >= 1 && cfg->beam_size <= kPfxBeamMax,
              "ctc_prefix_beam_search: beam_size %d is not supported (1..%d: the beam lives in one workgroup's LDS)",
              cfg->beam_size, kPfxBeamMax);
  SBK_REQUIRE(cfg->topk >= 1 && cfg->topk <= cfg->beam_size, "ctc_prefix_beam_search: topk %d outside [1, beam_size]",
              cfg->topk);
  SBK_REQUIRE(cfg->beam_prune_logp <= 0.0f, "ctc_prefix_beam_search: beam_prune_logp %g above 0 leaves no beam",
              (double)cfg->beam_prune_logp);
  const size_t need = sbk_ctc_prefix_beam_search_workspace_bytes(B, T, V, Vl, cfg->beam_size, cfg->topk);
  SBK_REQUIRE(workspace_bytes >= need, "ctc_prefix_beam_search: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  SBK_REQUIRE(aligned16(workspace), "ctc_prefix_beam_search: workspace must be 16-byte aligned");
  SBK_REQUIRE(cfg->char_base1 < kHashMod && cfg->char_base2 < kHashMod && cfg->space_code < kHashMod,
              "ctc_prefix_beam_search: hash constants >= 2^31-1");
  PfxArgs a;
  a.x = x, a.rel = rel_len, a.table = token_table;
  a.bp = static_cast<int32_t*>(workspace);
  a.fproc = a.bp + (size_t)B * T * cfg->beam_size;
  a.stats = a.fproc + (size_t)B * T;
  const size_t per_utt = ((size_t)T * cfg->beam_size + T + 4) * sizeof(int32_t);
  a.items = static_cast<unsigned char*>(workspace) + ((size_t)B * per_utt + 15) / 16 * 16;
  a.ws_cap = (int)pfx_ws_cap(V, Vl, cfg->beam_size);
  a.item_bytes = (pfx_frame_bytes(a.ws_cap) + 15) / 16 * 16;
  a.lds_cap = a.ws_cap < kPfxLdsItems ? pow2_ceil(a.ws_cap) : kPfxLdsItems;
  a.out_tokens = out_tokens, a.out_score = out_score, a.out_count = out_count;
  a.T = T, a.V = V, a.Vl = Vl, a.blank = cfg->blank, a.beam = cfg->beam_size, a.topk = cfg->topk;
  a.prune_history = cfg->prune_history;
  a.beam_prune_logp = cfg->beam_prune_logp, a.token_min_logp = cfg->token_prune_min_logp;
  a.blank_skip_logp = cfg->log_blank_skip_threshold;
  a.sp1 = cfg->char_base1, a.sp2 = cfg->char_base2, a.space_code = cfg->space_code;
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)2 * cfg->beam_size * sizeof(PfxBeam) + pfx_frame_bytes(a.lds_cap);
  if (allow_dyn_lds(ctc_prefix_kernel, lds) != hipSuccess)
    return fail(SBK_EINVAL, "ctc_prefix_beam_search: %zu bytes of LDS for beam_size %d not available", lds, cfg->beam_size);
  ProfScope prof("ctc_prefix_beam_search", 0.0, 4.0 * B * T * V + 4.0 * B * T * cfg->beam_size, st);
  SBK_LAUNCH(ctc_prefix_kernel, dim3(B), dim3(kPfxThreads), lds, st, a);
  return launch_status("ctc_prefix_beam_search");
}
