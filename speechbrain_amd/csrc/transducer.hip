// Transducer greedy decoding on the device: TransducerBeamSearcher.transducer_greedy_decode (decoders/transducer.py:156-291)
// for the prediction network [Embedding, LSTM, Linear], Transducer_joint(joint="sum") and one classifier Linear.  One
// workgroup per utterance runs every frame in ONE launch with the utterance's PN state in LDS; the weights stream from L2.
// The semantics reproduced here are listed in DESIGN.md section 5 ("Transducer greedy decoding").  Further down: the beam
// search of the same class (transducer_beam_search_decode, decoders/transducer.py:320-476) on the same step code, without an LM
// and with an RNNLM (lobes/models/RNNLM.py) fused into the scores.
#include <math.h>
#include <string.h>

#include "act.h"
#include "argmax.h"
#include "common.h"
#include "device.h"

namespace sbk {

namespace {

constexpr int kTdThreads = 512;
constexpr int kTdFrameMax = 8;       // frames whose joint shares one pass over the classifier's weights
constexpr int kTdFrameDefault = 8;
constexpr size_t kTdLdsMax = 160 * 1024;
// static LDS of the search kernel (s_dec, s_lp, s_first), which shares the 160 KiB with the dynamic window
constexpr size_t kTdStaticLds = 2 * kTdFrameMax * sizeof(float) + 16;
constexpr size_t kTdDynLdsMax = kTdLdsMax - kTdStaticLds;

// layer l's pointer from a per-layer array of the weights struct: a switch keeps the runtime index out of private memory
__device__ __forceinline__ const float* layer_ptr(const float* const (&p)[SBK_TRANSDUCER_MAX_LAYERS], int l) {
  static_assert(SBK_TRANSDUCER_MAX_LAYERS == 4, "layer_ptr covers four layers");
  switch (l) {
    case 0: return p[0];
    case 1: return p[1];
    case 2: return p[2];
    default: return p[3];
  }
}

struct TdArgs {
  sbk_transducer_weights W;
  const float* tn;  // [B,T,J]
  float* out_pn;    // [B,J]
  float* h;         // [L,B,H]
  float* c;         // [L,B,H]
  int32_t* tokens;  // [B,cap]
  int32_t* count;   // [B]
  float* score;     // [B]
  int B, T, F, S, blank, act, start;
};

// out[f * ldo + n] = bias[n] + sum_k w[n][k] * x[f * ldx + k] for f < nx, n < N; w [N][K] row-major (torch's layout), x in
// LDS.  One wave per group of R rows, lanes across k (float4 loads of w when K % 4 == 0), then a fixed butterfly: every
// output has one summation order whatever nx is.  Latency-bound at these sizes, so R rows' loads are issued together.
template <int NX, int R>
__device__ __forceinline__ void gemv_rows(const float* __restrict__ w, const float* __restrict__ bias, const float* x, int ldx,
                                          int nx, int K, int N, float* out, int ldo) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool vec = (K & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0;
  for (int n0 = wave * R; n0 < N; n0 += (kTdThreads / 64) * R) {
    float acc[R][NX];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int f = 0; f < NX; ++f) acc[r][f] = 0.0f;
    if (vec) {
      for (int k0 = lane * 4; k0 < K; k0 += 256) {
        float4 wv[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
          wv[r] = n0 + r < N ? *reinterpret_cast<const float4*>(w + (size_t)(n0 + r) * K + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int f = 0; f < NX; ++f) {
          if (f >= nx) break;
          const float* xf = x + (size_t)f * ldx + k0;
          const float x0 = xf[0], x1 = xf[1], x2 = xf[2], x3 = xf[3];
#pragma unroll
          for (int r = 0; r < R; ++r)
            acc[r][f] = fmaf(wv[r].w, x3, fmaf(wv[r].z, x2, fmaf(wv[r].y, x1, fmaf(wv[r].x, x0, acc[r][f]))));
        }
      }
    } else {
      for (int k = lane; k < K; k += 64) {
        float wv[R];
#pragma unroll
        for (int r = 0; r < R; ++r) wv[r] = n0 + r < N ? w[(size_t)(n0 + r) * K + k] : 0.0f;
#pragma unroll
        for (int f = 0; f < NX; ++f) {
          if (f >= nx) break;
          const float xk = x[(size_t)f * ldx + k];
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r][f] = fmaf(wv[r], xk, acc[r][f]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int f = 0; f < NX; ++f) {
        if (f >= nx) break;
        float v = acc[r][f];
        for (int m = 32; m >= 1; m >>= 1) v += shfl_xor(v, m);  // (sbk::wave_sum; its unroll pragma changes the greedy kernel's code)
        if (lane == 0 && n0 + r < N) out[(size_t)f * ldo + n0 + r] = bias ? v + bias[n0 + r] : v;
      }
    }
  }
}

// The cell update of one LSTM step from the gates' input part s_g and recurrent part s_gh (torch gate order i, f, g, o).
__device__ __forceinline__ void lstm_update(const float* s_g, const float* s_gh, float* hl, float* cl, int H) {
  for (int m = threadIdx.x; m < H; m += kTdThreads) {
    const float ig = sbk::sigmoid(s_g[m] + s_gh[m]);
    const float fg = sbk::sigmoid(s_g[H + m] + s_gh[H + m]);
    const float gg = tanhf(s_g[2 * H + m] + s_gh[2 * H + m]);
    const float og = sbk::sigmoid(s_g[3 * H + m] + s_gh[3 * H + m]);
    const float cn = fg * cl[m] + ig * gg;
    cl[m] = cn;
    hl[m] = og * tanhf(cn);
  }
}

// One PN step on token `tok`: every LSTM layer, then proj_dec into s_pn.  Ends with a barrier.
__device__ void pn_step(const TdArgs& a, int tok, float* s_pn, float* s_h, float* s_c, float* s_g, float* s_gh) {
  const sbk_transducer_weights& W = a.W;
  const int H = W.hidden, G = 4 * H, tid = threadIdx.x;
  for (int l = 0; l < W.n_layers; ++l) {
    float* hl = s_h + (size_t)l * H;
    float* cl = s_c + (size_t)l * H;
    // input part: the folded embedding row (layer 0) or W_ih_l . h_{l-1}
    if (l == 0) {
      const float* row = W.emb_ih + (size_t)tok * G;
      for (int n = tid; n < G; n += kTdThreads) s_g[n] = W.b_ih[0] ? row[n] + W.b_ih[0][n] : row[n];
    } else {
      gemv_rows<1, 8>(layer_ptr(W.w_ih, l), layer_ptr(W.b_ih, l), s_h + (size_t)(l - 1) * H, H, 1, H, G, s_g, G);
    }
    gemv_rows<1, 8>(layer_ptr(W.w_hh, l), layer_ptr(W.b_hh, l), hl, H, 1, H, G, s_gh, G);
    __syncthreads();
    lstm_update(s_g, s_gh, hl, cl, H);
    __syncthreads();
  }
  gemv_rows<1, 8>(W.proj, W.proj_b, s_h + (size_t)(W.n_layers - 1) * H, H, 1, H, W.joint, s_pn, W.joint);
  __syncthreads();
}

// The statistics of one wave's log-softmax over x[0..V): the log-probability of entry v is (x[v] - m) - ls.  Every lane of the
// wave calls it; the greedy and the beam search share it, so both see the same bits.
__device__ __forceinline__ void log_softmax_stats(const float* x, int V, float& m, float& ls) {
  const int lane = threadIdx.x & 63;
  m = -INFINITY;
  for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
  m = sbk::wave_max(m);
  float se = 0.0f;
  for (int v = lane; v < V; v += 64) se += expf(x[v] - m);
  se = sbk::wave_sum(se);
  ls = logf(se);
}

// block i's pointer from a per-block array of the RNNLM's struct (the same reason as layer_ptr)
__device__ __forceinline__ const float* dnn_ptr(const float* const (&p)[SBK_RNNLM_MAX_DNN], int i) {
  static_assert(SBK_RNNLM_MAX_DNN == 2, "dnn_ptr covers two blocks");
  return i == 0 ? p[0] : p[1];
}

// One RNNLM step on token `tok` (lobes/models/RNNLM.py forward at inference): the folded embedding row, every LSTM layer on
// s_h / s_c, the DNN blocks [Linear + bias, LayerNorm (two-pass mean / variance), activation] through s_d0 / s_d1, and the
// output Linear into s_out [vocab].  s_g / s_gh hold 4 * hidden floats each; s_stat two.  The products are pn_step's (8 rows
// per wave; with 16 the kernel spilled three times as much to scratch).  Ends with a barrier.
__device__ void lm_step(const sbk_rnnlm_weights& M, int tok, float* s_h, float* s_c, float* s_g, float* s_gh, float* s_d0,
                        float* s_d1, float* s_out, float* s_stat) {
  const int H = M.hidden, G = 4 * H, D = M.dnn, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int l = 0; l < M.n_layers; ++l) {
    float* hl = s_h + (size_t)l * H;
    float* cl = s_c + (size_t)l * H;
    if (l == 0) {
      const float* row = M.emb_ih + (size_t)tok * G;
      for (int n = tid; n < G; n += kTdThreads) s_g[n] = M.b_ih[0] ? row[n] + M.b_ih[0][n] : row[n];
    } else {
      gemv_rows<1, 8>(layer_ptr(M.w_ih, l), layer_ptr(M.b_ih, l), s_h + (size_t)(l - 1) * H, H, 1, H, G, s_g, G);
    }
    gemv_rows<1, 8>(layer_ptr(M.w_hh, l), layer_ptr(M.b_hh, l), hl, H, 1, H, G, s_gh, G);
    __syncthreads();
    lstm_update(s_g, s_gh, hl, cl, H);
    __syncthreads();
  }
  const float* x = s_h + (size_t)(M.n_layers - 1) * H;
  int K = H;
  for (int i = 0; i < M.n_dnn; ++i) {
    float* y = i == 0 ? s_d0 : s_d1;
    gemv_rows<1, 8>(dnn_ptr(M.dnn_w, i), dnn_ptr(M.dnn_b, i), x, K, 1, K, D, y, D);
    __syncthreads();
    if (wave == 0) {
      float s = 0.0f;
      for (int k = lane; k < D; k += 64) s += y[k];
      s = sbk::wave_sum(s);
      const float mean = s / (float)D;
      float q = 0.0f;
      for (int k = lane; k < D; k += 64) q += (y[k] - mean) * (y[k] - mean);
      q = sbk::wave_sum(q);
      if (lane == 0) s_stat[0] = mean, s_stat[1] = 1.0f / sqrtf(q / (float)D + (i == 0 ? M.ln_eps[0] : M.ln_eps[1]));
    }
    __syncthreads();
    const float mean = s_stat[0], rstd = s_stat[1];
    const float* g = dnn_ptr(M.ln_g, i);
    const float* be = dnn_ptr(M.ln_b, i);
    for (int k = tid; k < D; k += kTdThreads) y[k] = sbk::joint_act((y[k] - mean) * rstd * g[k] + be[k], M.act);
    __syncthreads();
    x = y, K = D;
  }
  gemv_rows<1, 8>(M.out, M.out_b, x, K, 1, K, M.vocab, s_out, M.vocab);
  __syncthreads();
}

__global__ __launch_bounds__(kTdThreads) void transducer_greedy_kernel(TdArgs a) {
  SBK_DYN_LDS(float, lds);
  const sbk_transducer_weights& W = a.W;
  const int H = W.hidden, G = 4 * H, J = W.joint, V = W.vocab, L = W.n_layers, F = a.F;
  float* s_z = lds;                          // [F][J] joint activations of the block
  float* s_logit = s_z + (size_t)F * J;      // [F][V]
  float* s_pn = s_logit + (size_t)F * V;     // [J]
  float* s_h = s_pn + J;                     // [L][H]
  float* s_c = s_h + (size_t)L * H;          // [L][H]
  float* s_g = s_c + (size_t)L * H;          // [G] input part of the gates
  float* s_gh = s_g + G;                     // [G] recurrent part
  __shared__ int s_dec[kTdFrameMax];
  __shared__ float s_lp[kTdFrameMax];
  __shared__ int s_first;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cap = a.T * (a.S + 1);
  const float* tnb = a.tn + (size_t)b * a.T * J;
  int32_t* tok_out = a.tokens + (size_t)b * cap;

  if (a.start) {
    for (int i = tid; i < L * H; i += kTdThreads) s_h[i] = 0.0f, s_c[i] = 0.0f;
    __syncthreads();
    pn_step(a, a.blank, s_pn, s_h, s_c, s_g, s_gh);
  } else {
    for (int j = tid; j < J; j += kTdThreads) s_pn[j] = a.out_pn[(size_t)b * J + j];
    for (int i = tid; i < L * H; i += kTdThreads) {
      const int l = i / H, m = i - l * H;
      s_h[i] = a.h[((size_t)l * a.B + b) * H + m];
      s_c[i] = a.c[((size_t)l * a.B + b) * H + m];
    }
    __syncthreads();
  }

  int t = 0, emitted = 0, n = 0;
  float score = 0.0f;
  while (t < a.T) {
    const int fe = min(F, a.T - t);
    // 1. joint activations act(tn[t + f] + out_PN) of the block's frames
    for (int i = tid; i < fe * J; i += kTdThreads) {
      const int f = i / J, k = i - f * J;
      s_z[i] = sbk::joint_act(tnb[(size_t)(t + f) * J + k] + s_pn[k], a.act);
    }
    __syncthreads();
    // 2. logits: one pass over the classifier's weights for the whole block
    gemv_rows<kTdFrameMax, 2>(W.out, W.out_b, s_z, J, fe, J, V, s_logit, V);
    __syncthreads();
    // 3. log-softmax and arg-max of each frame (one wave per frame)
    for (int f = wave; f < fe; f += kTdThreads / 64) {
      const float* x = s_logit + (size_t)f * V;
      float m, ls;
      log_softmax_stats(x, V, m, ls);
      float bv = NAN;
      int bi = 0x7fffffff;
      for (int v = lane; v < V; v += 64) {
        const float lp = (x[v] - m) - ls;
        if (bi == 0x7fffffff || arg_better(lp, v, bv, bi)) bv = lp, bi = v;
      }
      for (int s = 32; s >= 1; s >>= 1) {
        const float w = shfl_xor(bv, s);
        const int j = shfl_xor(bi, s);
        if (j != 0x7fffffff && (bi == 0x7fffffff || arg_better(w, j, bv, bi))) bv = w, bi = j;
      }
      if (lane == 0) s_dec[f] = bi, s_lp[f] = bv;
    }
    __syncthreads();
    if (tid == 0) {
      int first = fe;
      for (int f = 0; f < fe; ++f)
        if (s_dec[f] != a.blank) {
          first = f;
          break;
        }
      s_first = first;
    }
    __syncthreads();
    const int first = s_first;
    if (first == fe) {  // every frame of the block emits blank
      t += fe;
      emitted = 0;
      continue;
    }
    if (first > 0) t += first, emitted = 0;
    const int tok = s_dec[first];
    if (tid == 0 && n < cap) tok_out[n] = tok;
    ++n;
    score += s_lp[first];
    ++emitted;
    pn_step(a, tok, s_pn, s_h, s_c, s_g, s_gh);
    if (emitted > a.S) t += 1, emitted = 0;  // the frame's max_symbols_per_step + 1 emissions are spent
  }

  for (int j = tid; j < J; j += kTdThreads) a.out_pn[(size_t)b * J + j] = s_pn[j];
  for (int i = tid; i < L * H; i += kTdThreads) {
    const int l = i / H, m = i - l * H;
    a.h[((size_t)l * a.B + b) * H + m] = s_h[i];
    a.c[((size_t)l * a.B + b) * H + m] = s_c[i];
  }
  if (tid == 0) a.count[b] = min(n, cap), a.score[b] = score;
}

// One unidirectional LSTM layer over a whole sequence: xp [B,T,G] = x . W_ih^T (the input part, without bias), state h / c
// [B,H] read and overwritten, out [B,T,H].  One workgroup per sequence, the state in LDS.
__global__ __launch_bounds__(kTdThreads) void lstm_layer_kernel(const float* __restrict__ xp, const float* __restrict__ w_hh,
                                                         const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                                         float* h, float* c, float* out, int T, int H) {
  SBK_DYN_LDS(float, lds);
  const int G = 4 * H, b = blockIdx.x, tid = threadIdx.x;
  float* s_h = lds;
  float* s_c = s_h + H;
  float* s_g = s_c + H;
  float* s_gh = s_g + G;
  for (int m = tid; m < H; m += kTdThreads) s_h[m] = h[(size_t)b * H + m], s_c[m] = c[(size_t)b * H + m];
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float* row = xp + ((size_t)b * T + t) * G;
    for (int n = tid; n < G; n += kTdThreads) s_g[n] = b_ih ? row[n] + b_ih[n] : row[n];
    gemv_rows<1, 8>(w_hh, b_hh, s_h, H, 1, H, G, s_gh, G);
    __syncthreads();
    lstm_update(s_g, s_gh, s_h, s_c, H);
    __syncthreads();
    for (int m = tid; m < H; m += kTdThreads) out[((size_t)b * T + t) * H + m] = s_h[m];
  }
  for (int m = tid; m < H; m += kTdThreads) h[(size_t)b * H + m] = s_h[m], c[(size_t)b * H + m] = s_c[m];
}

// ------------------------------------------------------------------------------------------------------------ beam search
// TransducerBeamSearcher.transducer_beam_search_decode (decoders/transducer.py:320-476) without an LM; the rules are listed in
// DESIGN.md section 5 ("Transducer beam search").  One workgroup per utterance.  The lists A and B of a frame live in LDS; the
// token tree and the PN states (with the PN outputs they produced) live in the caller's workspace.
struct TbHyp {
  int node;     // the hypothesis' node of the utterance's token tree (parent, token)
  int tok;      // its last token: the PN's next input
  float score;  // logp_score
  int len;      // len(prediction), the leading blank included
  int state;    // the slot whose h / c are hidden_dec (-1: zeros)
  int pn;       // the slot that holds this (tok, state)'s PN step already (-1: not computed yet)
  int stamp;    // list order: the order of the appends
};

struct TbArgs {
  TdArgs g;      // W and tn (what pn_step reads)
  int2* nodes;   // [B][node_cap] (parent, token)
  float* slots;  // [B][n_slots][slot_floats]: out_PN [J], h [L*H], c [L*H] after one PN step
  int32_t* expansions;  // [B]
  int32_t* out_tokens;  // [B][nbest][max_tokens]
  int32_t* out_len;     // [B][nbest]
  float* out_score;     // [B][nbest]
  int32_t* out_count;   // [B]
  int32_t* out_status;  // [B]
  int beam, nbest, max_exp, max_tokens, cap_a, n_slots, slot_floats, node_cap;
  float state_beam, expand_beam;
  // LM fusion (read by the LM instantiation only): a slot then also holds the LM's h / c [LM.n_layers * LM.hidden] each after
  // the step and its log-probabilities over the classifier's V tokens
  sbk_rnnlm_weights lm;
  float lm_weight;
  int gmax;            // floats of each gate buffer: 4 * max(PN hidden, LM hidden)
  int32_t* lm_steps;   // [B]
};

// The sort key logp_score / len(prediction): an fp32 division.  (A NaN key ranks below everything, so that a search over
// non-finite inputs still picks one hypothesis.)
__device__ __forceinline__ float tb_key(const TbHyp& h) {
  const float k = h.score / (float)h.len;
  return isnan(k) ? -INFINITY : k;
}

// The index of the first maximal key of list[0..n), n > 0, in list order (the smallest stamp).  Every lane of one wave calls it.
__device__ __forceinline__ int tb_best(const TbHyp* list, int n) {
  const int lane = threadIdx.x & 63;
  float bk = -INFINITY;
  int bs = 0x7fffffff, bi = -1;
  for (int i = lane; i < n; i += 64) {
    const float k = tb_key(list[i]);
    const int s = list[i].stamp;
    if (bi < 0 || k > bk || (k == bk && s < bs)) bk = k, bs = s, bi = i;
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const float k = shfl_xor(bk, m);
    const int s = shfl_xor(bs, m), i = shfl_xor(bi, m);
    if (i >= 0 && (bi < 0 || k > bk || (k == bk && s < bs))) bk = k, bs = s, bi = i;
  }
  return bi;
}

// LM: shallow fusion with an RNNLM (rules 8-10 of that section); the instantiation without it is the search as it was.
template <bool LM>
__global__ __launch_bounds__(kTdThreads) void transducer_beam_kernel(TbArgs a) {
  SBK_DYN_LDS(float, lds);
  const sbk_transducer_weights& W = a.g.W;
  const int H = W.hidden, G = 4 * H, J = W.joint, V = W.vocab, L = W.n_layers, LH = L * H;
  const int GM = LM ? a.gmax : G;                            // the gate buffers serve pn_step and lm_step
  const int LLH = LM ? a.lm.n_layers * a.lm.hidden : 0;      // the LM's h (and c) of one state
  float* s_z = lds;             // [J] joint activations
  float* s_logit = s_z + J;     // [V]
  float* s_pn = s_logit + V;    // [J]
  float* s_h = s_pn + J;        // [L][H]
  float* s_c = s_h + LH;        // [L][H]
  float* s_g = s_c + LH;        // [GM]
  float* s_gh = s_g + GM;       // [GM]
  float* s_lh = s_gh + GM;      // LM only: [LM layers][LM hidden]
  float* s_lc = s_lh + LLH;     //          the same
  float* s_d0 = s_lc + LLH;     //          [dnn], [dnn]: the DNN blocks' outputs
  float* s_d1 = s_d0 + (LM ? a.lm.dnn : 0);
  float* s_lout = s_d1 + (LM ? a.lm.dnn : 0);       //   [LM vocab] the LM's logits
  float* s_topv = s_lout + (LM ? a.lm.vocab : 0);   // [beam] the top-k log-probabilities of an expansion ...
  int* s_topi = reinterpret_cast<int*>(s_topv + a.beam);  // [beam] ... and their tokens
  float* s_toplm = reinterpret_cast<float*>(s_topi + a.beam);  // LM only: [beam] the LM's log-probabilities of those tokens
  int* s_used = reinterpret_cast<int*>(s_toplm + (LM ? a.beam : 0));  // [n_slots] slot is referenced by a hypothesis of this frame
  TbHyp* A = reinterpret_cast<TbHyp*>(s_used + a.n_slots);  // [cap_a]
  TbHyp* Bl = A + a.cap_a;                                  // [beam]
  __shared__ int s_na, s_nb, s_act, s_slot, s_status, s_nodes, s_stamp, s_total, s_lmn;
  __shared__ TbHyp s_cur;
  __shared__ float s_stat[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blank = a.g.blank;
  const int o_lh = J + 2 * LH, o_lc = o_lh + LLH, o_lp = o_lc + LLH;  // a slot's LM part: h, c, log-probabilities [V]
  const float* tnb = a.g.tn + (size_t)b * a.g.T * J;
  int2* nodes = a.nodes + (size_t)b * a.node_cap;
  float* slots = a.slots + (size_t)b * a.n_slots * a.slot_floats;

  if (tid == 0) {
    nodes[0] = make_int2(-1, blank);
    A[0] = TbHyp{0, blank, 0.0f, 1, -1, -1, 0};
    s_na = 1, s_nb = 0, s_status = 0, s_nodes = 1, s_stamp = 1, s_total = 0, s_lmn = 0;
  }
  __syncthreads();

  for (int t = 0; t < a.g.T; ++t) {
    if (t > 0) {  // A = the previous B, B = {}
      const int n = s_nb;
      for (int i = tid; i < n; i += kTdThreads) A[i] = Bl[i];
      __syncthreads();
      if (tid == 0) s_na = n, s_nb = 0;
    }
    for (int i = tid; i < a.n_slots; i += kTdThreads) s_used[i] = 0;
    __syncthreads();
    for (int i = tid; i < s_na; i += kTdThreads) {
      if (A[i].state >= 0) s_used[A[i].state] = 1;
      if (A[i].pn >= 0) s_used[A[i].pn] = 1;
    }
    __syncthreads();

    int n_exp = 0;
    while (true) {
      // ---- the three exits and the selection (wave 0; lane 0 decides)
      if (wave == 0) {
        const int na = s_na, nb = s_nb;
        const int ai = na > 0 ? tb_best(A, na) : -1;
        const int bi = nb > 0 ? tb_best(Bl, nb) : -1;
        int fr = 0x7fffffff;  // the first free slot
        for (int i = lane; i < a.n_slots; i += 64)
          if (!s_used[i]) {
            fr = i;
            break;
          }
        for (int m = 32; m >= 1; m >>= 1) fr = min(fr, shfl_xor(fr, m));
        if (lane == 0) {
          int act = 0;
          if (nb < a.beam && ai >= 0 && !(bi >= 0 && Bl[bi].score >= a.state_beam + A[ai].score)) {
            if (n_exp >= a.max_exp || (A[ai].pn < 0 && fr == 0x7fffffff))
              s_status |= SBK_TBEAM_CAPPED;  // (n_slots covers max_exp new states per frame: the second test never holds)
            else
              act = 1;
          }
          if (act) {
            s_cur = A[ai];
            s_slot = A[ai].pn >= 0 ? A[ai].pn : fr;
            s_used[s_slot] = 1;
            A[ai] = A[na - 1];  // (list order is the stamps')
            s_na = na - 1;
          }
          s_act = act;
        }
      }
      __syncthreads();
      if (!s_act) break;

      // ---- one PN step on a_best's last token from its state, or the copy an earlier expansion of the same pair left
      const TbHyp cur = s_cur;
      const int slot = s_slot;
      float* sl = slots + (size_t)slot * a.slot_floats;
      if (cur.pn >= 0) {
        for (int j = tid; j < J; j += kTdThreads) s_pn[j] = sl[j];
        __syncthreads();
      } else {
        if (cur.state >= 0) {
          const float* src = slots + (size_t)cur.state * a.slot_floats + J;
          for (int i = tid; i < LH; i += kTdThreads) s_h[i] = src[i], s_c[i] = src[LH + i];
          if constexpr (LM) {
            const float* lsrc = slots + (size_t)cur.state * a.slot_floats;
            for (int i = tid; i < LLH; i += kTdThreads) s_lh[i] = lsrc[o_lh + i], s_lc[i] = lsrc[o_lc + i];
          }
        } else {
          for (int i = tid; i < LH; i += kTdThreads) s_h[i] = 0.0f, s_c[i] = 0.0f;
          if constexpr (LM)
            for (int i = tid; i < LLH; i += kTdThreads) s_lh[i] = 0.0f, s_lc[i] = 0.0f;
        }
        __syncthreads();
        pn_step(a.g, cur.tok, s_pn, s_h, s_c, s_g, s_gh);
        for (int j = tid; j < J; j += kTdThreads) sl[j] = s_pn[j];
        for (int i = tid; i < LH; i += kTdThreads) sl[J + i] = s_h[i], sl[J + LH + i] = s_c[i];
        if constexpr (LM) {
          // the LM moves with the PN: the same input token, the same slot; its log-softmax runs over its whole output
          lm_step(a.lm, cur.tok, s_lh, s_lc, s_g, s_gh, s_d0, s_d1, s_lout, s_stat);
          for (int i = tid; i < LLH; i += kTdThreads) sl[o_lh + i] = s_lh[i], sl[o_lc + i] = s_lc[i];
          if (wave == 0) {
            float m, ls;
            log_softmax_stats(s_lout, a.lm.vocab, m, ls);
            for (int v = lane; v < V; v += 64) sl[o_lp + v] = (s_lout[v] - m) - ls;
            if (lane == 0) s_lmn = s_lmn + 1;
          }
          __syncthreads();
        }
      }
      // ---- the joint with tn[b, t], the classifier, log-softmax and top-k
      const float* tnf = tnb + (size_t)t * J;
      for (int k = tid; k < J; k += kTdThreads) s_z[k] = sbk::joint_act(tnf[k] + s_pn[k], a.g.act);
      __syncthreads();
      gemv_rows<1, 8>(W.out, W.out_b, s_z, J, 1, J, V, s_logit, V);
      __syncthreads();
      if (wave == 0) {
        float m, ls;
        log_softmax_stats(s_logit, V, m, ls);
        float pv = 0.0f;
        int pi = -1;  // the previous pick: round r takes the best of what ranks below it (torch.topk's order)
        for (int r = 0; r < a.beam; ++r) {
          float bv = NAN;
          int bi = 0x7fffffff;
          for (int v = lane; v < V; v += 64) {
            const float lp = (s_logit[v] - m) - ls;
            if (pi >= 0 && !arg_better(pv, pi, lp, v)) continue;
            if (bi == 0x7fffffff || arg_better(lp, v, bv, bi)) bv = lp, bi = v;
          }
          for (int s = 32; s >= 1; s >>= 1) {
            const float w = shfl_xor(bv, s);
            const int j = shfl_xor(bi, s);
            if (j != 0x7fffffff && (bi == 0x7fffffff || arg_better(w, j, bv, bi))) bv = w, bi = j;
          }
          pv = bv, pi = bi;
          if (lane == 0) s_topv[r] = bv, s_topi[r] = bi;
        }
        if constexpr (LM) {  // the LM's log-probabilities of the picks, from the slot (this step's or the cached one's)
          wave_sync();
          for (int r = lane; r < a.beam; r += 64) {
            const int ti = s_topi[r];
            s_toplm[r] = (unsigned)ti < (unsigned)V ? sl[o_lp + ti] : 0.0f;
          }
          wave_sync();
        }
        // ---- the candidates in top-k order: blank joins B with the old state, the others join A with the new one
        if (lane == 0) {
          const float best = s_topi[0] != blank ? s_topv[0] : s_topv[1];
          const float thr = best - a.expand_beam;
          int na = s_na, nb = s_nb, nn = s_nodes, st = s_stamp;
          for (int j = 0; j < a.beam; ++j) {
            const float lp = s_topv[j];
            const int tok = s_topi[j];
            if (tok == blank) {
              if (nb < a.beam) Bl[nb++] = TbHyp{cur.node, cur.tok, cur.score + lp, cur.len, cur.state, slot, st++};
            } else if (lp >= thr && na < a.cap_a && nn < a.node_cap) {
              nodes[nn] = make_int2(cur.node, tok);
              float sc = cur.score + lp;
              if constexpr (LM) sc = add_rn(sc, mul_rn(a.lm_weight, s_toplm[j]));  // (product rounded, then added: no fma)
              A[na++] = TbHyp{nn++, tok, sc, cur.len + 1, slot, -1, st++};
            }
          }
          s_na = na, s_nb = nb, s_nodes = nn, s_stamp = st, s_total = s_total + 1;
        }
      }
      ++n_exp;
      __syncthreads();
    }

    // ---- a frame that stopped with an empty B (the cap, or non-finite scores): the beam best of A go on as they are
    if (wave == 0 && s_nb == 0) {
      int na = s_na, nb = 0;
      if (na == 0) {
        if (lane == 0) Bl[0] = s_cur, s_status |= SBK_TBEAM_EXHAUSTED;
        nb = 1;
      }
      for (; nb < a.beam && na > 0; ++nb, --na) {
        const int i = tb_best(A, na);
        if (lane == 0) Bl[nb] = A[i], A[i] = A[na - 1];
        wave_sync();
      }
      wave_sync();
      if (lane == 0) s_na = na, s_nb = nb;
    }
    __syncthreads();
  }

  // ---- B sorted by key (descending, stable: list order among equal keys), the first nbest of it
  int count = 0;
  if (wave == 0) {
    int nb = s_nb;
    for (; count < a.nbest && nb > 0; ++count, --nb) {
      const int i = tb_best(Bl, nb);
      if (lane == 0) A[count] = Bl[i], Bl[i] = Bl[nb - 1];
      wave_sync();
    }
    if (lane == 0) s_act = count;
  }
  __syncthreads();
  count = s_act;
  for (int r = tid; r < a.nbest; r += kTdThreads) {
    const size_t row = (size_t)b * a.nbest + r;
    if (r >= count) {
      a.out_len[row] = 0, a.out_score[row] = 0.0f;
      continue;
    }
    const TbHyp h = A[r];
    const int n = h.len - 1;  // without the leading blank
    a.out_len[row] = min(n, a.max_tokens);
    a.out_score[row] = h.score / (float)h.len;
    int32_t* dst = a.out_tokens + row * a.max_tokens;
    int node = h.node;
    for (int p = n - 1; p >= 0 && node > 0; --p) {
      const int2 e = nodes[node];
      if (p < a.max_tokens) dst[p] = e.y;
      node = e.x;
    }
  }
  if (tid == 0) {
    int status = s_status;
    for (int r = 0; r < count; ++r)
      if (A[r].len - 1 > a.max_tokens) status |= SBK_TBEAM_TRUNCATED;
    a.out_count[b] = count, a.out_status[b] = status, a.expansions[b] = s_total;
    if constexpr (LM) a.lm_steps[b] = s_lmn;
  }
}

size_t td_lds_bytes(const sbk_transducer_weights& W, int F) {
  return sizeof(float) * ((size_t)F * W.joint + (size_t)F * W.vocab + W.joint + 2 * (size_t)W.n_layers * W.hidden +
                          8 * (size_t)W.hidden);
}

}  // namespace

}  // namespace sbk

using namespace sbk;

extern "C" int sbk_transducer_greedy_f32(const sbk_transducer_weights* W, const sbk_transducer_config* cfg, const float* tn,
                                         float* out_pn, float* h, float* c, int32_t* tokens, int32_t* count, float* score,
                                         int B, int T, sbk_stream_t stream) {
  if (B == 0) return 0;
  SBK_REQUIRE(W && cfg, "transducer_greedy: weights or cfg is NULL");
  SBK_REQUIRE(tn && out_pn && h && c && tokens && count && score && B > 0 && T > 0,
              "transducer_greedy: bad arguments (B=%d T=%d)", B, T);
  SBK_REQUIRE(W->n_layers >= 1 && W->n_layers <= SBK_TRANSDUCER_MAX_LAYERS,
              "transducer_greedy: %d LSTM layers (1..%d supported)", W->n_layers, SBK_TRANSDUCER_MAX_LAYERS);
  SBK_REQUIRE(W->hidden > 0 && W->joint > 0 && W->vocab > 0 && W->n_emb >= W->vocab,
              "transducer_greedy: bad sizes (hidden=%d joint=%d vocab=%d n_emb=%d; vocab <= n_emb)", W->hidden, W->joint,
              W->vocab, W->n_emb);
  SBK_REQUIRE(W->emb_ih && W->proj && W->out, "transducer_greedy: emb_ih, proj and out are required");
  for (int l = 0; l < W->n_layers; ++l)
    SBK_REQUIRE(W->w_hh[l] && (l == 0 || W->w_ih[l]), "transducer_greedy: weights of LSTM layer %d missing", l);
  SBK_REQUIRE(cfg->blank >= 0 && cfg->blank < W->vocab, "transducer_greedy: blank %d outside [0, %d)", cfg->blank, W->vocab);
  SBK_REQUIRE(cfg->max_symbols_per_step >= 0, "transducer_greedy: max_symbols_per_step %d < 0", cfg->max_symbols_per_step);
  SBK_REQUIRE((long long)T * (cfg->max_symbols_per_step + 1) < (1LL << 31), "transducer_greedy: T * (max_symbols + 1) too large");
  SBK_REQUIRE(cfg->frame_block >= 0 && cfg->frame_block <= kTdFrameMax, "transducer_greedy: frame_block %d outside [0, %d]",
              cfg->frame_block, kTdFrameMax);
  SBK_REQUIRE(sbk::joint_act_known(cfg->act), "transducer_greedy: joint activation %d is not supported", cfg->act);
  int F = cfg->frame_block > 0 ? cfg->frame_block : kTdFrameDefault;
  F = min(F, T);
  while (F > 1 && td_lds_bytes(*W, F) > kTdDynLdsMax) --F;  // (the result does not depend on F)
  const size_t lds = td_lds_bytes(*W, F);
  SBK_REQUIRE(lds <= kTdDynLdsMax, "transducer_greedy: %zu bytes of LDS needed (joint %d, vocab %d, hidden %d)", lds, W->joint,
              W->vocab, W->hidden);
  TdArgs a;
  a.W = *W;
  a.tn = tn, a.out_pn = out_pn, a.h = h, a.c = c, a.tokens = tokens, a.count = count, a.score = score;
  a.B = B, a.T = T, a.F = F, a.S = cfg->max_symbols_per_step, a.blank = cfg->blank, a.act = cfg->act;
  a.start = cfg->start_from_blank ? 1 : 0;
  hipStream_t st = as_stream(stream);
  if (allow_dyn_lds(transducer_greedy_kernel, lds) != hipSuccess)
    return fail(SBK_EINVAL, "transducer_greedy: %zu bytes of LDS not available", lds);
  const double G = 4.0 * W->hidden;
  ProfScope prof("transducer_greedy", 0.0, 4.0 * B * T * W->joint + 4.0 * (double)W->joint * W->vocab * B * cdiv(T, F) +
                                               4.0 * G * W->hidden * W->n_layers * B, st);
  SBK_LAUNCH(transducer_greedy_kernel, dim3(B), dim3(kTdThreads), lds, st, a);
  return launch_status("transducer_greedy");
}

namespace {

constexpr size_t kTbStaticLds = 256;  // the beam kernel's counters and s_cur

struct TbSizes {
  long long cap_a, n_slots, slot_floats, node_cap;
  size_t lds, gmax, head_bytes, node_bytes, slot_bytes, total;
};

// The sizes of one beam search (M: the RNNLM of a search with LM fusion, or NULL); `why` names the limit a refused size breaks.
bool tb_sizes(const sbk_transducer_weights& W, const sbk_rnnlm_weights* M, const sbk_transducer_beam_config& c, int B, int T,
              TbSizes& z, const char** why) {
  const long long beam = c.beam_size, me = c.max_expansions;
  z.cap_a = beam + me * beam;   // the previous B plus at most beam children per expansion
  z.n_slots = 2 * beam + me;    // the states and cached steps B carries in, plus one new state per expansion
  const long long lm_state = M ? 2LL * M->n_layers * M->hidden : 0;  // with an LM a slot also holds its h / c and [V] log-probs
  z.slot_floats = ((long long)W.joint + 2LL * W.n_layers * W.hidden + lm_state + (M ? W.vocab : 0) + 3) / 4 * 4;
  z.node_cap = 1 + (long long)T * me * beam;
  *why = "max_expansions * beam_size * T too large";
  if (z.node_cap >= (1LL << 31) || z.cap_a >= (1LL << 24)) return false;
  z.gmax = 4 * (size_t)(M && M->hidden > W.hidden ? M->hidden : W.hidden);  // the gate buffers are shared by the PN and the LM
  const size_t lm_floats = M ? (size_t)lm_state + 2 * (size_t)M->dnn + (size_t)M->vocab + (size_t)beam : 0;
  z.lds = sizeof(float) * (2 * (size_t)W.joint + W.vocab + 2 * (size_t)W.n_layers * W.hidden + 2 * z.gmax + lm_floats) +
          sizeof(int) * (2 * (size_t)beam + (size_t)z.n_slots) + sizeof(TbHyp) * (size_t)(z.cap_a + beam);
  *why = M ? "the hypothesis lists (beam_size * max_expansions), the network's and the LM's vectors do not fit in LDS"
           : "the hypothesis lists (beam_size * max_expansions) and the network's vectors do not fit in LDS";
  if (z.lds > kTdLdsMax - kTbStaticLds) return false;
  z.head_bytes = ((size_t)B * (M ? 2 : 1) * sizeof(int32_t) + 15) / 16 * 16;  // expansions [B], with an LM also LM steps [B]
  z.node_bytes = (size_t)B * (size_t)z.node_cap * sizeof(int2);
  z.slot_bytes = (size_t)B * (size_t)z.n_slots * (size_t)z.slot_floats * sizeof(float);
  z.total = z.head_bytes + z.node_bytes + z.slot_bytes;
  return true;
}

int tb_check(const sbk_transducer_weights* W, const sbk_transducer_beam_config* cfg, int B, int T) {
  SBK_REQUIRE(W && cfg, "transducer_beam_search: weights or cfg is NULL");
  SBK_REQUIRE(B > 0 && T > 0, "transducer_beam_search: bad arguments (B=%d T=%d)", B, T);
  SBK_REQUIRE(W->n_layers >= 1 && W->n_layers <= SBK_TRANSDUCER_MAX_LAYERS,
              "transducer_beam_search: %d LSTM layers (1..%d supported)", W->n_layers, SBK_TRANSDUCER_MAX_LAYERS);
  SBK_REQUIRE(W->hidden > 0 && W->joint > 0 && W->vocab > 0 && W->n_emb >= W->vocab,
              "transducer_beam_search: bad sizes (hidden=%d joint=%d vocab=%d n_emb=%d; vocab <= n_emb)", W->hidden, W->joint,
              W->vocab, W->n_emb);
  SBK_REQUIRE(W->emb_ih && W->proj && W->out, "transducer_beam_search: emb_ih, proj and out are required");
  for (int l = 0; l < W->n_layers; ++l)
    SBK_REQUIRE(W->w_hh[l] && (l == 0 || W->w_ih[l]), "transducer_beam_search: weights of LSTM layer %d missing", l);
  SBK_REQUIRE(cfg->blank >= 0 && cfg->blank < W->vocab, "transducer_beam_search: blank %d outside [0, %d)", cfg->blank,
              W->vocab);
  SBK_REQUIRE(cfg->beam_size >= 2, "transducer_beam_search: beam_size %d < 2 (the greedy entry decodes beam_size 1)",
              cfg->beam_size);
  SBK_REQUIRE(cfg->beam_size <= SBK_TRANSDUCER_MAX_BEAM, "transducer_beam_search: beam_size %d above the maximum %d",
              cfg->beam_size, SBK_TRANSDUCER_MAX_BEAM);
  SBK_REQUIRE(cfg->beam_size <= W->vocab, "transducer_beam_search: beam_size %d above the vocabulary %d", cfg->beam_size,
              W->vocab);
  SBK_REQUIRE(cfg->nbest >= 1, "transducer_beam_search: nbest %d < 1", cfg->nbest);
  SBK_REQUIRE(cfg->max_expansions >= 1, "transducer_beam_search: max_expansions %d < 1", cfg->max_expansions);
  SBK_REQUIRE(cfg->max_tokens >= 1, "transducer_beam_search: max_tokens %d < 1", cfg->max_tokens);
  SBK_REQUIRE((long long)B * cfg->nbest * cfg->max_tokens < (1LL << 40), "transducer_beam_search: output too large");
  SBK_REQUIRE(sbk::joint_act_known(cfg->act), "transducer_beam_search: joint activation %d is not supported", cfg->act);
  return 0;
}

int tb_lm_check(const sbk_transducer_weights* W, const sbk_rnnlm_weights* M, float lm_weight) {
  SBK_REQUIRE(M, "transducer_beam_search_lm: the LM's weights are NULL");
  SBK_REQUIRE(isfinite(lm_weight) && lm_weight > 0.0f, "transducer_beam_search_lm: lm_weight %g is not a finite value > 0",
              (double)lm_weight);
  SBK_REQUIRE(M->n_layers >= 1 && M->n_layers <= SBK_TRANSDUCER_MAX_LAYERS,
              "transducer_beam_search_lm: %d LSTM layers in the LM (1..%d supported)", M->n_layers, SBK_TRANSDUCER_MAX_LAYERS);
  SBK_REQUIRE(M->n_dnn >= 1 && M->n_dnn <= SBK_RNNLM_MAX_DNN, "transducer_beam_search_lm: n_dnn %d DNN blocks in the LM (1..%d supported)",
              M->n_dnn, SBK_RNNLM_MAX_DNN);
  SBK_REQUIRE(M->hidden > 0 && M->dnn > 0 && M->vocab > 0 && M->hidden < (1 << 24) && M->dnn < (1 << 24) && M->vocab < (1 << 24),
              "transducer_beam_search_lm: bad LM sizes (hidden=%d dnn=%d vocab=%d)", M->hidden, M->dnn, M->vocab);
  SBK_REQUIRE(M->vocab >= W->vocab && M->n_emb >= W->vocab,
              "transducer_beam_search_lm: the LM's vocab %d (n_emb %d) is below the classifier's %d outputs", M->vocab, M->n_emb,
              W->vocab);
  SBK_REQUIRE(M->emb_ih && M->out, "transducer_beam_search_lm: the LM's emb_ih and out are required");
  for (int l = 0; l < M->n_layers; ++l)
    SBK_REQUIRE(M->w_hh[l] && (l == 0 || M->w_ih[l]), "transducer_beam_search_lm: weights of the LM's LSTM layer %d missing", l);
  for (int i = 0; i < M->n_dnn; ++i)
    SBK_REQUIRE(M->dnn_w[i] && M->ln_g[i] && M->ln_b[i] && M->ln_eps[i] >= 0.0f,
                "transducer_beam_search_lm: weights of the LM's DNN block %d missing (w, ln_g, ln_b; ln_eps >= 0)", i);
  SBK_REQUIRE(sbk::joint_act_known(M->act), "transducer_beam_search_lm: the LM's activation %d is not supported", M->act);
  return 0;
}

}  // namespace

extern "C" size_t sbk_transducer_beam_workspace_bytes(const sbk_transducer_weights* W, const sbk_transducer_beam_config* cfg,
                                                      int B, int T) {
  TbSizes z;
  const char* why;
  if (B == 0) return 0;
  if (tb_check(W, cfg, B, T) != 0) return 0;
  if (!tb_sizes(*W, nullptr, *cfg, B, T, z, &why)) {
    fail(SBK_EINVAL, "transducer_beam_search: %s (beam_size=%d max_expansions=%d T=%d)", why, cfg->beam_size,
         cfg->max_expansions, T);
    return 0;
  }
  return z.total;
}

extern "C" int sbk_transducer_beam_search_f32(const sbk_transducer_weights* W, const sbk_transducer_beam_config* cfg,
                                              const float* tn, void* workspace, size_t workspace_bytes, int32_t* out_tokens,
                                              int32_t* out_len, float* out_score, int32_t* out_count, int32_t* out_status,
                                              int B, int T, sbk_stream_t stream) {
  if (B == 0) return 0;
  if (const int rc = tb_check(W, cfg, B, T)) return rc;
  SBK_REQUIRE(tn && workspace && out_tokens && out_len && out_score && out_count && out_status,
              "transducer_beam_search: a NULL pointer among tn, workspace and the outputs");
  TbSizes z;
  const char* why;
  SBK_REQUIRE(tb_sizes(*W, nullptr, *cfg, B, T, z, &why), "transducer_beam_search: %s (beam_size=%d max_expansions=%d T=%d)", why,
              cfg->beam_size, cfg->max_expansions, T);
  SBK_REQUIRE(aligned16(workspace), "transducer_beam_search: the workspace is not 16-byte aligned");
  SBK_REQUIRE(workspace_bytes >= z.total, "transducer_beam_search: workspace of %zu bytes, %zu needed", workspace_bytes, z.total);
  TbArgs a;
  memset(&a, 0, sizeof(a));
  a.g.W = *W;
  a.g.tn = tn, a.g.B = B, a.g.T = T, a.g.blank = cfg->blank, a.g.act = cfg->act;
  char* ws = static_cast<char*>(workspace);
  a.expansions = reinterpret_cast<int32_t*>(ws);
  a.nodes = reinterpret_cast<int2*>(ws + z.head_bytes);
  a.slots = reinterpret_cast<float*>(ws + z.head_bytes + z.node_bytes);
  a.out_tokens = out_tokens, a.out_len = out_len, a.out_score = out_score, a.out_count = out_count, a.out_status = out_status;
  a.beam = cfg->beam_size, a.nbest = cfg->nbest, a.max_exp = cfg->max_expansions, a.max_tokens = cfg->max_tokens;
  a.cap_a = (int)z.cap_a, a.n_slots = (int)z.n_slots, a.slot_floats = (int)z.slot_floats, a.node_cap = (int)z.node_cap;
  a.state_beam = cfg->state_beam, a.expand_beam = cfg->expand_beam;
  hipStream_t st = as_stream(stream);
  if (allow_dyn_lds(transducer_beam_kernel<false>, z.lds) != hipSuccess)
    return fail(SBK_EINVAL, "transducer_beam_search: %zu bytes of LDS not available", z.lds);
  ProfScope prof("transducer_beam", 0.0, 4.0 * B * T * W->joint + 4.0 * (double)W->joint * W->vocab * B * T, st);
  SBK_LAUNCH(transducer_beam_kernel<false>, dim3(B), dim3(kTdThreads), z.lds, st, a);
  return launch_status("transducer_beam_search");
}

extern "C" size_t sbk_transducer_beam_lm_workspace_bytes(const sbk_transducer_weights* W, const sbk_rnnlm_weights* LM,
                                                         const sbk_transducer_beam_config* cfg, int B, int T) {
  TbSizes z;
  const char* why;
  if (B == 0) return 0;
  if (tb_check(W, cfg, B, T) != 0) return 0;
  if (tb_lm_check(W, LM, 1.0f) != 0) return 0;
  if (!tb_sizes(*W, LM, *cfg, B, T, z, &why)) {
    fail(SBK_EINVAL, "transducer_beam_search_lm: %s (beam_size=%d max_expansions=%d T=%d LM hidden=%d)", why, cfg->beam_size,
         cfg->max_expansions, T, LM->hidden);
    return 0;
  }
  return z.total;
}

extern "C" int sbk_transducer_beam_search_lm_f32(const sbk_transducer_weights* W, const sbk_rnnlm_weights* LM, float lm_weight,
                                                 const sbk_transducer_beam_config* cfg, const float* tn, void* workspace,
                                                 size_t workspace_bytes, int32_t* out_tokens, int32_t* out_len,
                                                 float* out_score, int32_t* out_count, int32_t* out_status, int B, int T,
                                                 sbk_stream_t stream) {
  if (B == 0) return 0;
  if (const int rc = tb_check(W, cfg, B, T)) return rc;
  if (const int rc = tb_lm_check(W, LM, lm_weight)) return rc;
  SBK_REQUIRE(tn && workspace && out_tokens && out_len && out_score && out_count && out_status,
              "transducer_beam_search_lm: a NULL pointer among tn, workspace and the outputs");
  TbSizes z;
  const char* why;
  SBK_REQUIRE(tb_sizes(*W, LM, *cfg, B, T, z, &why), "transducer_beam_search_lm: %s (beam_size=%d max_expansions=%d T=%d LM hidden=%d)",
              why, cfg->beam_size, cfg->max_expansions, T, LM->hidden);
  SBK_REQUIRE(aligned16(workspace), "transducer_beam_search_lm: the workspace is not 16-byte aligned");
  SBK_REQUIRE(workspace_bytes >= z.total, "transducer_beam_search_lm: workspace of %zu bytes, %zu needed", workspace_bytes, z.total);
  TbArgs a;
  memset(&a, 0, sizeof(a));
  a.g.W = *W;
  a.g.tn = tn, a.g.B = B, a.g.T = T, a.g.blank = cfg->blank, a.g.act = cfg->act;
  char* ws = static_cast<char*>(workspace);
  a.expansions = reinterpret_cast<int32_t*>(ws);
  a.lm_steps = a.expansions + B;
  a.nodes = reinterpret_cast<int2*>(ws + z.head_bytes);
  a.slots = reinterpret_cast<float*>(ws + z.head_bytes + z.node_bytes);
  a.out_tokens = out_tokens, a.out_len = out_len, a.out_score = out_score, a.out_count = out_count, a.out_status = out_status;
  a.beam = cfg->beam_size, a.nbest = cfg->nbest, a.max_exp = cfg->max_expansions, a.max_tokens = cfg->max_tokens;
  a.cap_a = (int)z.cap_a, a.n_slots = (int)z.n_slots, a.slot_floats = (int)z.slot_floats, a.node_cap = (int)z.node_cap;
  a.state_beam = cfg->state_beam, a.expand_beam = cfg->expand_beam;
  a.lm = *LM, a.lm_weight = lm_weight, a.gmax = (int)z.gmax;
  hipStream_t st = as_stream(stream);
  if (allow_dyn_lds(transducer_beam_kernel<true>, z.lds) != hipSuccess)
    return fail(SBK_EINVAL, "transducer_beam_search_lm: %zu bytes of LDS not available", z.lds);
  ProfScope prof("transducer_beam_lm", 0.0, 4.0 * B * T * W->joint + 4.0 * (double)W->joint * W->vocab * B * T, st);
  SBK_LAUNCH(transducer_beam_kernel<true>, dim3(B), dim3(kTdThreads), z.lds, st, a);
  return launch_status("transducer_beam_search_lm");
}

extern "C" int sbk_lstm_f32(const float* xp, const float* w_hh, const float* b_ih, const float* b_hh, float* h, float* c,
                            float* out, int B, int T, int H, sbk_stream_t stream) {
  if (B == 0) return 0;
  SBK_REQUIRE(xp && w_hh && h && c && out && B > 0 && T > 0 && H > 0, "lstm: bad arguments (B=%d T=%d H=%d)", B, T, H);
  const size_t lds = sizeof(float) * 10 * (size_t)H;
  SBK_REQUIRE(lds <= kTdLdsMax, "lstm: hidden size %d too large", H);  // (lstm_layer_kernel has no static LDS)
  hipStream_t st = as_stream(stream);
  if (allow_dyn_lds(lstm_layer_kernel, lds) != hipSuccess)
    return fail(SBK_EINVAL, "lstm: %zu bytes of LDS not available", lds);
  ProfScope prof("lstm", 2.0 * B * T * 4.0 * H * H, 4.0 * B * T * 5.0 * H + 16.0 * H * H * B, st);
  SBK_LAUNCH(lstm_layer_kernel, dim3(B), dim3(kTdThreads), lds, st, xp, w_hh, b_ih, b_hh, h, c, out, T, H);
  return launch_status("lstm");
}
