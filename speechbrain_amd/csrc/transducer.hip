// Transducer greedy decoding on the device: TransducerBeamSearcher.transducer_greedy_decode (decoders/transducer.py:156-291)
// for the prediction network [Embedding, LSTM, Linear], Transducer_joint(joint="sum") and one classifier Linear.  One
// workgroup per utterance runs every frame in ONE launch with the utterance's PN state in LDS; the weights stream from L2.
// The semantics reproduced here are listed in DESIGN.md section 5 ("Transducer greedy decoding").
#include <math.h>

#include "argmax.h"
#include "common.h"

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

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float joint_act(float x, int act) {
  switch (act) {
    case SBK_ACT_GELU: return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
    case SBK_ACT_LEAKY_RELU: return x > 0.0f ? x : x * 0.01f;
    case SBK_ACT_RELU: return x <= 0.0f ? 0.0f : x;  // (NaN stays NaN, as torch.relu)
    default: return tanhf(x);
  }
}

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
        for (int m = 32; m >= 1; m >>= 1) v += shfl_xor(v, m);
        if (lane == 0 && n0 + r < N) out[(size_t)f * ldo + n0 + r] = bias ? v + bias[n0 + r] : v;
      }
    }
  }
}

// The cell update of one LSTM step from the gates' input part s_g and recurrent part s_gh (torch gate order i, f, g, o).
__device__ __forceinline__ void lstm_update(const float* s_g, const float* s_gh, float* hl, float* cl, int H) {
  for (int m = threadIdx.x; m < H; m += kTdThreads) {
    const float ig = sigmoid_f32(s_g[m] + s_gh[m]);
    const float fg = sigmoid_f32(s_g[H + m] + s_gh[H + m]);
    const float gg = tanhf(s_g[2 * H + m] + s_gh[2 * H + m]);
    const float og = sigmoid_f32(s_g[3 * H + m] + s_gh[3 * H + m]);
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
      s_z[i] = joint_act(tnb[(size_t)(t + f) * J + k] + s_pn[k], a.act);
    }
    __syncthreads();
    // 2. logits: one pass over the classifier's weights for the whole block
    gemv_rows<kTdFrameMax, 2>(W.out, W.out_b, s_z, J, fe, J, V, s_logit, V);
    __syncthreads();
    // 3. log-softmax and arg-max of each frame (one wave per frame)
    for (int f = wave; f < fe; f += kTdThreads / 64) {
      const float* x = s_logit + (size_t)f * V;
      float m = -INFINITY;
      for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
      for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, shfl_xor(m, s));
      float se = 0.0f;
      for (int v = lane; v < V; v += 64) se += expf(x[v] - m);
      for (int s = 32; s >= 1; s >>= 1) se += shfl_xor(se, s);
      const float ls = logf(se);
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
  SBK_REQUIRE(cfg->act == SBK_ACT_GELU || cfg->act == SBK_ACT_LEAKY_RELU || cfg->act == SBK_ACT_RELU ||
                  cfg->act == SBK_ACT_TANH,
              "transducer_greedy: joint activation %d is not supported", cfg->act);
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
  if (lds > 64 * 1024 && (int)SBK_ALLOW_DYN_LDS(transducer_greedy_kernel, lds) != 0)
    return fail(SBK_EINVAL, "transducer_greedy: %zu bytes of LDS not available", lds);
  const double G = 4.0 * W->hidden;
  ProfScope prof("transducer_greedy", 0.0, 4.0 * B * T * W->joint + 4.0 * (double)W->joint * W->vocab * B * cdiv(T, F) +
                                               4.0 * G * W->hidden * W->n_layers * B, st);
  SBK_LAUNCH(transducer_greedy_kernel, dim3(B), dim3(kTdThreads), lds, st, a);
  return launch_status("transducer_greedy");
}

extern "C" int sbk_lstm_f32(const float* xp, const float* w_hh, const float* b_ih, const float* b_hh, float* h, float* c,
                            float* out, int B, int T, int H, sbk_stream_t stream) {
  if (B == 0) return 0;
  SBK_REQUIRE(xp && w_hh && h && c && out && B > 0 && T > 0 && H > 0, "lstm: bad arguments (B=%d T=%d H=%d)", B, T, H);
  const size_t lds = sizeof(float) * 10 * (size_t)H;
  SBK_REQUIRE(lds <= kTdLdsMax, "lstm: hidden size %d too large", H);  // (lstm_layer_kernel has no static LDS)
  hipStream_t st = as_stream(stream);
  if (lds > 64 * 1024 && (int)SBK_ALLOW_DYN_LDS(lstm_layer_kernel, lds) != 0)
    return fail(SBK_EINVAL, "lstm: %zu bytes of LDS not available", lds);
  ProfScope prof("lstm", 2.0 * B * T * 4.0 * H * H, 4.0 * B * T * 5.0 * H + 16.0 * H * H * B, st);
  SBK_LAUNCH(lstm_layer_kernel, dim3(B), dim3(kTdThreads), lds, st, xp, w_hh, b_ih, b_hh, h, c, out, T, H);
  return launch_status("lstm");
}
