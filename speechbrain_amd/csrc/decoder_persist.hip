// The decoding step of a FEW hypothesis rows as ONE cooperative launch (reference: TransformerDecoderLayer.forward,
// lobes/models/transformer/Transformer.py:751-834, driven by S2STransformerBeamSearcher.forward_step,
// decoders/seq2seq.py:1632-1723 -- the single-utterance regime, beam <= 16 rows).
//
// Why: at 10 rows a step of the launch-per-operation path is ~70 dependent launches of ~9 us (p50 27 ms for a 10-s
// utterance, three rounds flat), although its work is streaming ~100 MB of weights once.  Here the whole decoder stack of a
// step is one kernel whose G workgroups stay resident and meet at grid barriers between sub-layers:
//
//   embed | per layer: [norm1 + in_proj] | self-attention | [out_proj + x] | [norm2 + q proj] | cross-attention |
//   [out_proj + x] | [norm3 + ffn.0 + act] | [ffn.3 + x] | ... | [decoder.norm + seq_lin]
//
// * projections: weight-stationary -- a workgroup owns 16 output columns (its 16 x K weight slice, 32 KB at K = 512) for
//   ALL rows; the four waves split K, 16 x 16 x 4 fp32 MFMAs, fixed-order LDS reduction.  The rows (16 x K fp32) are staged
//   into LDS by every workgroup, LayerNorm statistics included (gamma / beta are folded into the weights, sbk.h).
//   The first weight loads of the NEXT projection are issued before the barrier wait: weights do not depend on activations,
//   so their HBM latency hides behind the barrier.
// * activations between workgroups travel through agent-scope (sc1) accesses, never through L2 write-back / invalidate
//   (hip/sbk_device.h: ld_agent / st_agent / grid_arrive / grid_wait; tools/persist_probe.hip measured both).
// * self-attention: one wave per (row, head) over the KV cache (the layout and arithmetic of self_attn_step_kernel);
//   cross-attention: one workgroup per (utterance, head), the four waves walk the memory in 64-frame runs with all K / V rows
//   of a run in flight, online softmax per wave, merge through LDS.
// Results: same algorithm, another summation order than the launch-per-operation kernels (tests: ids equal, 1e-4).
#include <math.h>

#include "act.h"
#include "internal.h"

#include <string.h>

#include <mutex>
#include <vector>

namespace {

constexpr int kPRows = 16;        // hypothesis rows a launch serves (the MFMA tile height)
constexpr int kMaxPLayers = 16;   // (kernel arguments are passed by value: 16 x 15 pointers)

struct PLayer {
  const float *sa_in_wf, *sa_in_bf, *sa_out_w, *sa_out_b, *ca_q_wf, *ca_q_bf, *ca_out_w, *ca_out_b, *ff1_wf, *ff1_bf, *ff2_w, *ff2_b;
  float *kcache, *vcache;  // [slot][Lmax][d]
  const float* ckv;        // [B][T][2d]: K (d) then V (d) per frame
};

struct PStepArgs {
  PLayer L[kMaxPLayers];
  const int32_t *tok, *kv_slot, *enc_len;
  const float *emb, *pe_row;
  float *x, *qkv, *ctx, *q, *ff, *h, *logits;
  const float *fin_g, *fin_b, *seq_wf, *seq_bf;
  long long* stamps;  // optional (knob 49): workgroup 0 writes the 100 MHz wall clock at the end of every phase and barrier
  int* bar;      // arrival counter of the grid barriers (monotonic over the launches of a search)
  int bar_base;  // its value when this launch starts
  // two-level arrival (knob 59): workgroup b arrives at sub-counter b % 8 (its own 128-byte line); the arrival that completes a
  // sub-counter's round arrives at `bar`.  G atomics on ONE address are served one after the other (~25 ns each: 3.4-3.8 us of a
  // barrier among 128 workgroups); eight lines take them side by side.  ord_base: barriers passed before this launch.
  int* sub;
  int tree, ord_base;
  int n, B, T, beam, d, H, dffn, V, nl, step, Lmax, act, want_logits;
  float eps, emb_scale, attn_scale;
};

constexpr int kWB = 16;  // operand loads (16 bytes each, 16 k apart) a wave keeps in flight per block: 256 k of its K quarter
struct WPref {           // the first block of this wave's first tile of the NEXT projection
  float4 w[kWB];
};

// address of this lane's first operand of tile `tile` (16 columns from tile * 16; rows past N re-read row N - 1)
__device__ __forceinline__ const float* w_lane_ptr(const float* W, int K, int N, int tile) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int col = tile * 16 + (lane & 15);
  col = col < N ? col : N - 1;
  return W + (size_t)col * K + wave * (K >> 2) + 4 * (lane >> 4);
}

__device__ __forceinline__ void prefetch_w(WPref& pf, const float* W, int K, int N) {
  if ((int)blockIdx.x * 16 >= N) return;
  const float* wp = w_lane_ptr(W, K, N, blockIdx.x);
  const int nb = K >> 6;  // 16-deep operand groups of this wave's K quarter
#pragma unroll
  for (int j = 0; j < kWB; ++j)
    if (j < nb) pf.w[j] = *reinterpret_cast<const float4*>(wp + 16 * j);
}

// rows of X [n][K] (written by other workgroups of this launch) -> xs [16][K + 4] in LDS, rows >= n zero; LN: normalised
// (K <= 1 024 then).  A lane owns column pairs c = 2 tid + 512 j of EVERY row: 32 eight-byte agent-scope loads in flight per
// lane and pass (one pass for K <= 1 024).  Issued one by one they cost a round trip each -- the first version of this kernel
// spent most of its 800 us per step there (profiles/r05_b_*).
template <bool LN>
__device__ __forceinline__ void stage_rows(const PStepArgs& a, float* xs, const float* X, int K) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, KP = K + 4;
  __syncthreads();  // (the previous user of this LDS region is done)
  for (int c0 = 2 * tid; c0 < K; c0 += 1024) {
    float2 v[2][kPRows];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + 512 * j;
#pragma unroll
      for (int r = 0; r < kPRows; ++r) {
        v[j][r] = make_float2(0.0f, 0.0f);
        if (c < K && r < a.n) v[j][r] = sbk::ld_agent2(X + (size_t)r * K + c);
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + 512 * j;
      if (c < K) {
#pragma unroll
        for (int r = 0; r < kPRows; ++r) {
          xs[r * KP + c] = v[j][r].x;
          xs[r * KP + c + 1] = v[j][r].y;
        }
      }
    }
  }
  __syncthreads();
  if (LN) {
    // a row per 16-lane group (wave w, group g: row 4 w + g), 16-byte pieces c = 4 cq + 64 e in registers, sums over the group on
    // the VALU (DPP): all sixteen rows at once.  (A row per wave with wave-wide reductions took ~6 us of dependent latency per
    // phase at one wave per SIMD: profiles/r05_d_*.)
    const int row = 4 * wave + (lane >> 4), cq = lane & 15;
    float* xr = xs + row * KP + 4 * cq;
    float4 xv[16];
    float sm = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      xv[e] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (64 * e < K) xv[e] = *reinterpret_cast<const float4*>(xr + 64 * e);
      sm += (xv[e].x + xv[e].y) + (xv[e].z + xv[e].w);
    }
    const float mean = sbk::group_sum<16>(sm) / (float)K;
    float qs = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (64 * e < K) {
        const float d0 = xv[e].x - mean, d1 = xv[e].y - mean, d2 = xv[e].z - mean, d3 = xv[e].w - mean;
        qs += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
      }
    }
    const float rstd = rsqrtf(sbk::group_sum<16>(qs) / (float)K + a.eps);
    if (row < a.n) {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (64 * e < K)
          *reinterpret_cast<float4*>(xr + 64 * e) = make_float4((xv[e].x - mean) * rstd, (xv[e].y - mean) * rstd, (xv[e].z - mean) * rstd,
                                                                (xv[e].w - mean) * rstd);
    }
    __syncthreads();
  }
}

// C[n][N] (+ R) = act(xs . W^T + bias) for this workgroup's column tiles; xs staged by stage_rows.  K % 64 == 0.
__device__ __forceinline__ void tiles_gemm(const PStepArgs& a, const float* xs, float* red, int K, const float* W, const float* bias,
                                           const float* R, float* C, int N, int act, const WPref& pf) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, KP = K + 4, G = gridDim.x;
  const int ntiles = (N + 15) >> 4, nb = K >> 6;
  const float* xa = xs + (lane & 15) * KP + wave * (K >> 2) + 4 * (lane >> 4);
  float4 wc[kWB];
  for (int tile = blockIdx.x; tile < ntiles; tile += G) {
    const float* wp = w_lane_ptr(W, K, N, tile);
    const int row = tid >> 4, col = tile * 16 + (tid & 15);
    const bool out_ok = row < a.n && col < N;
    float rv = 0.0f;
    if (R && out_ok) rv = sbk::ld_agent(R + (size_t)row * N + col);  // (in flight under the products)
    if (tile == (int)blockIdx.x) {
#pragma unroll
      for (int j = 0; j < kWB; ++j) wc[j] = pf.w[j];
    }  // (a later tile: wc was loaded under the previous tile's reduction, below)
    // four independent accumulation chains (one per element of the 16-byte operands): a single chain would serialise
    // K / 16 dependent MFMAs per wave
    sbk::f32x4 a0 = {0.0f, 0.0f, 0.0f, 0.0f}, a1 = a0, a2 = a0, a3 = a0;
    for (int jb = 0; jb < nb; jb += kWB) {
      float4 wn[kWB];
      if (jb + kWB < nb) {  // the next block's operands fly under this block's products
#pragma unroll
        for (int j = 0; j < kWB; ++j)
          if (jb + kWB + j < nb) wn[j] = *reinterpret_cast<const float4*>(wp + 16 * (jb + kWB + j));
      }
#pragma unroll
      for (int j = 0; j < kWB; ++j) {
        if (jb + j < nb) {
          const float4 x4 = *reinterpret_cast<const float4*>(xa + 16 * (jb + j));
          a0 = sbk::mfma_16x16x4(x4.x, wc[j].x, a0);
          a1 = sbk::mfma_16x16x4(x4.y, wc[j].y, a1);
          a2 = sbk::mfma_16x16x4(x4.z, wc[j].z, a2);
          a3 = sbk::mfma_16x16x4(x4.w, wc[j].w, a3);
        }
      }
      if (jb + kWB < nb) {
#pragma unroll
        for (int j = 0; j < kWB; ++j) wc[j] = wn[j];
      }
    }
    if (tile + G < ntiles) {  // the next tile's first block flies under this tile's reduction and stores
      const float* wq = w_lane_ptr(W, K, N, tile + G);
#pragma unroll
      for (int j = 0; j < kWB; ++j)
        if (j < nb) wc[j] = *reinterpret_cast<const float4*>(wq + 16 * j);
    }
    __syncthreads();  // (red free again)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave * 256 + (4 * (lane >> 4) + r) * 16 + (lane & 15)] = (a0[r] + a1[r]) + (a2[r] + a3[r]);
    __syncthreads();
    if (out_ok) {
      float v = (red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid]);
      v = sbk::act(v + (bias ? bias[col] : 0.0f), act) + rv;
      sbk::st_agent(C + (size_t)row * N + col, v);
    }
  }
}

// One workgroup: hypothesis row i, head h (head_dim 64).  SELF: over the KV cache (layout of self_attn_step_kernel: rows
// [slot][pos][d], ancestry table kv_slot[hyp][pos]; the new token's K / V come from qkv and are appended), 64 positions per pass;
// otherwise over the utterance's encoder memory ([T][2d]: K then V), 256 frames per pass.  A pass is split over the four waves,
// a wave's lanes are 4 position groups x 16 lanes x 16-byte pieces of the head row, and EVERY K and V row of the pass is in
// flight before any arithmetic.  Softmax as a running (max, sum, context) per wave, the four waves merged through LDS.
// (One wave per item with all beams took 27 us per cross-attention phase -- a lone wave issues an instruction every four cycles:
// profiles/r05_d_*; spreading rows x heads over the workgroups divides the instruction stream of a wave by ~20.)
template <bool SELF>
__device__ __forceinline__ void attn_item(const PStepArgs& a, const PLayer& L, float* lds, int i, int h) {
  constexpr int GPW = SELF ? 4 : 16;            // position groups of four per wave and pass
  constexpr int PASS = 4 * 4 * GPW;              // positions per pass of the workgroup
  float* wm = lds;                               // [4] running maxima of the waves
  float* wl = lds + 4;                           // [4] their sums
  float* wacc = lds + 8;                         // [4][64] their un-normalised contexts
  int* slot = reinterpret_cast<int*>(lds + 8 + 256);  // SELF: [step] cache slots of this row's prefix
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pg = lane >> 4, cq = lane & 15, d = a.d;
  const size_t hoff = (size_t)h * 64 + cq * 4;
  float4 q4, kn = make_float4(0.f, 0.f, 0.f, 0.f), vn = kn;
  int len;
  const float* mem = nullptr;
  __syncthreads();  // (the previous item's merge has read the LDS)
  if (SELF) {
    const float* qp = a.qkv + (size_t)i * 3 * d + hoff;
    const float2 q0 = sbk::ld_agent2(qp), q1 = sbk::ld_agent2(qp + 2);
    const float2 k0 = sbk::ld_agent2(qp + d), k1 = sbk::ld_agent2(qp + d + 2);
    const float2 v0 = sbk::ld_agent2(qp + 2 * d), v1 = sbk::ld_agent2(qp + 2 * d + 2);
    for (int p = tid; p < a.step; p += 256) slot[p] = a.kv_slot[(size_t)i * a.Lmax + p];
    q4 = make_float4(q0.x * a.attn_scale, q0.y * a.attn_scale, q1.x * a.attn_scale, q1.y * a.attn_scale);
    kn = make_float4(k0.x, k0.y, k1.x, k1.y);
    vn = make_float4(v0.x, v0.y, v1.x, v1.y);
    len = a.step + 1;
    if (wave == 0 && pg == 0) {  // append this token's K / V head slice (slot = hypothesis index); read by LATER launches only
      const size_t o = ((size_t)i * a.Lmax + a.step) * d + hoff;
      *reinterpret_cast<float4*>(L.kcache + o) = kn;
      *reinterpret_cast<float4*>(L.vcache + o) = vn;
    }
    __syncthreads();
  } else {
    const float* qp = a.q + (size_t)i * d + hoff;
    const float2 q0 = sbk::ld_agent2(qp), q1 = sbk::ld_agent2(qp + 2);
    q4 = make_float4(q0.x * a.attn_scale, q0.y * a.attn_scale, q1.x * a.attn_scale, q1.y * a.attn_scale);
    const int u = i / a.beam;
    int klen = a.enc_len[u];
    len = klen < 1 ? 1 : (klen > a.T ? a.T : klen);
    mem = L.ckv + (size_t)u * a.T * 2 * d + hoff;
  }
  float m = -INFINITY, l = 0.0f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = wave * 4 * GPW; c0 < len; c0 += PASS) {
    float4 kk[GPW], vv[GPW];
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
      const int p = c0 + 4 * g + pg;
      if (SELF) {
        kk[g] = kn;
        vv[g] = vn;
        if (p < a.step) {
          const size_t o = ((size_t)slot[p] * a.Lmax + p) * d + hoff;
          kk[g] = *reinterpret_cast<const float4*>(L.kcache + o);
          vv[g] = *reinterpret_cast<const float4*>(L.vcache + o);
        }
      } else {
        const float* rp = mem + (size_t)(p < len ? p : c0) * 2 * d;
        kk[g] = *reinterpret_cast<const float4*>(rp);
        vv[g] = *reinterpret_cast<const float4*>(rp + d);
      }
    }
    float s[GPW];
    float cm = -INFINITY;
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
      float sv = (q4.x * kk[g].x + q4.y * kk[g].y) + (q4.z * kk[g].z + q4.w * kk[g].w);
      sv = sbk::group_sum<16>(sv);
      s[g] = (c0 + 4 * g + pg) < len ? sv : -INFINITY;
      cm = fmaxf(cm, s[g]);
    }
    cm = fmaxf(cm, sbk::shfl_xor(cm, 16));
    cm = fmaxf(cm, sbk::shfl_xor(cm, 32));  // (finite: position c0 < len belongs to this wave's share of the pass)
    const float mn = fmaxf(m, cm), corr = expf(m - mn);
    l *= corr;
    acc.x *= corr; acc.y *= corr; acc.z *= corr; acc.w *= corr;
#pragma unroll
    for (int g = 0; g < GPW; ++g) {
      const float p = expf(s[g] - mn);
      l += p;
      acc.x = fmaf(p, vv[g].x, acc.x);
      acc.y = fmaf(p, vv[g].y, acc.y);
      acc.z = fmaf(p, vv[g].z, acc.z);
      acc.w = fmaf(p, vv[g].w, acc.w);
    }
    m = mn;
  }
  l += sbk::shfl_xor(l, 16);
  l += sbk::shfl_xor(l, 32);
  float o[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    o[e] += sbk::shfl_xor(o[e], 16);
    o[e] += sbk::shfl_xor(o[e], 32);
  }
  if (pg == 0) {
    *reinterpret_cast<float4*>(wacc + wave * 64 + cq * 4) = make_float4(o[0], o[1], o[2], o[3]);
    if (cq == 0) {
      wm[wave] = m;
      wl[wave] = l;
    }
  }
  __syncthreads();
  if (tid < 16) {  // merge of the four waves (a wave without positions: max -inf, sum 0 -> weight exp(-inf) = 0)
    const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    float den = 0.0f;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float e = expf(wm[w] - M);
      den = fmaf(wl[w], e, den);
      const float4 v = *reinterpret_cast<const float4*>(wacc + w * 64 + tid * 4);
      r.x = fmaf(v.x, e, r.x);
      r.y = fmaf(v.y, e, r.y);
      r.z = fmaf(v.z, e, r.z);
      r.w = fmaf(v.w, e, r.w);
    }
    float* op = a.ctx + (size_t)i * d + (size_t)h * 64 + tid * 4;
    sbk::st_agent(op, r.x / den);
    sbk::st_agent(op + 1, r.y / den);
    sbk::st_agent(op + 2, r.z / den);
    sbk::st_agent(op + 3, r.w / den);
  }
}

__global__ void __launch_bounds__(256) decoder_step_persist_kernel(PStepArgs a) {
  SBK_DYN_LDS(float, lds);
  const int tid = threadIdx.x, G = gridDim.x;
  const int d = a.d, Kmax = d > a.dffn ? d : a.dffn;
  float* xs = lds;                                  // [16][K + 4] staged rows; the attention phases' scratch
  float* red = lds + (size_t)kPRows * (Kmax + 4);   // [4][256] K-split partial tiles
  int bar = a.bar_base;
  int ord = a.ord_base;                                             // barriers of this search passed so far
  const int nsub = G < 8 ? G : 8, sub_k = (int)blockIdx.x & 7;
  const int cnt_k = (G - sub_k + 7) >> 3;                           // workgroups that arrive at this sub-counter
  int* const subp = a.sub + 32 * sub_k;
  WPref pf;
#pragma unroll
  for (int j = 0; j < kWB; ++j) pf.w[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  // barrier in two halves: the next projection's first weight loads are issued between arrival and wait
  int n_stamp = 0;
#define SBK_PSTEP_STAMP()                                                                  \
  do {                                                                                     \
    if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[n_stamp] = sbk::wall_clock();     \
    ++n_stamp;                                                                             \
  } while (0)
#define SBK_PSTEP_BARRIER(W_, K_, N_)            \
  do {                                           \
    bar += G;                                    \
    ++ord;                                       \
    SBK_PSTEP_STAMP();                           \
    if (a.tree) {                                \
      sbk::grid_arrive_tree(subp, ord * cnt_k, a.bar); \
    } else {                                     \
      sbk::grid_arrive(a.bar);                   \
    }                                            \
    if ((W_) != nullptr) prefetch_w(pf, (W_), (K_), (N_)); \
    sbk::grid_wait(a.bar, a.tree ? ord * nsub : bar); \
    SBK_PSTEP_STAMP();                           \
  } while (0)
  SBK_PSTEP_STAMP();

  // embedding + position (NormalizedEmbedding, PositionalEncoding): x = emb[tok] * scale + pe[pos]
  for (int i = blockIdx.x; i < a.n; i += G) {
    const float* e = a.emb + (size_t)a.tok[i] * d;
    for (int c = tid; c < d; c += 256) sbk::st_agent(a.x + (size_t)i * d + c, e[c] * a.emb_scale + a.pe_row[c]);
  }
  SBK_PSTEP_BARRIER(a.L[0].sa_in_wf, d, 3 * d);
  for (int l = 0; l < a.nl; ++l) {
    const PLayer& L = a.L[l];
    // norm1 + self-attention in_proj
    stage_rows<true>(a, xs, a.x, d);
    tiles_gemm(a, xs, red, d, L.sa_in_wf, L.sa_in_bf, nullptr, a.qkv, 3 * d, SBK_ACT_NONE, pf);
    SBK_PSTEP_BARRIER(L.sa_out_w, d, d);
    // self-attention over the KV cache: a workgroup per (row, head)
    for (int it = blockIdx.x; it < a.n * a.H; it += G) attn_item<true>(a, L, xs, it / a.H, it % a.H);
    SBK_PSTEP_BARRIER((const float*)nullptr, 0, 0);
    stage_rows<false>(a, xs, a.ctx, d);
    tiles_gemm(a, xs, red, d, L.sa_out_w, L.sa_out_b, a.x, a.x, d, SBK_ACT_NONE, pf);
    SBK_PSTEP_BARRIER(L.ca_q_wf, d, d);
    // norm2 + the query rows of the cross-attention in_proj
    stage_rows<true>(a, xs, a.x, d);
    tiles_gemm(a, xs, red, d, L.ca_q_wf, L.ca_q_bf, nullptr, a.q, d, SBK_ACT_NONE, pf);
    SBK_PSTEP_BARRIER(L.ca_out_w, d, d);
    for (int it = blockIdx.x; it < a.n * a.H; it += G) attn_item<false>(a, L, xs, it / a.H, it % a.H);
    SBK_PSTEP_BARRIER((const float*)nullptr, 0, 0);
    stage_rows<false>(a, xs, a.ctx, d);
    tiles_gemm(a, xs, red, d, L.ca_out_w, L.ca_out_b, a.x, a.x, d, SBK_ACT_NONE, pf);
    SBK_PSTEP_BARRIER(L.ff1_wf, d, a.dffn);
    // norm3 + the feed-forward pair
    stage_rows<true>(a, xs, a.x, d);
    tiles_gemm(a, xs, red, d, L.ff1_wf, L.ff1_bf, nullptr, a.ff, a.dffn, a.act, pf);
    SBK_PSTEP_BARRIER(L.ff2_w, a.dffn, d);
    stage_rows<false>(a, xs, a.ff, a.dffn);
    tiles_gemm(a, xs, red, a.dffn, L.ff2_w, L.ff2_b, a.x, a.x, d, SBK_ACT_NONE, pf);
    if (l + 1 < a.nl) {
      SBK_PSTEP_BARRIER(a.L[l + 1].sa_in_wf, d, 3 * d);
    } else if (a.want_logits) {
      SBK_PSTEP_BARRIER(a.seq_wf, d, a.V);
    } else {
      SBK_PSTEP_BARRIER((const float*)nullptr, 0, 0);
    }
  }
#undef SBK_PSTEP_BARRIER
  // decoder.norm (+ seq_lin): every workgroup normalises the rows for its column tiles; workgroup 0 also writes h
  stage_rows<true>(a, xs, a.x, d);
  if (blockIdx.x == 0 && a.h) {
    for (int idx = tid; idx < a.n * d; idx += 256) {
      const int row = idx / d, c = idx - row * d;
      a.h[idx] = xs[row * (d + 4) + c] * a.fin_g[c] + a.fin_b[c];
    }
  }
  if (a.want_logits) tiles_gemm(a, xs, red, d, a.seq_wf, a.seq_bf, nullptr, a.logits, a.V, SBK_ACT_NONE, pf);
  SBK_PSTEP_STAMP();
#undef SBK_PSTEP_STAMP
}

}  // namespace

namespace sbk {

int g_persist = 1;        // tuning knob (key 47): 0 = off; 1 = the persistent step for <= 16 hypothesis rows; 2 = the same as a PLAIN launch
                          // (18.9 against 19.7 ms per 10-s utterance: no ~11-us gaps around the kernel -- but ONLY safe while one search at a
                          // time uses the device: the cooperative queue runs such kernels one after the other, plain launches of several
                          // searches could each keep part of the CUs and spin on the rest)
int g_persist_grid = 128; // tuning knob (key 48): workgroups of the cooperative launch (clamped to what the device holds)
int g_persist_tree = 1;   // key 59: 1 (default) = the grid barriers count arrivals on eight sub-counters + a top counter (0 = one counter):
                          // the persistent step 324 against 395 us, a 10-s utterance 19.7 against 22.6 ms (profiles/r06_o_*)
int g_persist_stamps = 0; // measurement knob (key 49): phase time stamps of the launches (sbk_prof_persist_stamps reads the last launch's)
static long long* g_last_stamps = nullptr;  // device buffer of the most recent stamped launch (the caller's workspace)
static int g_last_stamp_count = 0;

// grid barriers of one launch: 1 (embedding) + 8 per layer
int persist_barriers(int n_layers) { return 1 + 8 * n_layers; }

// What a launch of this model needs and whether this device can make it: dynamic LDS of a workgroup, the LDS window raised, the
// largest co-resident grid, the architecture the hand-over protocol was validated on.  Cached per (device, LDS bytes): the graph
// decision of a search (persist_eligible) and every step (decoder_step_persist) read the SAME answer, and the occupancy query
// runs once, not per step.
struct PersistPlan {
  int dev;
  size_t lds;
  int maxg;  // 0 = not feasible on this device
};
static std::mutex g_plan_mu;
static std::vector<PersistPlan> g_plans;

static size_t persist_lds_bytes(const sbk_decoder_weights* W, int Lmax) {
  const int d = W->d_model, Kmax = d > W->d_ffn ? d : W->d_ffn;
  size_t region = (size_t)kPRows * (Kmax + 4);
  const size_t attn = 8 + 256 + (size_t)Lmax + 64;  // attn_item: wave maxima / sums / contexts + the row's cache slots
  if (region < attn) region = attn;
  // (the region is sized for the rows AND the attention scratch; red follows the rows' extent)
  return (region + 1024 + 64) * sizeof(float);
}

static int persist_max_grid(const sbk_decoder_weights* W, int Lmax, size_t* lds_out) {
  const size_t lds = persist_lds_bytes(W, Lmax);
  if (lds_out) *lds_out = lds;
  if (lds > 160 * 1024 - 512) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  std::lock_guard<std::mutex> lk(g_plan_mu);
  for (const PersistPlan& p : g_plans)
    if (p.dev == dev && p.lds == lds) return p.maxg;
  PersistPlan p{dev, lds, 0};
  hipDeviceProp_t prop;
  // agent-scope relaxed accesses + a drained vmcnt as the hand-over between workgroups is outside the HIP memory model: it is
  // what gfx950 does (tools/persist_probe.hip, profiles/r05_a_*), so the path is offered on that architecture only
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0 &&
      allow_dyn_lds(decoder_step_persist_kernel, 160 * 1024 - 512) == hipSuccess) {
    int maxg = 0;
    if (SBK_COOP_MAX_GRID(decoder_step_persist_kernel, 256, lds, maxg) == hipSuccess && maxg >= 1) p.maxg = maxg;
  }
  if (p.maxg == 0) (void)hipGetLastError();  // (a failed query must not surface in the next launch_status())
  g_plans.push_back(p);
  return p.maxg;
}

bool persist_eligible(const sbk_decoder_weights* W, int n, int B, int beam, int Lmax) {
  if (!g_persist || n < 1 || n > kPRows || beam < 1 || beam > kPRows || B * beam != n) return false;
  const int d = W->d_model;
  if (W->n_layers < 1 || W->n_layers > kMaxPLayers || W->nhead < 1 || d != W->nhead * 64 || d > 1024 || W->d_ffn % 64 != 0) return false;
  if (!W->emb || !W->pe || !W->final_ln_g || !W->final_ln_b) return false;
  if (W->seq_w && !(W->seq_wf && W->seq_bf && aligned16(W->seq_wf))) return false;
  for (int l = 0; l < W->n_layers; ++l) {
    const sbk_decoder_layer& L = W->layers[l];
    if (!(L.sa_in_wf && L.sa_in_bf && L.ca_q_wf && L.ca_q_bf && L.ff1_wf && L.ff1_bf && L.sa_out_w && L.ca_out_w && L.ff2_w)) return false;
    if (!(aligned16(L.sa_in_wf) && aligned16(L.ca_q_wf) && aligned16(L.ff1_wf) && aligned16(L.sa_out_w) && aligned16(L.ca_out_w) &&
          aligned16(L.ff2_w)))
      return false;
  }
  return Lmax <= 16384 && persist_max_grid(W, Lmax, nullptr) >= 1;
}

// One decoder step for n <= 16 hypothesis rows (n = B * beam) at position `step`: d.x .. d.logits as decoder_step leaves
// them (the final LayerNorm output in h, the seq_lin logits when want_logits).  bar / bar_seq: the search's barrier counter
// (zero when the search starts) and the number of persistent launches issued on it so far.  grid_io: the search's grid (0 = not
// chosen yet): chosen by the FIRST launch of a search and kept for all of them -- the barrier targets are bar_seq * barriers * G,
// so a grid that changed between two launches (knob 48, another occupancy answer) would leave the counter past every target and
// every barrier would fall through.
int decoder_step_persist(const sbk_decoder_weights* W, const int32_t* tokens, const int32_t* kv_slot, const int32_t* enc_len,
                         float* x, float* qkv, float* ctx, float* q, float* ff, float* h, float* logits, float* const* kcache,
                         float* const* vcache, float* const* ckv, int* bar, int bar_seq, int* grid_io, int step, int n, int B, int T,
                         int beam, int Lmax, bool want_logits, hipStream_t st) {
  PStepArgs a;
  // (bar points at 64 ints; the stamps live behind them in the same carve: 256 x 8 bytes)
  a.stamps = g_persist_stamps ? reinterpret_cast<long long*>(bar + 64) : nullptr;
  if (a.stamps) {
    g_last_stamps = a.stamps;
    g_last_stamp_count = 2 + 2 * persist_barriers(W->n_layers);
  }
  const int d = W->d_model;
  for (int l = 0; l < W->n_layers; ++l) {
    const sbk_decoder_layer& L = W->layers[l];
    a.L[l] = PLayer{L.sa_in_wf, L.sa_in_bf, L.sa_out_w, L.sa_out_b, L.ca_q_wf, L.ca_q_bf, L.ca_out_w, L.ca_out_b,
                    L.ff1_wf, L.ff1_bf, L.ff2_w, L.ff2_b, kcache[l], vcache[l], ckv[l]};
  }
  a.tok = tokens; a.kv_slot = kv_slot; a.enc_len = enc_len;
  a.emb = W->emb; a.pe_row = W->pe + (size_t)step * d;
  a.x = x; a.qkv = qkv; a.ctx = ctx; a.q = q; a.ff = ff; a.h = h; a.logits = logits;
  a.fin_g = W->final_ln_g; a.fin_b = W->final_ln_b; a.seq_wf = W->seq_wf; a.seq_bf = W->seq_bf;
  a.bar = bar;
  a.n = n; a.B = B; a.T = T; a.beam = beam; a.d = d; a.H = W->nhead; a.dffn = W->d_ffn; a.V = W->vocab; a.nl = W->n_layers;
  a.step = step; a.Lmax = Lmax; a.act = W->ffn_act; a.want_logits = want_logits && W->seq_wf ? 1 : 0;
  a.eps = W->ln_eps; a.emb_scale = W->emb_scale > 0.0f ? W->emb_scale : sqrtf((float)d);
  a.attn_scale = 1.0f / sqrtf(64.0f);
  size_t lds = 0;
  const int maxg = persist_max_grid(W, Lmax, &lds);
  if (maxg < 1) return -1;
  int G = grid_io && *grid_io > 0 ? (*grid_io & 0xffff) : (g_persist_grid < 1 ? 1 : g_persist_grid);
  if (G > 0xffff) G = 0xffff;
  if (G > maxg) {
    if (grid_io && *grid_io > 0) return fail(SBK_EINVAL, "decoder_step_persist: the search's grid (%d) no longer fits the device (%d)", G, maxg);
    G = maxg;
  }
  const int tree = grid_io && *grid_io > 0 ? (*grid_io >> 16) & 1 : (g_persist_tree != 0);  // (fixed per search, like the grid)
  if (grid_io) *grid_io = G | (tree << 16);
  a.sub = bar + 64 + 512;  // (behind the flat counter's line and the stamps: carve_decoder)
  a.tree = tree;
  a.ord_base = bar_seq * persist_barriers(W->n_layers);
  a.bar_base = bar_seq * persist_barriers(W->n_layers) * G;
  ProfScope prof("decoder_step_persist", 2.0 * n * (double)(W->n_layers * (4.0 * d * d + 2.0 * d * W->d_ffn) + (want_logits ? (double)d * W->vocab : 0.0)),
                 4.0 * (W->n_layers * (4.0 * d * d + 2.0 * d * W->d_ffn) + (want_logits ? (double)d * W->vocab : 0.0)), st);
  if (g_persist == 2) {
    // OPT-IN (knob 47 = 2; one search per device at a time): the same grid as a PLAIN launch.  MI355X_MICROARCH.md: plain, cooperative
    // and graph launches give identical residency; the cooperative launch adds the check of the grid against the occupancy query
    // (done above: G <= maxg), an ~11-us gap on either side of the kernel in the B = 1 timeline (profiles/r06_h_*, r06_o_*) -- and
    // mutual exclusion among cooperative kernels, which is what makes several concurrent searches safe
    SBK_LAUNCH(decoder_step_persist_kernel, dim3(G), dim3(256), lds, st, a);
    return launch_status("decoder_step_persist");
  }
  const hipError_t e = SBK_LAUNCH_COOP(decoder_step_persist_kernel, dim3(G), dim3(256), lds, st, a);
  if (e != hipSuccess) return fail((int)e, "decoder_step_persist: cooperative launch: %s", hipGetErrorString(e));
  return 0;
}

}  // namespace sbk

// Measurement: the phase time stamps (100 MHz wall clock ticks) workgroup 0 wrote during the most recent stamped launch
// (knob 49): [start, (end of phase, end of barrier) x barriers, end].  Synchronises the device.  Returns the count.
extern "C" int sbk_prof_persist_stamps(long long* out, int cap) {
  if (!sbk::g_last_stamps || !out || cap <= 0) return 0;
  const int n = sbk::g_last_stamp_count < cap ? sbk::g_last_stamp_count : cap;
  if (hipDeviceSynchronize() != hipSuccess) return 0;
  if (hipMemcpy(out, sbk::g_last_stamps, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  return n;
}
