// WavLM self-attention: scaled-dot-product attention with the GATED RELATIVE-POSITION BIAS fused in
//                                                      (sbk_wavlm_attention_f32)
//   p      = gate_w x[b,i,h*Dh:(h+1)*Dh] + gate_b                      (8 values, gru_rel_pos_linear, shared by the heads)
//   ga, gb = sigmoid(p0+p1+p2+p3), sigmoid(p4+p5+p6+p7)
//   gate   = ga * (gb * gate_const[h] - 1) + 2
//   s[i,j] = scale * q_i.k_j + gate * tab[h, j - i + T - 1]            keys j < key_len[b]; the others -inf
//   out_i  = softmax_j(s[i,:]) V
// HuggingFace's WavLMAttention forms the bias as a [B*H, T, T] tensor per layer and hands it to
// F.multi_head_attention_forward.  The bias is a per-query scalar times a Toeplitz table of 2T-1 values per head
// (tab[h, r + T - 1] = rel_attn_embed[bucket(r), h], the same in every layer), so here nothing T x T reaches HBM.
//
// Scheme: that of rope_flash_t_kernel (csrc/relpos_attn.hip).  The wave computes S^T = K Q^T on v_mfma_f32_32x32x2, so a
// lane holds ONE query (its column jl) and 16 of the tile's 32 keys; the online-softmax statistics are lane-local, the
// probabilities are the B operand of O^T = V^T P^T as they stand.  One workgroup = 4 waves x 32 queries of one (batch, head).
// Added to it:
//   * the gate, in the prologue: the lane that owns query i loads its half of x's head slice (the run the Q load takes from
//     qkv) and dots it with the 8 x Dh/2 weights of its half; one shuffle with the other half-wave completes the 8 sums.
//   * the head's table row, staged ONCE per workgroup in LDS: 2T-1 floats and 31 zeros behind them, so that the keys of a
//     ragged last tile (which are masked) read inside the allocation.  A lane reads
//         tab_s[(T - 1 - i) + j0 + keyoff(r, half)]
//     -- across the lanes of a half-wave the stride is -1 float: conflict-free.
//   * the bias, after the MFMA score tile and before the mask and the maximum: one fused multiply-add per accumulator register.
// LDS: 4 (2T + 30) bytes per workgroup -- 12 KB at T = 1499 (30 s of audio), 64 KiB at the bound T = 8177: two workgroups
// per CU, as __launch_bounds__(256, 2) asks of the registers, at every accepted T, and no LDS opt-in.
#include "act.h"
#include "common.h"
#include "internal.h"
#include "kernel_util.h"

namespace {

using sbk::f32x16;
using sbk::load_run;

constexpr int kTabPad = 31;                          // zeros behind the table row: the masked keys of a ragged last tile
constexpr int kMaxT = (65536 / 4 - kTabPad + 1) / 2;  // 2T - 1 + 31 floats <= 64 KiB: T <= 8177

struct WavlmArgs {
  const float* qkv;        // [B,T,H,3*DH]
  const float* x;          // [B,T,H*DH]
  const float* gate_w;     // [8,DH]
  const float* gate_b;     // [8]
  const float* gate_const; // [H]
  const float* tab;        // [H,2T-1]
  const int32_t* key_len;  // [B] or null
  float* out;              // [B,T,H*DH]
  int B, T, H;
  float scale;
};

template <int DH>
__global__ void __launch_bounds__(256, 2) wavlm_flash_t_kernel(WavlmArgs a) {
  constexpr int DH2 = DH / 2;
  constexpr int NC = (DH + 31) / 32;
  SBK_DYN_LDS(float, tab_s);  // [2T - 1 + kTabPad]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int jl = lane & 31, half = lane >> 5;
  const int i0 = (blockIdx.x * 4 + wave) * 32, h = blockIdx.y, b = blockIdx.z;
  const int T = a.T, d = a.H * DH;
  {
    const int n = 2 * T - 1;
    const float* row = a.tab + (size_t)h * n;
    for (int e = tid; e < n + kTabPad; e += 256) tab_s[e] = e < n ? row[e] : 0.0f;
  }
  __syncthreads();
  if (i0 >= T) return;  // (a wave without queries: after the workgroup's only barrier)
  const size_t row3 = (size_t)3 * d;
  const float* qkv_b = a.qkv + (size_t)b * T * row3 + (size_t)h * 3 * DH;
  const int qrow = min(i0 + jl, T - 1);  // this lane's query (B operand column / output row)

  float gate;
  {
    float xr[DH2];
    load_run<DH2>(xr, a.x + ((size_t)b * T + qrow) * d + h * DH + half * DH2);
    float p[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      float w[DH2];
      load_run<DH2>(w, a.gate_w + g * DH + half * DH2);
      float s = 0.0f;
#pragma unroll
      for (int c = 0; c < DH2; ++c) s = fmaf(w[c], xr[c], s);
      p[g] = s + sbk::shfl_xor(s, 32) + a.gate_b[g];
    }
    const float ga = sbk::sigmoid((p[0] + p[1]) + (p[2] + p[3])), gb = sbk::sigmoid((p[4] + p[5]) + (p[6] + p[7]));
    gate = ga * (gb * a.gate_const[h] - 1.0f) + 2.0f;
  }

  float qu[DH2];
  load_run<DH2>(qu, qkv_b + (size_t)qrow * row3 + half * DH2);
#pragma unroll
  for (int s = 0; s < DH2; ++s) qu[s] *= a.scale;

  int klen = T;
  if (a.key_len) klen = min(max(a.key_len[b], 1), T);
  const int nkt = (klen + 31) / 32;
  // this lane's window of the table: entry (key - qrow + T - 1) of the row; + 4*half = its half-wave's keys of a register
  const float* tq = tab_s + (T - 1 - qrow) + 4 * half;
  float m_run = -INFINITY, l_run = 0.0f;
  f32x16 o[NC];
#pragma unroll
  for (int ct = 0; ct < NC; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[ct][r] = 0.0f;

  for (int kt = 0; kt < nkt; ++kt) {
    const int j0 = kt * 32;
    float kreg[DH2];
    load_run<DH2>(kreg, qkv_b + (size_t)min(j0 + jl, T - 1) * row3 + DH + half * DH2);
    f32x16 acc;  // S^T: row = key (r&3) + 8(r>>2) + 4*half of the tile, column = query jl
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
    for (int s = 0; s < DH2; ++s) acc = sbk::mfma_32x32x2(kreg[s], qu[s], acc);
    // V^T operand of the second product, in the key order of the accumulator registers (requested before the softmax)
    float vv[NC][16];
#pragma unroll
    for (int ct = 0; ct < NC; ++ct) {
      const int col = ct * 32 + jl;
      const float* vbase = qkv_b + 2 * DH + (col < DH ? col : 0);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = min(j0 + (r & 3) + 8 * (r >> 2) + 4 * half, T - 1);
        vv[ct][r] = col < DH ? vbase[(size_t)t * row3] : 0.0f;
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ko = (r & 3) + 8 * (r >> 2);  // (j0 + ko + 4*half <= nkt*32 - 1 <= T + 30: inside the padded row)
      acc[r] = fmaf(gate, tq[j0 + ko], acc[r]);
      if (j0 + ko + 4 * half >= klen) acc[r] = -INFINITY;
      mx = fmaxf(mx, acc[r]);
    }
    mx = fmaxf(mx, sbk::shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = m_new == -INFINITY ? 1.0f : expf(m_run - m_new);
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc[r] = acc[r] == -INFINITY ? 0.0f : expf(acc[r] - m_new);
      sum += acc[r];
    }
    sum += sbk::shfl_xor(sum, 32);
    l_run = l_run * alpha + sum;
    m_run = m_new;
#pragma unroll
    for (int ct = 0; ct < NC; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int ct = 0; ct < NC; ++ct) o[ct] = sbk::mfma_32x32x2(vv[ct][r], acc[r], o[ct]);
  }
  // O^T: column = this lane's query, row = channel (r&3) + 8(r>>2) + 4*half + 32*ct
  if (i0 + jl < T) {
    const float inv = l_run > 0.0f ? 1.0f / l_run : 0.0f;
    float* orow = a.out + ((size_t)b * T + i0 + jl) * d + h * DH;
#pragma unroll
    for (int ct = 0; ct < NC; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = ct * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (c < DH) orow[c] = o[ct][r] * inv;
      }
  }
}

template <int DH>
int launch_wavlm(const WavlmArgs& a, hipStream_t st) {
  const size_t lds = (size_t)(2 * a.T - 1 + kTabPad) * sizeof(float);
  sbk::ProfScope prof("wavlm_attention", 4.0 * a.B * a.H * (double)a.T * a.T * DH + 2.0 * a.B * a.H * (double)a.T * a.T,
                      4.0 * a.B * a.T * (5.0 * a.H * DH) + 4.0 * (2.0 * a.T - 1) * a.H, st);
  SBK_LAUNCH((wavlm_flash_t_kernel<DH>), dim3((a.T + 127) / 128, a.H, a.B), dim3(256), lds, st, a);
  return sbk::launch_status("sbk_wavlm_attention_f32");
}

}  // namespace

extern "C" int sbk_wavlm_attention_max_frames(void) { return kMaxT; }

extern "C" int sbk_wavlm_attention_f32(const float* qkv, const float* x, const float* gate_w, const float* gate_b,
                                       const float* gate_const, const float* tab, const int32_t* key_len, float* out, int B,
                                       int T, int H, int Dh, float scale, sbk_stream_t stream) {
  SBK_REQUIRE(B >= 0 && T >= 0 && H > 0 && Dh > 0, "wavlm_attention: bad shape");
  if (B == 0 || T == 0) return 0;  // empty batch: nothing to launch, the data pointers may be NULL
  SBK_REQUIRE(qkv && x && gate_w && gate_b && gate_const && tab && out, "wavlm_attention: null operand");
  SBK_REQUIRE(Dh == 64 || Dh == 32 || Dh == 16, "wavlm_attention: head_dim %d not instantiated (16,32,64)", Dh);
  SBK_REQUIRE(T <= kMaxT, "wavlm_attention: T=%d frames: the head's bias table (2T-1 floats) is staged in 64 KiB of LDS, T <= %d",
              T, kMaxT);
  SBK_REQUIRE(sbk::aligned16(qkv) && sbk::aligned16(x) && sbk::aligned16(gate_w),
              "wavlm_attention: qkv, x and gate_w must be 16-byte aligned");
  const WavlmArgs a{qkv, x, gate_w, gate_b, gate_const, tab, key_len, out, B, T, H, scale};
  const hipStream_t st = sbk::as_stream(stream);
  switch (Dh) {
    case 64: return launch_wavlm<64>(a, st);
    case 32: return launch_wavlm<32>(a, st);
    default: return launch_wavlm<16>(a, st);
  }
}
