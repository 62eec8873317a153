// Convolutional Spatial Gating Unit of the Branchformer cgMLP branch      (sbk_csgu_f32)
//
// lobes/models/convolution.py:92-113:  x1, x2 = h.chunk(2, -1);  y = act(conv(LayerNorm(x2))) * x1, where conv is
// nnet/CNN.py Conv1d(padding="same", padding_mode="reflect", groups = C): a depthwise filter over time whose padding
// MIRRORS the sequence at both ends of the padded batch length T (F.pad "reflect": index -i -> i, T-1+i -> T-1-i).
// Nothing is masked by utterance length: the reference runs this branch unmasked (Branchformer.py:224-228).
//
// Roofline: HBM (12*C bytes per frame: read [T,2C], write [T,C]; 2*ksize + 8 flop per output element).
//  1. csgu_stats_kernel: mean and 1/std of every frame's x2 half (one wave per frame, the half row in registers, mean
//     first and then the squared deviations, like layernorm_kernel) into the caller's scratch [B*T][2] -- the statistics
//     need all C channels of a frame, the convolution tile below holds 64 of them.
//  2. csgu_kernel: one workgroup = (batch, 64-frame tile, 64-channel tile).  The NORMALISED x2 of the tile plus the
//     (ksize-1)-frame halo -- reflected where it leaves [0,T) -- is staged once into LDS ([frame][channel], channel
//     fastest: a wave reads and writes 64 consecutive banks), each thread keeps the ksize taps of its channel and a
//     window of 16 + ksize - 1 staged frames in registers, slides over its 16 output frames, applies the gate
//     activation and multiplies by x1 on the way out.
#include "act.h"
#include "common.h"

namespace {

constexpr int kTT = 64;             // output frames per workgroup
constexpr int kCT = 64;             // channels per workgroup
constexpr int kNOUT = kTT / 4;      // output frames per thread (4 waves = 4 frame quarters)

// The gate's activation: NONE, SWISH, GELU or RELU (sbk_csgu_f32 refuses the rest).  Not sbk::act: its LEAKY_RELU arm, which
// no launch can reach, would add 580 bytes to every instantiation of csgu_kernel.
__device__ __forceinline__ float gate_f(float v, int act) {
  if (act == SBK_ACT_SWISH) return sbk::swish(v);
  if (act == SBK_ACT_GELU) return sbk::gelu_erf(v);
  if (act == SBK_ACT_RELU) return sbk::relu(v);
  return v;
}

// stats[row] = {mean, rstd} of h[row][C : 2C]   (biased variance, eps inside the root, as torch.nn.LayerNorm)
// MAXV = float4 slots kept in registers per lane (C % 4 == 0, C <= 256 * MAXV): the half row is read once with 16-byte loads,
// all requested before the first is used (layernorm_kernel's form, csrc/norm.hip).
template <int MAXV>
__global__ void __launch_bounds__(256) csgu_stats_kernel(const float* __restrict__ h, float* __restrict__ stats, int rows,
                                                         int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = row < rows;
  // idle waves shadow the last row: shuffles stay full-width
  const float4* xr = reinterpret_cast<const float4*>(h + (size_t)(live ? row : rows - 1) * 2 * C + C);
  const int nv = C >> 2;
  float4 v[MAXV];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) v[i] = xr[min(lane + i * 64, nv - 1)];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    if (lane + i * 64 >= nv) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = sbk::wave_sum(s) / (float)C;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i)
    if (lane + i * 64 < nv) {
      const float a = v[i].x - mean, b = v[i].y - mean, cc = v[i].z - mean, dd = v[i].w - mean;
      q += (a * a + b * b) + (cc * cc + dd * dd);
    }
  const float rstd = rsqrtf(sbk::wave_sum(q) / (float)C + eps);
  if (live && lane == 0) {
    stats[(size_t)row * 2] = mean;
    stats[(size_t)row * 2 + 1] = rstd;
  }
}

// Any C (scalar loads, two passes over an L1/L2-resident half row).
__global__ void __launch_bounds__(256) csgu_stats_generic_kernel(const float* __restrict__ h, float* __restrict__ stats,
                                                                 int rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = row < rows;
  const float* xr = h + (size_t)(live ? row : rows - 1) * 2 * C + C;
  float s = 0.0f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mean = sbk::wave_sum(s) / (float)C;
  float q = 0.0f;
  for (int c = lane; c < C; c += 64) {
    const float a = xr[c] - mean;
    q += a * a;
  }
  const float rstd = rsqrtf(sbk::wave_sum(q) / (float)C + eps);
  if (live && lane == 0) {
    stats[(size_t)row * 2] = mean;
    stats[(size_t)row * 2 + 1] = rstd;
  }
}

template <int KS>
__global__ void __launch_bounds__(256) csgu_kernel(const float* __restrict__ h, const float* __restrict__ stats,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ y, int T, int C, int act) {
  constexpr int HALO = (KS - 1) / 2;
  constexpr int ROWS = kTT + KS - 1;
  constexpr int NI = (ROWS + 3) / 4;  // staged rows per thread
  __shared__ float g[ROWS][kCT];
  const int tid = threadIdx.x;
  const int t0 = blockIdx.x * kTT, c0 = blockIdx.y * kCT, b = blockIdx.z;
  const int c = tid & 63, tq = sbk::uniform(tid >> 6);  // (the wave index: a frame's statistics are one scalar load per wave)
  const int ch = c0 + c;
  const bool ch_ok = ch < C;
  const int chc = ch_ok ? ch : C - 1;  // loads are unconditional on clamped addresses (a load under a lane mask is a branch and a full wait)
  const float* hb = h + (size_t)b * T * 2 * C;
  const float* sb = stats + (size_t)b * T * 2;
  const float gm = gamma[chc], bt = beta[chc];
  // stage: every row of the tile requested before the first is used
  float xv[NI], mu[NI], rs[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int t = t0 + tq + 4 * i - HALO;
    // reflect padding over the padded batch length (T > HALO: one reflection reaches every frame an output of [0,T) reads);
    // rows of a ragged last tile that no such output reads fall outside [0,T) again: clamped here, zeroed below
    const int s = t < 0 ? -t : (t >= T ? 2 * (T - 1) - t : t);
    const int sc = min(max(s, 0), T - 1);
    xv[i] = hb[(size_t)sc * 2 * C + C + chc];
    mu[i] = sb[2 * sc];
    rs[i] = sb[2 * sc + 1];
  }
  float wk[KS];
#pragma unroll
  for (int k = 0; k < KS; ++k) wk[k] = w[(size_t)chc * KS + k];
  const float bv = bias[chc];
  const int tl = tq * kNOUT;
  float x1[kNOUT];  // the gate's other factor: requested here, used after the taps
#pragma unroll
  for (int o = 0; o < kNOUT; ++o) x1[o] = hb[(size_t)min(t0 + tl + o, T - 1) * 2 * C + chc];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int r = tq + 4 * i;
    const int t = t0 + r - HALO;
    const int s = t < 0 ? -t : (t >= T ? 2 * (T - 1) - t : t);
    if (r < ROWS) g[r][c] = (ch_ok && s >= 0 && s < T) ? (xv[i] - mu[i]) * rs[i] * gm + bt : 0.0f;
  }
  __syncthreads();
  float win[kNOUT + KS - 1];  // every staged frame is read from LDS once per thread, not once per tap
#pragma unroll
  for (int i = 0; i < kNOUT + KS - 1; ++i) win[i] = g[tl + i][c];
#pragma unroll
  for (int o = 0; o < kNOUT; ++o) {
    const int t = t0 + tl + o;
    float acc = bv;
#pragma unroll
    for (int k = 0; k < KS; ++k) acc = fmaf(wk[k], win[o + k], acc);  // orientation of torch conv1d: tap k reads frame t + k - HALO
    if (ch_ok && t < T) y[((size_t)b * T + t) * C + ch] = gate_f(acc, act) * x1[o];
  }
}

}  // namespace

extern "C" int sbk_csgu_f32(const float* h, const float* gamma, const float* beta, float eps, const float* w,
                            const float* bias, float* y, float* stats, int B, int T, int C, int ksize, int gate_act,
                            sbk_stream_t stream) {
  SBK_REQUIRE(B >= 0 && T >= 0 && C > 0 && B <= 65535 && (double)B * T < 1073741824.0, "csgu: bad shape B=%d T=%d C=%d", B, T, C);
  SBK_REQUIRE(ksize == 3 || ksize == 5 || ksize == 7 || ksize == 15 || ksize == 31,
              "csgu: kernel size %d not instantiated (3,5,7,15,31)", ksize);
  if (B == 0 || T == 0) return 0;  // empty batch: nothing to launch, the data pointers may be NULL
  SBK_REQUIRE(T > (ksize - 1) / 2, "csgu: T=%d frames cannot be reflect-padded by %d (ksize=%d needs T > (ksize-1)/2)", T,
              (ksize - 1) / 2, ksize);
  SBK_REQUIRE(gate_act == SBK_ACT_NONE || gate_act == SBK_ACT_SWISH || gate_act == SBK_ACT_GELU || gate_act == SBK_ACT_RELU,
              "csgu: gate activation %d (none, swish, gelu, relu)", gate_act);
  SBK_REQUIRE(h && gamma && beta && w && bias && y && stats, "csgu: null operand");
  hipStream_t st = sbk::as_stream(stream);
  const double n = (double)B * T * C;
  {
    sbk::ProfScope prof("csgu_stats", 5.0 * n, 4.0 * n + 8.0 * B * T, st);
    const dim3 sgrid(sbk::cdiv(B * T, 4)), sblock(256);
    if (C % 4 == 0 && sbk::aligned16(h) && C <= 256 * 2) {
      SBK_LAUNCH((csgu_stats_kernel<2>), sgrid, sblock, 0, st, h, stats, B * T, C, eps);
    } else if (C % 4 == 0 && sbk::aligned16(h) && C <= 256 * 8) {  // the recipe's 1 536 channels
      SBK_LAUNCH((csgu_stats_kernel<8>), sgrid, sblock, 0, st, h, stats, B * T, C, eps);
    } else {
      SBK_LAUNCH(csgu_stats_generic_kernel, sgrid, sblock, 0, st, h, stats, B * T, C, eps);
    }
  }
  dim3 grid(sbk::cdiv(T, kTT), sbk::cdiv(C, kCT), B), block(256);
  sbk::ProfScope prof("csgu", (2.0 * ksize + 8.0) * n, 12.0 * n + 8.0 * B * T, st);
  switch (ksize) {
    case 31: SBK_LAUNCH((csgu_kernel<31>), grid, block, 0, st, h, stats, gamma, beta, w, bias, y, T, C, gate_act); break;
    case 15: SBK_LAUNCH((csgu_kernel<15>), grid, block, 0, st, h, stats, gamma, beta, w, bias, y, T, C, gate_act); break;
    case 7: SBK_LAUNCH((csgu_kernel<7>), grid, block, 0, st, h, stats, gamma, beta, w, bias, y, T, C, gate_act); break;
    case 5: SBK_LAUNCH((csgu_kernel<5>), grid, block, 0, st, h, stats, gamma, beta, w, bias, y, T, C, gate_act); break;
    default: SBK_LAUNCH((csgu_kernel<3>), grid, block, 0, st, h, stats, gamma, beta, w, bias, y, T, C, gate_act); break;
  }
  return sbk::launch_status("sbk_csgu_f32");
}
