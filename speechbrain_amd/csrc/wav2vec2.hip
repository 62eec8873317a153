// wav2vec 2.0: the first convolution of the feature encoder over the raw waveform, and the grouped positional convolution
//                                                (sbk_w2v_conv0_stats_f32, sbk_w2v_conv0_f32, sbk_w2v_posconv_f32)
//
// ---- layer 0 of the feature encoder (HuggingFace Wav2Vec2GroupNormConvLayer / Wav2Vec2LayerNormConvLayer, C_in = 1)
//   y[b,t,c] = bias[c] + sum_j w[c,j] * x'[b, t*s + j],   x' = (wav - mu_b) * r_b  (the feature extractor's do_normalize) or wav
//   "group": GroupNorm(C0, C0) -- per (utterance, channel) mean / variance over ALL T0 frames of the padded row -- then GELU
//   "layer": LayerNorm over the C0 channels of a frame, then GELU
// written time-major [B,T0,C0], which the strided-window GEMM of layers 1-6 reads in place.
//
// Roofline: HBM writes (4 bytes per output element, written exactly once; the waveform is 1/C0 of that).  The group-norm
// statistics do NOT need the conv output: it is linear in the waveform, so with m = the mean and Cov = the covariance of the
// stride-s windows of an utterance (a k-vector and a k x k matrix),  mean_c = w_c . m + bias_c  and  var_c = w_c^T Cov w_c.
//  1. w2v_moments_kernel<0>: per (utterance, chunk of frames) the sums of the samples and of the k window taps (fp64 partials);
//  2. w2v_moments_kernel<1>: the same chunks again, CENTRED on the means of pass 1: sum (x - mu)^2 and the k(k+1)/2 products
//     (x_i - m_i)(x_j - m_j).  Centring first is what keeps a DC offset out of the variance (E[y^2] - E[y]^2 loses there);
//  3. w2v_conv0_finalize_kernel: sums the partials, writes (mu, r) of the waveform and (mean, rstd) of every channel.
// All three accumulate in fp64 (a few million fp64 fma per utterance: nothing next to the main pass).
//  4. w2v_conv0_kernel: one workgroup = (utterance, 32 frames, all channels).  The normalised window of the waveform is staged
//     in LDS (a broadcast read per tap), each thread keeps the taps of its channels and its 32 x CPT outputs in registers;
//     "layer" statistics are reduced across the workgroup per frame (mean first, then the squared deviations).
//
// ---- positional convolution (Wav2Vec2PositionalConvEmbedding + the masking of Wav2Vec2Encoder.forward in front of it)
//   xm = x with the frames >= key_len[b] zeroed;  out = xm + GELU(conv(xm) + bias), conv = Conv1d(d, d, k, padding k/2, groups G)
//   with the last frame dropped for even k: out frame t reads frames t - k/2 + j, j < k.
// Per group a [T x cg*k] . [cg*k x cg] product: matrix cores, v_mfma_f32_16x16x4_f32 (cg is a multiple of 16, not of 32).
// One workgroup = (utterance, group, 64 frames): the (64 + k - 1)-frame halo of the group's cg channels is staged ONCE in LDS,
// masked on the way in (rows outside [0, key_len) are zeros; never another utterance's frames), and re-used by all k taps.
// Waves: 2 frame halves x 2 tap parities; each holds 2 x cg/16 accumulator tiles and reads per 16 input channels of a tap one
// float4 of the halo per frame tile and one float4 of the tap-major weight [d][k*cg] per channel tile (the k index inside an
// instruction is permuted so that both are contiguous).  Taps whose 32 halo rows are all padding are skipped.  The two
// parities are summed through LDS; bias, GELU and the residual (the halo's centre rows) are applied on the way out.
// With (gamma, beta) the LayerNorm over d follows as a second launch, in place (a row needs all G groups).
#include "act.h"
#include "common.h"

namespace {

constexpr int kMaxK = 16;                      // taps of layer 0
constexpr int kPairs = kMaxK * (kMaxK + 1) / 2;
constexpr int kSlot = kMaxK + 1 + kPairs + 1;  // doubles per (utterance, chunk): k tap sums, sample sum | pairs, squares

static inline int w2v_chunk_frames(int s) { return ((12288 / s) / 64) * 64; }

// PASS 0: ws[b][blk][0..k) = sum over the chunk's frames of x[t*s + j],  [kMaxK] = sum of the chunk's samples
// PASS 1: ws[b][blk][kMaxK+1 + p] = sum of (x_i - m_i)(x_j - m_j) for pair p = (i <= j),  [kSlot-1] = sum (x - mu)^2
template <int PASS>
__global__ void __launch_bounds__(256) w2v_moments_kernel(const float* __restrict__ wav, double* __restrict__ ws, int N, int T0,
                                                          int k, int s, int FR, int nblk) {
  __shared__ double red[256];
  __shared__ double mean[kMaxK + 1];
  __shared__ double acc_out[kPairs + 1];
  const int tid = threadIdx.x, blk = blockIdx.x, b = blockIdx.y;
  const float* x = wav + (size_t)b * N;
  double* slot = ws + ((size_t)b * nblk + blk) * kSlot;
  const int f0 = blk * FR, f1 = min(f0 + FR, T0);
  const long n0 = (long)f0 * s, n1 = blk == nblk - 1 ? (long)N : (long)(f0 + FR) * s;  // this chunk's share of the samples
  if (PASS == 1) {
    if (tid <= kMaxK) {
      double a = 0.0;
      for (int q = 0; q < nblk; ++q) a += ws[((size_t)b * nblk + q) * kSlot + tid];
      mean[tid] = a / (tid == kMaxK ? (double)N : (double)T0);
    }
    __syncthreads();
  }
  // ---- the per-sample sum
  {
    const double mu = PASS == 1 ? mean[kMaxK] : 0.0;
    double a = 0.0;
    for (long n = n0 + tid; n < n1; n += 256) {
      const double v = (double)x[n] - mu;
      a += PASS == 1 ? v * v : v;
    }
    red[tid] = a;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (tid < h) red[tid] += red[tid + h];
      __syncthreads();
    }
    if (tid == 0) slot[PASS == 1 ? kSlot - 1 : kMaxK] = red[0];
    __syncthreads();
  }
  // ---- the window sums: 32 column lanes (a tap, or a pair of taps) x 8 frame groups
  const int col = tid & 31, fg = tid >> 5;
  const int ncol = PASS == 1 ? k * (k + 1) / 2 : k;
  for (int c0 = 0; c0 < ncol; c0 += 32) {
    const int c = c0 + col;
    int i = 0, j = 0;
    if (PASS == 1) {  // pair index -> (i <= j), row-major over the upper triangle
      int p = min(c, ncol - 1);
      while (p >= k - i) {
        p -= k - i;
        ++i;
      }
      j = i + p;
    } else {
      i = j = min(c, k - 1);
    }
    const double mi = PASS == 1 ? mean[i] : 0.0, mj = PASS == 1 ? mean[j] : 0.0;
    double a = 0.0;
    if (c < ncol)
      for (int f = f0 + fg; f < f1; f += 8) {
        const float* xw = x + (size_t)f * s;
        a += PASS == 1 ? ((double)xw[i] - mi) * ((double)xw[j] - mj) : (double)xw[i];
      }
    red[tid] = a;
    __syncthreads();
    if (tid < 32) {
      double t = 0.0;
      for (int q = 0; q < 8; ++q) t += red[q * 32 + tid];
      if (c < ncol) acc_out[min(c, kPairs)] = t;
    }
    __syncthreads();
  }
  for (int c = tid; c < ncol; c += 256) slot[(PASS == 1 ? kMaxK + 1 : 0) + c] = acc_out[c];
}

// wstat[b] = {mu, rstd} of the whole padded row (F.layer_norm(wav, wav.shape[1:]), eps inside the root) when `normalize`;
// cstat[b][c] = {mean, rstd} over the T0 frames of channel c of the convolution of the (normalised) waveform, when w is given
__global__ void __launch_bounds__(256) w2v_conv0_finalize_kernel(const double* __restrict__ ws, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, float* __restrict__ wstat,
                                                                 float* __restrict__ cstat, int N, int T0, int C0, int k,
                                                                 int nblk, int normalize, float wav_eps, float eps) {
  __shared__ double tot[kSlot];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int e = tid; e < kSlot; e += 256) {
    double a = 0.0;
    for (int q = 0; q < nblk; ++q) a += ws[((size_t)b * nblk + q) * kSlot + e];
    tot[e] = a;
  }
  __syncthreads();
  const double mu_raw = tot[kMaxK] / (double)N;
  const double var_raw = tot[kSlot - 1] / (double)N;
  const double mu = normalize ? mu_raw : 0.0;
  const double r = normalize ? 1.0 / sqrt(var_raw + (double)wav_eps) : 1.0;
  if (tid == 0 && wstat) {
    wstat[2 * b] = (float)mu_raw;
    wstat[2 * b + 1] = (float)(1.0 / sqrt(var_raw + (double)wav_eps));
  }
  if (!w) return;
  for (int c = tid; c < C0; c += 256) {
    const float* wc = w + (size_t)c * k;
    double m = bias ? (double)bias[c] : 0.0, v = 0.0;
    int p = kMaxK + 1;
    for (int i = 0; i < k; ++i) {
      m += (double)wc[i] * (tot[i] / (double)T0 - mu) * r;
      for (int j = i; j < k; ++j, ++p) v += (i == j ? 1.0 : 2.0) * (double)wc[i] * (double)wc[j] * (tot[p] / (double)T0);
    }
    v = fmax(v * r * r, 0.0);
    cstat[((size_t)b * C0 + c) * 2] = (float)m;
    cstat[((size_t)b * C0 + c) * 2 + 1] = (float)(1.0 / sqrt(v + (double)eps));
  }
}

constexpr int kC0TT = 32;       // frames per workgroup of the main pass
constexpr int kModeGroup = 1, kModeLayer = 2;

template <int CPT, int MODE, int KU>  // KU: taps unrolled (>= k; the taps past k carry a zero weight)
__global__ void __launch_bounds__(256) w2v_conv0_kernel(const float* __restrict__ wav, const float* __restrict__ wstat,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        const float* __restrict__ cstat, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ y, int N, int T0,
                                                        int C0, int k, int s, float eps) {
  __shared__ float xs[(kC0TT - 1) * kMaxK + kMaxK];
  __shared__ float red[kC0TT][16];
  __shared__ float stat[kC0TT];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int t0 = blockIdx.x * kC0TT;
  const int nf = min(kC0TT, T0 - t0);
  const float mu = wstat ? wstat[2 * b] : 0.0f, r = wstat ? wstat[2 * b + 1] : 1.0f;
  const float* x = wav + (size_t)b * N;
  const int span = (nf - 1) * s + k;  // t0*s + span <= (T0-1)*s + k <= N
  for (int i = tid; i < (kC0TT - 1) * kMaxK + kMaxK; i += 256) xs[i] = i < span ? (x[(size_t)t0 * s + i] - mu) * r : 0.0f;
  float wk[CPT][KU], bv[CPT], gm[CPT], bt[CPT], cm[CPT], cr[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int c = tid + 256 * i;
    const int cc = min(c, C0 - 1);
#pragma unroll
    for (int j = 0; j < KU; ++j) wk[i][j] = j < k ? w[(size_t)cc * k + j] : 0.0f;
    bv[i] = bias ? bias[cc] : 0.0f;
    gm[i] = gamma[cc];
    bt[i] = beta[cc];
    cm[i] = MODE == kModeGroup && T0 > kC0TT ? cstat[((size_t)b * C0 + cc) * 2] : 0.0f;
    cr[i] = MODE == kModeGroup && T0 > kC0TT ? cstat[((size_t)b * C0 + cc) * 2 + 1] : 1.0f;
  }
  __syncthreads();
  float acc[CPT][kC0TT];
#pragma unroll
  for (int f = 0; f < kC0TT; ++f) {
    const float* xw = xs + f * s;  // (frames >= nf read staged zeros or the tail of the window: inside xs, never stored)
    float xv[KU];
#pragma unroll
    for (int j = 0; j < KU; ++j) xv[j] = xw[min(j, k - 1)];
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      float a = 0.0f;
#pragma unroll
      for (int j = 0; j < KU; ++j) a = fmaf(wk[i][j], xv[j], a);
      acc[i][f] = a + bv[i];
    }
  }
  if (MODE == kModeLayer) {
    const int lane = tid & 63, wave = tid >> 6;
    float mean[kC0TT];
    // mean over the channels of every frame: 16-lane DPP sums, 16 partials per frame through LDS
#pragma unroll
    for (int f = 0; f < kC0TT; ++f) {
      float p = 0.0f;
#pragma unroll
      for (int i = 0; i < CPT; ++i) p += (tid + 256 * i < C0) ? acc[i][f] : 0.0f;
      p = sbk::group_sum<16>(p);
      if ((lane & 15) == 0) red[f][wave * 4 + (lane >> 4)] = p;
    }
    __syncthreads();
    if (tid < kC0TT) {
      float t = 0.0f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += red[tid][q];
      stat[tid] = t / (float)C0;
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < kC0TT; ++f) mean[f] = stat[f];
#pragma unroll
    for (int f = 0; f < kC0TT; ++f) {
      float p = 0.0f;
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        const float dv = acc[i][f] - mean[f];
        p += (tid + 256 * i < C0) ? dv * dv : 0.0f;
      }
      p = sbk::group_sum<16>(p);
      if ((lane & 15) == 0) red[f][wave * 4 + (lane >> 4)] = p;
    }
    __syncthreads();  // (every thread has read stat[] above: the barrier before this one's writes is the one in front of them)
    if (tid < kC0TT) {
      float t = 0.0f;
#pragma unroll
      for (int q = 0; q < 16; ++q) t += red[tid][q];
      stat[tid] = rsqrtf(t / (float)C0 + eps);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < kC0TT; ++f) {
      const float rs = stat[f];
#pragma unroll
      for (int i = 0; i < CPT; ++i) acc[i][f] = (acc[i][f] - mean[f]) * rs;
    }
  } else {
    if (T0 <= kC0TT) {
      // the whole utterance is this one tile: a thread holds every frame of its channels, and takes their statistics from the
      // values themselves (mean, then squared deviations) -- with a handful of frames the variance can be ~0 and 1/sqrt(eps)
      // would magnify the rounding between these values and a mean formed any other way
#pragma unroll
      for (int i = 0; i < CPT; ++i) {
        float sm = 0.0f, sq = 0.0f;
#pragma unroll
        for (int f = 0; f < kC0TT; ++f) sm += f < nf ? acc[i][f] : 0.0f;
        cm[i] = sm / (float)nf;
#pragma unroll
        for (int f = 0; f < kC0TT; ++f) sq += f < nf ? (acc[i][f] - cm[i]) * (acc[i][f] - cm[i]) : 0.0f;
        cr[i] = rsqrtf(sq / (float)nf + eps);
      }
    }
#pragma unroll
    for (int f = 0; f < kC0TT; ++f)
#pragma unroll
      for (int i = 0; i < CPT; ++i) acc[i][f] = (acc[i][f] - cm[i]) * cr[i];
  }
  float* yb = y + ((size_t)b * T0 + t0) * C0;
#pragma unroll
  for (int f = 0; f < kC0TT; ++f)
#pragma unroll
    for (int i = 0; i < CPT; ++i) {
      const int c = tid + 256 * i;
      if (f < nf && c < C0) yb[(size_t)f * C0 + c] = sbk::gelu_erf(fmaf(acc[i][f], gm[i], bt[i]));
    }
}

// ---------------------------------------------------------------------------------------------- positional convolution
constexpr int kPT = 64;                   // output frames per workgroup
constexpr int kPMaxK = 128;               // taps
constexpr int kPMaxCg = 64;               // channels of a group
constexpr int kPRows = kPT + kPMaxK - 1;  // halo rows

template <int CT>  // channel tiles of 16: cg = 16 * CT
__global__ void __launch_bounds__(256) w2v_posconv_kernel(const float* __restrict__ x, const int32_t* __restrict__ key_len,
                                                          const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ y, int T, int d, int k) {
  constexpr int CG = 16 * CT, P = CG + 4;  // halo row pitch: a 16-lane phase of a float4 read covers 64 distinct banks
  __shared__ __attribute__((aligned(16))) float halo[kPRows * (kPMaxCg + 4)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = sbk::uniform(tid >> 6);
  const int fh = wave & 1, kh = wave >> 1;  // frame half, tap parity
  const int tile = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
  const int t0 = tile * kPT, pad = k / 2;
  int klen = T;
  if (key_len) klen = min(max(key_len[b], 0), T);
  const float* xb = x + (size_t)b * T * d + g * CG;
  // ---- stage the masked halo: row r holds frame t0 - pad + r of THIS utterance, zeros outside [0, klen)
  const int rows = kPT + k - 1;
  for (int e = tid; e < rows * (CG / 4); e += 256) {
    const int rr = e / (CG / 4), q = e - rr * (CG / 4);
    const int f = t0 - pad + rr;
    const bool ok = f >= 0 && f < klen;
    const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)min(max(f, 0), T - 1) * d + 4 * q);
    *reinterpret_cast<float4*>(halo + rr * P + 4 * q) = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  // halo rows that hold frames of [0, klen): [vlo, vhi)
  const int vlo = max(pad - t0, 0), vhi = min(klen - t0 + pad, rows);
  // two levels of accumulation: the matrix cores chain 8 taps (<= 512 products) into `acc`, which is then added to `tot` --
  // one fp32 chain over the 4 096 products of a parity would carry ~4x the rounding of torch's blocked sums
  sbk::f32x4 acc[2][CT], tot[2][CT];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) tot[rt][ct] = acc[rt][ct] = sbk::f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  int chained = 0;
  const int row = lane & 15, ks = lane >> 4;
  const int rb = fh * 32;  // this wave's first output frame inside the tile
  const bool live = t0 + rb < T;  // (wave-uniform) a ragged last tile: no output frame of this wave exists
  const size_t K = (size_t)k * CG;
  const float* wl = w + ((size_t)g * CG + row) * K + 4 * ks;
  if (live)
    for (int j = kh; j < k; j += 2) {
      if (rb + j + 32 <= vlo || rb + j >= vhi) continue;  // (wave-uniform) all 32 rows of this tap are padding
      const float* hl = halo + (rb + row + j) * P + 4 * ks;
      const float* wj = wl + (size_t)j * CG;
#pragma unroll
      for (int c0 = 0; c0 < CG; c0 += 16) {
        float4 a4[2], b4[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) b4[ct] = *reinterpret_cast<const float4*>(wj + (size_t)ct * 16 * K + c0);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) a4[rt] = *reinterpret_cast<const float4*>(hl + rt * 16 * P + c0);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            // instruction e contracts input channels c0 + 4*ks + e (ks = the lane's k slice): both operands are one float4
            acc[rt][ct] = sbk::mfma_16x16x4(a4[rt].x, b4[ct].x, acc[rt][ct]);
            acc[rt][ct] = sbk::mfma_16x16x4(a4[rt].y, b4[ct].y, acc[rt][ct]);
            acc[rt][ct] = sbk::mfma_16x16x4(a4[rt].z, b4[ct].z, acc[rt][ct]);
            acc[rt][ct] = sbk::mfma_16x16x4(a4[rt].w, b4[ct].w, acc[rt][ct]);
          }
      }
      if ((++chained & 7) == 0) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              tot[rt][ct][r] += acc[rt][ct][r];
              acc[rt][ct][r] = 0.0f;
            }
      }
    }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[rt][ct][r] += tot[rt][ct][r];
  // ---- residual = the centre rows of the halo, read before the halo is re-used for the sum of the two tap parities
  // acc[rt][ct][r] is frame rb + 16 rt + 4 ks + r, channel 16 ct + row
  float res[2][CT][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) res[rt][ct][r] = halo[(rb + 16 * rt + 4 * ks + r + pad) * P + 16 * ct + row];
  __syncthreads();
  float* part = halo;  // [frame half][64 lanes][2 * CT * 4]
  if (kh == 1) {
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((rt * CT + ct) * 4 + r) * 128 + fh * 64 + lane] = acc[rt][ct][r];
  }
  __syncthreads();
  if (kh == 0 && live) {
    float* yb = y + (size_t)b * T * d + g * CG;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        const int c = 16 * ct + row;
        const float bv = bias[g * CG + c];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = t0 + rb + 16 * rt + 4 * ks + r;
          const float v = acc[rt][ct][r] + part[((rt * CT + ct) * 4 + r) * 128 + fh * 64 + lane] + bv;
          if (t < T) yb[(size_t)t * d + c] = res[rt][ct][r] + sbk::gelu_erf(v);
        }
      }
  }
}

// LayerNorm over the d channels of every row, IN PLACE (one wave per row; a lane re-writes only what it read itself)
__global__ void __launch_bounds__(256) w2v_row_ln_kernel(float* y, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int rows, int d, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool ok = row < rows;
  float* yr = y + (size_t)(ok ? row : rows - 1) * d;  // idle waves shadow the last row: shuffles stay full-width
  float s = 0.0f;
  for (int c = lane; c < d; c += 64) s += yr[c];
  const float mean = sbk::wave_sum(s) / (float)d;
  float q = 0.0f;
  for (int c = lane; c < d; c += 64) {
    const float a = yr[c] - mean;
    q += a * a;
  }
  const float rstd = rsqrtf(sbk::wave_sum(q) / (float)d + eps);
  if (ok)
    for (int c = lane; c < d; c += 64) yr[c] = (yr[c] - mean) * rstd * gamma[c] + beta[c];
}

// The wrapper's output_norm: F.layer_norm over ALL n = T' * d values of an utterance (no affine; padded frames included).
// One workgroup per utterance, three passes over an L2-resident row, fp64 partial sums; in place is fine (a thread re-writes
// only what it read itself).
__global__ void __launch_bounds__(256) w2v_utt_norm_kernel(const float* x, float* y, long n, float eps) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float* xr = x + (size_t)blockIdx.x * n;
  float* yr = y + (size_t)blockIdx.x * n;
  double a = 0.0;
  for (long i = tid; i < n; i += 256) a += (double)xr[i];
  red[tid] = a;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const double mean = red[0] / (double)n;
  __syncthreads();
  a = 0.0;
  for (long i = tid; i < n; i += 256) {
    const double v = (double)xr[i] - mean;
    a += v * v;
  }
  red[tid] = a;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  const float rstd = (float)(1.0 / sqrt(red[0] / (double)n + (double)eps)), mf = (float)mean;
  for (long i = tid; i < n; i += 256) yr[i] = (xr[i] - mf) * rstd;
}

int conv0_shape(int B, int N, int C0, int k, int s, const char* who) {
  SBK_REQUIRE(B >= 0 && B <= 65535 && N >= 0 && C0 > 0 && C0 <= 1024, "%s: bad shape B=%d N=%d C0=%d (C0 <= 1024)", who, B, N, C0);
  SBK_REQUIRE(k >= 1 && k <= kMaxK && s >= 1 && s <= k, "%s: kernel %d / stride %d (1 <= stride <= kernel <= %d)", who, k, s, kMaxK);
  SBK_REQUIRE(B == 0 || N >= k, "%s: N=%d samples are fewer than the kernel's %d", who, N, k);
  return 0;
}

}  // namespace

extern "C" size_t sbk_w2v_conv0_stats_workspace_bytes(int B, int N, int k, int s) {
  if (B <= 0 || k < 1 || s < 1 || N < k) return 0;
  const int T0 = (N - k) / s + 1;
  return (size_t)B * sbk::cdiv(T0, w2v_chunk_frames(s)) * kSlot * sizeof(double);
}

extern "C" int sbk_w2v_conv0_stats_f32(const float* wav, const float* w, const float* bias, int normalize, float wav_eps,
                                       float eps, float* wstat, float* cstat, void* workspace, size_t workspace_bytes, int B,
                                       int N, int C0, int k, int s, sbk_stream_t stream) {
  if (const int rc = conv0_shape(B, N, C0, k, s, "w2v_conv0_stats")) return rc;
  if (B == 0) return 0;
  SBK_REQUIRE(wav && workspace && (wstat || w), "w2v_conv0_stats: null operand");
  SBK_REQUIRE(!w || cstat, "w2v_conv0_stats: channel statistics asked for (w) without cstat");
  SBK_REQUIRE(!normalize || wstat, "w2v_conv0_stats: normalize without wstat");
  SBK_REQUIRE(workspace_bytes >= sbk_w2v_conv0_stats_workspace_bytes(B, N, k, s) &&
                  (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
              "w2v_conv0_stats: workspace of %zu bytes (8-byte aligned) needed", sbk_w2v_conv0_stats_workspace_bytes(B, N, k, s));
  hipStream_t st = sbk::as_stream(stream);
  const int T0 = (N - k) / s + 1, FR = w2v_chunk_frames(s), nblk = sbk::cdiv(T0, FR);
  double* ws = reinterpret_cast<double*>(workspace);
  const double n = (double)B * N;
  sbk::ProfScope prof("w2v_conv0_stats", n * (2.0 + (double)k * (k + 3) / s), 8.0 * n, st);
  dim3 grid(nblk, B), block(256);
  SBK_LAUNCH((w2v_moments_kernel<0>), grid, block, 0, st, wav, ws, N, T0, k, s, FR, nblk);
  SBK_LAUNCH((w2v_moments_kernel<1>), grid, block, 0, st, wav, ws, N, T0, k, s, FR, nblk);
  SBK_LAUNCH(w2v_conv0_finalize_kernel, dim3(B), block, 0, st, ws, w, bias, wstat, cstat, N, T0, C0, k, nblk, normalize, wav_eps,
             eps);
  return sbk::launch_status("sbk_w2v_conv0_stats_f32");
}

extern "C" int sbk_w2v_conv0_f32(const float* wav, const float* wstat, const float* w, const float* bias, int mode,
                                 const float* cstat, const float* gamma, const float* beta, float eps, float* y, int B, int N,
                                 int C0, int k, int s, sbk_stream_t stream) {
  if (const int rc = conv0_shape(B, N, C0, k, s, "w2v_conv0")) return rc;
  SBK_REQUIRE(mode == kModeGroup || mode == kModeLayer, "w2v_conv0: mode %d (1 = group norm, 2 = layer norm)", mode);
  if (B == 0) return 0;
  const int T0 = (N - k) / s + 1;
  SBK_REQUIRE(wav && w && gamma && beta && y && (mode != kModeGroup || cstat || T0 <= kC0TT), "w2v_conv0: null operand");
  hipStream_t st = sbk::as_stream(stream);
  const double n = (double)B * T0 * C0;
  sbk::ProfScope prof("w2v_conv0", (2.0 * k + 12.0) * n, 4.0 * n + 4.0 * B * N, st);
  dim3 grid(sbk::cdiv(T0, kC0TT), B), block(256);
#define SBK_W2V_CONV0_(CPT, MODE, KU) \
  SBK_LAUNCH((w2v_conv0_kernel<CPT, MODE, KU>), grid, block, 0, st, wav, wstat, w, bias, cstat, gamma, beta, y, N, T0, C0, k, s, eps)
#define SBK_W2V_CONV0(CPT)                                                       \
  do {                                                                           \
    if (mode == kModeGroup) {                                                    \
      if (k <= 4) SBK_W2V_CONV0_(CPT, kModeGroup, 4);                            \
      else if (k <= 10) SBK_W2V_CONV0_(CPT, kModeGroup, 10);                     \
      else SBK_W2V_CONV0_(CPT, kModeGroup, kMaxK);                               \
    } else {                                                                     \
      if (k <= 4) SBK_W2V_CONV0_(CPT, kModeLayer, 4);                            \
      else if (k <= 10) SBK_W2V_CONV0_(CPT, kModeLayer, 10);                     \
      else SBK_W2V_CONV0_(CPT, kModeLayer, kMaxK);                               \
    }                                                                            \
  } while (0)
  if (C0 <= 256) SBK_W2V_CONV0(1);
  else if (C0 <= 512) SBK_W2V_CONV0(2);
  else SBK_W2V_CONV0(4);
#undef SBK_W2V_CONV0_
#undef SBK_W2V_CONV0
  return sbk::launch_status("sbk_w2v_conv0_f32");
}

extern "C" int sbk_w2v_posconv_f32(const float* x, const int32_t* key_len, const float* w, const float* bias, const float* gamma,
                                   const float* beta, float eps, float* y, int B, int T, int d, int G, int k,
                                   sbk_stream_t stream) {
  SBK_REQUIRE(B >= 0 && B <= 65535 && T >= 0 && d > 0 && G > 0 && G <= 65535 && d % G == 0, "w2v_posconv: bad shape B=%d T=%d d=%d G=%d",
              B, T, d, G);
  const int cg = d / G;
  SBK_REQUIRE(cg == 16 || cg == 32 || cg == 48 || cg == 64, "w2v_posconv: group width %d not instantiated (16,32,48,64)", cg);
  SBK_REQUIRE(k >= 1 && k <= kPMaxK, "w2v_posconv: %d taps (1..%d)", k, kPMaxK);
  SBK_REQUIRE((double)B * T * d < 2147483648.0, "w2v_posconv: B*T*d too large");
  if (B == 0 || T == 0) return 0;
  SBK_REQUIRE(x && w && bias && y && (!gamma == !beta), "w2v_posconv: null operand");
  SBK_REQUIRE(sbk::aligned16(x) && sbk::aligned16(w), "w2v_posconv: x and w must be 16-byte aligned");
  SBK_REQUIRE(x != y, "w2v_posconv: in place (a workgroup reads frames its neighbours write)");
  hipStream_t st = sbk::as_stream(stream);
  {
    const double n = (double)B * T * d;
    sbk::ProfScope prof("w2v_posconv", 2.0 * n * cg * k, 8.0 * n + 4.0 * (double)d * cg * k, st);
    dim3 grid(sbk::cdiv(T, kPT), G, B), block(256);
    switch (cg) {
      case 16: SBK_LAUNCH((w2v_posconv_kernel<1>), grid, block, 0, st, x, key_len, w, bias, y, T, d, k); break;
      case 32: SBK_LAUNCH((w2v_posconv_kernel<2>), grid, block, 0, st, x, key_len, w, bias, y, T, d, k); break;
      case 48: SBK_LAUNCH((w2v_posconv_kernel<3>), grid, block, 0, st, x, key_len, w, bias, y, T, d, k); break;
      default: SBK_LAUNCH((w2v_posconv_kernel<4>), grid, block, 0, st, x, key_len, w, bias, y, T, d, k); break;
    }
  }
  if (gamma) {
    sbk::ProfScope prof("w2v_posconv_ln", 8.0 * B * T * d, 8.0 * B * T * d, st);
    SBK_LAUNCH(w2v_row_ln_kernel, dim3(sbk::cdiv(B * T, 4)), dim3(256), 0, st, y, gamma, beta, B * T, d, eps);
  }
  return sbk::launch_status("sbk_w2v_posconv_f32");
}

extern "C" int sbk_w2v_utt_norm_f32(const float* x, float* y, int rows, long n, float eps, sbk_stream_t stream) {
  SBK_REQUIRE(rows >= 0 && n > 0, "w2v_utt_norm: bad shape rows=%d n=%ld", rows, n);
  if (rows == 0) return 0;
  SBK_REQUIRE(x && y, "w2v_utt_norm: null operand");
  hipStream_t st = sbk::as_stream(stream);
  sbk::ProfScope prof("w2v_utt_norm", 5.0 * rows * n, 8.0 * rows * n, st);
  SBK_LAUNCH(w2v_utt_norm_kernel, dim3(rows), dim3(256), 0, st, x, y, n, eps);
  return sbk::launch_status("sbk_w2v_utt_norm_f32");
}
