// ConvolutionFrontEnd block:  reflect-pad(1) -> Conv2d 3x3 stride 2 (+bias)
//   -> LayerNorm over (F',C) -> LeakyReLU(0.01)          (sbk_conv_block_f32)
// and the blocks of the transformer.yaml front end (kernel_sizes 5, 5, 1; strides 2, 2, 1; residuals F, F, T):
//   reflect-pad(2) -> Conv2d 5x5 stride 2 -> LayerNorm -> LeakyReLU           (sbk_conv_block_k_f32: the kernel below with five taps,
//                                                                              or conv5_mfma_kernel for 64 output channels)
//   LeakyReLU(LN(conv1x1(x))) + LN(reduce_conv1x1(x))                          (sbk_conv_block_res1x1_f32)
//
// Roofline: HBM for block 0 (C_in = 1: 320 B in, 10 KB out per output frame);
// block 1 (64 -> 32 channels) is a small implicit GEMM kept on the vector ALU
// in this revision (5.9 GFLOP per 32 x 10 s batch, < 4 % of the encoder).
//
// Layout: activations are [B,T,F,C] (C fastest) on both sides, exactly the
// tensors the reference hands between blocks, so no transposes exist.  One
// workgroup produces one output frame (all F' x C' values): the 3 input frames
// it needs are staged in LDS with the reflect padding resolved at staging
// time, the 3x3 taps are read from a [C_in*9, C_out] re-laid-out weight
// (coalesced across output channels), and the (F',C') LayerNorm statistics are
// a workgroup reduction over values still in registers -- the pre-norm
// activation never goes to HBM.
#include "common.h"
#include "device.h"
#include "kernel_util.h"

namespace {

constexpr int kNPT = 10;  // outputs kept per thread (F'*C' <= 2560 with 256 threads)

struct ConvArgs {
  const float* x;      // [B,Tin,Fin,Cin]
  const float* wt;     // [Cin*KS*KS, Cout], row = (ci*KS+kf)*KS+kt
  const float* bias;   // [Cout]
  const float* gamma;  // [Fout*Cout]
  const float* beta;
  float* y;            // [B,Tout,Fout,Cout]
  int B, Tin, Fin, Cin, Tout, Fout, Cout;
  float eps, slope;
};

using sbk::block_sum;
using sbk::reflect1;

template <int KS>  // KS x KS taps, stride 2, reflect padding KS / 2 (3 or 5)
__global__ void __launch_bounds__(256) conv_block_kernel(ConvArgs a) {
  constexpr int PAD = KS / 2;
  SBK_DYN_LDS(float, patch);  // [KS][Fin+2*PAD][Cin]
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, to = blockIdx.x;
  const int Fp = a.Fin + 2 * PAD;
  const int rowlen = Fp * a.Cin;
  for (int i = tid; i < KS * rowlen; i += 256) {
    const int kt = i / rowlen, rem = i % rowlen;
    const int fp = rem / a.Cin, ci = rem % a.Cin;
    const int ti = reflect1(2 * to + kt - PAD, a.Tin);
    const int fi = reflect1(fp - PAD, a.Fin);
    patch[i] = a.x[(((size_t)b * a.Tin + ti) * a.Fin + fi) * a.Cin + ci];
  }
  __syncthreads();

  const int nout = a.Fout * a.Cout;
  float acc[kNPT];
#pragma unroll
  for (int s = 0; s < kNPT; ++s) {
    const int o = tid + s * 256;
    float v = 0.0f;
    if (o < nout) {
      const int c = o % a.Cout, fo = o / a.Cout;
      v = a.bias[c];
      for (int ci = 0; ci < a.Cin; ++ci) {
        for (int kf = 0; kf < KS; ++kf) {
          const float* prow = patch + (size_t)(2 * fo + kf) * a.Cin + ci;
          const float* wrow = a.wt + (size_t)((ci * KS + kf) * KS) * a.Cout + c;
#pragma unroll
          for (int kt = 0; kt < KS; ++kt) v = fmaf(prow[kt * rowlen], wrow[kt * a.Cout], v);
        }
      }
    }
    acc[s] = v;
  }

  float s1 = 0.0f;
#pragma unroll
  for (int s = 0; s < kNPT; ++s)
    if (tid + s * 256 < nout) s1 += acc[s];
  const float mean = block_sum(s1, red) / (float)nout;
  float s2 = 0.0f;
#pragma unroll
  for (int s = 0; s < kNPT; ++s)
    if (tid + s * 256 < nout) s2 += (acc[s] - mean) * (acc[s] - mean);
  const float rstd = rsqrtf(block_sum(s2, red) / (float)nout + a.eps);

  float* yo = a.y + ((size_t)b * a.Tout + to) * nout;
#pragma unroll
  for (int s = 0; s < kNPT; ++s) {
    const int o = tid + s * 256;
    if (o < nout) {
      const float v = (acc[s] - mean) * rstd * a.gamma[o] + a.beta[o];
      yo[o] = v > 0.0f ? v : a.slope * v;
    }
  }
}


// ---- 5x5 stride 2, 64 -> 64 channels on the fp32 matrix cores (block 2 of the transformer.yaml front end: 64 -> 64 channels,
// K = 25 * 64 = 1600, 32.8 GFLOP per 32 x 10 s batch).  A workgroup owns TF consecutive output frames of one utterance (the host
// picks TF): its rows are the (frame, f') pairs, R = TF * F' of them in MT = ceil(R / 32) row tiles, its columns the 64 output
// channels in two column tiles.  The 2 TF + 3 input frames it needs are staged in LDS once, [frame][Fin + 4][Cin + 4], reflect padding
// resolved at staging (pitch Cin + 4: the 16-byte operand reads of neighbouring rows -- 2 (Cin + 4) floats apart -- spread over
// the banks).  v_mfma_f32_32x32x2_f32: A[m][k] = the staged input of row m at (tap, channel), B[k][n] = the weight panel; the two
// k-slices of MFMA e of a channel group of 8 are channels 8 g + e and 8 g + 4 + e, so a lane reads its four A values as ONE 16-byte
// LDS read and its four B values as ONE 16-byte global read of the panel
//   wp [kt][kf][Cin / 8][2][Cout][4]  =  conv.weight[co][8 g + 4 h + e][kf][kt]
// (512 contiguous bytes per half-wave).  Wave w takes column tile w & 1 and the row tiles (w >> 1), (w >> 1) + 2: a weight read serves
// both.  The accumulators (+ bias) then go to LDS over the staged input -- [R][Cout + 1] -- and each output frame's LayerNorm over
// (F', C') is a wave reduction there: the statistics of a frame never leave the workgroup, the pre-norm activation never reaches HBM.
struct Conv5MfmaArgs {
  const float* x;
  const float* wp;
  const float* bias;
  const float* gamma;
  const float* beta;
  float* y;
  int B, Tin, Fin, Cin, Tout, Fout, TF;
  float eps, slope;
};

__global__ void __launch_bounds__(256) conv5_mfma_kernel(Conv5MfmaArgs a) {
  constexpr int KS = 5, PAD = 2, COUT = 64, OP = COUT + 1, CIN = 64, G = CIN / 8;
  SBK_DYN_LDS(float, lds);  // [2 TF + 3][Fin + 4][Cin + 4], later [R][OP]
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int jl = lane & 31, half = lane >> 5;
  const int b = blockIdx.y, to0 = blockIdx.x * a.TF;
  const int Fp = a.Fin + 2 * PAD, CP = a.Cin + 4, NFR = 2 * a.TF + 3;
  const int Cin = CIN, Fout = a.Fout;
  const int R = a.TF * Fout, MT = (R + 31) / 32;

  for (int i = tid; i < NFR * Fp * Cin; i += 256) {
    const int ci = i % Cin, rest = i / Cin;
    const int fp = rest % Fp, fr = rest / Fp;
    // (frames past the last output frame of the utterance feed rows that are never written: any valid frame will do)
    const int ti = min(max(reflect1(2 * to0 - PAD + fr, a.Tin), 0), a.Tin - 1);
    const int fi = reflect1(fp - PAD, a.Fin);
    lds[(fr * Fp + fp) * CP + ci] = a.x[(((size_t)b * a.Tin + ti) * a.Fin + fi) * Cin + ci];
  }
  __syncthreads();

  const int nt = wave & 1, mt0 = wave >> 1;
  const bool two = mt0 + 2 < MT;  // (uniform) this wave has a second row tile
  int abase[2];                   // LDS offset of (row, tap 0, channel 4 * half)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int m = min((mt0 + 2 * u) * 32 + jl, R - 1);  // rows past R repeat the last one (never written)
    abase[u] = ((2 * (m / Fout)) * Fp + 2 * (m % Fout)) * CP + 4 * half;
  }
  sbk::f32x16 acc[2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;
  if (mt0 < MT) {
    // the weight pieces of the NEXT tap are requested before the current tap's 32 / 64 MFMAs (one wave per SIMD: nobody else hides them)
    const float4* wp4 = reinterpret_cast<const float4*>(a.wp) + (size_t)half * COUT + nt * 32 + jl;
    auto fetch_w = [&](int tap, float4 (&w)[G]) {
#pragma unroll
      for (int g = 0; g < G; ++g) w[g] = wp4[((size_t)tap * G + g) * 2 * COUT];
    };
    auto tap_product = [&](int tap, const float4 (&w)[G]) {
      const int toff = ((tap / KS) * Fp + tap % KS) * CP;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float4 x0 = *reinterpret_cast<const float4*>(lds + abase[0] + toff + 8 * g);
        acc[0] = sbk::mfma_32x32x2(x0.x, w[g].x, acc[0]);
        acc[0] = sbk::mfma_32x32x2(x0.y, w[g].y, acc[0]);
        acc[0] = sbk::mfma_32x32x2(x0.z, w[g].z, acc[0]);
        acc[0] = sbk::mfma_32x32x2(x0.w, w[g].w, acc[0]);
      }
      if (two) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float4 x1 = *reinterpret_cast<const float4*>(lds + abase[1] + toff + 8 * g);
          acc[1] = sbk::mfma_32x32x2(x1.x, w[g].x, acc[1]);
          acc[1] = sbk::mfma_32x32x2(x1.y, w[g].y, acc[1]);
          acc[1] = sbk::mfma_32x32x2(x1.z, w[g].z, acc[1]);
          acc[1] = sbk::mfma_32x32x2(x1.w, w[g].w, acc[1]);
        }
      }
    };
    float4 wA[G], wB[G];
    fetch_w(0, wA);
#pragma unroll 1
    for (int tap = 0; tap < KS * KS; tap += 2) {  // (25 taps: the last trip has no second half)
      if (tap + 1 < KS * KS) fetch_w(tap + 1, wB);
      tap_product(tap, wA);
      if (tap + 1 < KS * KS) {
        fetch_w(tap + 2, wA);
        tap_product(tap + 1, wB);
      }
    }
  }
  __syncthreads();  // every wave is done with the staged input
  {
    const float bn = a.bias[nt * 32 + jl];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (mt0 + 2 * u) * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;  // (m >= R for a row tile this wave does not have)
        if (m < R) lds[m * OP + nt * 32 + jl] = acc[u][r] + bn;
      }
    }
  }
  __syncthreads();
  const int nout = Fout * COUT;
  for (int tl = wave; tl < a.TF; tl += 4) {  // a wave per output frame
    const int to = to0 + tl;
    if (to >= a.Tout) break;
    const float* v = lds + (size_t)tl * Fout * OP;
    float s1 = 0.0f;
    for (int o = lane; o < nout; o += 64) s1 += v[(o >> 6) * OP + (o & 63)];
    const float mean = sbk::wave_sum(s1) / (float)nout;
    float s2 = 0.0f;
    for (int o = lane; o < nout; o += 64) {
      const float dv = v[(o >> 6) * OP + (o & 63)] - mean;
      s2 += dv * dv;
    }
    const float rstd = rsqrtf(sbk::wave_sum(s2) / (float)nout + a.eps);
    float* yo = a.y + ((size_t)b * a.Tout + to) * nout;
    for (int o = lane; o < nout; o += 64) {
      const float z = (v[(o >> 6) * OP + (o & 63)] - mean) * rstd * a.gamma[o] + a.beta[o];
      yo[o] = z > 0.0f ? z : a.slope * z;
    }
  }
}

// ---- the residual 1x1 block (block 3 of the transformer.yaml front end), one launch:
//   y = LeakyReLU(LN_1(x W1^T + b1)) + LN_2(x W2^T + b2)        x [B,T,F,Cin] -> y [B,T,F,Cout], LayerNorms over (F, Cout)
// One workgroup per frame.  Cout divides 256, so a thread keeps ONE output channel (tid % Cout) and the rows tid / Cout + s * (256 /
// Cout): per input channel it reads its two weights once and the staged input by LDS broadcast.  Both pre-norm activations stay in
// registers through the four workgroup reductions.
struct Res1x1Args {
  const float* x;
  const float *w1t, *b1, *g1, *be1;  // w1t [Cin, Cout] = convs.conv_0 weight transposed; g1 / be1 [F*Cout]
  const float *w2t, *b2, *g2, *be2;  // reduce_conv
  float* y;
  int F, Cin, Cout;
  float eps1, eps2, slope;
};

__global__ void __launch_bounds__(256) conv_res1x1_kernel(Res1x1Args a) {
  SBK_DYN_LDS(float, xs);  // [F][Cin]
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int n_in = a.F * a.Cin, nout = a.F * a.Cout;
  const float* xf = a.x + (size_t)blockIdx.x * n_in;
  for (int i = tid; i < n_in; i += 256) xs[i] = xf[i];
  __syncthreads();
  const int c = tid % a.Cout, f0 = tid / a.Cout, fstep = 256 / a.Cout;
  float u1[kNPT], u2[kNPT];
  {
    const float b1 = a.b1[c], b2 = a.b2[c];
#pragma unroll
    for (int s = 0; s < kNPT; ++s) u1[s] = b1, u2[s] = b2;
  }
  for (int ci = 0; ci < a.Cin; ++ci) {
    const float w1 = a.w1t[(size_t)ci * a.Cout + c], w2 = a.w2t[(size_t)ci * a.Cout + c];
#pragma unroll
    for (int s = 0; s < kNPT; ++s) {
      const int f = f0 + s * fstep;
      const float xv = f < a.F ? xs[f * a.Cin + ci] : 0.0f;
      u1[s] = fmaf(xv, w1, u1[s]);
      u2[s] = fmaf(xv, w2, u2[s]);
    }
  }
  float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
  for (int s = 0; s < kNPT; ++s)
    if (f0 + s * fstep < a.F) s1 += u1[s], s2 += u2[s];
  const float mean1 = block_sum(s1, red) / (float)nout;
  const float mean2 = block_sum(s2, red) / (float)nout;
  s1 = s2 = 0.0f;
#pragma unroll
  for (int s = 0; s < kNPT; ++s)
    if (f0 + s * fstep < a.F) {
      s1 += (u1[s] - mean1) * (u1[s] - mean1);
      s2 += (u2[s] - mean2) * (u2[s] - mean2);
    }
  const float rstd1 = rsqrtf(block_sum(s1, red) / (float)nout + a.eps1);
  const float rstd2 = rsqrtf(block_sum(s2, red) / (float)nout + a.eps2);
  float* yo = a.y + (size_t)blockIdx.x * nout;
#pragma unroll
  for (int s = 0; s < kNPT; ++s) {
    const int f = f0 + s * fstep;
    if (f < a.F) {
      const int o = f * a.Cout + c;
      const float v1 = (u1[s] - mean1) * rstd1 * a.g1[o] + a.be1[o];
      const float v2 = (u2[s] - mean2) * rstd2 * a.g2[o] + a.be2[o];
      yo[o] = (v1 > 0.0f ? v1 : a.slope * v1) + v2;
    }
  }
}

// Output frames per workgroup of conv5_mfma_kernel: the candidate that fills its 32-row tiles best (at most four tiles, the staged
// input within 144 KiB), the larger on a tie -- F' = 20 (the recipe): 3 frames, 60 of 64 rows, 105 KiB.
int conv5_frames_per_group(int Fin, int Cin, int Fout, int Tout, size_t* lds_bytes) {
  int best = 0;
  double best_fill = 0.0;
  for (int tf = 1; tf <= 16 && tf <= Tout; ++tf) {
    const int R = tf * Fout;
    const size_t stage = (size_t)(2 * tf + 3) * (Fin + 4) * (Cin + 4) * sizeof(float), outb = (size_t)R * 65 * sizeof(float);
    if (R > 128 || stage > 144 * 1024 || outb > stage) break;
    const double fill = (double)R / (32.0 * ((R + 31) / 32));
    if (fill >= best_fill) best = tf, best_fill = fill, *lds_bytes = stage;
  }
  return best;
}

}  // namespace

extern "C" int sbk_conv_block_f32(const float* x, const float* wt, const float* bias, const float* gamma,
                                  const float* beta, float* y, int B, int Tin, int Fin, int Cin, int Cout, float eps,
                                  float slope, sbk_stream_t stream) {
  if (B == 0) return 0;  // empty batch: nothing to launch, the data pointers may be NULL
  SBK_REQUIRE(x && wt && bias && gamma && beta && y, "conv_block: null operand");
  SBK_REQUIRE(B >= 0 && Tin >= 2 && Fin >= 2 && Cin >= 1 && Cout >= 1, "conv_block: bad shape");
  const int Tout = (Tin - 1) / 2 + 1, Fout = (Fin - 1) / 2 + 1;  // floor((n + 2 - 3) / 2) + 1
  SBK_REQUIRE(Fout * Cout <= kNPT * 256, "conv_block: F'*C' = %d exceeds %d", Fout * Cout, kNPT * 256);
  const size_t lds = (size_t)3 * (Fin + 2) * Cin * sizeof(float);
  SBK_REQUIRE(lds <= 64 * 1024, "conv_block: input patch of %zu B does not fit the LDS window", lds);
  if (B == 0) return 0;
  ConvArgs a{x, wt, bias, gamma, beta, y, B, Tin, Fin, Cin, Tout, Fout, Cout, eps, slope};
  sbk::ProfScope prof(Cin == 1 ? "conv_block_cin1" : "conv_block", 2.0 * 9 * Cin * (double)B * Tout * Fout * Cout,
                      4.0 * B * ((double)Tin * Fin * Cin + (double)Tout * Fout * Cout), sbk::as_stream(stream));
  SBK_LAUNCH(conv_block_kernel<3>, dim3(Tout, B), dim3(256), lds, sbk::as_stream(stream), a);
  return sbk::launch_status("sbk_conv_block_f32");
}

extern "C" int sbk_conv_block_k_layout(int Cin, int Cout, int ksize) {
  return ksize == 5 && Cout == 64 && Cin == 64 ? 1 : 0;
}

extern "C" int sbk_conv_block_k_f32(const float* x, const float* wt, const float* bias, const float* gamma, const float* beta,
                                    float* y, int B, int Tin, int Fin, int Cin, int Cout, int ksize, int stride, float eps,
                                    float slope, sbk_stream_t stream) {
  SBK_REQUIRE(stride == 2 && (ksize == 3 || ksize == 5), "conv_block_k: kernel size %d with stride %d not instantiated ((3, 2) and (5, 2))",
              ksize, stride);
  if (ksize == 3) return sbk_conv_block_f32(x, wt, bias, gamma, beta, y, B, Tin, Fin, Cin, Cout, eps, slope, stream);
  if (B == 0) return 0;
  SBK_REQUIRE(x && wt && bias && gamma && beta && y, "conv_block_k: null operand");
  // (reflect padding by 2 needs three samples on both axes, as F.pad(mode="reflect") does)
  SBK_REQUIRE(B >= 0 && Tin >= 3 && Fin >= 3 && Cin >= 1 && Cout >= 1, "conv_block_k: bad shape");
  const int Tout = (Tin - 1) / 2 + 1, Fout = (Fin - 1) / 2 + 1;  // floor((n + 4 - 5) / 2) + 1
  hipStream_t st = sbk::as_stream(stream);
  const double flops = 2.0 * 25 * Cin * (double)B * Tout * Fout * Cout;
  const double bytes = 4.0 * B * ((double)Tin * Fin * Cin + (double)Tout * Fout * Cout);
  if (sbk_conv_block_k_layout(Cin, Cout, ksize) == 1) {
    SBK_REQUIRE(sbk::aligned16(wt), "conv_block_k: the weight panel must be 16-byte aligned");
    size_t lds = 0;
    const int tf = conv5_frames_per_group(Fin, Cin, Fout, Tout, &lds);
    SBK_REQUIRE(tf >= 1, "conv_block_k: F = %d, Cin = %d does not fit the LDS staging of the 5x5 matrix-core kernel", Fin, Cin);
    if (const int rc = sbk::require_dyn_lds(conv5_mfma_kernel, lds, "conv_block_k")) return rc;
    Conv5MfmaArgs a{x, wt, bias, gamma, beta, y, B, Tin, Fin, Cin, Tout, Fout, tf, eps, slope};
    sbk::ProfScope prof("conv_block5_mfma", flops, bytes, st);
    SBK_LAUNCH(conv5_mfma_kernel, dim3((Tout + tf - 1) / tf, B), dim3(256), lds, st, a);
    return sbk::launch_status("sbk_conv_block_k_f32");
  }
  SBK_REQUIRE(Fout * Cout <= kNPT * 256, "conv_block_k: F'*C' = %d exceeds %d", Fout * Cout, kNPT * 256);
  const size_t lds = (size_t)5 * (Fin + 4) * Cin * sizeof(float);
  SBK_REQUIRE(lds <= 64 * 1024, "conv_block_k: input patch of %zu B does not fit the LDS window", lds);
  ConvArgs a{x, wt, bias, gamma, beta, y, B, Tin, Fin, Cin, Tout, Fout, Cout, eps, slope};
  sbk::ProfScope prof(Cin == 1 ? "conv_block5_cin1" : "conv_block5", flops, bytes, st);
  SBK_LAUNCH(conv_block_kernel<5>, dim3(Tout, B), dim3(256), lds, st, a);
  return sbk::launch_status("sbk_conv_block_k_f32");
}

extern "C" int sbk_conv_block_res1x1_f32(const float* x, const float* w1t, const float* b1, const float* gamma1,
                                         const float* beta1, float eps1, const float* w2t, const float* b2,
                                         const float* gamma2, const float* beta2, float eps2, float* y, int B, int T, int F,
                                         int Cin, int Cout, float slope, sbk_stream_t stream) {
  if (B == 0 || T == 0) return 0;
  SBK_REQUIRE(x && w1t && b1 && gamma1 && beta1 && w2t && b2 && gamma2 && beta2 && y, "conv_block_res1x1: null operand");
  SBK_REQUIRE(B >= 0 && T >= 0 && F >= 1 && Cin >= 1 && Cout >= 1, "conv_block_res1x1: bad shape");
  SBK_REQUIRE(Cout <= 256 && 256 % Cout == 0, "conv_block_res1x1: %d output channels not instantiated (a divisor of 256)", Cout);
  SBK_REQUIRE(F <= kNPT * (256 / Cout), "conv_block_res1x1: F*C' = %d exceeds %d", F * Cout, kNPT * 256);
  const size_t lds = (size_t)F * Cin * sizeof(float);
  SBK_REQUIRE(lds <= 64 * 1024, "conv_block_res1x1: input frame of %zu B does not fit the LDS window", lds);
  SBK_REQUIRE((size_t)B * T <= 0x7fffffffu, "conv_block_res1x1: too many frames");
  hipStream_t st = sbk::as_stream(stream);
  Res1x1Args a{x, w1t, b1, gamma1, beta1, w2t, b2, gamma2, beta2, y, F, Cin, Cout, eps1, eps2, slope};
  sbk::ProfScope prof("conv_block_res1x1", 4.0 * Cin * (double)B * T * F * Cout, 4.0 * B * (double)T * F * (Cin + Cout), st);
  SBK_LAUNCH(conv_res1x1_kernel, dim3(B * T), dim3(256), lds, st, a);
  return sbk::launch_status("sbk_conv_block_res1x1_f32");
}
