// The convolution blocks of a CRDNN encoder (lobes/models/CRDNN.py:199-278), activations [B,T,F,C] (C fastest) over the PADDED
// batch exactly as the reference computes them:
//   reflect-pad(1) -> Conv2d(3x3, stride 1, bias) -> LayerNorm over (F,C) -> LeakyReLU      twice, then
//   max-pool over frequency (kernel = stride = pool_f, floor) [-> after the last block: max-pool over time (pool_t, floor)]
//
// Three kernels:
//   * crdnn_frame_kernel<true>: the FIRST convolution (one input channel: nine taps, K = 9, is no contraction for the matrix
//     cores).  One workgroup per output frame: the F x C outputs of the frame are formed in LDS from the three input frames it
//     needs, normalised and activated there and written once (sbk_crdnn_conv1_f32).
//   * crdnn_im2col_kernel: for Cin >= 2 the convolution is a contraction with K = 9 Cin.  The patches of a bounded run of frames
//     are written as rows [(frame, f)][(kf, kt, ci)] (reflect padding resolved here) and contracted with the re-laid-out weight
//     [Cout, 9 Cin] by the library's fp32 GEMM routing, bias in its epilogue (sbk_crdnn_im2col_f32; native.crdnn_conv drives the
//     chunks, so the patch matrix never exceeds its budget).
//   * crdnn_frame_kernel<false>: LayerNorm over (F,C) + LeakyReLU + frequency max-pool + time max-pool in one pass over a
//     convolution's output: a workgroup owns one OUTPUT frame, walks its pool_t input frames through LDS and writes only the
//     pooled tensor (sbk_crdnn_norm_pool_f32; pool_f = pool_t = 1 is the plain LayerNorm + LeakyReLU behind conv_1).
// LayerNorm statistics in the two-pass form of sbk_layernorm_f32 (biased variance, eps inside the root).
#include "common.h"
#include "device.h"
#include "kernel_util.h"

namespace {

constexpr int kMaxFrame = 16384;  // F * C floats of a frame held in LDS (64 KiB) next to its pooled image

struct FrameArgs {
  const float* x;      // CONV1: [B,T,F] features; else [B,T,F,C] convolution output
  const float* w;      // CONV1: [9, C], row kf * 3 + kt
  const float* bias;   // CONV1: [C]
  const float* gamma;  // [F*C]
  const float* beta;
  float* y;            // [B,T/pool_t,F/pool_f,C]
  int B, T, F, C, pool_f, pool_t;
  float eps, slope;
};

using sbk::block_sum;
using sbk::reflect1;

template <bool CONV1>
__global__ void __launch_bounds__(256) crdnn_frame_kernel(FrameArgs a) {
  SBK_DYN_LDS(float, lds);  // frame [F*C] | pooled [Fo*C] | CONV1: patch [3][F+2]
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const int b = blockIdx.y, to = blockIdx.x;
  const int n = a.F * a.C, Fo = a.F / a.pool_f, no = Fo * a.C, To = a.T / a.pool_t;
  float* frame = lds;
  float* pooled = lds + n;
  float* patch = pooled + no;
  for (int tt = 0; tt < a.pool_t; ++tt) {
    const int t = to * a.pool_t + tt;
    __syncthreads();  // the previous frame has been consumed
    if constexpr (CONV1) {
      const int Fp = a.F + 2;
      for (int i = tid; i < 3 * Fp; i += 256) {
        const int kt = i / Fp, fp = i % Fp;
        patch[i] = a.x[((size_t)b * a.T + reflect1(t + kt - 1, a.T)) * a.F + reflect1(fp - 1, a.F)];
      }
      __syncthreads();
      for (int o = tid; o < n; o += 256) {
        const int c = o % a.C, f = o / a.C;
        float v = a.bias[c];
#pragma unroll
        for (int kf = 0; kf < 3; ++kf)
#pragma unroll
          for (int kt = 0; kt < 3; ++kt) v = fmaf(patch[kt * Fp + f + kf], a.w[(kf * 3 + kt) * a.C + c], v);
        frame[o] = v;
      }
    } else {
      const float* src = a.x + ((size_t)b * a.T + t) * n;
      for (int o = tid; o < n; o += 256) frame[o] = src[o];
    }
    // (each thread reads back the elements it wrote: no barrier needed before the sums; block_sum barriers before the pooling)
    float s1 = 0.0f;
    for (int o = tid; o < n; o += 256) s1 += frame[o];
    const float mean = block_sum(s1, red) / (float)n;
    float s2 = 0.0f;
    for (int o = tid; o < n; o += 256) s2 += (frame[o] - mean) * (frame[o] - mean);
    const float rstd = rsqrtf(block_sum(s2, red) / (float)n + a.eps);
    for (int o = tid; o < no; o += 256) {
      const int c = o % a.C, fo = o / a.C;
      float m = 0.0f;
      for (int p = 0; p < a.pool_f; ++p) {
        const int i = (fo * a.pool_f + p) * a.C + c;
        float v = (frame[i] - mean) * rstd * a.gamma[i] + a.beta[i];
        v = v > 0.0f ? v : a.slope * v;
        m = p == 0 ? v : fmaxf(m, v);
      }
      pooled[o] = tt == 0 ? m : fmaxf(pooled[o], m);
    }
  }
  float* yo = a.y + ((size_t)b * To + to) * no;
  for (int o = tid; o < no; o += 256) yo[o] = pooled[o];  // (the elements this thread pooled)
}

struct ColArgs {
  const float* x;  // [NF, ...]: all frames of the batch, [B,T,F,Cin]
  float* col;      // [frames * F, 9 * Cin]
  int T, F, Cin, frame0, frames;
};

// One workgroup per (frame, f) row of the patch matrix: 9 runs of Cin contiguous floats.
__global__ void __launch_bounds__(256) crdnn_im2col_kernel(ColArgs a) {
  const int row = blockIdx.x;  // frame-local * F + f
  const int fr = a.frame0 + row / a.F, f = row % a.F;
  const int b = fr / a.T, t = fr % a.T;
  const int K = 9 * a.Cin;
  float* dst = a.col + (size_t)row * K;
  for (int i = threadIdx.x; i < K; i += 256) {
    const int tap = i / a.Cin, ci = i % a.Cin;
    const int kf = tap / 3, kt = tap % 3;
    dst[i] = a.x[(((size_t)b * a.T + reflect1(t + kt - 1, a.T)) * a.F + reflect1(f + kf - 1, a.F)) * a.Cin + ci];
  }
}

size_t frame_lds_bytes(int F, int C, int pool_f, bool conv1) {
  return sizeof(float) * ((size_t)F * C + (size_t)(F / pool_f) * C + (conv1 ? 3 * (F + 2) : 0));
}

int check_frame(const char* who, int B, int T, int F, int C, int pool_f, int pool_t) {
  SBK_REQUIRE(B >= 1 && B <= 65535 && C >= 1, "%s: bad shape B=%d C=%d (1 <= B <= 65535, C >= 1)", who, B, C);
  SBK_REQUIRE(T >= 2 && F >= 2, "%s: T=%d F=%d: the reflect padding of one frame / bin needs T >= 2 and F >= 2", who, T, F);
  SBK_REQUIRE(pool_f >= 1 && pool_t >= 1 && F / pool_f >= 1 && T / pool_t >= 1,
              "%s: pooling pool_f=%d pool_t=%d leaves no output for F=%d T=%d", who, pool_f, pool_t, F, T);
  SBK_REQUIRE((long)F * C <= kMaxFrame, "%s: F * C = %ld exceeds the limit F * C <= %d (a frame is held in LDS)", who, (long)F * C,
              kMaxFrame);
  return 0;
}

}  // namespace

extern "C" int sbk_crdnn_conv1_f32(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                                   float* y, int B, int T, int F, int C, float eps, float slope, sbk_stream_t stream) {
  if (const int rc = check_frame("crdnn_conv1", B, T, F, C, 1, 1)) return rc;
  SBK_REQUIRE(x && w && bias && gamma && beta && y, "crdnn_conv1: null operand");
  FrameArgs a;
  a.x = x; a.w = w; a.bias = bias; a.gamma = gamma; a.beta = beta; a.y = y;
  a.B = B; a.T = T; a.F = F; a.C = C; a.pool_f = 1; a.pool_t = 1; a.eps = eps; a.slope = slope;
  const hipStream_t st = sbk::as_stream(stream);
  const size_t lds = frame_lds_bytes(F, C, 1, true);
  if (const int rc = sbk::require_dyn_lds(crdnn_frame_kernel<true>, lds, "sbk_crdnn_conv1_f32")) return rc;
  sbk::ProfScope prof("crdnn_conv1", 2.0 * 9.0 * B * T * F * C + 8.0 * B * T * F * C, 4.0 * B * T * F * (1.0 + C), st);
  SBK_LAUNCH(crdnn_frame_kernel<true>, dim3(T, B), dim3(256), lds, st, a);
  return sbk::launch_status("sbk_crdnn_conv1_f32");
}

extern "C" int sbk_crdnn_norm_pool_f32(const float* x, const float* gamma, const float* beta, float* y, int B, int T, int F,
                                       int C, int pool_f, int pool_t, float eps, float slope, sbk_stream_t stream) {
  if (const int rc = check_frame("crdnn_norm_pool", B, T, F, C, pool_f, pool_t)) return rc;
  SBK_REQUIRE(x && gamma && beta && y, "crdnn_norm_pool: null operand");
  SBK_REQUIRE(x != y || (pool_f == 1 && pool_t == 1), "crdnn_norm_pool: y may alias x only without pooling");
  FrameArgs a;
  a.x = x; a.w = nullptr; a.bias = nullptr; a.gamma = gamma; a.beta = beta; a.y = y;
  a.B = B; a.T = T; a.F = F; a.C = C; a.pool_f = pool_f; a.pool_t = pool_t; a.eps = eps; a.slope = slope;
  const hipStream_t st = sbk::as_stream(stream);
  const size_t lds = frame_lds_bytes(F, C, pool_f, false);
  if (const int rc = sbk::require_dyn_lds(crdnn_frame_kernel<false>, lds, "sbk_crdnn_norm_pool_f32")) return rc;
  const double elems = (double)B * T * F * C;
  sbk::ProfScope prof("crdnn_norm_pool", 10.0 * elems, 4.0 * elems * (1.0 + 1.0 / ((double)pool_f * pool_t)), st);
  SBK_LAUNCH(crdnn_frame_kernel<false>, dim3(T / pool_t, B), dim3(256), lds, st, a);
  return sbk::launch_status("sbk_crdnn_norm_pool_f32");
}

extern "C" int sbk_crdnn_im2col_f32(const float* x, float* col, int B, int T, int F, int Cin, int frame0, int frames,
                                    sbk_stream_t stream) {
  SBK_REQUIRE(B >= 1 && Cin >= 1, "crdnn_im2col: bad shape B=%d Cin=%d", B, Cin);
  SBK_REQUIRE(T >= 2 && F >= 2, "crdnn_im2col: T=%d F=%d: the reflect padding of one frame / bin needs T >= 2 and F >= 2", T, F);
  SBK_REQUIRE(frame0 >= 0 && frames >= 1 && (long)frame0 + frames <= (long)B * T,
              "crdnn_im2col: frames [%d, %d + %d) are not inside the batch's B * T = %ld", frame0, frame0, frames, (long)B * T);
  SBK_REQUIRE((long)frames * F <= 0x7fffffffL, "crdnn_im2col: frames * F = %ld rows exceed one launch", (long)frames * F);
  SBK_REQUIRE(x && col, "crdnn_im2col: null operand");
  ColArgs a;
  a.x = x; a.col = col; a.T = T; a.F = F; a.Cin = Cin; a.frame0 = frame0; a.frames = frames;
  const hipStream_t st = sbk::as_stream(stream);
  const double bytes = 4.0 * frames * F * 9.0 * Cin;
  sbk::ProfScope prof("crdnn_im2col", 0.0, bytes * (1.0 + 1.0 / 9.0), st);
  SBK_LAUNCH(crdnn_im2col_kernel, dim3(frames * F), dim3(256), 0, st, a);
  return sbk::launch_status("sbk_crdnn_im2col_f32");
}
