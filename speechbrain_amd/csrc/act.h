// The activations of the library (SBK_ACT_* of include/sbk.h), each formula once: a kernel file defines none of its own.
// Plain C++ on expf / erff / tanhf, so the CPU emulator (tools/kernel_emu) compiles this header as it stands.
#pragma once
#include <sbk_device.h>

#include "common.h"

namespace sbk {

__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float swish(float x) { return x / (1.0f + expf(-x)); }
// GELU, erf form, on libm's erff: the fp32 parity path.  The reduced-precision contractions use sbk::gelu_erfc
// (sbk_device.h) instead, see act_tile.
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float relu(float x) { return x > 0.0f ? x : 0.0f; }  // NaN -> 0
// torch.relu's rule, NaN stays NaN.  Only the transducer joint (joint_act) needs it: its arg-max treats a NaN
// log-probability as the reference does (NaN above everything), which a NaN frame must reach as NaN; every epilogue
// and LayerNorm uses relu above.
__device__ __forceinline__ float relu_keep_nan(float x) { return x <= 0.0f ? 0.0f : x; }
__device__ __forceinline__ float leaky_relu(float x) { return x > 0.0f ? x : 0.01f * x; }

__device__ __forceinline__ float act(float v, int kind) {
  switch (kind) {
    case SBK_ACT_SWISH: return swish(v);
    case SBK_ACT_GELU: return gelu_erf(v);
    case SBK_ACT_RELU: return relu(v);
    case SBK_ACT_LEAKY_RELU: return leaky_relu(v);
    default: return v;
  }
}

// Nonlinearity of the transducer joint network and of the RNNLM's DNN blocks (csrc/transducer.hip): GELU, LEAKY_RELU, RELU
// or TANH under torch's rules.
__device__ __forceinline__ float joint_act(float x, int kind) {
  switch (kind) {
    case SBK_ACT_GELU: return gelu_erf(x);
    case SBK_ACT_LEAKY_RELU: return leaky_relu(x);
    case SBK_ACT_RELU: return relu_keep_nan(x);
    default: return tanhf(x);
  }
}

enum class Gelu { erf, erfc };  // gelu_erf above / sbk::gelu_erfc (the bf16- and e4m3-activation contractions)

// The activation of a register tile: ONE uniform switch outside the unrolled loop over the N registers (a switch per
// element makes the epilogue branchy, see tile_epilogue_32x32 in gemm.hip).
template <int N, Gelu G = Gelu::erf>
__device__ __forceinline__ void act_tile(float (&v)[N], int kind) {
  switch (kind) {  // uniform
    case SBK_ACT_SWISH:
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] = swish(v[q]);
      break;
    case SBK_ACT_GELU:
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] = G == Gelu::erfc ? gelu_erfc(v[q]) : gelu_erf(v[q]);
      break;
    case SBK_ACT_RELU:
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] = relu(v[q]);
      break;
    case SBK_ACT_LEAKY_RELU:
#pragma unroll
      for (int q = 0; q < N; ++q) v[q] = leaky_relu(v[q]);
      break;
    default: break;
  }
}

// what the launchers accept
inline bool act_known(int kind) { return kind >= SBK_ACT_NONE && kind <= SBK_ACT_LEAKY_RELU; }
inline bool joint_act_known(int kind) {
  return kind == SBK_ACT_GELU || kind == SBK_ACT_LEAKY_RELU || kind == SBK_ACT_RELU || kind == SBK_ACT_TANH;
}

}  // namespace sbk
