// What the CTC searches (csrc/ctc_decode.hip, csrc/ctc_prefix_search.hip) share: the arithmetic of the polynomial string
// hashes that stand for a hypothesis' text (include/sbk.h) and numpy's fp32 logaddexp.
#pragma once
#include <math.h>
#include <stdint.h>

#include <sbk_device.h>

namespace sbk {

constexpr uint32_t kHashMod = 2147483647u;  // 2^31 - 1: two polynomial hashes of a string's characters

__device__ __forceinline__ uint32_t hmul(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) % kHashMod); }
__device__ __forceinline__ uint32_t hadd(uint32_t a, uint32_t b) {
  const uint32_t s = a + b;  // (a, b < 2^31: no wrap)
  return s >= kHashMod ? s - kHashMod : s;
}

// numpy's npy_logaddexpf
__device__ __forceinline__ float logaddexp_f32(float x, float y) {
  if (x == y) return x + 0.693147180559945309f;
  const float d = x - y;
  if (d > 0.0f) return x + log1pf(expf(-d));
  if (d <= 0.0f) return y + log1pf(expf(d));
  return d;  // NaN
}

}  // namespace sbk
