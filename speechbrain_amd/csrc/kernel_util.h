// Small device helpers that more than one kernel file needs, each once: a kernel file keeps no copy of them.
#pragma once
#include <sbk_device.h>

namespace sbk {

// index i of a row of n under reflect padding by at most n - 1 (torch's "reflect": the edge element is not repeated)
__device__ __forceinline__ int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// Sum over a workgroup of 256 threads through red[4], in every thread; fixed order (r0 + r1) + (r2 + r3).
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// the order-preserving unsigned image of a float: x < y  <=>  order_key(x) < order_key(y)
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// dst[0..N) = p[0..N) in the widest pieces N allows (p aligned to that piece)
template <int N>
__device__ __forceinline__ void load_run(float (&dst)[N], const float* __restrict__ p) {
  if constexpr (N % 4 == 0) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const float4 v = reinterpret_cast<const float4*>(p)[i];
      dst[4 * i] = v.x; dst[4 * i + 1] = v.y; dst[4 * i + 2] = v.z; dst[4 * i + 3] = v.w;
    }
  } else if constexpr (N % 2 == 0) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float2 v = reinterpret_cast<const float2*>(p)[i];
      dst[2 * i] = v.x; dst[2 * i + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i] = p[i];
  }
}

}  // namespace sbk
