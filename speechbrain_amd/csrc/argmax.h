// The arg-max rule of the decoders (torch.max / numpy.argmax), shared by csrc/ctc_decode.hip and csrc/transducer.hip.
#pragma once
#include <sbk_device.h>

namespace sbk {

// "x better than y" under torch.max / numpy.argmax: the larger value, NaN above everything, the first index on ties
__device__ __forceinline__ bool arg_better(float v, int i, float w, int j) {
  const bool vn = isnan(v), wn = isnan(w);
  if (vn != wn) return vn;
  if (!vn && v != w) return v > w;
  return i < j;
}

}  // namespace sbk
