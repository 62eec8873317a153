// The two "better candidate" rules of the decoders: arg_better (torch.max / numpy.argmax; csrc/ctc_decode.hip,
// csrc/transducer.hip) and better (the top-k of the attention beam search, csrc/search.hip).
#pragma once
#include <math.h>
#include <sbk_device.h>

namespace sbk {

// "x better than y" under torch.max / numpy.argmax: the larger value, NaN above everything, the first index on ties
__device__ __forceinline__ bool arg_better(float v, int i, float w, int j) {
  const bool vn = isnan(v), wn = isnan(w);
  if (vn != wn) return vn;
  if (!vn && v != w) return v > w;
  return i < j;
}

// The same order for numbers: the larger value, the lower index on ties.  It differs from arg_better for NaN only: here
// every comparison with a NaN is false in both directions (a NaN neither displaces a candidate nor is displaced by one),
// where arg_better puts NaN above everything.  Both behaviours are kept as they are.
__device__ __forceinline__ bool better(float v, int i, float v2, int i2) { return v > v2 || (v == v2 && i < i2); }

}  // namespace sbk
