// Shared by the contraction translation units (gemm.hip, gemm_lp.hip): the fp32 launch record (the epilogue's activation is act.h).
#pragma once
#include "act.h"
#include "common.h"

namespace {

struct GemmArgs {
  const float* A;
  const float* W;
  const float* bias;
  const float* R;
  float* C;
  int lda, ldw, ldr, ldc, M, N, K, act;
  float alpha;
  const int32_t* seq_len;  // optional: rows are [batch][rows_per_seq]; rows >= seq_len[batch] produce v = 0
  int rows_per_seq;
};

}  // namespace
