// One step of an RNNLM (lobes/models/RNNLM.py) for the n hypothesis rows of a beam search: RNNLMScorer.score followed by the
// permute_mem of the previous step (decoders/scorer.py, RNNLMScorer), as sbk_rnnlm_step_f32.
//
// The permute is free: the LSTM kernel reads h and c of row r from row parent[r] of state_in and writes row r of state_out, so no
// permuted copy of the [layers, n, H] state is ever made; the caller swaps the two state buffers between steps.
//
// One launch per LSTM layer (rnnlm_lstm_kernel).  A workgroup owns kJS = 8 hidden units with all four of their gate rows -- 32
// columns, one v_mfma_f32_32x32x2_f32 tile wide -- and up to RT = 4 tiles of 32 hypothesis rows, whose accumulators it holds in
// registers side by side.  Its four waves split K into four contiguous quarters.  A lane loads its piece of a gate row ONCE per K
// chunk and uses it for the MFMAs of all RT row tiles: that register reuse, not LDS, is what cuts the weight traffic per row
// (the B operand of this MFMA is private to a lane -- no two lanes of a workgroup need the same weight element, so staging the
// slice in LDS would only add a trip).  The h rows stream in through the parent map.  Layer 0 has no input product: the weight
// table holds Embedding . W_ih0^T, and row tokens[r] of it is added in the epilogue.  A layer above runs a second pass of the same
// loop over the h' that the layer below has just written (rows by identity) against its w_ih.  The four waves' partial tiles meet
// in LDS and are added in wave order, then the biases and the cell update (i, f, g, o) are applied from registers: every sum has a
// fixed order, two runs give the same bits on any stream.  Rows past n and units past H load zeros and store nothing.
//
// The DNN blocks and the output layer are the routed contractions (sbk::gemm_nt_ws) with one LayerNorm + activation kernel between
// them (the activation follows the LayerNorm, so it cannot ride in the contraction's epilogue), then sbk::log_softmax_rows with the
// temperature and the scorer's weight folded in.  tokens and parent are clamped where they index; the C entry also checks them on
// the device and refuses values outside their range.
#include "act.h"
#include "common.h"
#include "internal.h"
#include "kernel_util.h"

#define SBK_HIP(expr)                                                              \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess) return sbk::fail((int)e__, "%s: %s", #expr, hipGetErrorString(e__)); \
  } while (0)

#define SBK_TRY(expr)        \
  do {                       \
    int rc__ = (expr);       \
    if (rc__) return rc__;   \
  } while (0)

namespace {

constexpr int kJS = 8;            // hidden units of a workgroup (x 4 gates = the 32 columns of an MFMA tile)
constexpr int kBT = 32;           // hypothesis rows of a tile (the 32 rows of an MFMA tile)
constexpr int kMaxRT = 4;         // row tiles a workgroup holds in registers
constexpr int kMaxH = 2048;       // the limit of sbk_rnnlm_weights
constexpr int kMaxRows = 65535;   // as csrc/attn_rnn.hip

struct LstmArgs {
  const float* w_x;       // [4H,H] w_ih of a layer above the first; nullptr for layer 0
  const float* w_h;       // [4H,H]
  const float* b_ih;      // [4H] or nullptr
  const float* b_hh;
  const float* emb_ih;    // [n_emb,4H] (layer 0)
  const int32_t* tokens;  // [n] (layer 0)
  const int32_t* parent;  // [n] or nullptr (identity)
  const float* x;         // [n,H] h' of the layer below (layers above the first)
  const float* h_in;      // [n,H] or nullptr (zeros: the first step)
  const float* c_in;
  float* h_out;           // [n,H]
  float* c_out;
  int n, H, n_emb;
};

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// four consecutive k of a row, zeros past K and for a null row (a width that is no multiple of 4: scalar loads)
__device__ __forceinline__ float4 load_k4(const float* row, int k, int K, bool vec) {
  if (row == nullptr) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (vec) return k < K ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return make_float4(k < K ? row[k] : 0.0f, k + 1 < K ? row[k + 1] : 0.0f, k + 2 < K ? row[k + 2] : 0.0f,
                     k + 3 < K ? row[k + 3] : 0.0f);
}

// acc[t] += A_t . W^T over this wave's quarter of K: arow[t] the lane's operand row of tile t (nullptr: zeros), wrow its gate row.
// Inside a chunk of 8 k lanes 0-31 supply k 0..3 and lanes 32-63 k 4..7 of the four MFMAs.
template <int RT>
__device__ __forceinline__ void accumulate(sbk::f32x16 (&acc)[RT], const float* (&arow)[RT], const float* wrow, int H, int wave,
                                           int half, bool vec) {
  constexpr int kUnroll = RT == 1 ? 8 : 4;  // chunks in flight: one tile is bound by the latency of the weight rows
  const int kq = sbk::uniform(((H + 31) / 32) * 8);  // a wave's quarter of K, in whole chunks of 8
  const int kend = min(H, (wave + 1) * kq);
  for (int k0 = wave * kq; k0 < kend; k0 += 8 * kUnroll) {
    float4 wv[kUnroll], hv[RT][kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int k = k0 + 8 * u + 4 * half;
      wv[u] = load_k4(wrow, k, kend, vec);
#pragma unroll
      for (int t = 0; t < RT; ++t) hv[t][u] = load_k4(arow[t], k, kend, vec);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = sbk::mfma_32x32x2(hv[t][u].x, wv[u].x, acc[t]);
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = sbk::mfma_32x32x2(hv[t][u].y, wv[u].y, acc[t]);
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = sbk::mfma_32x32x2(hv[t][u].z, wv[u].z, acc[t]);
#pragma unroll
      for (int t = 0; t < RT; ++t) acc[t] = sbk::mfma_32x32x2(hv[t][u].w, wv[u].w, acc[t]);
    }
  }
}

template <int RT>
__global__ void __launch_bounds__(256) rnnlm_lstm_kernel(LstmArgs a) {
  __shared__ float part[4 * kBT * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int H = a.H, n = a.n, j0 = blockIdx.x * kJS, r0 = blockIdx.y * (RT * kBT);
  const bool vec = (H & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.w_h) | reinterpret_cast<uintptr_t>(a.w_x) |
                                     reinterpret_cast<uintptr_t>(a.h_in) | reinterpret_cast<uintptr_t>(a.x)) & 15) == 0;
  // this lane's operands: B = the gate row of column col = gate * kJS + unit; A = the state / input row of tile row col
  const int gate = col / kJS, unit = j0 + col % kJS;
  const size_t wofs = ((size_t)gate * H + unit) * H;
  const float* hrow[RT];
  const float* xrow[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int r = r0 + t * kBT + col;
    const int p = r < n ? (a.parent != nullptr ? clampi(a.parent[r], n - 1) : r) : 0;
    hrow[t] = (r < n && a.h_in != nullptr) ? a.h_in + (size_t)p * H : nullptr;
    xrow[t] = (r < n && a.x != nullptr) ? a.x + (size_t)r * H : nullptr;
  }
  sbk::f32x16 acc[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
  if (a.w_x != nullptr) accumulate<RT>(acc, xrow, unit < H ? a.w_x + wofs : nullptr, H, wave, half, vec);
  if (a.h_in != nullptr) accumulate<RT>(acc, hrow, unit < H ? a.w_h + wofs : nullptr, H, wave, half, vec);

  // thread -> (row of the tile, unit): the four gates of one cell
  const int bl = tid / kJS, jj = tid % kJS, j = j0 + jj;
  float* mine = part + wave * (kBT * 33);
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if (t > 0) __syncthreads();  // (the previous tile's partials have been read)
#pragma unroll
    for (int q = 0; q < 16; ++q) mine[((q & 3) + 8 * (q >> 2) + 4 * half) * 33 + col] = acc[t][q];
    __syncthreads();
    const int r = r0 + t * kBT + bl;
    if (r < n && j < H) {
      const float* erow = a.w_x == nullptr ? a.emb_ih + (size_t)clampi(a.tokens[r], a.n_emb - 1) * 4 * H : nullptr;
      float g4[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = bl * 33 + g * kJS + jj;
        float v = (part[c] + part[kBT * 33 + c]) + (part[2 * kBT * 33 + c] + part[3 * kBT * 33 + c]);
        const int gi = g * H + j;
        if (erow != nullptr) v += erow[gi];
        if (a.b_ih != nullptr) v += a.b_ih[gi];
        if (a.b_hh != nullptr) v += a.b_hh[gi];
        g4[g] = v;
      }
      float c_prev = 0.0f;
      if (a.c_in != nullptr) c_prev = a.c_in[(size_t)(a.parent != nullptr ? clampi(a.parent[r], n - 1) : r) * H + j];
      const float c_new = sbk::sigmoid(g4[1]) * c_prev + sbk::sigmoid(g4[0]) * tanhf(g4[2]);
      a.c_out[(size_t)r * H + j] = c_new;
      a.h_out[(size_t)r * H + j] = sbk::sigmoid(g4[3]) * tanhf(c_new);
    }
  }
}

// y = act(LayerNorm(y)) in place, one workgroup per row: two-pass mean / variance, the RNNLM's activations (torch's rules)
__global__ void __launch_bounds__(256) rnnlm_ln_act_kernel(float* y, const float* gamma, const float* beta, int D, float eps, int act) {
  __shared__ float red[4];
  float* row = y + (size_t)blockIdx.x * D;
  float s = 0.0f;
  for (int k = threadIdx.x; k < D; k += 256) s += row[k];
  const float mean = sbk::block_sum(s, red) / (float)D;
  float q = 0.0f;
  for (int k = threadIdx.x; k < D; k += 256) q += (row[k] - mean) * (row[k] - mean);
  const float rstd = 1.0f / sqrtf(sbk::block_sum(q, red) / (float)D + eps);
  for (int k = threadIdx.x; k < D; k += 256) row[k] = sbk::joint_act((row[k] - mean) * rstd * gamma[k] + beta[k], act);
}

// flag = max(flag, 1) for a token outside [0, n_emb), max(flag, 2) for a parent outside [0, n)
__global__ void __launch_bounds__(256) rnnlm_validate_kernel(const int32_t* tokens, const int32_t* parent, int n, int n_emb, int* flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (tokens[i] < 0 || tokens[i] >= n_emb) atomicMax(flag, 1);
  if (parent != nullptr && (parent[i] < 0 || parent[i] >= n)) atomicMax(flag, 2);
}

__global__ void __launch_bounds__(256) rnnlm_zero_kernel(float* p, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < count) p[i] = 0.0f;
}

template <int RT>
int launch_lstm(const LstmArgs& a, hipStream_t st) {
  const dim3 grid(sbk::cdiv(a.H, kJS), sbk::cdiv(a.n, RT * kBT));
  const double K = (a.w_x ? 1.0 : 0.0) + (a.h_in ? 1.0 : 0.0), tiles = (double)grid.x * grid.y;
  sbk::ProfScope prof("rnnlm_lstm", 2.0 * RT * kBT * 32.0 * a.H * K * tiles + 30.0 * a.n * a.H,
                      4.0 * (32.0 + RT * kBT) * a.H * K * tiles + 4.0 * 8.0 * a.n * a.H, st);
  SBK_LAUNCH(rnnlm_lstm_kernel<RT>, grid, dim3(256), 0, st, a);
  return sbk::launch_status("rnnlm_lstm");
}

int check_lm(const sbk_rnnlm_weights* M, const char* who) {
  SBK_REQUIRE(M != nullptr, "%s: null weights", who);
  SBK_REQUIRE(M->n_layers >= 1 && M->n_layers <= SBK_TRANSDUCER_MAX_LAYERS, "%s: n_layers=%d is outside the limits 1 <= n_layers <= %d",
              who, M->n_layers, SBK_TRANSDUCER_MAX_LAYERS);
  SBK_REQUIRE(M->hidden >= 1 && M->hidden <= kMaxH, "%s: H=%d is outside the limits 1 <= H <= %d", who, M->hidden, kMaxH);
  SBK_REQUIRE(M->n_dnn >= 1 && M->n_dnn <= SBK_RNNLM_MAX_DNN, "%s: n_dnn=%d DNN blocks in the LM (1..%d supported)", who, M->n_dnn,
              SBK_RNNLM_MAX_DNN);
  SBK_REQUIRE(M->dnn >= 1 && M->vocab >= 1 && M->n_emb >= 1, "%s: dnn=%d vocab=%d n_emb=%d (each >= 1)", who, M->dnn, M->vocab, M->n_emb);
  SBK_REQUIRE(sbk::joint_act_known(M->act), "%s: act=%d (LEAKY_RELU, RELU, GELU or TANH)", who, M->act);
  SBK_REQUIRE(M->emb_ih && M->out, "%s: null emb_ih / out", who);
  for (int l = 0; l < M->n_layers; ++l) {
    SBK_REQUIRE(M->w_hh[l] && (l == 0 || M->w_ih[l]), "%s: null LSTM weight of layer %d", who, l);
    SBK_REQUIRE((M->b_ih[l] == nullptr) == (M->b_hh[l] == nullptr), "%s: b_ih and b_hh of layer %d are given together or not at all", who, l);
  }
  for (int i = 0; i < M->n_dnn; ++i) SBK_REQUIRE(M->dnn_w[i] && M->ln_g[i] && M->ln_b[i], "%s: null weight of DNN block %d", who, i);
  return 0;
}

inline size_t align4(size_t v) { return (v + 3) & ~(size_t)3; }

}  // namespace

namespace sbk {

size_t rnnlm_step_workspace_floats(const sbk_rnnlm_weights* M, int n) { return M->n_dnn * align4((size_t)n * M->dnn) + 4; }

int rnnlm_state_zero(float* state, const sbk_rnnlm_weights* M, int n, hipStream_t st) {
  const size_t count = (size_t)M->n_layers * 2 * n * M->hidden;
  SBK_LAUNCH(rnnlm_zero_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, state, count);
  return launch_status("rnnlm_state_zero");
}

// The step without the argument checks of the C entry (the search calls it once per decoding step: the kernels clamp).
int rnnlm_step(const sbk_rnnlm_weights* M, const int32_t* tokens, const int32_t* parent, const float* state_in, float* state_out,
               float* ws, float* out, float weight, float temperature, int n, hipStream_t st) {
  const int H = M->hidden, D = M->dnn;
  const size_t nh = (size_t)n * H;
  const int tiles = cdiv(n, kBT);
  for (int l = 0; l < M->n_layers; ++l) {
    LstmArgs a;
    a.w_x = l == 0 ? nullptr : M->w_ih[l];
    a.w_h = M->w_hh[l];
    a.b_ih = M->b_ih[l];
    a.b_hh = M->b_hh[l];
    a.emb_ih = M->emb_ih;
    a.tokens = tokens;
    a.parent = parent;
    a.x = l == 0 ? nullptr : state_out + (size_t)(l - 1) * 2 * nh;
    a.h_in = state_in != nullptr ? state_in + (size_t)l * 2 * nh : nullptr;
    a.c_in = state_in != nullptr ? a.h_in + nh : nullptr;
    a.h_out = state_out + (size_t)l * 2 * nh;
    a.c_out = a.h_out + nh;
    a.n = n, a.H = H, a.n_emb = M->n_emb;
    SBK_TRY(tiles == 1 ? launch_lstm<1>(a, st) : tiles == 2 ? launch_lstm<2>(a, st) : launch_lstm<kMaxRT>(a, st));
  }
  const float* x = state_out + (size_t)(M->n_layers - 1) * 2 * nh;
  int K = H;
  for (int i = 0; i < M->n_dnn; ++i) {
    float* y = ws + (size_t)i * align4((size_t)n * D);
    SBK_TRY(gemm_nt_ws(x, K, M->dnn_w[i], K, M->dnn_b[i], nullptr, 0, y, D, n, D, K, SBK_ACT_NONE, 1.0f, nullptr, 0, nullptr, 0, st));
    {
      ProfScope prof("rnnlm_ln_act", 10.0 * n * D, 4.0 * 2.0 * n * D, st);
      SBK_LAUNCH(rnnlm_ln_act_kernel, dim3(n), dim3(256), 0, st, y, M->ln_g[i], M->ln_b[i], D, M->ln_eps[i], M->act);
    }
    SBK_TRY(launch_status("rnnlm_ln_act"));
    x = y, K = D;
  }
  SBK_TRY(gemm_nt_ws(x, K, M->out, K, M->out_b, nullptr, 0, out, M->vocab, n, M->vocab, K, SBK_ACT_NONE, 1.0f, nullptr, 0, nullptr, 0, st));
  return log_softmax_rows(out, out, n, M->vocab, temperature, weight, st);
}

int rnnlm_check(const sbk_rnnlm_weights* M, const char* who) { return check_lm(M, who); }

}  // namespace sbk

extern "C" size_t sbk_rnnlm_step_workspace_bytes(const sbk_rnnlm_weights* LM, int n) {
  if (!LM || n < 1 || n > kMaxRows || LM->n_dnn < 1 || LM->n_dnn > SBK_RNNLM_MAX_DNN || LM->dnn < 1) return 0;
  return sbk::rnnlm_step_workspace_floats(LM, n) * sizeof(float);
}

extern "C" int sbk_rnnlm_step_f32(const sbk_rnnlm_weights* LM, const int32_t* tokens, const int32_t* parent, const float* state_in,
                                  float* state_out, void* workspace, size_t workspace_bytes, float* out, float weight,
                                  float temperature, int n, sbk_stream_t stream) {
  SBK_TRY(check_lm(LM, "rnnlm_step"));
  SBK_REQUIRE(n >= 1 && n <= kMaxRows, "rnnlm_step: n=%d is outside the limits 1 <= n <= %d", n, kMaxRows);
  SBK_REQUIRE(tokens && state_out && workspace && out, "rnnlm_step: null operand (tokens, state_out, workspace and out are required)");
  SBK_REQUIRE(state_in != state_out, "rnnlm_step: state_out must not alias state_in");
  SBK_REQUIRE(temperature > 0.0f, "rnnlm_step: temperature=%g (temperature > 0)", (double)temperature);
  SBK_REQUIRE(workspace_bytes >= sbk_rnnlm_step_workspace_bytes(LM, n), "rnnlm_step: workspace too small");
  const hipStream_t st = sbk::as_stream(stream);
  float* ws = static_cast<float*>(workspace);
  // tokens in [0, n_emb) and parent in [0, n), checked on the device (one 4-byte read-back; the kernels themselves clamp)
  int* flag = reinterpret_cast<int*>(ws + sbk::rnnlm_step_workspace_floats(LM, n) - 4);
  SBK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  SBK_LAUNCH(rnnlm_validate_kernel, dim3(sbk::cdiv(n, 256)), dim3(256), 0, st, tokens, parent, n, LM->n_emb, flag);
  SBK_TRY(sbk::launch_status("rnnlm_validate"));
  int host = 0;
  SBK_HIP(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  SBK_HIP(hipStreamSynchronize(st));
  SBK_REQUIRE(host != 1, "rnnlm_step: a token in tokens is outside the limits 0 <= token < n_emb = %d", LM->n_emb);
  SBK_REQUIRE(host != 2, "rnnlm_step: a row in parent is outside the limits 0 <= parent < n = %d", n);
  return sbk::rnnlm_step(LM, tokens, parent, state_in, state_out, ws, out, weight, temperature, n, st);
}
