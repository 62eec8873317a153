// One SLi-GRU layer for every utterance and both directions over the padded length (sbk_sligru_layer_f32): the recurrent stack of
// a CRDNN encoder with rnn_class SLiGRU (nnet/RNN.py:1623-1804).  Per step
//     gates = xp[:, t] + LayerNorm_{2H}(h_{t-1} . u^T);   a, z = gates.chunk(2)
//     h_t   = sigmoid(z) * h_{t-1} + (1 - sigmoid(z)) * act(a)
// The sibling of csrc/rnn.hip, with three differences that decide its shape:
//   * the LayerNorm spans ALL 2H columns of the recurrent product, so the cell update of a unit cannot be fused behind the
//     product of the workgroup that owns the unit's columns: a step is TWO launches, the product and the norm-and-cell pass;
//   * the two directions share u (and the norm): they are rows of ONE product, D*B rows direction-major, and a workgroup's slice
//     of u is loaded once for both.  Direction 1 at scan step s reads xp at frame T-1-s and writes at that frame;
//   * there is no c state: `out` is the history and the state buffer, as in the LSTM layer.
//
// Product launch (sligru_product_kernel): a workgroup owns kJS = 8 hidden units with both of their gate rows -- 16 columns, one
// v_mfma_f32_16x16x4_f32 tile wide -- and a tile of 32 rows (two MFMA tiles that share the u operand).  H/8 x ceil(D*B/32)
// workgroups: 256 at the recipe shape (H 1024, D 2, B 32), one per CU; the 32-wide instruction with 16 units per workgroup would
// give 128.  Its four waves split K = H into four contiguous parts; the partial tiles meet in LDS and are added in wave order
// (a fixed summation order: the same bits on every run and stream).  The raw slice goes to the workspace as [D*B, 2H].
//
// Norm-and-cell launch (sligru_cell_kernel): one workgroup per row.  A thread holds the a and z values of up to 8 units in
// registers, the mean and then the centred sum of squares are reduced over the workgroup (two passes over registers, a fixed
// butterfly inside a wave and wave order across the four), then the affine, xp, the cell, h_t to `out` (and `hn` on the last step).
// Nothing of size T*2H besides xp and out is written.  No atomics.
#include "act.h"
#include "common.h"
#include "device.h"
#include "kernel_util.h"

namespace {

constexpr int kJS = 8;        // hidden units of a workgroup's slice (x 2 gates = the 16 columns of an MFMA tile)
constexpr int kRT = 32;       // rows (direction x utterance) of a row tile: two 16-row MFMA tiles
constexpr int kKC = 16;       // k of a chunk: four MFMAs, a float4 per lane and operand row
constexpr int kMaxH = 2048;   // widest layer accepted, as csrc/rnn.hip
constexpr int kPer = kMaxH / 256;  // units of a thread in the norm-and-cell pass
constexpr float kEps = 1e-5f;      // torch.nn.LayerNorm's default, the reference's

struct SligruArgs {
  const float* xp;     // [B,T,2H]
  const float* u;      // [2H,H]
  const float* gamma;  // [2H] or nullptr
  const float* beta;
  const float* h0;     // [D,B,H] or nullptr
  float* out;          // [B,T,D*H]
  float* hn;           // [D,B,H]
  float* raw;          // the workspace [D*B,2H]
  int B, T, H, D, act, step;
};

// four consecutive k of a row, zeros past K (rows of a width that is no multiple of 4 are not 16-byte aligned: scalar loads)
__device__ __forceinline__ float4 load_k4(const float* row, int k, int K, bool vec) {
  if (row == nullptr) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (vec) return k < K ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return make_float4(k < K ? row[k] : 0.0f, k + 1 < K ? row[k + 1] : 0.0f, k + 2 < K ? row[k + 2] : 0.0f,
                     k + 3 < K ? row[k + 3] : 0.0f);
}

// h_{t-1} of row r = d * B + b at scan step s: the previous frame of the same direction in `out`, h0 at the first step
__device__ __forceinline__ const float* prev_row(const SligruArgs& a, int r) {
  const int d = r / a.B, b = r % a.B;
  if (a.step == 0) return a.h0 != nullptr ? a.h0 + (size_t)r * a.H : nullptr;
  const int tp = d == 0 ? a.step - 1 : a.T - a.step;
  return a.out + ((size_t)b * a.T + tp) * ((size_t)a.D * a.H) + (size_t)d * a.H;
}

__global__ void __launch_bounds__(256) sligru_product_kernel(SligruArgs a) {
  __shared__ float part[4 * kRT * 17];
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int col = lane & 15, kg = lane >> 4;
  const int H = a.H, R = a.D * a.B;
  const int j0 = blockIdx.x * kJS, r0 = blockIdx.y * kRT;
  // this lane's operand rows: A = h_{t-1} of rows r0 + col and r0 + 16 + col, B = the row of u of column col = gate * kJS + unit
  const int unit = j0 + col % kJS;
  const float* urow = unit < H ? a.u + ((size_t)(col / kJS) * H + unit) * H : nullptr;
  const float* hrow0 = r0 + col < R ? prev_row(a, r0 + col) : nullptr;
  const float* hrow1 = r0 + 16 + col < R ? prev_row(a, r0 + 16 + col) : nullptr;
  const bool vec = (H & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.u) | reinterpret_cast<uintptr_t>(a.out) |
                                     reinterpret_cast<uintptr_t>(a.h0)) & 15) == 0;
  sbk::f32x4 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc0[r] = acc1[r] = 0.0f;
  // wave w takes the w-th part of K in whole chunks of 16; inside a chunk the lanes of k group kg supply k 4 kg .. 4 kg + 3, one
  // per MFMA.  kUnroll chunks per trip: their 3 x kUnroll 16-byte loads are issued before the first MFMA that needs one (a step is
  // bound by the latency of the rows of u, not by the 8 MFMAs of a chunk); chunks past the part load zeros and add nothing
  constexpr int kUnroll = 8;
  const int kq = sbk::uniform(((H + 4 * kKC - 1) / (4 * kKC)) * kKC);
  const int kend = min(H, (wave + 1) * kq);
  for (int k0 = wave * kq; k0 < kend; k0 += kKC * kUnroll) {
    float4 uv[kUnroll], h0v[kUnroll], h1v[kUnroll];
#pragma unroll
    for (int c = 0; c < kUnroll; ++c) {
      const int k = k0 + kKC * c + 4 * kg;  // a trip reads 128 consecutive k of every row: whole 128-byte lines
      uv[c] = load_k4(urow, k, kend, vec);
      h0v[c] = load_k4(hrow0, k, kend, vec);
      h1v[c] = load_k4(hrow1, k, kend, vec);
    }
#pragma unroll
    for (int c = 0; c < kUnroll; ++c) {
      acc0 = sbk::mfma_16x16x4(h0v[c].x, uv[c].x, acc0);
      acc1 = sbk::mfma_16x16x4(h1v[c].x, uv[c].x, acc1);
      acc0 = sbk::mfma_16x16x4(h0v[c].y, uv[c].y, acc0);
      acc1 = sbk::mfma_16x16x4(h1v[c].y, uv[c].y, acc1);
      acc0 = sbk::mfma_16x16x4(h0v[c].z, uv[c].z, acc0);
      acc1 = sbk::mfma_16x16x4(h1v[c].z, uv[c].z, acc1);
      acc0 = sbk::mfma_16x16x4(h0v[c].w, uv[c].w, acc0);
      acc1 = sbk::mfma_16x16x4(h1v[c].w, uv[c].w, acc1);
    }
  }
  float* mine = part + wave * (kRT * 17);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mine[(4 * kg + r) * 17 + col] = acc0[r];
    mine[(16 + 4 * kg + r) * 17 + col] = acc1[r];
  }
  __syncthreads();
  // thread -> (row, unit): both gates of one unit, added in wave order
  const int rl = tid / kJS, row = r0 + rl, jj = tid % kJS, j = j0 + jj;
  if (row < R && j < H) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int c = rl * 17 + g * kJS + jj;
      a.raw[(size_t)row * 2 * H + (size_t)g * H + j] =
          (part[c] + part[kRT * 17 + c]) + (part[2 * kRT * 17 + c] + part[3 * kRT * 17 + c]);
    }
  }
}

__device__ __forceinline__ float cell_act(float v, int kind) {
  switch (kind) {  // uniform
    case SBK_SLIGRU_TANH: return tanhf(v);
    case SBK_SLIGRU_SIN: return sinf(v);
    case SBK_SLIGRU_LEAKY_RELU: return sbk::leaky_relu(v);
    default: return v <= 0.0f ? 0.0f : v;  // torch.relu's rule
  }
}

// raw_zero: the first step of a layer without h0 -- the product of a zero state was not launched
__global__ void __launch_bounds__(256) sligru_cell_kernel(SligruArgs a, int raw_zero) {
  __shared__ float red[4];
  const int tid = threadIdx.x, r = blockIdx.x, H = a.H;
  const int d = r / a.B, b = r % a.B;
  const int t = d == 0 ? a.step : a.T - 1 - a.step;
  const float* raw = a.raw + (size_t)r * 2 * H;
  float va[kPer], vz[kPer];
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int j = tid + 256 * i;
    const bool in = j < H && !raw_zero;
    va[i] = in ? raw[j] : 0.0f;
    vz[i] = in ? raw[H + j] : 0.0f;
    s += va[i] + vz[i];
  }
  const float n = 2.0f * (float)H;
  const float mean = sbk::block_sum(s, red) / n;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    if (tid + 256 * i < H) {
      const float ca = va[i] - mean, cz = vz[i] - mean;
      q += ca * ca + cz * cz;
    }
  }
  const float rstd = 1.0f / sqrtf(sbk::block_sum(q, red) / n + kEps);
  const float* hprev = prev_row(a, r);
  const float* xrow = a.xp + ((size_t)b * a.T + t) * 2 * H;
  float* orow = a.out + ((size_t)b * a.T + t) * ((size_t)a.D * H) + (size_t)d * H;
  const bool last = a.step == a.T - 1;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int j = tid + 256 * i;
    if (j < H) {
      float ya = (va[i] - mean) * rstd, yz = (vz[i] - mean) * rstd;
      if (a.gamma != nullptr) {
        ya = ya * a.gamma[j] + a.beta[j];
        yz = yz * a.gamma[H + j] + a.beta[H + j];
      }
      const float z = sbk::sigmoid(xrow[H + j] + yz);
      const float hp = hprev != nullptr ? hprev[j] : 0.0f;
      const float h = z * hp + (1.0f - z) * cell_act(xrow[j] + ya, a.act);
      orow[j] = h;
      if (last) a.hn[(size_t)r * H + j] = h;
    }
  }
}

size_t raw_bytes_of(int B, int H, int D) { return (((size_t)D * B * 2 * H * sizeof(float)) + 15) & ~(size_t)15; }
bool shape_ok(int B, int H, int D) { return H >= 1 && H <= kMaxH && (D == 1 || D == 2) && B >= 1 && B <= 65535 * kRT / 2; }

}  // namespace

extern "C" size_t sbk_sligru_layer_workspace_bytes(int B, int H, int D) { return shape_ok(B, H, D) ? raw_bytes_of(B, H, D) : 0; }

extern "C" int sbk_sligru_layer_f32(const float* xp, const float* u, const float* ln_gamma, const float* ln_beta, const float* h0,
                                    float* out, float* hn, void* workspace, size_t workspace_bytes, int B, int T, int H, int D,
                                    int act, sbk_stream_t stream) {
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "sligru_layer: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(D == 1 || D == 2, "sligru_layer: D=%d directions (D is 1 or 2)", D);
  SBK_REQUIRE(B >= 1 && B <= 65535 * kRT / 2, "sligru_layer: B=%d is outside the limits 1 <= B <= %d", B, 65535 * kRT / 2);
  SBK_REQUIRE(T >= 1, "sligru_layer: T=%d (T >= 1)", T);
  SBK_REQUIRE(act >= SBK_SLIGRU_RELU && act <= SBK_SLIGRU_LEAKY_RELU,
              "sligru_layer: act=%d (SBK_SLIGRU_RELU, _TANH, _SIN and _LEAKY_RELU are implemented)", act);
  SBK_REQUIRE(xp && u && out && hn && workspace,
              "sligru_layer: null operand (xp, u, out, hn and workspace are required)");
  SBK_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr), "sligru_layer: ln_gamma and ln_beta are given together or not at all");
  SBK_REQUIRE(h0 == nullptr || (h0 != hn && h0 != out), "sligru_layer: h0 must not alias hn or out");
  SBK_REQUIRE(workspace_bytes >= raw_bytes_of(B, H, D), "sligru_layer: workspace of %zu bytes is too small (%zu needed)",
              workspace_bytes, raw_bytes_of(B, H, D));
  SBK_REQUIRE(sbk::aligned16(workspace), "sligru_layer: workspace must be 16-byte aligned");
  SligruArgs a;
  a.xp = xp; a.u = u; a.gamma = ln_gamma; a.beta = ln_beta; a.h0 = h0; a.out = out; a.hn = hn;
  a.raw = static_cast<float*>(workspace);
  a.B = B; a.T = T; a.H = H; a.D = D; a.act = act;
  const hipStream_t st = sbk::as_stream(stream);
  const int R = D * B;
  const dim3 grid(sbk::cdiv(H, kJS), sbk::cdiv(R, kRT));
  const double tiles = (double)grid.x * grid.y;
  for (int s = 0; s < T; ++s) {
    a.step = s;
    const int raw_zero = s == 0 && h0 == nullptr;
    if (!raw_zero) {
      sbk::ProfScope prof("sligru_product", 2.0 * kRT * 16.0 * H * tiles, 4.0 * (16.0 + kRT) * H * tiles + 4.0 * 2.0 * R * H, st);
      SBK_LAUNCH(sligru_product_kernel, grid, dim3(256), 0, st, a);
    }
    sbk::ProfScope prof("sligru_norm_cell", 24.0 * R * H, 4.0 * 6.0 * R * H, st);
    SBK_LAUNCH(sligru_cell_kernel, dim3(R), dim3(256), 0, st, a, raw_zero);
  }
  return sbk::launch_status("sbk_sligru_layer_f32");
}
