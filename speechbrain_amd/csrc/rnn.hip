// One recurrent layer for every utterance and every direction over the padded length (sbk_rnn_layer_f32): the LSTM stack of a
// CRDNN encoder (lobes/models/CRDNN.py:158-185 with nnet/RNN.py:187-302, torch.nn.LSTM semantics, gate order i, f, g, o).
//
// The recurrence is BATCHED: a step of one direction is the product [B,H] x [H,4H].  A workgroup owns kJS = 8 hidden units of one
// direction together with all four of their gate rows -- 32 columns, one v_mfma_f32_32x32x2_f32 tile wide -- and a tile of 32
// utterances, so the cell update is fused behind the product and a unit's four gates never leave the workgroup.  Its four waves
// split K = H into four contiguous quarters; the four partial tiles meet in LDS and are added in wave order (a fixed summation order:
// two runs give the same bits).  B is padded to the tile in registers only (rows past B load zeros and store nothing).
//
// Step launches: one launch per time step covers both directions and the whole batch, H/8 x D x ceil(B/32) workgroups (256 at the
// recipe shape H 1024, D 2, B 32: one per CU).  There is no communication between workgroups inside a launch: h of the previous
// step is read from `out` itself -- the row of the previous time index of the same direction, written by the previous launch --
// so the history doubles as the state buffer; c lives in `cn`, where element (d, b, j) is read and written by one thread only.
// Direction 1 scans t = T-1 .. 0 and writes at its own t.
//
// (A persistent form -- one cooperative launch per layer, the W_hh slices resident in LDS, a bounded grid barrier per step -- was
// built from the same device function, gave the same bits and was slower at B 32 and B 1: removed)
//
// Per step and direction the workgroups together read W_hh once per batch tile (16 MiB at H 1024: it stays in the Infinity Cache
// between steps) and the [B,H] state once per workgroup.
#include "act.h"
#include "common.h"
#include "device.h"

namespace {

constexpr int kJS = 8;        // hidden units of a workgroup's slice (x 4 gates = the 32 columns of an MFMA tile)
constexpr int kBT = 32;       // utterances of a batch tile (the 32 rows of an MFMA tile)
constexpr int kMaxH = 2048;   // widest layer accepted (tests/test_rnn_kernels.py runs H 2048 on the GPU)

struct RnnArgs {
  const float* xp;    // [B,T,D,4H]
  const float* w_hh;  // [D,4H,H]
  const float* b_ih;  // [D,4H] or nullptr
  const float* b_hh;
  const float* h0;    // [D,B,H] or nullptr
  const float* c0;
  float* out;         // [B,T,D*H]
  float* hn;          // [D,B,H]
  float* cn;
  int B, T, H, D, step;
};

// four consecutive k of a row, zeros past K (rows of a width that is no multiple of 4 are not 16-byte aligned: scalar loads)
__device__ __forceinline__ float4 load_k4(const float* row, int k, int K, bool vec) {
  if (row == nullptr) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (vec) return k < K ? *reinterpret_cast<const float4*>(row + k) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  return make_float4(k < K ? row[k] : 0.0f, k + 1 < K ? row[k + 1] : 0.0f, k + 2 < K ? row[k + 2] : 0.0f,
                     k + 3 < K ? row[k + 3] : 0.0f);
}

// The slice product and the cell update of one (direction, slice of hidden units, batch tile) at one step.  hprev: the rows of
// h_{t-1} (row stride ldh) or nullptr for zeros; part: LDS [4 waves][32 rows][33].
__device__ __forceinline__ void lstm_slice_step(const RnnArgs& a, int d, int j0, int b0, int t, const float* hprev, long ldh,
                                                bool first, bool last, float* part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int H = a.H;
  const bool vec = (H & 3) == 0 && (ldh & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(a.w_hh) | reinterpret_cast<uintptr_t>(hprev)) & 15) == 0;
  // this lane's operand rows: A = h_{t-1} of utterance b0 + col, B = the gate row of column col = gate * kJS + unit
  const int b_row = b0 + col, gate = col / kJS, unit = j0 + col % kJS;
  const float* hrow = (hprev != nullptr && b_row < a.B) ? hprev + (size_t)b_row * ldh : nullptr;
  const float* wrow = unit < H ? a.w_hh + ((size_t)d * 4 * H + (size_t)gate * H + unit) * H : nullptr;
  sbk::f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  if (hprev != nullptr) {
    // wave w takes the w-th quarter of K; inside a chunk of 8 k lanes 0-31 supply k 0..3 and lanes 32-63 k 4..7 of the four MFMAs
    // kUnroll chunks per trip: their 2 x kUnroll 16-byte loads are issued before the first MFMA that needs one (a step is
    // bound by the latency of the W_hh rows, not by the 4 MFMAs of a chunk); chunks past the quarter load zeros and add nothing
    constexpr int kUnroll = 8;
    const int kq = sbk::uniform(((H + 31) / 32) * 8);  // a wave's quarter of K, in whole chunks of 8
    const int kend = min(H, (wave + 1) * kq);
    for (int k0 = wave * kq; k0 < kend; k0 += 8 * kUnroll) {
      float4 hv[kUnroll], wv[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int k = k0 + 8 * u + 4 * half;  // a trip reads 64 consecutive k of every row: whole 128-byte lines
        wv[u] = load_k4(wrow, k, kend, vec);
        hv[u] = load_k4(hrow, k, kend, vec);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        acc = sbk::mfma_32x32x2(hv[u].x, wv[u].x, acc);
        acc = sbk::mfma_32x32x2(hv[u].y, wv[u].y, acc);
        acc = sbk::mfma_32x32x2(hv[u].z, wv[u].z, acc);
        acc = sbk::mfma_32x32x2(hv[u].w, wv[u].w, acc);
      }
    }
  }
  float* mine = part + wave * (kBT * 33);
#pragma unroll
  for (int r = 0; r < 16; ++r) mine[((r & 3) + 8 * (r >> 2) + 4 * half) * 33 + col] = acc[r];
  __syncthreads();
  // thread -> (utterance, unit): the four gates of one cell
  const int bl = tid / kJS, b = b0 + bl, jj = tid % kJS, j = j0 + jj;
  if (b < a.B && j < H) {
    float g4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = bl * 33 + g * kJS + jj;
      float v = (part[c] + part[kBT * 33 + c]) + (part[2 * kBT * 33 + c] + part[3 * kBT * 33 + c]);
      const size_t gi = (size_t)d * 4 * H + (size_t)g * H + j;
      if (a.b_hh != nullptr) v += a.b_hh[gi];
      float x = a.xp[(((size_t)b * a.T + t) * a.D + d) * 4 * H + (size_t)g * H + j];
      if (a.b_ih != nullptr) x += a.b_ih[gi];
      g4[g] = x + v;
    }
    const size_t si = ((size_t)d * a.B + b) * H + j;
    const float c_prev = first ? (a.c0 != nullptr ? a.c0[si] : 0.0f) : a.cn[si];
    const float c_new = sbk::sigmoid(g4[1]) * c_prev + sbk::sigmoid(g4[0]) * tanhf(g4[2]);
    const float h_new = sbk::sigmoid(g4[3]) * tanhf(c_new);
    a.cn[si] = c_new;
    a.out[((size_t)b * a.T + t) * ((size_t)a.D * H) + (size_t)d * H + j] = h_new;
    if (last) a.hn[si] = h_new;
  }
}

__global__ void __launch_bounds__(256) rnn_lstm_step_kernel(RnnArgs a) {
  __shared__ float part[4 * kBT * 33];
  const int d = blockIdx.y, j0 = blockIdx.x * kJS, b0 = blockIdx.z * kBT;
  const int s = a.step, t = d == 0 ? s : a.T - 1 - s;
  const long ldo = (long)a.T * a.D * a.H;  // floats between the same (t, direction) of consecutive utterances in `out`
  const float* hprev;
  long ldh;
  if (s == 0) {
    hprev = a.h0 != nullptr ? a.h0 + (size_t)d * a.B * a.H : nullptr;
    ldh = a.H;
  } else {
    const int tp = d == 0 ? t - 1 : t + 1;
    hprev = a.out + (size_t)tp * a.D * a.H + (size_t)d * a.H;
    ldh = ldo;
  }
  lstm_slice_step(a, d, j0, b0, t, hprev, ldh, s == 0, s == a.T - 1, part);
}

}  // namespace

extern "C" int sbk_rnn_layer_route(int B, int T, int H, int D) {
  if (B < 1 || T < 1 || H < 1 || H > kMaxH || D < 1 || D > 2) return 0;
  return 1;  // step launches (the one route of this revision)
}

extern "C" int sbk_rnn_layer_f32(const float* xp, const float* w_hh, const float* b_ih, const float* b_hh, const float* h0,
                                 const float* c0, float* out, float* hn, float* cn, int B, int T, int H, int D, int cell,
                                 int route, sbk_stream_t stream) {
  SBK_REQUIRE(cell == SBK_RNN_LSTM, "rnn_layer: cell=%d is not implemented (SBK_RNN_LSTM = %d is)", cell, SBK_RNN_LSTM);
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "rnn_layer: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(D == 1 || D == 2, "rnn_layer: D=%d directions (D is 1 or 2)", D);
  SBK_REQUIRE(B >= 1 && B <= 65535 * kBT, "rnn_layer: B=%d is outside the limits 1 <= B <= %d", B, 65535 * kBT);
  SBK_REQUIRE(T >= 1, "rnn_layer: T=%d (T >= 1)", T);
  SBK_REQUIRE(route == 0 || route == 1, "rnn_layer: route=%d (0 = the default, 1 = step launches)", route);
  SBK_REQUIRE(xp && w_hh && out && hn && cn, "rnn_layer: null operand (xp, w_hh, out, hn and cn are required)");
  SBK_REQUIRE((b_ih == nullptr) == (b_hh == nullptr), "rnn_layer: b_ih and b_hh are given together or not at all");
  SBK_REQUIRE(h0 == nullptr || (h0 != hn && h0 != out), "rnn_layer: h0 must not alias hn or out");
  RnnArgs a;
  a.xp = xp; a.w_hh = w_hh; a.b_ih = b_ih; a.b_hh = b_hh; a.h0 = h0; a.c0 = c0; a.out = out; a.hn = hn; a.cn = cn;
  a.B = B; a.T = T; a.H = H; a.D = D;
  const hipStream_t st = sbk::as_stream(stream);
  const dim3 grid(sbk::cdiv(H, kJS), D, sbk::cdiv(B, kBT));
  const double tiles = (double)grid.x * D * grid.z;
  sbk::ProfScope prof("rnn_lstm_steps", (double)T * (2.0 * kBT * 32.0 * H * tiles + 30.0 * B * H * D),
                      (double)T * (4.0 * (32.0 + kBT) * H * tiles + 4.0 * 6.0 * B * H * D), st);
  for (int s = 0; s < T; ++s) {
    a.step = s;
    SBK_LAUNCH(rnn_lstm_step_kernel, grid, dim3(256), 0, st, a);
  }
  return sbk::launch_status("sbk_rnn_layer_f32");
}
