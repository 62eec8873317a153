// The recurrent layer of csrc/rnn.hip with its product h_{t-1} . W_hh^T on the bf16 matrix pipe (sbk_rnn_layer_bf16): the opt-in
// precision "bf16" of a CRDNN encoder's LSTM stack.  Same semantics (torch.nn.LSTM, gate order i, f, g, o, direction 1 scans
// t = T-1 .. 0, `out` is the history, h0 / c0 optional, hn / cn returned) and the same ownership: a workgroup owns kJS = 8 hidden
// units x 4 gates (the 32 columns of an MFMA tile) of one direction and a tile of 32 utterances, its four waves take contiguous
// quarters of K, the partial tiles meet in LDS and are added in wave order, the cell update is fused behind the product and
// c(d, b, j) belongs to one thread.  One launch per time step covers both directions and all batch tiles.
//
// What is rounded: W_hh and h_{t-1}, to bf16 (nearest even), and ONLY as operands of the product.  The accumulators, the input
// projection xp added to them, both biases, the gate non-linearities, c, and the h written to `out` and `hn` are fp32.
//
// What differs from the fp32 kernel, and why:
//   * v_mfma_f32_32x32x16_bf16 consumes 16 of K per issue where v_mfma_f32_32x32x2_f32 consumes 2: a wave's quarter of K = 1024 is
//     16 issues instead of 128.  They go round-robin to kAcc = 2 INDEPENDENT accumulators that are added once at the end (a fixed
//     order), so no issue waits for the one before it.
//   * W_hh is read from an IMAGE made once per weight (sbk_rnn_whh_bf16_image): [D][ceil(H/8) slices][Hpad/16 chunks][64 lanes][8]
//     bf16, Hpad = H rounded up to 16, zeros past H (units and k).  The 8 bf16 of a lane's MFMA operand are one 16-byte load and
//     the 64 lanes of a wave read one contiguous KiB per chunk; there is no scalar tail path for any H.
//   * h_{t-1} is read from a bf16 SHADOW of the state in the caller's workspace, not from `out`: the cell update writes h twice
//     (fp32 to `out`, bf16 to the shadow), which halves the state bytes a workgroup reads and takes the conversion out of the
//     product's load path.  Two shadows ping-pong (a step's workgroups read one while they write the other).  The shadow is kept
//     in the OPERAND order of the product -- [2][D][ceil(B/32) tiles][Hpad/16 chunks][64 lanes][8], lane = row + 32 * (k / 8 % 2)
//     -- not as [B][Hpad] rows: a wave's load of a chunk is then one contiguous KiB as well, instead of 32 rows' 32-byte
//     pieces, and the 8 threads that own the 8 units of a slice for one utterance still write 16 contiguous bytes.  Rows past B
//     are padded in registers only (they load zeros and store nothing); an entry kernel writes bf16(h0) or zeros, and the zeros
//     of the padding, before the first step.
// No atomics, fixed summation order: the same bits on every run and every stream.
#include "act.h"
#include "common.h"
#include "device.h"

namespace {

constexpr int kJS = 8;        // hidden units of a workgroup's slice (x 4 gates = the 32 columns of an MFMA tile)
constexpr int kBT = 32;       // utterances of a batch tile (the 32 rows of an MFMA tile)
constexpr int kKC = 16;       // k of one MFMA (a chunk)
constexpr int kMaxH = 2048;   // as csrc/rnn.hip
constexpr int kAcc = 2;       // independent accumulator chains of a wave
constexpr size_t kChunkBytes = 64 * 8 * sizeof(unsigned short);  // one operand chunk of a wave: 1 KiB

struct RnnBf16Args {
  const float* xp;             // [B,T,D,4H]
  const unsigned short* whh;   // the image [D][S][C][64][8]
  const float* b_ih;           // [D,4H] or nullptr
  const float* b_hh;
  const float* h0;             // [D,B,H] or nullptr
  const float* c0;
  float* out;                  // [B,T,D*H]
  float* hn;                   // [D,B,H]
  float* cn;
  unsigned short* shadow;      // [2][D][BT][C][64][8]
  int B, T, H, D, step;
};

constexpr int chunks_of(int H) { return (H + kKC - 1) / kKC; }

// fp32 [D,4H,H] -> the image.  One thread per lane operand (8 bf16, 16 bytes).
__global__ void __launch_bounds__(256) rnn_whh_image_kernel(const float* w_hh, unsigned short* image, int H, int D) {
  const int S = (H + kJS - 1) / kJS, C = chunks_of(H);
  const long n = (long)D * S * C * 64;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int lane = (int)(i & 63);
  const long r = i >> 6;
  const int chunk = (int)(r % C), slice = (int)((r / C) % S), d = (int)(r / ((long)C * S));
  const int col = lane & 31, gate = col / kJS, unit = slice * kJS + col % kJS, k0 = chunk * kKC + 8 * (lane >> 5);
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    x[e] = (unit < H && k0 + e < H) ? w_hh[((size_t)d * 4 * H + (size_t)gate * H + unit) * H + k0 + e] : 0.0f;
  *reinterpret_cast<sbk::bf16x8*>(image + i * 8) = sbk::cvt_bf16x8(x);
}

// Both shadows before the first step: shadow 0 = bf16(h0) (zeros without h0), shadow 1 and every padding element = zeros.
__global__ void __launch_bounds__(256) rnn_shadow_init_kernel(const float* h0, unsigned short* shadow, int B, int H, int D) {
  const int C = chunks_of(H), BT = (B + kBT - 1) / kBT;
  const long half = (long)D * BT * C * 64, n = 2 * half;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0.0f;
  if (h0 != nullptr && i < half) {
    const int lane = (int)(i & 63);
    const long r = i >> 6;
    const int chunk = (int)(r % C), tile = (int)((r / C) % BT), d = (int)(r / ((long)C * BT));
    const int b = tile * kBT + (lane & 31), k0 = chunk * kKC + 8 * (lane >> 5);
    if (b < B) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k0 + e < H) x[e] = h0[((size_t)d * B + b) * H + k0 + e];
    }
  }
  *reinterpret_cast<sbk::bf16x8*>(shadow + i * 8) = sbk::cvt_bf16x8(x);
}

__global__ void __launch_bounds__(256) rnn_lstm_step_bf16_kernel(RnnBf16Args a) {
  __shared__ float part[4 * kBT * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int col = lane & 31, half = lane >> 5;
  const int d = blockIdx.y, slice = blockIdx.x, j0 = slice * kJS, tile = blockIdx.z, b0 = tile * kBT;
  const int H = a.H, s = a.step, t = d == 0 ? s : a.T - 1 - s;
  const int S = gridDim.x, BT = gridDim.z, C = chunks_of(H);
  const size_t shadow_elems = (size_t)a.D * BT * C * 64 * 8;  // one of the two shadows
  const unsigned short* hsrc = a.shadow + (size_t)(s & 1) * shadow_elems + ((size_t)d * BT + tile) * C * 64 * 8;
  unsigned short* hdst = a.shadow + (size_t)((s + 1) & 1) * shadow_elems + ((size_t)d * BT + tile) * C * 64 * 8;
  const unsigned short* wsrc = a.whh + ((size_t)d * S + slice) * C * 64 * 8;

  sbk::f32x16 acc[kAcc];
#pragma unroll
  for (int c = 0; c < kAcc; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.0f;
  if (s > 0 || a.h0 != nullptr) {  // (a zero state adds nothing)
    // wave w takes the w-th quarter of the chunks.  kUnroll chunks per trip: their 2 x kUnroll 16-byte loads are issued before
    // the first MFMA that needs one; chunk u of a trip goes to accumulator u % kAcc (kUnroll is a multiple of kAcc, so the
    // assignment is round-robin over the whole quarter).  Rows past B supply zeros without a load.
    constexpr int kUnroll = 8;
    static_assert(kUnroll % kAcc == 0, "round-robin over the accumulators");
    const int cq = sbk::uniform((C + 3) / 4);
    const int cend = min(C, (wave + 1) * cq);
    const bool row_ok = b0 + col < a.B;
    for (int c0 = wave * cq; c0 < cend; c0 += kUnroll) {
      sbk::bf16x8 hv[kUnroll], wv[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const bool in = c0 + u < cend;
        const size_t off = ((size_t)(c0 + u) * 64 + lane) * 8;
        wv[u] = in ? *reinterpret_cast<const sbk::bf16x8*>(wsrc + off) : sbk::bf16x8_from_words(0u, 0u, 0u, 0u);
        hv[u] = (in && row_ok) ? *reinterpret_cast<const sbk::bf16x8*>(hsrc + off) : sbk::bf16x8_from_words(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) acc[u % kAcc] = sbk::mfma_32x32x16_bf16(hv[u], wv[u], acc[u % kAcc]);
    }
  }
  float* mine = part + wave * (kBT * 33);
#pragma unroll
  for (int r = 0; r < 16; ++r) mine[((r & 3) + 8 * (r >> 2) + 4 * half) * 33 + col] = acc[0][r] + acc[1][r];
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
    const float c_prev = s == 0 ? (a.c0 != nullptr ? a.c0[si] : 0.0f) : a.cn[si];
    const float c_new = sbk::sigmoid(g4[1]) * c_prev + sbk::sigmoid(g4[0]) * tanhf(g4[2]);
    const float h_new = sbk::sigmoid(g4[3]) * tanhf(c_new);
    a.cn[si] = c_new;
    a.out[((size_t)b * a.T + t) * ((size_t)a.D * H) + (size_t)d * H + j] = h_new;
    if (s == a.T - 1) {
      a.hn[si] = h_new;
    } else {  // the next step's operand: chunk j / 16, lane = row + 32 * (j / 8 % 2), element j % 8 (= jj: j0 is a multiple of 8)
      hdst[((size_t)(j / kKC) * 64 + bl + 32 * ((j / 8) & 1)) * 8 + jj] = sbk::f32_to_bf16(h_new);
    }
  }
}

size_t image_bytes_of(int H, int D) { return (size_t)D * sbk::cdiv(H, kJS) * chunks_of(H) * kChunkBytes; }
size_t shadow_bytes_of(int B, int H, int D) { return 2 * (size_t)D * sbk::cdiv(B, kBT) * chunks_of(H) * kChunkBytes; }
bool shape_ok(int H, int D) { return H >= 1 && H <= kMaxH && (D == 1 || D == 2); }

}  // namespace

extern "C" size_t sbk_rnn_whh_bf16_image_bytes(int H, int D) { return shape_ok(H, D) ? image_bytes_of(H, D) : 0; }

extern "C" int sbk_rnn_whh_bf16_image(const float* w_hh, void* image, size_t image_bytes, int H, int D, sbk_stream_t stream) {
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "rnn_whh_bf16_image: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(D == 1 || D == 2, "rnn_whh_bf16_image: D=%d directions (D is 1 or 2)", D);
  SBK_REQUIRE(w_hh && image && sbk::aligned16(image), "rnn_whh_bf16_image: w_hh and a 16-byte aligned image are required");
  SBK_REQUIRE(image_bytes == image_bytes_of(H, D), "rnn_whh_bf16_image: image of %zu bytes, H=%d D=%d needs %zu", image_bytes, H,
              D, image_bytes_of(H, D));
  const long n = (long)(image_bytes / 16);
  SBK_LAUNCH(rnn_whh_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sbk::as_stream(stream), w_hh,
             static_cast<unsigned short*>(image), H, D);
  return sbk::launch_status("sbk_rnn_whh_bf16_image");
}

extern "C" size_t sbk_rnn_layer_bf16_workspace_bytes(int B, int H, int D) {
  return (shape_ok(H, D) && B >= 1 && B <= 65535 * kBT) ? shadow_bytes_of(B, H, D) : 0;
}

extern "C" int sbk_rnn_layer_bf16(const float* xp, const void* whh_image, size_t image_bytes, const float* b_ih,
                                  const float* b_hh, const float* h0, const float* c0, float* out, float* hn, float* cn,
                                  void* workspace, size_t workspace_bytes, int B, int T, int H, int D, int cell,
                                  sbk_stream_t stream) {
  SBK_REQUIRE(cell == SBK_RNN_LSTM, "rnn_layer_bf16: cell=%d is not implemented (SBK_RNN_LSTM = %d is)", cell, SBK_RNN_LSTM);
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "rnn_layer_bf16: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(D == 1 || D == 2, "rnn_layer_bf16: D=%d directions (D is 1 or 2)", D);
  SBK_REQUIRE(B >= 1 && B <= 65535 * kBT, "rnn_layer_bf16: B=%d is outside the limits 1 <= B <= %d", B, 65535 * kBT);
  SBK_REQUIRE(T >= 1, "rnn_layer_bf16: T=%d (T >= 1)", T);
  SBK_REQUIRE(xp && whh_image && out && hn && cn && workspace,
              "rnn_layer_bf16: null operand (xp, whh_image, out, hn, cn and workspace are required)");
  SBK_REQUIRE((b_ih == nullptr) == (b_hh == nullptr), "rnn_layer_bf16: b_ih and b_hh are given together or not at all");
  SBK_REQUIRE(h0 == nullptr || (h0 != hn && h0 != out), "rnn_layer_bf16: h0 must not alias hn or out");
  SBK_REQUIRE(image_bytes == image_bytes_of(H, D),
              "rnn_layer_bf16: W_hh image of %zu bytes was not made for H=%d D=%d (sbk_rnn_whh_bf16_image: %zu bytes)",
              image_bytes, H, D, image_bytes_of(H, D));
  SBK_REQUIRE(workspace_bytes >= shadow_bytes_of(B, H, D), "rnn_layer_bf16: workspace of %zu bytes is too small (%zu needed)",
              workspace_bytes, shadow_bytes_of(B, H, D));
  SBK_REQUIRE(sbk::aligned16(whh_image) && sbk::aligned16(workspace),
              "rnn_layer_bf16: whh_image and workspace must be 16-byte aligned");
  RnnBf16Args a;
  a.xp = xp; a.whh = static_cast<const unsigned short*>(whh_image); a.b_ih = b_ih; a.b_hh = b_hh; a.h0 = h0; a.c0 = c0;
  a.out = out; a.hn = hn; a.cn = cn; a.shadow = static_cast<unsigned short*>(workspace);
  a.B = B; a.T = T; a.H = H; a.D = D;
  const hipStream_t st = sbk::as_stream(stream);
  const dim3 grid(sbk::cdiv(H, kJS), D, sbk::cdiv(B, kBT));
  const double tiles = (double)grid.x * D * grid.z, Hp = (double)chunks_of(H) * kKC;
  sbk::ProfScope prof("rnn_lstm_steps_bf16", (double)T * (2.0 * kBT * 32.0 * H * tiles + 30.0 * B * H * D),
                      (double)T * (2.0 * (32.0 + kBT) * Hp * tiles + (4.0 * 6.0 + 2.0) * B * H * D), st);
  const long n = (long)(shadow_bytes_of(B, H, D) / 16);
  SBK_LAUNCH(rnn_shadow_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h0, a.shadow, B, H, D);
  for (int s = 0; s < T; ++s) {
    a.step = s;
    SBK_LAUNCH(rnn_lstm_step_bf16_kernel, grid, dim3(256), 0, st, a);
  }
  return sbk::launch_status("sbk_rnn_layer_bf16");
}
