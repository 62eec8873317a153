// The SLi-GRU layer of csrc/sligru.hip with its recurrent product h_{t-1} . u^T on the bf16 matrix pipe (sbk_sligru_layer_bf16):
// the opt-in precision "bf16" of a CRDNN encoder with rnn_class SLiGRU.  Same semantics (gates = xp_t + LayerNorm_2H(h_{t-1} . u^T),
// a, z = gates.chunk(2), h_t = sigmoid(z) h_{t-1} + (1 - sigmoid(z)) act(a); direction 1 scans t = T-1 .. 0 and writes at its own
// frame; `out` is the history, h0 optional, hn returned) and the same two launches per step, because the LayerNorm still spans all
// 2H columns of the product.
//
// What is rounded: u and h_{t-1}, to bf16 (nearest even), and ONLY as operands of their product.  The accumulators, the raw
// product, the LayerNorm statistics and affine, xp, the cell -- its sigmoid(z) h_{t-1} term reads the fp32 h_{t-1} -- and the h
// written to `out` and `hn` are fp32.
//
// Product launch (sligru_product_bf16_kernel): a workgroup owns 8 hidden units x 2 gates -- the 16 columns of a
// v_mfma_f32_16x16x32_bf16 tile -- and 32 of the D*B rows (direction-major): two 16-row tiles that share the u operand and have
// accumulators of their own.  ceil(H/8) x ceil(D*B/32) workgroups, 256 at H 1024, D 2, B 32 as in the fp32 kernel (the 32x32x16
// instruction with 16 units per workgroup would give 128).  One issue consumes 32 of K where v_mfma_f32_16x16x4_f32 consumes 4: a
// wave's quarter of K = 1024 is 8 chunks, 16 issues instead of 256.
//   * u is read from an IMAGE made once per weight (sbk_sligru_u_bf16_image): [ceil(H/8) slices][ceil(H/32) chunks][64 lanes][8]
//     bf16, lane l holding the 8 consecutive k of column l & 15 = gate * 8 + unit and k block l >> 4, zeros past H (units and k).
//     A lane's operand is one 16-byte load, a wave's chunk one contiguous KiB, and any H runs one loop with no scalar tail.
//   * h_{t-1} is read from a bf16 SHADOW of the state in the workspace, not from `out`: two shadows ping-pong, each kept in the
//     operand order of the product, [ceil(D*B/16) row tiles][ceil(H/32) chunks][64 lanes][8] with lane = row % 16 + 16 * (k / 8 % 4),
//     so a wave's chunk of the state is one contiguous KiB too.  Rows past D*B load zeros without a load and store nothing; an
//     entry kernel writes bf16(h0) or zeros, and the zeros of the padding, before the first step.
//   * the four waves take contiguous quarters of the chunks, the loads of up to 8 chunks (3 x 16 bytes per lane and chunk) are
//     issued before the first MFMA that needs one, the partial tiles meet in LDS and are added in wave order.
//
// Norm-and-cell launch (sligru_cell_bf16_kernel): one workgroup per row, with a mapping of its own: thread tid holds the a and z
// values of the 8 CONSECUTIVE units 8 tid .. 8 tid + 7 (256 threads cover H <= 2048), so raw, xp, h_{t-1}, the affine and `out`
// move as 16-byte accesses where H is a multiple of 4, and the 8 bf16 of h_t that the next step's product reads are ONE 16-byte
// store into the other shadow (none on the last step).  Statistics as in the fp32 kernel: the mean, then the centred squares, a
// fixed butterfly inside a wave and the waves added in order.
// No atomics, fixed summation order: the same bits on every run and every stream.
#include "act.h"
#include "common.h"
#include "device.h"
#include "kernel_util.h"

namespace {

constexpr int kJS = 8;        // hidden units of a workgroup's slice (x 2 gates = the 16 columns of an MFMA tile)
constexpr int kRT = 32;       // rows of a workgroup: two 16-row MFMA tiles
constexpr int kKC = 32;       // k of one MFMA (a chunk)
constexpr int kMaxH = 2048;   // as csrc/sligru.hip
constexpr int kPer = 8;       // consecutive units of a thread in the norm-and-cell pass (256 threads x 8 = kMaxH)
constexpr float kEps = 1e-5f; // torch.nn.LayerNorm's default, the reference's
constexpr size_t kChunkElems = 64 * 8;                                 // one operand chunk of a wave: 1 KiB of bf16
constexpr size_t kChunkBytes = kChunkElems * sizeof(unsigned short);

struct SligruBf16Args {
  const float* xp;             // [B,T,2H]
  const unsigned short* u;     // the image [S][C][64][8]
  const float* gamma;          // [2H] or nullptr
  const float* beta;
  const float* h0;             // [D,B,H] or nullptr
  float* out;                  // [B,T,D*H]
  float* hn;                   // [D,B,H]
  float* raw;                  // workspace: [D*B,2H]
  unsigned short* shadow;      // workspace: [2][RT][C][64][8]
  int B, T, H, D, act, step;
  int vec;                     // every fp32 row of the cell pass is 16-byte aligned (H % 4 == 0 and aligned operands)
};

constexpr int chunks_of(int H) { return (H + kKC - 1) / kKC; }
constexpr int row_tiles_of(int R) { return (R + 15) / 16; }

// fp32 [2H,H] -> the image.  One thread per lane operand (8 bf16, 16 bytes).
__global__ void __launch_bounds__(256) sligru_u_image_kernel(const float* u, unsigned short* image, int H) {
  const int C = chunks_of(H);
  const long n = (long)((H + kJS - 1) / kJS) * C * 64;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int lane = (int)(i & 63);
  const long r = i >> 6;
  const int chunk = (int)(r % C), slice = (int)(r / C);
  const int col = lane & 15, gate = col / kJS, unit = slice * kJS + col % kJS, k0 = chunk * kKC + 8 * (lane >> 4);
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = (unit < H && k0 + e < H) ? u[((size_t)gate * H + unit) * H + k0 + e] : 0.0f;
  *reinterpret_cast<sbk::bf16x8*>(image + i * 8) = sbk::cvt_bf16x8(x);
}

// Both shadows before the first step: shadow 0 = bf16(h0) (zeros without h0), shadow 1 and every padding element = zeros.
__global__ void __launch_bounds__(256) sligru_shadow_init_kernel(const float* h0, unsigned short* shadow, int R, int H) {
  const int C = chunks_of(H);
  const long half = (long)row_tiles_of(R) * C * 64, n = 2 * half;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0.0f;
  if (h0 != nullptr && i < half) {
    const int lane = (int)(i & 63);
    const long r = i >> 6;
    const int chunk = (int)(r % C);
    const long row = (r / C) * 16 + (lane & 15);
    const int k0 = chunk * kKC + 8 * (lane >> 4);
    if (row < R) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (k0 + e < H) x[e] = h0[(size_t)row * H + k0 + e];
    }
  }
  *reinterpret_cast<sbk::bf16x8*>(shadow + i * 8) = sbk::cvt_bf16x8(x);
}

__global__ void __launch_bounds__(256) sligru_product_bf16_kernel(SligruBf16Args a) {
  __shared__ float part[4 * kRT * 17];
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int col = lane & 15, kg = lane >> 4;
  const int H = a.H, R = a.D * a.B, C = chunks_of(H);
  const int slice = blockIdx.x, j0 = slice * kJS, r0 = blockIdx.y * kRT;
  // this workgroup's operands: its slice of the image, and row tiles 2 y and 2 y + 1 of the shadow the last step wrote
  const unsigned short* usrc = a.u + (size_t)slice * C * kChunkElems;
  const unsigned short* hsrc0 = a.shadow + ((size_t)(a.step & 1) * row_tiles_of(R) + 2 * (size_t)blockIdx.y) * C * kChunkElems;
  const unsigned short* hsrc1 = hsrc0 + (size_t)C * kChunkElems;  // (past the shadow when R has no such tile: never loaded then)
  const bool row_ok0 = r0 + col < R, row_ok1 = r0 + 16 + col < R;
  sbk::f32x4 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc0[r] = acc1[r] = 0.0f;
  // wave w takes the w-th quarter of the chunks.  kUnroll chunks per trip: their 3 x kUnroll 16-byte loads are issued before the
  // first MFMA that needs one (a step is bound by the latency of its operands, not by its 16 issues); chunks past the quarter and
  // rows past D*B supply zeros without a load
  constexpr int kUnroll = 8;
  const int cq = sbk::uniform((C + 3) / 4);
  const int cend = min(C, (wave + 1) * cq);
  const sbk::bf16x8 zero = sbk::bf16x8_from_words(0u, 0u, 0u, 0u);
  for (int c0 = wave * cq; c0 < cend; c0 += kUnroll) {
    sbk::bf16x8 uv[kUnroll], h0v[kUnroll], h1v[kUnroll];
#pragma unroll
    for (int c = 0; c < kUnroll; ++c) {
      const bool in = c0 + c < cend;
      const size_t off = ((size_t)(c0 + c) * 64 + lane) * 8;
      uv[c] = in ? *reinterpret_cast<const sbk::bf16x8*>(usrc + off) : zero;
      h0v[c] = (in && row_ok0) ? *reinterpret_cast<const sbk::bf16x8*>(hsrc0 + off) : zero;
      h1v[c] = (in && row_ok1) ? *reinterpret_cast<const sbk::bf16x8*>(hsrc1 + off) : zero;
    }
#pragma unroll
    for (int c = 0; c < kUnroll; ++c) {
      acc0 = sbk::mfma_16x16x32_bf16(h0v[c], uv[c], acc0);
      acc1 = sbk::mfma_16x16x32_bf16(h1v[c], uv[c], acc1);
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

// v[0..8) = p[0..left) then zeros (left <= 0: nothing is read, p may be null): two 16-byte loads where the rows are 16-byte
// aligned (vec: left is then a multiple of 4), scalar loads otherwise
__device__ __forceinline__ void load_units(float (&v)[kPer], const float* p, int left, bool vec) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < kPer / 4; ++q) {
      const float4 x = 4 * q < left ? *reinterpret_cast<const float4*>(p + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e) v[e] = e < left ? p[e] : 0.0f;
  }
}
__device__ __forceinline__ void store_units(float* p, const float (&v)[kPer], int left, bool vec) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < kPer / 4; ++q)
      if (4 * q < left) *reinterpret_cast<float4*>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int e = 0; e < kPer; ++e)
      if (e < left) p[e] = v[e];
  }
}

// the cell's activation over a thread's units: one uniform switch outside the unrolled loop
__device__ __forceinline__ void cell_act_units(float (&v)[kPer], int kind) {
  switch (kind) {  // uniform
    case SBK_SLIGRU_TANH:
#pragma unroll
      for (int e = 0; e < kPer; ++e) v[e] = tanhf(v[e]);
      break;
    case SBK_SLIGRU_SIN:
#pragma unroll
      for (int e = 0; e < kPer; ++e) v[e] = sinf(v[e]);
      break;
    case SBK_SLIGRU_LEAKY_RELU:
#pragma unroll
      for (int e = 0; e < kPer; ++e) v[e] = sbk::leaky_relu(v[e]);
      break;
    default:
#pragma unroll
      for (int e = 0; e < kPer; ++e) v[e] = sbk::relu_keep_nan(v[e]);  // torch.relu's rule
      break;
  }
}

// raw_zero: the first step of a layer without h0 -- the product of a zero state was not launched
__global__ void __launch_bounds__(256) sligru_cell_bf16_kernel(SligruBf16Args a, int raw_zero) {
  __shared__ float red[4];
  const int tid = threadIdx.x, r = blockIdx.x, H = a.H, R = a.D * a.B;
  const int d = r / a.B, b = r % a.B;
  const int t = d == 0 ? a.step : a.T - 1 - a.step;
  const int j = kPer * tid, left = H - j;  // this thread's units j .. j + 7, `left` of them exist (<= 0: none)
  const bool vec = a.vec != 0;
  const float* raw = a.raw + (size_t)r * 2 * H + j;
  float va[kPer], vz[kPer];
  load_units(va, raw, raw_zero ? 0 : left, vec);
  load_units(vz, raw + H, raw_zero ? 0 : left, vec);
  float s = 0.0f;
#pragma unroll
  for (int e = 0; e < kPer; ++e) s += va[e] + vz[e];
  const float n = 2.0f * (float)H;
  const float mean = sbk::block_sum(s, red) / n;
  float q = 0.0f;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    if (e < left) {
      const float ca = va[e] - mean, cz = vz[e] - mean;
      q += ca * ca + cz * cz;
    }
  }
  const float rstd = 1.0f / sqrtf(sbk::block_sum(q, red) / n + kEps);
  if (left <= 0) return;  // (behind the last barrier)
  // h_{t-1} in fp32: the previous frame of the same direction in `out`, h0 at the first step
  const float* hprev;
  if (a.step == 0) {
    hprev = a.h0 != nullptr ? a.h0 + (size_t)r * H + j : nullptr;
  } else {
    const int tp = d == 0 ? a.step - 1 : a.T - a.step;
    hprev = a.out + ((size_t)b * a.T + tp) * ((size_t)a.D * H) + (size_t)d * H + j;
  }
  const float* xrow = a.xp + ((size_t)b * a.T + t) * 2 * H + j;
  float xa[kPer], xz[kPer], hp[kPer];
  load_units(xa, xrow, left, vec);
  load_units(xz, xrow + H, left, vec);
  load_units(hp, hprev, hprev != nullptr ? left : 0, vec);
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    va[e] = (va[e] - mean) * rstd;
    vz[e] = (vz[e] - mean) * rstd;
  }
  if (a.gamma != nullptr) {
    float ga[kPer], gz[kPer], ba[kPer], bz[kPer];
    load_units(ga, a.gamma + j, left, vec);
    load_units(gz, a.gamma + H + j, left, vec);
    load_units(ba, a.beta + j, left, vec);
    load_units(bz, a.beta + H + j, left, vec);
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      va[e] = va[e] * ga[e] + ba[e];
      vz[e] = vz[e] * gz[e] + bz[e];
    }
  }
#pragma unroll
  for (int e = 0; e < kPer; ++e) va[e] += xa[e];
  cell_act_units(va, a.act);
  float h[kPer];
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    const float z = sbk::sigmoid(xz[e] + vz[e]);
    h[e] = e < left ? z * hp[e] + (1.0f - z) * va[e] : 0.0f;  // (zeros past H: what the shadow holds there)
  }
  store_units(a.out + ((size_t)b * a.T + t) * ((size_t)a.D * H) + (size_t)d * H + j, h, left, vec);
  if (a.step == a.T - 1) {
    store_units(a.hn + (size_t)r * H + j, h, left, vec);
  } else {  // the next step's operand: row tile r / 16, chunk j / 32, lane = r % 16 + 16 * (j / 8 % 4), all 8 elements
    unsigned short* hdst = a.shadow + (size_t)((a.step + 1) & 1) * row_tiles_of(R) * chunks_of(H) * kChunkElems;
    const size_t lane_op = ((size_t)(r / 16) * chunks_of(H) + tid / 4) * 64 + (r % 16) + 16 * (tid % 4);
    *reinterpret_cast<sbk::bf16x8*>(hdst + lane_op * 8) = sbk::cvt_bf16x8(h);
  }
}

size_t image_bytes_of(int H) { return (size_t)sbk::cdiv(H, kJS) * chunks_of(H) * kChunkBytes; }
size_t raw_bytes_of(int B, int H, int D) { return (((size_t)D * B * 2 * H * sizeof(float)) + 15) & ~(size_t)15; }
size_t shadow_bytes_of(int B, int H, int D) { return 2 * (size_t)row_tiles_of(D * B) * chunks_of(H) * kChunkBytes; }
bool shape_ok(int B, int H, int D) { return H >= 1 && H <= kMaxH && (D == 1 || D == 2) && B >= 1 && B <= 65535 * kRT / 2; }

}  // namespace

extern "C" size_t sbk_sligru_u_bf16_image_bytes(int H) { return (H >= 1 && H <= kMaxH) ? image_bytes_of(H) : 0; }

extern "C" int sbk_sligru_u_bf16_image(const float* u, void* image, size_t image_bytes, int H, sbk_stream_t stream) {
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "sligru_u_bf16_image: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(u && image && sbk::aligned16(image), "sligru_u_bf16_image: u and a 16-byte aligned image are required");
  SBK_REQUIRE(image_bytes == image_bytes_of(H), "sligru_u_bf16_image: image of %zu bytes, H=%d needs %zu", image_bytes, H,
              image_bytes_of(H));
  const hipStream_t st = sbk::as_stream(stream);
  const long n = (long)(image_bytes / 16);
  sbk::ProfScope prof("sligru_u_image", 0.0, 4.0 * 2.0 * H * H + (double)image_bytes, st);
  SBK_LAUNCH(sligru_u_image_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, u, static_cast<unsigned short*>(image), H);
  return sbk::launch_status("sbk_sligru_u_bf16_image");
}

extern "C" size_t sbk_sligru_layer_bf16_workspace_bytes(int B, int H, int D) {
  return shape_ok(B, H, D) ? raw_bytes_of(B, H, D) + shadow_bytes_of(B, H, D) : 0;
}

extern "C" int sbk_sligru_layer_bf16(const float* xp, const void* u_image, size_t image_bytes, const float* ln_gamma,
                                     const float* ln_beta, const float* h0, float* out, float* hn, void* workspace,
                                     size_t workspace_bytes, int B, int T, int H, int D, int act, sbk_stream_t stream) {
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "sligru_layer_bf16: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(D == 1 || D == 2, "sligru_layer_bf16: D=%d directions (D is 1 or 2)", D);
  SBK_REQUIRE(B >= 1 && B <= 65535 * kRT / 2, "sligru_layer_bf16: B=%d is outside the limits 1 <= B <= %d", B, 65535 * kRT / 2);
  SBK_REQUIRE(T >= 1, "sligru_layer_bf16: T=%d (T >= 1)", T);
  SBK_REQUIRE(act >= SBK_SLIGRU_RELU && act <= SBK_SLIGRU_LEAKY_RELU,
              "sligru_layer_bf16: act=%d (SBK_SLIGRU_RELU, _TANH, _SIN and _LEAKY_RELU are implemented)", act);
  SBK_REQUIRE(xp && u_image && out && hn && workspace,
              "sligru_layer_bf16: null operand (xp, u_image, out, hn and workspace are required)");
  SBK_REQUIRE((ln_gamma == nullptr) == (ln_beta == nullptr),
              "sligru_layer_bf16: ln_gamma and ln_beta are given together or not at all");
  SBK_REQUIRE(h0 == nullptr || (h0 != hn && h0 != out), "sligru_layer_bf16: h0 must not alias hn or out");
  SBK_REQUIRE(image_bytes == image_bytes_of(H),
              "sligru_layer_bf16: u image of %zu bytes was not made for H=%d (sbk_sligru_u_bf16_image: %zu bytes)", image_bytes, H,
              image_bytes_of(H));
  const size_t need = raw_bytes_of(B, H, D) + shadow_bytes_of(B, H, D);
  SBK_REQUIRE(workspace_bytes >= need, "sligru_layer_bf16: workspace of %zu bytes is too small (%zu needed)", workspace_bytes, need);
  SBK_REQUIRE(sbk::aligned16(u_image) && sbk::aligned16(workspace),
              "sligru_layer_bf16: u_image and workspace must be 16-byte aligned");
  SligruBf16Args a;
  a.xp = xp; a.u = static_cast<const unsigned short*>(u_image); a.gamma = ln_gamma; a.beta = ln_beta; a.h0 = h0; a.out = out;
  a.hn = hn; a.raw = static_cast<float*>(workspace);
  a.shadow = reinterpret_cast<unsigned short*>(static_cast<char*>(workspace) + raw_bytes_of(B, H, D));
  a.B = B; a.T = T; a.H = H; a.D = D; a.act = act;
  a.vec = (H & 3) == 0 && sbk::aligned16(xp) && sbk::aligned16(out) && sbk::aligned16(hn) && sbk::aligned16(h0) &&
          sbk::aligned16(ln_gamma) && sbk::aligned16(ln_beta);
  const hipStream_t st = sbk::as_stream(stream);
  const int R = D * B;
  const dim3 grid(sbk::cdiv(H, kJS), sbk::cdiv(R, kRT));
  const double tiles = (double)grid.x * grid.y, Hp = (double)chunks_of(H) * kKC;
  // (the entry kernel is one small launch per layer, outside the per-step tags)
  const long n = (long)(shadow_bytes_of(B, H, D) / 16);
  SBK_LAUNCH(sligru_shadow_init_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h0, a.shadow, R, H);
  for (int s = 0; s < T; ++s) {
    a.step = s;
    const int raw_zero = s == 0 && h0 == nullptr;
    if (!raw_zero) {
      sbk::ProfScope prof("sligru_product_bf16", 2.0 * kRT * 16.0 * H * tiles, 2.0 * (16.0 + kRT) * Hp * tiles + 4.0 * 2.0 * R * H, st);
      SBK_LAUNCH(sligru_product_bf16_kernel, grid, dim3(256), 0, st, a);
    }
    sbk::ProfScope prof("sligru_norm_cell_bf16", 24.0 * R * H, (4.0 * 6.0 + 2.0) * R * H, st);
    SBK_LAUNCH(sligru_cell_bf16_kernel, dim3(R), dim3(256), 0, st, a, raw_zero);
  }
  return sbk::launch_status("sbk_sligru_layer_bf16");
}
