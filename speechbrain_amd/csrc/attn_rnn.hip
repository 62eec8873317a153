// The GRU attention decoder of the CRDNN seq2seq recipes: one decode step of AttentionalRNNDecoder (nnet/RNN.py:932-967) with
// LocationAwareAttention / ContentBasedAttention (nnet/attention.py:203-251 / :80-117) and the GRU cell stack (nnet/RNN.py:576-648),
// teacher-forced decoding (nnet/RNN.py:969-1013) and S2SRNNGreedySearcher (decoders/seq2seq.py:176-327, :638-708).
//
// The attention of a step is two launches for all n hypothesis rows:
//   attn_energy_kernel       grid (ceil(T/32), n): a workgroup owns 32 frames of one row.  It stages conv_loc's taps and the window of
//                            the previous attention it needs in LDS, forms the location feature loc[c, t] of its frames there, and each
//                            of its four waves reduces eight frames' v . tanh(enc_h + dec_h + mlp_loc(loc)) over A, lanes along A (the
//                            rows of enc_h are read as whole lines).  Frames past the utterance's length are not computed.  Only the
//                            energies [n, T] leave the kernel: nothing of size n*T*A is written.
//   attn_softmax_ctx_kernel  grid (ceil(E/64), n): every workgroup of a row forms the same softmax over the row's energies in LDS (the
//                            same bits: one summation order) and contracts it with 64 columns of enc, waves along T, lanes along E; the
//                            workgroup of the first columns also writes the attention.
// Every sum has a fixed order: two runs give the same bits.  enc_len and row_utt are clamped where they index (no caller-supplied
// length reaches an address unclamped); the C entries also check them on the device and refuse values outside their range.
//
// A decode step strings these together with the routed contractions (sbk::gemm_nt_ws) and three small kernels (row gather, GRU cell
// update, arg-max with its log-softmax value).  The step's operands sit side by side in one row buffer [emb | c | cell_out], so that
// the cell input [emb | c] and the projection input [c | cell_out] are both windows of it and no concatenation is ever copied.
#include <limits.h>

#include "act.h"
#include "argmax.h"
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

constexpr int kFR = 8;         // frames of a wave in attn_energy_kernel
constexpr int kTT = 4 * kFR;   // frames of a workgroup
constexpr int kMaxA = 2048, kMaxE = 2048, kMaxT = 4096, kMaxC = 32, kMaxK = 128, kMaxH = 2048;
constexpr int kMaxRows = 65535;  // rows are a grid dimension

struct AttendArgs {
  const float* enc;        // [B,T,E]
  const float* enc_h;      // [B,T,A]
  const int32_t* enc_len;  // [B]
  const int32_t* row_utt;  // [n] or nullptr (identity)
  const float* dec_h;      // [n,A]
  const float* prev;       // [n,T], row stride ld_prev (unused when C == 0)
  const float* conv_w;     // [C,2k+1]
  const float* loc_w;      // [A,C]
  const float* loc_b;      // [A]
  const float* v;          // [A]
  float* energy;           // [n,T] scratch
  float* attn;             // [n,T], row stride ld_attn
  float* ctx;              // [n,E]
  long ld_prev, ld_attn;
  int n, B, T, A, E, C, k;
  float scaling;
};

__device__ __forceinline__ int utt_of(const int32_t* row_utt, int r, int B) {
  const int u = row_utt != nullptr ? row_utt[r] : r;
  return min(max(u, 0), B - 1);
}
__device__ __forceinline__ int len_of(const int32_t* enc_len, int u, int T) { return min(max(enc_len[u], 1), T); }

// Max over a workgroup of 256 threads through red[4], in every thread.
__device__ __forceinline__ float block_max(float v, float* red) {
  v = sbk::wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// flag = max(flag, 1) for an enc_len outside [1, T], max(flag, 2) for a row_utt outside [0, B)
__global__ void __launch_bounds__(256) attn_validate_kernel(const int32_t* enc_len, const int32_t* row_utt, int B, int n, int T,
                                                            int* flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B && (enc_len[i] < 1 || enc_len[i] > T)) atomicMax(flag, 1);
  if (row_utt != nullptr && i < n && (row_utt[i] < 0 || row_utt[i] >= B)) atomicMax(flag, 2);
}

// the first prev_attn (attention.py:226): 1 / enc_len on the valid frames, 0 behind them
__global__ void __launch_bounds__(256) attn_init_kernel(const int32_t* enc_len, const int32_t* row_utt, float* attn, long ld, int B,
                                                        int T) {
  const int r = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  const int len = len_of(enc_len, utt_of(row_utt, r, B), T);
  attn[(size_t)r * ld + t] = t < len ? 1.0f / (float)len : 0.0f;
}

__global__ void __launch_bounds__(256) attn_energy_kernel(AttendArgs a) {
  __shared__ float w_s[kMaxC * (2 * kMaxK + 1)];
  __shared__ float p_s[kTT + 2 * kMaxK];
  __shared__ float loc_s[kMaxC * kTT];
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int r = blockIdx.y, t0 = blockIdx.x * kTT;
  const int u = utt_of(a.row_utt, r, a.B), len = len_of(a.enc_len, u, a.T);
  if (t0 >= len) return;  // (the whole workgroup: masked frames have no energy)
  const int C = a.C, A = a.A, T = a.T;
  if (C > 0) {
    // loc[c, t] = sum_j w[c, j] * prev[t + j - k], zeros outside [0, T): a cross-correlation (torch's Conv1d)
    const int taps = 2 * a.k + 1;
    for (int i = tid; i < C * taps; i += 256) w_s[i] = a.conv_w[i];
    const float* prev = a.prev + (size_t)r * a.ld_prev;
    for (int i = tid; i < kTT + 2 * a.k; i += 256) {
      const int t = t0 - a.k + i;
      p_s[i] = (t >= 0 && t < T) ? prev[t] : 0.0f;
    }
    __syncthreads();
    for (int o = tid; o < C * kTT; o += 256) {
      const int c = o / kTT, tl = o % kTT;
      const float* w = w_s + c * taps;
      float acc = 0.0f;
      for (int j = 0; j < taps; ++j) acc = fmaf(w[j], p_s[tl + j], acc);
      loc_s[o] = acc;
    }
    __syncthreads();
  }
  const int tw = t0 + wave * kFR;  // this wave's first frame
  if (tw >= len) return;           // (the whole wave; no barrier follows)
  const float* eh = a.enc_h + (size_t)u * T * A;
  const float* dh = a.dec_h + (size_t)r * A;
  const float* loc = loc_s + wave * kFR;
  float acc[kFR];
#pragma unroll
  for (int f = 0; f < kFR; ++f) acc[f] = 0.0f;
  for (int j = lane; j < A; j += 64) {
    const float base = C > 0 ? dh[j] + a.loc_b[j] : dh[j];
    float s[kFR];
#pragma unroll
    for (int f = 0; f < kFR; ++f) s[f] = tw + f < len ? eh[(size_t)(tw + f) * A + j] + base : 0.0f;
    for (int c = 0; c < C; ++c) {
      const float w = a.loc_w[(size_t)j * C + c];
#pragma unroll
      for (int f = 0; f < kFR; ++f) s[f] = fmaf(w, loc[c * kTT + f], s[f]);
    }
    const float vj = a.v[j];
#pragma unroll
    for (int f = 0; f < kFR; ++f) acc[f] = fmaf(vj, tanhf(s[f]), acc[f]);
  }
#pragma unroll
  for (int f = 0; f < kFR; ++f) acc[f] = sbk::wave_sum(acc[f]);
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < kFR; ++f)
      if (tw + f < len) a.energy[(size_t)r * T + tw + f] = acc[f];
  }
}

__global__ void __launch_bounds__(256) attn_softmax_ctx_kernel(AttendArgs a) {
  __shared__ float p_s[kMaxT];
  __shared__ float red[4];
  __shared__ float part[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = sbk::uniform(tid >> 6);
  const int r = blockIdx.y, T = a.T, E = a.E;
  const int u = utt_of(a.row_utt, r, a.B), len = len_of(a.enc_len, u, T);
  const float* e = a.energy + (size_t)r * T;
  // softmax(scaling * e) over the valid frames (masked frames hold -inf in the reference: exactly 0 here)
  float m = -INFINITY;
  for (int t = tid; t < len; t += 256) {
    const float x = a.scaling * e[t];
    p_s[t] = x;
    m = fmaxf(m, x);
  }
  m = block_max(m, red);
  float s = 0.0f;
  for (int t = tid; t < len; t += 256) {
    const float p = expf(p_s[t] - m);
    p_s[t] = p;
    s += p;
  }
  s = sbk::block_sum(s, red);
  for (int t = tid; t < T; t += 256) {
    const float p = t < len ? p_s[t] / s : 0.0f;
    if (t < len) p_s[t] = p;
    if (blockIdx.x == 0) a.attn[(size_t)r * a.ld_attn + t] = p;
  }
  __syncthreads();
  // ctx[col] = sum_t attn[t] * enc[u, t, col]: wave w takes t = w, w + 4, ...; the four partial sums meet in a fixed order
  const int col = blockIdx.x * 64 + lane;
  const float* en = a.enc + (size_t)u * T * E;
  float acc = 0.0f;
  if (col < E) {
#pragma unroll 4
    for (int t = wave; t < len; t += 4) acc = fmaf(p_s[t], en[(size_t)t * E + col], acc);
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && col < E) a.ctx[(size_t)r * E + col] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
}

struct GruArgs {
  const float* gi;      // [n,3H]
  const float* gh;      // [n,3H]
  const float* b_ih;    // [3H] or nullptr
  const float* b_hh;
  const float* h_prev;  // [n,H], row stride ld_hp, or nullptr (zeros)
  float* h_out;         // [n,H], row stride ld_ho
  long ld_hp, ld_ho;
  int n, H;
};

// torch.nn.GRUCell: gate order r, z, n; n = tanh(gi_n + b_in + r * (gh_n + b_hn)); h' = (1 - z) * n + z * h
__global__ void __launch_bounds__(256) gru_cell_kernel(GruArgs a) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.n * a.H) return;
  const int r = (int)(idx / a.H), j = (int)(idx % a.H), H = a.H;
  const float* gi = a.gi + (size_t)r * 3 * H;
  const float* gh = a.gh + (size_t)r * 3 * H;
  float ir = gi[j], iz = gi[H + j], in = gi[2 * H + j];
  float hr = gh[j], hz = gh[H + j], hn = gh[2 * H + j];
  if (a.b_ih != nullptr) {
    ir += a.b_ih[j]; iz += a.b_ih[H + j]; in += a.b_ih[2 * H + j];
    hr += a.b_hh[j]; hz += a.b_hh[H + j]; hn += a.b_hh[2 * H + j];
  }
  const float rg = sbk::sigmoid(ir + hr), z = sbk::sigmoid(iz + hz);
  const float ng = tanhf(in + rg * hn);
  const float h = a.h_prev != nullptr ? a.h_prev[(size_t)r * a.ld_hp + j] : 0.0f;
  a.h_out[(size_t)r * a.ld_ho + j] = (1.0f - z) * ng + z * h;
}

// dst[r, 0..width) = src[idx ? idx[r] (clamped to the table) : r, 0..width): the embedding gather and the strided row copies
__global__ void __launch_bounds__(256) gather_rows_kernel(const float* src, const int32_t* idx, long src_stride, int n_src, float* dst,
                                                          long dst_stride, int width) {
  const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= width) return;
  const int s = idx != nullptr ? min(max(idx[r], 0), n_src - 1) : r;
  dst[(size_t)r * dst_stride + c] = src[(size_t)s * src_stride + c];
}

__global__ void __launch_bounds__(256) fill_i32_kernel(int32_t* out, long n, int value) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = value;
}

__global__ void __launch_bounds__(256) greedy_init_kernel(int32_t* tok, int32_t* ended, int32_t* n_ended, int B, int bos) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) {
    tok[i] = bos;
    ended[i] = 0;
  }
  if (i == 0) *n_ended = 0;
}

// One row of logits: the arg-max as torch.argmax picks it (the first of equal maxima, NaN above everything) and the log-softmax
// value there; then S2SGreedySearcher's bookkeeping (seq2seq.py:252-264): a row that has emitted eos -- at this step or before --
// records (eos, 0) and feeds eos on.
__global__ void __launch_bounds__(256) greedy_select_kernel(const float* logits, int V, int eos, int step, int L, int32_t* tok,
                                                            int32_t* ended, int32_t* n_ended, int32_t* out_tok, float* out_sc) {
  __shared__ float red[4];
  __shared__ float wv[4];
  __shared__ int wi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  const float* x = logits + (size_t)r * V;
  float bv = -INFINITY;
  int bi = INT_MAX;
  for (int i = tid; i < V; i += 256) {
    const float v = x[i];
    if (bi == INT_MAX || sbk::arg_better(v, i, bv, bi)) {
      bv = v;
      bi = i;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const float ov = sbk::shfl_xor(bv, m);
    const int oi = sbk::shfl_xor(bi, m);
    if (oi != INT_MAX && (bi == INT_MAX || sbk::arg_better(ov, oi, bv, bi))) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    wv[wave] = bv;
    wi[wave] = bi;
  }
  __syncthreads();
  bv = wv[0];
  bi = wi[0];
  for (int w = 1; w < 4; ++w)
    if (wi[w] != INT_MAX && sbk::arg_better(wv[w], wi[w], bv, bi)) {
      bv = wv[w];
      bi = wi[w];
    }
  float s = 0.0f;
  for (int i = tid; i < V; i += 256) s += expf(x[i] - bv);
  s = sbk::block_sum(s, red);
  if (tid == 0) {
    const int was = ended[r];
    const bool end = was != 0 || bi == eos;
    out_tok[(size_t)r * L + step] = end ? eos : bi;
    out_sc[(size_t)r * L + step] = end ? 0.0f : -logf(s);  // log_softmax at the maximum: (x - max) - log(sum) with x = max
    tok[r] = end ? eos : bi;
    if (!was && end) {
      ended[r] = 1;
      atomicAdd(n_ended, 1);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- launchers
int launch_attend(const AttendArgs& a, hipStream_t st) {
  {
    sbk::ProfScope prof("attn_rnn_energy", (double)a.n * a.T * a.A * (2.0 * a.C + 4.0) + 2.0 * a.n * a.T * a.C * (2.0 * a.k + 1.0),
                        4.0 * ((double)a.n * a.T * a.A + (double)a.n * a.A + 2.0 * a.n * a.T), st);
    SBK_LAUNCH(attn_energy_kernel, dim3(sbk::cdiv(a.T, kTT), a.n), dim3(256), 0, st, a);
  }
  {
    sbk::ProfScope prof("attn_rnn_softmax_ctx", 2.0 * a.n * a.T * a.E + 6.0 * a.n * a.T,
                        4.0 * ((double)a.n * a.T * a.E + 2.0 * a.n * a.T + (double)a.n * a.E), st);
    SBK_LAUNCH(attn_softmax_ctx_kernel, dim3(sbk::cdiv(a.E, 64), a.n), dim3(256), 0, st, a);
  }
  return sbk::launch_status("attn_rnn_attend");
}

int launch_gru_cell(const GruArgs& g, hipStream_t st) {
  sbk::ProfScope prof("gru_cell", 20.0 * g.n * g.H, 4.0 * 8.0 * g.n * g.H, st);
  SBK_LAUNCH(gru_cell_kernel, dim3((unsigned)(((long)g.n * g.H + 255) / 256)), dim3(256), 0, st, g);
  return sbk::launch_status("gru_cell");
}

int launch_gather(const float* src, const int32_t* idx, long src_stride, int n_src, float* dst, long dst_stride, int width, int n,
                  hipStream_t st) {
  sbk::ProfScope prof("attn_rnn_gather", 0.0, 8.0 * n * width, st);
  SBK_LAUNCH(gather_rows_kernel, dim3(sbk::cdiv(width, 256), n), dim3(256), 0, st, src, idx, src_stride, n_src, dst, dst_stride, width);
  return sbk::launch_status("attn_rnn_gather");
}

// enc_len in [1, T] and row_utt in [0, B), checked on the device (one 4-byte read-back: the entries below are called once per
// search or per test, the kernels themselves clamp)
int validate_lengths(const int32_t* enc_len, const int32_t* row_utt, int B, int n, int T, int* flag, const char* who, hipStream_t st) {
  SBK_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
  SBK_LAUNCH(attn_validate_kernel, dim3(sbk::cdiv(B > n ? B : n, 256)), dim3(256), 0, st, enc_len, row_utt, B, n, T, flag);
  SBK_TRY(sbk::launch_status("attn_rnn_validate"));
  int host = 0;
  SBK_HIP(hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  SBK_HIP(hipStreamSynchronize(st));
  SBK_REQUIRE(host != 1, "%s: an enc_len is outside the limits 1 <= enc_len <= T = %d", who, T);
  SBK_REQUIRE(host != 2, "%s: a row_utt is outside the limits 0 <= row_utt < B = %d", who, B);
  return 0;
}

int check_attend_shape(const char* who, int n, int B, int T, int A, int E, int C, int k) {
  SBK_REQUIRE(n >= 1 && n <= kMaxRows, "%s: n=%d is outside the limits 1 <= n <= %d", who, n, kMaxRows);
  SBK_REQUIRE(B >= 1, "%s: B=%d (B >= 1)", who, B);
  SBK_REQUIRE(T >= 1 && T <= kMaxT, "%s: T=%d is outside the limits 1 <= T <= %d", who, T, kMaxT);
  SBK_REQUIRE(A >= 1 && A <= kMaxA, "%s: A=%d is outside the limits 1 <= A <= %d", who, A, kMaxA);
  SBK_REQUIRE(E >= 1 && E <= kMaxE, "%s: E=%d is outside the limits 1 <= E <= %d", who, E, kMaxE);
  SBK_REQUIRE(C >= 0 && C <= kMaxC, "%s: C=%d is outside the limits 0 <= C <= %d", who, C, kMaxC);
  SBK_REQUIRE(C == 0 || (k >= 0 && k <= kMaxK), "%s: k=%d is outside the limits 0 <= k <= %d", who, k, kMaxK);
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- the decode step
inline size_t align4(size_t n) { return (n + 3) & ~(size_t)3; }

struct StepLayout {
  float* enc_h;   // [B,T,A]
  float* row;     // [B,ld]: emb | c | cell_out (the top layer's h)
  float* hbuf;    // [layers-1,B,H]: h of the layers below the top one
  float* gi;      // [B,3H]
  float* gh;
  float* dec_h;   // [B,A]
  float* ctx;     // [B,E]
  float* energy;  // [B,T]
  float* attn[2]; // [B,T] each: the first prev_attn / the greedy search's two attention buffers
  float* dec_out; // [B,H]   (greedy)
  float* logits;  // [B,V]   (greedy)
  int32_t* tok;   // [B]
  int32_t* ended; // [B]
  int32_t* n_ended;
  int32_t* flag;
  long ld;
};

size_t carve(StepLayout& lay, void* base, const sbk_attn_rnn_weights* W, int B, int T, bool greedy) {
  const size_t H = W->hidden, A = W->attn_dim, E = W->enc_dim, in = W->in_dim, V = greedy ? W->vocab : 0;
  float* p = static_cast<float*>(base);
  size_t off = 0;
  auto take = [&](size_t n) {
    float* q = p != nullptr ? p + off : nullptr;
    off += align4(n);
    return q;
  };
  lay.ld = (long)align4(in + A + H);
  lay.enc_h = take((size_t)B * T * A);
  lay.row = take((size_t)B * lay.ld);
  lay.hbuf = take((size_t)(W->n_layers - 1) * B * H);
  lay.gi = take((size_t)B * 3 * H);
  lay.gh = take((size_t)B * 3 * H);
  lay.dec_h = take((size_t)B * A);
  lay.ctx = take((size_t)B * E);
  lay.energy = take((size_t)B * T);
  lay.attn[0] = take((size_t)B * T);
  lay.attn[1] = take((size_t)B * T);
  lay.dec_out = take(greedy ? (size_t)B * H : 0);
  lay.logits = take((size_t)B * V);
  lay.tok = reinterpret_cast<int32_t*>(take(B));
  lay.ended = reinterpret_cast<int32_t*>(take(B));
  lay.n_ended = reinterpret_cast<int32_t*>(take(4));
  lay.flag = reinterpret_cast<int32_t*>(take(4));
  return off * sizeof(float);
}

int check_weights(const sbk_attn_rnn_weights* W, const char* who, bool greedy) {
  SBK_REQUIRE(W != nullptr, "%s: null weights", who);
  SBK_REQUIRE(W->n_layers >= 1 && W->n_layers <= SBK_ATTN_RNN_MAX_LAYERS, "%s: n_layers=%d is outside the limits 1 <= n_layers <= %d",
              who, W->n_layers, SBK_ATTN_RNN_MAX_LAYERS);
  SBK_REQUIRE(W->hidden >= 1 && W->hidden <= kMaxH, "%s: H=%d is outside the limits 1 <= H <= %d", who, W->hidden, kMaxH);
  SBK_REQUIRE(W->in_dim >= 1, "%s: in_dim=%d (in_dim >= 1)", who, W->in_dim);
  for (int l = 0; l < W->n_layers; ++l) {
    SBK_REQUIRE(W->w_ih[l] && W->w_hh[l], "%s: null GRU weight of layer %d", who, l);
    SBK_REQUIRE((W->b_ih[l] == nullptr) == (W->b_hh[l] == nullptr), "%s: b_ih and b_hh of layer %d are given together or not at all", who, l);
  }
  SBK_REQUIRE(W->enc_w && W->dec_w && W->attn_v && W->out_w && W->proj_w, "%s: null attention / projection weight", who);
  SBK_REQUIRE(W->channels == 0 || (W->conv_w && W->loc_w && W->loc_b), "%s: null location weight with channels=%d", who, W->channels);
  SBK_REQUIRE(!greedy || (W->emb && W->fc_w && W->vocab >= 1 && W->n_emb >= 1), "%s: the search needs emb, fc_w, vocab and n_emb", who);
  return 0;
}

int gemm(const float* A, int lda, const float* Wt, const float* bias, float* C, int ldc, int M, int N, int K, hipStream_t st) {
  return sbk::gemm_nt_ws(A, lda, Wt, K, bias, nullptr, 0, C, ldc, M, N, K, SBK_ACT_NONE, 1.0f, nullptr, 0, nullptr, 0, st);
}

// One step of AttentionalRNNDecoder.forward_step for B rows: row[:, 0:in] holds the step's input and row[:, in:in+A] the previous
// context on entry; on return row[:, in:in+A] holds the new context, the h of every layer is advanced and dec_out is written.
int decoder_step(const sbk_attn_rnn_weights* W, const StepLayout& lay, const float* enc, const int32_t* enc_len, const float* prev,
                 long ld_prev, float* attn, long ld_attn, float* dec_out, int ld_out, bool first, int B, int T, hipStream_t st) {
  const int H = W->hidden, A = W->attn_dim, E = W->enc_dim, in = W->in_dim, top = W->n_layers - 1;
  float* cell_out = lay.row + in + A;
  for (int l = 0; l <= top; ++l) {
    const float* x = l == 0 ? lay.row : lay.hbuf + (size_t)(l - 1) * B * H;
    const int ldx = l == 0 ? (int)lay.ld : H, K = l == 0 ? in + A : H;
    float* h = l == top ? cell_out : lay.hbuf + (size_t)l * B * H;
    const long ldh = l == top ? lay.ld : H;
    SBK_TRY(gemm(x, ldx, W->w_ih[l], nullptr, lay.gi, 3 * H, B, 3 * H, K, st));
    if (!first) SBK_TRY(gemm(h, (int)ldh, W->w_hh[l], nullptr, lay.gh, 3 * H, B, 3 * H, H, st));  // (h = 0 at the first step: gh = 0, set once)
    GruArgs g{lay.gi, lay.gh, W->b_ih[l], W->b_hh[l], first ? nullptr : h, h, ldh, ldh, B, H};
    SBK_TRY(launch_gru_cell(g, st));
  }
  SBK_TRY(gemm(cell_out, (int)lay.ld, W->dec_w, W->dec_b, lay.dec_h, A, B, A, H, st));
  AttendArgs a{enc, lay.enc_h, enc_len, nullptr, lay.dec_h, prev, W->conv_w, W->loc_w, W->loc_b, W->attn_v, lay.energy, attn, lay.ctx,
               ld_prev, ld_attn, B, B, T, A, E, W->channels, W->kernel, W->scaling};
  SBK_TRY(launch_attend(a, st));
  SBK_TRY(gemm(lay.ctx, E, W->out_w, W->out_b, lay.row + in, (int)lay.ld, B, A, E, st));
  return gemm(lay.row + in, (int)lay.ld, W->proj_w, W->proj_b, dec_out, ld_out, B, H, A + H, st);
}

// what both whole-search entries do first: checks, the layout, mlp_enc(enc) once, c = 0, gh = 0, the first prev_attn
int begin_search(const sbk_attn_rnn_weights* W, StepLayout& lay, const float* enc, const int32_t* enc_len, void* workspace,
                 size_t workspace_bytes, int B, int T, bool greedy, const char* who, hipStream_t st) {
  SBK_TRY(check_weights(W, who, greedy));
  SBK_TRY(check_attend_shape(who, B, B, T, W->attn_dim, W->enc_dim, W->channels, W->kernel));
  SBK_REQUIRE(enc && enc_len && workspace, "%s: null operand (enc, enc_len and workspace are required)", who);
  SBK_REQUIRE(workspace_bytes >= carve(lay, workspace, W, B, T, greedy), "%s: workspace too small", who);
  SBK_TRY(validate_lengths(enc_len, nullptr, B, B, T, lay.flag, who, st));
  SBK_TRY(gemm(enc, W->enc_dim, W->enc_w, W->enc_b, lay.enc_h, W->attn_dim, B * T, W->attn_dim, W->enc_dim, st));
  SBK_HIP(hipMemsetAsync(lay.row, 0, (size_t)B * lay.ld * sizeof(float), st));
  SBK_HIP(hipMemsetAsync(lay.gh, 0, (size_t)B * 3 * W->hidden * sizeof(float), st));
  if (W->channels > 0) {
    SBK_LAUNCH(attn_init_kernel, dim3(sbk::cdiv(T, 256), B), dim3(256), 0, st, enc_len, (const int32_t*)nullptr, lay.attn[0], (long)T, B, T);
    SBK_TRY(sbk::launch_status("attn_rnn_attn_init"));
  }
  return 0;
}

// The stop rule's poll (as csrc/search.hip's): a 4-byte copy of the "ended" counter every check_every steps, read back two polls
// later so that the stream is never drained.  One ring per host thread.
struct EndedPoll {
  static constexpr int kRing = 4;
  int32_t* host = nullptr;  // pinned
  hipEvent_t ev[kRing] = {};
  int issued = 0;
  bool ok = false;
  bool begin() {
    if (!ok) {
      if (hipHostMalloc(reinterpret_cast<void**>(&host), kRing * sizeof(int32_t), 0) != hipSuccess) return false;
      for (int i = 0; i < kRing; ++i)
        if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
      ok = true;
    }
    for (int j = issued > kRing ? issued - kRing : 0; j < issued; ++j) (void)hipEventSynchronize(ev[j % kRing]);
    issued = 0;
    return true;
  }
  int poll(const int32_t* counter_dev, int target, hipStream_t st) {  // 1: reached; 0: go on; -1: error
    const int k = issued % kRing;
    if (hipMemcpyAsync(host + k, counter_dev, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipEventRecord(ev[k], st) != hipSuccess)
      return -1;
    ++issued;
    if (issued >= 3) {
      const int j = (issued - 3) % kRing;
      if (hipEventSynchronize(ev[j]) != hipSuccess) return -1;
      if (host[j] >= target) return 1;
    }
    return 0;
  }
};
thread_local EndedPoll g_ended_poll;

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- C ABI
extern "C" size_t sbk_attn_rnn_attend_workspace_bytes(int n, int T) {
  return n >= 1 && T >= 1 ? ((size_t)n * T + 4) * sizeof(float) : 0;
}

extern "C" int sbk_attn_rnn_attend_f32(const float* enc, const float* enc_h, const int32_t* enc_len, const int32_t* row_utt,
                                       const float* dec_h, const float* prev_attn, const float* conv_w, const float* loc_w,
                                       const float* loc_b, const float* attn_v, float scaling, float* attn, float* ctx,
                                       void* workspace, size_t workspace_bytes, int n, int B, int T, int A, int E, int C, int k,
                                       sbk_stream_t stream) {
  SBK_TRY(check_attend_shape("attn_rnn_attend", n, B, T, A, E, C, k));
  SBK_REQUIRE(row_utt != nullptr || n == B, "attn_rnn_attend: row_utt is NULL (identity) with n=%d != B=%d", n, B);
  SBK_REQUIRE(enc && enc_h && enc_len && dec_h && attn_v && attn && ctx && workspace,
              "attn_rnn_attend: null operand (enc, enc_h, enc_len, dec_h, attn_v, attn, ctx and workspace are required)");
  SBK_REQUIRE(C == 0 || (prev_attn && conv_w && loc_w && loc_b),
              "attn_rnn_attend: null location operand with C=%d (prev_attn, conv_w, loc_w and loc_b are required)", C);
  SBK_REQUIRE(C == 0 || prev_attn != attn, "attn_rnn_attend: attn must not alias prev_attn");
  SBK_REQUIRE(workspace_bytes >= sbk_attn_rnn_attend_workspace_bytes(n, T), "attn_rnn_attend: workspace too small");
  const hipStream_t st = sbk::as_stream(stream);
  float* energy = static_cast<float*>(workspace);
  SBK_TRY(validate_lengths(enc_len, row_utt, B, n, T, reinterpret_cast<int*>(energy + (size_t)n * T), "attn_rnn_attend", st));
  AttendArgs a{enc, enc_h, enc_len, row_utt, dec_h, prev_attn, conv_w, loc_w, loc_b, attn_v, energy, attn, ctx,
               (long)T, (long)T, n, B, T, A, E, C, C > 0 ? k : 0, scaling};
  return launch_attend(a, st);
}

extern "C" int sbk_attn_rnn_attn_init_f32(const int32_t* enc_len, const int32_t* row_utt, float* attn, int n, int B, int T,
                                          sbk_stream_t stream) {
  SBK_REQUIRE(n >= 1 && n <= kMaxRows, "attn_rnn_attn_init: n=%d is outside the limits 1 <= n <= %d", n, kMaxRows);
  SBK_REQUIRE(B >= 1, "attn_rnn_attn_init: B=%d (B >= 1)", B);
  SBK_REQUIRE(T >= 1 && T <= kMaxT, "attn_rnn_attn_init: T=%d is outside the limits 1 <= T <= %d", T, kMaxT);
  SBK_REQUIRE(row_utt != nullptr || n == B, "attn_rnn_attn_init: row_utt is NULL (identity) with n=%d != B=%d", n, B);
  SBK_REQUIRE(enc_len && attn, "attn_rnn_attn_init: null operand");
  SBK_LAUNCH(attn_init_kernel, dim3(sbk::cdiv(T, 256), n), dim3(256), 0, sbk::as_stream(stream), enc_len, row_utt, attn, (long)T, B, T);
  return sbk::launch_status("sbk_attn_rnn_attn_init_f32");
}

extern "C" int sbk_gru_cell_f32(const float* gi, const float* gh, const float* b_ih, const float* b_hh, const float* h_prev,
                                float* h_out, int n, int H, sbk_stream_t stream) {
  SBK_REQUIRE(n >= 1, "gru_cell: n=%d (n >= 1)", n);
  SBK_REQUIRE(H >= 1 && H <= kMaxH, "gru_cell: H=%d is outside the limits 1 <= H <= %d", H, kMaxH);
  SBK_REQUIRE(gi && gh && h_out, "gru_cell: null operand (gi, gh and h_out are required)");
  SBK_REQUIRE((b_ih == nullptr) == (b_hh == nullptr), "gru_cell: b_ih and b_hh are given together or not at all");
  GruArgs g{gi, gh, b_ih, b_hh, h_prev, h_out, (long)H, (long)H, n, H};
  return launch_gru_cell(g, sbk::as_stream(stream));
}

extern "C" size_t sbk_attn_rnn_greedy_workspace_bytes(const sbk_attn_rnn_weights* W, int B, int T) {
  if (!W || B < 1 || T < 1 || W->n_layers < 1) return 0;
  StepLayout lay;
  return carve(lay, nullptr, W, B, T, true);
}

extern "C" int sbk_attn_rnn_greedy_f32(const sbk_attn_rnn_weights* W, const float* enc, const int32_t* enc_len, void* workspace,
                                       size_t workspace_bytes, int32_t* out_tokens, float* out_scores, int32_t* steps_run, int B,
                                       int T, int max_steps, int bos, int eos, int check_every, sbk_stream_t stream) {
  if (steps_run) *steps_run = 0;
  SBK_REQUIRE(max_steps >= 1, "attn_rnn_greedy: max_steps=%d (max_steps >= 1)", max_steps);
  SBK_REQUIRE(out_tokens && out_scores, "attn_rnn_greedy: null output");
  const hipStream_t st = sbk::as_stream(stream);
  StepLayout lay;
  SBK_TRY(begin_search(W, lay, enc, enc_len, workspace, workspace_bytes, B, T, true, "attn_rnn_greedy", st));
  const int H = W->hidden, V = W->vocab, L = max_steps;
  SBK_LAUNCH(greedy_init_kernel, dim3(sbk::cdiv(B, 256)), dim3(256), 0, st, lay.tok, lay.ended, lay.n_ended, B, bos);
  SBK_TRY(sbk::launch_status("attn_rnn_greedy_init"));
  // (steps that are not run -- the search stopped early -- read as (eos, 0), what an ended row records)
  SBK_LAUNCH(fill_i32_kernel, dim3((unsigned)(((long)B * L + 255) / 256)), dim3(256), 0, st, out_tokens, (long)B * L, eos);
  SBK_TRY(sbk::launch_status("attn_rnn_greedy_fill"));
  SBK_HIP(hipMemsetAsync(out_scores, 0, (size_t)B * L * sizeof(float), st));
  if (check_every < 1) check_every = 8;
  if (!g_ended_poll.begin()) return sbk::fail(-1, "attn_rnn_greedy: cannot allocate the stop-rule poll");
  int s = 0;
  for (; s < L; ++s) {
    SBK_TRY(launch_gather(W->emb, lay.tok, W->in_dim, W->n_emb, lay.row, lay.ld, W->in_dim, B, st));
    SBK_TRY(decoder_step(W, lay, enc, enc_len, lay.attn[s & 1], T, lay.attn[(s + 1) & 1], T, lay.dec_out, H, s == 0, B, T, st));
    SBK_TRY(gemm(lay.dec_out, H, W->fc_w, W->fc_b, lay.logits, V, B, V, H, st));
    {
      sbk::ProfScope prof("attn_rnn_select", 4.0 * B * V, 8.0 * B * V, st);
      SBK_LAUNCH(greedy_select_kernel, dim3(B), dim3(256), 0, st, (const float*)lay.logits, V, eos, s, L, lay.tok, lay.ended,
                 lay.n_ended, out_tokens, out_scores);
    }
    SBK_TRY(sbk::launch_status("attn_rnn_greedy_select"));
    if ((s + 1) % check_every == 0 && s + 1 < L) {
      const int rc = g_ended_poll.poll(lay.n_ended, B, st);
      if (rc < 0) return sbk::fail(-1, "attn_rnn_greedy: the stop-rule poll failed");
      if (rc == 1) {
        ++s;
        break;
      }
    }
  }
  if (steps_run) *steps_run = s;
  return 0;
}

extern "C" size_t sbk_attn_rnn_decode_workspace_bytes(const sbk_attn_rnn_weights* W, int B, int T) {
  if (!W || B < 1 || T < 1 || W->n_layers < 1) return 0;
  StepLayout lay;
  return carve(lay, nullptr, W, B, T, false);
}

extern "C" int sbk_attn_rnn_decode_f32(const sbk_attn_rnn_weights* W, const float* inp, const float* enc, const int32_t* enc_len,
                                       void* workspace, size_t workspace_bytes, float* outputs, float* attn, float* hs, float* c,
                                       int B, int T, int L, sbk_stream_t stream) {
  SBK_REQUIRE(L >= 1, "attn_rnn_decode: L=%d (L >= 1)", L);
  SBK_REQUIRE(inp && outputs && attn, "attn_rnn_decode: null operand (inp, outputs and attn are required)");
  const hipStream_t st = sbk::as_stream(stream);
  StepLayout lay;
  SBK_TRY(begin_search(W, lay, enc, enc_len, workspace, workspace_bytes, B, T, false, "attn_rnn_decode", st));
  const int H = W->hidden, A = W->attn_dim, in = W->in_dim;
  const long lda = (long)L * T;
  for (int s = 0; s < L; ++s) {
    SBK_TRY(launch_gather(inp + (size_t)s * in, nullptr, (long)L * in, B, lay.row, lay.ld, in, B, st));
    // the attention of step s is written into attn[:, s, :] and read from there as the next step's prev_attn
    const float* prev = s == 0 ? lay.attn[0] : attn + (size_t)(s - 1) * T;
    SBK_TRY(decoder_step(W, lay, enc, enc_len, prev, s == 0 ? (long)T : lda, attn + (size_t)s * T, lda, outputs + (size_t)s * H, L * H,
                         s == 0, B, T, st));
  }
  if (hs != nullptr)
    for (int l = 0; l < W->n_layers; ++l) {
      const bool top = l == W->n_layers - 1;
      SBK_TRY(launch_gather(top ? lay.row + in + A : lay.hbuf + (size_t)l * B * H, nullptr, top ? lay.ld : (long)H, B,
                            hs + (size_t)l * B * H, H, H, B, st));
    }
  if (c != nullptr) SBK_TRY(launch_gather(lay.row + in, nullptr, lay.ld, B, c, A, A, B, st));
  return 0;
}
