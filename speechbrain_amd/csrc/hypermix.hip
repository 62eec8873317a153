// HyperMixing token mixing (the HyperConformer recipes' replacement for self-attention), fused       (sbk_hypermix_f32)
//   u[t,:]    = h[b,t,:] for t < key_len[b], else 0;   p[t,:] = u[t,:] + pe[t,:]
//   per head m (slice of Dh channels), generator g in (1,2):
//     z_g[t,:] = GELU(p[t,m] fc1_g[m]^T + b1_g[m])                                   [Dh]
//     W_g[t,:] = z_g[t,:] fc2_g[m]^T + b2_g[m]     for t < key_len[b], else 0        [k]
//   A[f,j]    = GELU(sum_t u[t,m,f] W_1[t,j])                                        [Dh,k]
//   y[t,m,f]  = sum_j A[f,j] W_2[t,j];     out = LayerNorm_d(y) (+ residual)
// The composition writes W_1 and W_2, [B,H,T,k] each, to memory and reads them back.  Here neither exists, not even as a tile:
// W_g is AFFINE in z_g, so both contractions over k are moved off the time axis.  With ze = [z | 1] (Dh+1 columns; the row is
// zero on padded frames) and W_ge = [fc2_g[m] | b2_g[m]]  ([k, Dh+1]):
//     S  = u^T ze_1                       [Dh, Dh+1]   the only sum over time                       (reduce)
//     A  = GELU(S W_1e^T)                 [Dh, k]      once per (b, m), in LDS
//     G  = A W_2e                         [Dh, Dh+1]   once per (b, m)                               (finalise)
//     y  = ze_2 G^T                       [T, Dh]                                                    (apply)
// which is the same sum in another order: per frame 4 Dh (Dh+1) flops per head instead of 4 Dh k, and the only intermediate in
// memory is G [B,H,Dh,Dh+1] (plus the partial S of a split time axis) -- smaller than A [B,H,Dh,k] by k / (Dh+1).
//
// Launches:
//   hypermix_reduce   grid (splits, H, B).  A workgroup walks its kSplitFrames frames of one (b, m) 32 at a time: stages u and p,
//                     forms ze_1 in LDS, accumulates S in registers (16 x 16 thread grid, NA x NC values per thread).
//                     splits == 1 (T <= kSplitFrames: the recipes' 10 s batches): the same workgroup finalises, G goes to memory.
//                     Otherwise its partial S goes to the workspace and
//   hypermix_combine  grid (H, B) sums the partials in split order and finalises.
//   hypermix_apply    grid (ceil(T/16), B).  A workgroup owns 16 frames and ALL heads: per head it forms ze_2 and y in LDS; then
//                     one wave per frame normalises the d channels, adds the skip and stores.
// Determinism: no atomics; splits = ceil(T / kSplitFrames) depends on T only; a thread's sums run in index order.
// Contractions are vector FMAs on LDS operands (every operand is zero-padded to 16 columns in LDS, never read out of range).
#include "act.h"
#include "common.h"
#include "internal.h"

namespace {

constexpr int kMaxDh = 64, kMaxK = 256, kMaxT = 3000, kMaxD = 1024;
constexpr int kSplitFrames = 256;  // frames of one reduce workgroup; splits = ceil(T / kSplitFrames)
constexpr int kRT = 32;            // frames per step of the reduce loop
constexpr int kAT = 16;            // frames of an apply workgroup
constexpr int kJT = 32;            // columns of A per step of the finalise loop

struct HmArgs {
  const float* h;        // [B,T,d]
  const int32_t* key_len;
  const float* pe;       // [T,d]
  const float* fc1w[2];  // [H,Dh,Dh]
  const float* fc1b[2];  // [H,Dh]
  const float* fc2w[2];  // [H,k,Dh]
  const float* fc2b[2];  // [H,k]
  const float* gamma;
  const float* beta;
  const float* residual;  // [B,T,d] or null
  float* out;             // [B,T,d]
  float* G;               // [B,H,Dh,Dh+1]
  float* part;            // [B,H,splits,Dh,Dh+1]
  int B, T, H, Dh, k, splits;
  float eps;
};

// acc[a][c] += sum_{r < R} X[r * ldx + tf + 16 a] * Y[r * ldy + te + 16 c]
template <int NA, int NC>
__device__ __forceinline__ void rank_update(float (&acc)[NA][NC], const float* X, int ldx, const float* Y, int ldy, int R, int tf,
                                            int te) {
  for (int r = 0; r < R; ++r) {
    float xv[NA], yv[NC];
#pragma unroll
    for (int a = 0; a < NA; ++a) xv[a] = X[r * ldx + tf + 16 * a];
#pragma unroll
    for (int c = 0; c < NC; ++c) yv[c] = Y[r * ldy + te + 16 * c];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
      for (int c = 0; c < NC; ++c) acc[a][c] = fmaf(xv[a], yv[c], acc[a][c]);
  }
}

// S_s [DP][EP] (zero beyond [Dh][Dh+1]) at the head of `lds` -> G[b,m] in memory.  Every thread of the workgroup calls it; the
// caller has synchronised after writing S_s.
template <int NA, int NC>
__device__ __forceinline__ void finalise(const HmArgs& a, float* lds, int b, int m) {
  constexpr int DP = 16 * NA, EP = 16 * NC;
  const int Dh = a.Dh, E = Dh + 1, k = a.k, WS = E | 1;
  const int tid = threadIdx.x;
  float* S_s = lds;                     // [DP][EP]
  float* W1_s = S_s + DP * EP;          // [kJT][WS]   rows of [fc2_1 | b2_1]
  float* At_s = W1_s + kJT * (kMaxDh + 1);  // [kJT][DP+1] the tile of A, transposed
  float* W2_s = At_s + kJT * (DP + 1);  // [kJT][EP]   rows of [fc2_2 | b2_2]
  const float* w1 = a.fc2w[0] + (size_t)m * k * Dh;
  const float* c1 = a.fc2b[0] + (size_t)m * k;
  const float* w2 = a.fc2w[1] + (size_t)m * k * Dh;
  const float* c2 = a.fc2b[1] + (size_t)m * k;
  const int tf = tid >> 4, te = tid & 15;
  const int tj = tid & 31, tg = tid >> 5;
  float g[NA][NC];
#pragma unroll
  for (int x = 0; x < NA; ++x)
#pragma unroll
    for (int c = 0; c < NC; ++c) g[x][c] = 0.0f;
  for (int j0 = 0; j0 < k; j0 += kJT) {
    const int nj = min(kJT, k - j0);
    for (int i = tid; i < kJT * E; i += 256) {
      const int jj = i / E, e = i - jj * E;
      float v = 0.0f;
      if (jj < nj) v = e < Dh ? w1[(size_t)(j0 + jj) * Dh + e] : c1[j0 + jj];
      W1_s[jj * WS + e] = v;
    }
    for (int i = tid; i < kJT * EP; i += 256) {
      const int jj = i / EP, e = i - jj * EP;
      float v = 0.0f;
      if (jj < nj && e < E) v = e < Dh ? w2[(size_t)(j0 + jj) * Dh + e] : c2[j0 + jj];
      W2_s[i] = v;
    }
    __syncthreads();
    {  // A[f, j0 + tj] for f = tg + 8 x
      float s[2 * NA];
#pragma unroll
      for (int x = 0; x < 2 * NA; ++x) s[x] = 0.0f;
      for (int e = 0; e < E; ++e) {
        const float wv = W1_s[tj * WS + e];
#pragma unroll
        for (int x = 0; x < 2 * NA; ++x) s[x] = fmaf(S_s[(tg + 8 * x) * EP + e], wv, s[x]);
      }
#pragma unroll
      for (int x = 0; x < 2 * NA; ++x) {
        const int f = tg + 8 * x;
        At_s[tj * (DP + 1) + f] = (tj < nj && f < Dh) ? sbk::gelu_erf(s[x]) : 0.0f;
      }
    }
    __syncthreads();
    rank_update<NA, NC>(g, At_s, DP + 1, W2_s, EP, kJT, tf, te);
    __syncthreads();
  }
  float* Gm = a.G + ((size_t)b * a.H + m) * Dh * E;
#pragma unroll
  for (int x = 0; x < NA; ++x)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = tf + 16 * x, e = te + 16 * c;
      if (f < Dh && e < E) Gm[f * E + e] = g[x][c];
    }
}

template <int NA, int NC>
constexpr int finalise_floats() {
  return 16 * NA * 16 * NC + kJT * (kMaxDh + 1) + kJT * (16 * NA + 1) + kJT * 16 * NC;
}
template <int NA, int NC>
constexpr int reduce_floats() {
  return 16 * NA * (16 * NA + 1) + 16 * NA + 2 * kRT * 16 * NA + kRT * 16 * NC;
}

template <int NA, int NC>
__global__ void __launch_bounds__(256) hypermix_reduce_kernel(HmArgs a) {
  constexpr int DP = 16 * NA, EP = 16 * NC, WP = DP + 1;
  SBK_DYN_LDS(float, lds);
  float* w_s = lds;            // [DP][WP]  fc1_1[m] transposed: w_s[f * WP + e]
  float* b_s = w_s + DP * WP;  // [DP]
  float* u_s = b_s + DP;       // [kRT][DP]
  float* p_s = u_s + kRT * DP; // [kRT][DP]
  float* z_s = p_s + kRT * DP; // [kRT][EP]  [z | 1], zero rows past the last valid frame
  const int tid = threadIdx.x, s = blockIdx.x, m = blockIdx.y, b = blockIdx.z;
  const int T = a.T, Dh = a.Dh, d = a.H * Dh, E = Dh + 1;
  const int tf = tid >> 4, te = tid & 15;
  int klen = T;
  if (a.key_len) klen = min(max(a.key_len[b], 0), T);
  const int t_end = min((s + 1) * kSplitFrames, klen);

  for (int i = tid; i < DP * WP; i += 256) w_s[i] = 0.0f;
  if (tid < DP) b_s[tid] = tid < Dh ? a.fc1b[0][m * Dh + tid] : 0.0f;
  __syncthreads();
  {
    const float* w = a.fc1w[0] + (size_t)m * Dh * Dh;
    for (int i = tid; i < Dh * Dh; i += 256) {
      const int e = i / Dh, f = i - e * Dh;
      w_s[f * WP + e] = w[i];
    }
  }
  float acc[NA][NC];
#pragma unroll
  for (int x = 0; x < NA; ++x)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[x][c] = 0.0f;

  for (int t0 = s * kSplitFrames; t0 < t_end; t0 += kRT) {
    const int nt = min(kRT, t_end - t0);
    for (int i = tid; i < kRT * DP; i += 256) {
      const int r = i / DP, f = i - r * DP;
      float uv = 0.0f, pv = 0.0f;
      if (r < nt && f < Dh) {
        const size_t col = (size_t)m * Dh + f;
        uv = a.h[((size_t)b * T + t0 + r) * d + col];
        pv = uv + a.pe[(size_t)(t0 + r) * d + col];
      }
      u_s[i] = uv;
      p_s[i] = pv;
    }
    __syncthreads();
    {  // ze rows tf and tf + 16, columns te + 16 c
      float zz[2][NA];
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int c = 0; c < NA; ++c) zz[x][c] = 0.0f;
      for (int f = 0; f < Dh; ++f) {
        const float p0 = p_s[tf * DP + f], p1 = p_s[(tf + 16) * DP + f];
#pragma unroll
        for (int c = 0; c < NA; ++c) {
          const float wv = w_s[f * WP + te + 16 * c];
          zz[0][c] = fmaf(p0, wv, zz[0][c]);
          zz[1][c] = fmaf(p1, wv, zz[1][c]);
        }
      }
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int r = tf + 16 * x;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int e = te + 16 * c;
          float v = 0.0f;
          if (r < nt) {
            if (c < NA && e < Dh) v = sbk::gelu_erf(zz[x][c < NA ? c : 0] + b_s[e]);
            else if (e == Dh) v = 1.0f;
          }
          z_s[r * EP + e] = v;
        }
      }
    }
    __syncthreads();
    rank_update<NA, NC>(acc, u_s, DP, z_s, EP, kRT, tf, te);
    __syncthreads();
  }

  if (a.splits > 1) {
    float* P = a.part + (((size_t)b * a.H + m) * a.splits + s) * Dh * E;
#pragma unroll
    for (int x = 0; x < NA; ++x)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int f = tf + 16 * x, e = te + 16 * c;
        if (f < Dh && e < E) P[f * E + e] = acc[x][c];
      }
    return;
  }
  __syncthreads();  // (the staging buffers are dead: S takes their place)
#pragma unroll
  for (int x = 0; x < NA; ++x)
#pragma unroll
    for (int c = 0; c < NC; ++c) lds[(tf + 16 * x) * EP + te + 16 * c] = acc[x][c];
  __syncthreads();
  finalise<NA, NC>(a, lds, b, m);
}

template <int NA, int NC>
__global__ void __launch_bounds__(256) hypermix_combine_kernel(HmArgs a) {
  constexpr int DP = 16 * NA, EP = 16 * NC;
  SBK_DYN_LDS(float, lds);
  const int tid = threadIdx.x, m = blockIdx.x, b = blockIdx.y;
  const int Dh = a.Dh, E = Dh + 1;
  const float* P = a.part + ((size_t)b * a.H + m) * a.splits * Dh * E;
  for (int i = tid; i < DP * EP; i += 256) {
    const int f = i / EP, e = i - f * EP;
    float v = 0.0f;
    if (f < Dh && e < E)
      for (int s = 0; s < a.splits; ++s) v += P[(size_t)s * Dh * E + f * E + e];  // split order: fixed by T alone
    lds[i] = v;
  }
  __syncthreads();
  finalise<NA, NC>(a, lds, b, m);
}

__host__ __device__ inline int apply_row_stride(int d) { return d % 32 == 0 ? d + 16 : d; }
template <int NA, int NC>
int apply_floats(int d) {
  return kAT * apply_row_stride(d) + 16 * NA * (16 * NA + 1) + 16 * NA + kAT * 16 * NA + kAT * 16 * NC + 16 * NC * (16 * NA + 1);
}

template <int NA, int NC>
__global__ void __launch_bounds__(256) hypermix_apply_kernel(HmArgs a) {
  constexpr int DP = 16 * NA, EP = 16 * NC, WP = DP + 1;
  SBK_DYN_LDS(float, lds);
  const int tid = threadIdx.x, t0 = blockIdx.x * kAT, b = blockIdx.y;
  const int T = a.T, Dh = a.Dh, H = a.H, d = H * Dh, E = Dh + 1;
  const int YS = apply_row_stride(d);
  float* y_s = lds;              // [kAT][YS]
  float* w_s = y_s + kAT * YS;   // [DP][WP]  fc1_2[m] transposed
  float* b_s = w_s + DP * WP;    // [DP]
  float* p_s = b_s + DP;         // [kAT][DP]
  float* z_s = p_s + kAT * DP;   // [kAT][EP]
  float* g_s = z_s + kAT * EP;   // [EP][WP]  G[b,m] transposed: g_s[e * WP + f]
  const int tt = tid >> 4, te = tid & 15;
  int klen = T;
  if (a.key_len) klen = min(max(a.key_len[b], 0), T);
  const bool row_ok = t0 + tt < klen;

  for (int i = tid; i < DP * WP + DP + kAT * DP + kAT * EP + EP * WP; i += 256) w_s[i] = 0.0f;
  __syncthreads();
  for (int m = 0; m < H; ++m) {
    {
      const float* w = a.fc1w[1] + (size_t)m * Dh * Dh;
      for (int i = tid; i < Dh * Dh; i += 256) {
        const int e = i / Dh, f = i - e * Dh;
        w_s[f * WP + e] = w[i];
      }
      if (tid < Dh) b_s[tid] = a.fc1b[1][m * Dh + tid];
      const float* Gm = a.G + ((size_t)b * H + m) * Dh * E;
      for (int i = tid; i < Dh * E; i += 256) {
        const int f = i / E, e = i - f * E;
        g_s[e * WP + f] = Gm[i];
      }
      for (int i = tid; i < kAT * Dh; i += 256) {
        const int r = i / Dh, f = i - r * Dh;
        const int t = t0 + r;
        const size_t col = (size_t)m * Dh + f;
        float pv = 0.0f;
        if (t < klen) pv = a.h[((size_t)b * T + t) * d + col] + a.pe[(size_t)t * d + col];
        p_s[r * DP + f] = pv;
      }
    }
    __syncthreads();
    {
      float zz[NA];
#pragma unroll
      for (int c = 0; c < NA; ++c) zz[c] = 0.0f;
      for (int f = 0; f < Dh; ++f) {
        const float pv = p_s[tt * DP + f];
#pragma unroll
        for (int c = 0; c < NA; ++c) zz[c] = fmaf(pv, w_s[f * WP + te + 16 * c], zz[c]);
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int e = te + 16 * c;
        float v = 0.0f;
        if (row_ok) {
          if (c < NA && e < Dh) v = sbk::gelu_erf(zz[c < NA ? c : 0] + b_s[e]);
          else if (e == Dh) v = 1.0f;
        }
        z_s[tt * EP + e] = v;
      }
    }
    __syncthreads();
    {
      float yy[NA];
#pragma unroll
      for (int c = 0; c < NA; ++c) yy[c] = 0.0f;
      for (int e = 0; e < E; ++e) {
        const float zv = z_s[tt * EP + e];
#pragma unroll
        for (int c = 0; c < NA; ++c) yy[c] = fmaf(zv, g_s[e * WP + te + 16 * c], yy[c]);
      }
#pragma unroll
      for (int c = 0; c < NA; ++c) {
        const int f = te + 16 * c;
        if (f < Dh) y_s[tt * YS + m * Dh + f] = yy[c];
      }
    }
    __syncthreads();
  }
  // LayerNorm over d, one wave per frame (4 frames each), + the skip
  const int lane = tid & 63, wave = tid >> 6;
  const float inv_d = 1.0f / (float)d;
  for (int q = 0; q < kAT / 4; ++q) {
    const int r = wave * (kAT / 4) + q, t = t0 + r;
    const float* yr = y_s + r * YS;
    float sum = 0.0f;
    for (int c = lane; c < d; c += 64) sum += yr[c];
    const float mean = sbk::wave_sum(sum) * inv_d;
    float sq = 0.0f;
    for (int c = lane; c < d; c += 64) {
      const float v = yr[c] - mean;
      sq = fmaf(v, v, sq);
    }
    const float rstd = rsqrtf(sbk::wave_sum(sq) * inv_d + a.eps);
    if (t < T) {
      const size_t row = ((size_t)b * T + t) * d;
      for (int c = lane; c < d; c += 64) {
        float v = fmaf((yr[c] - mean) * rstd, a.gamma[c], a.beta[c]);
        if (a.residual) v += a.residual[row + c];
        a.out[row + c] = v;
      }
    }
  }
}

template <int NA, int NC>
int launch_hypermix(const HmArgs& a, hipStream_t st) {
  const int Dh = a.Dh, d = a.H * Dh;
  const double BT = (double)a.B * a.T, per_bm = 4.0 * Dh * (Dh + 1.0) * a.k;
  const double wbytes = 4.0 * a.H * (2.0 * Dh * Dh + 2.0 * Dh + 2.0 * a.k * Dh + 2.0 * a.k);
  const size_t lds_f = sizeof(float) * (size_t)finalise_floats<NA, NC>();
  const size_t lds_red = sizeof(float) * (size_t)reduce_floats<NA, NC>();
  const size_t lds_r = lds_red > lds_f ? lds_red : lds_f;
  {
    if (const int rc = sbk::require_dyn_lds(hypermix_reduce_kernel<NA, NC>, lds_r, "sbk_hypermix_f32")) return rc;
    sbk::ProfScope prof("hypermix_reduce", BT * d * (4.0 * Dh + 2.0) + (a.splits == 1 ? per_bm * a.B * a.H : 0.0),
                        8.0 * BT * d + wbytes / 2, st);
    SBK_LAUNCH((hypermix_reduce_kernel<NA, NC>), dim3(a.splits, a.H, a.B), dim3(256), lds_r, st, a);
  }
  if (a.splits > 1) {
    if (const int rc = sbk::require_dyn_lds(hypermix_combine_kernel<NA, NC>, lds_f, "sbk_hypermix_f32")) return rc;
    sbk::ProfScope prof("hypermix_combine", per_bm * a.B * a.H, 4.0 * a.B * a.H * Dh * (Dh + 1.0) * (a.splits + 1.0), st);
    SBK_LAUNCH((hypermix_combine_kernel<NA, NC>), dim3(a.H, a.B), dim3(256), lds_f, st, a);
  }
  const size_t lds_a = sizeof(float) * (size_t)apply_floats<NA, NC>(d);
  if (const int rc = sbk::require_dyn_lds(hypermix_apply_kernel<NA, NC>, lds_a, "sbk_hypermix_f32")) return rc;
  sbk::ProfScope prof("hypermix_apply", BT * d * (4.0 * Dh + 2.0 + 8.0), (a.residual ? 16.0 : 12.0) * BT * d + wbytes / 2, st);
  SBK_LAUNCH((hypermix_apply_kernel<NA, NC>), dim3(sbk::cdiv(a.T, kAT), a.B), dim3(256), lds_a, st, a);
  return sbk::launch_status("sbk_hypermix_f32");
}

int splits_of(int T) { return sbk::cdiv(T, kSplitFrames); }

size_t workspace_floats(int B, int T, int H, int Dh) {
  const int s = splits_of(T);
  return (size_t)B * H * Dh * (Dh + 1) * (size_t)(1 + (s > 1 ? s : 0));
}

}  // namespace

extern "C" int sbk_hypermix_split_frames(void) { return kSplitFrames; }

extern "C" size_t sbk_hypermix_workspace_bytes(int B, int T, int H, int Dh) {
  if (B <= 0 || T <= 0 || H <= 0 || Dh <= 0) return 0;
  return workspace_floats(B, T, H, Dh) * sizeof(float);
}

extern "C" int sbk_hypermix_f32(const float* h, const int32_t* key_len, const float* pe, const float* w1_fc1_w,
                                const float* w1_fc1_b, const float* w1_fc2_w, const float* w1_fc2_b, const float* w2_fc1_w,
                                const float* w2_fc1_b, const float* w2_fc2_w, const float* w2_fc2_b, const float* ln_w,
                                const float* ln_b, float eps, const float* residual, float* out, void* workspace,
                                size_t workspace_bytes, int B, int T, int H, int Dh, int k, sbk_stream_t stream) {
  SBK_REQUIRE(B >= 0 && T >= 0 && H > 0 && Dh > 0 && k > 0 && B <= 65535 && H <= 65535, "hypermix: bad shape B=%d T=%d H=%d", B, T, H);
  SBK_REQUIRE(Dh <= kMaxDh, "hypermix: head width Dh=%d exceeds the limit Dh <= %d", Dh, kMaxDh);
  SBK_REQUIRE(k <= kMaxK, "hypermix: hypernet width per head k=%d exceeds the limit k <= %d", k, kMaxK);
  SBK_REQUIRE(T <= kMaxT, "hypermix: T=%d frames exceed the limit T <= %d", T, kMaxT);
  SBK_REQUIRE((long)H * Dh <= kMaxD, "hypermix: d = H * Dh = %ld exceeds the limit d <= %d (a frame tile of all heads is held in LDS)",
              (long)H * Dh, kMaxD);
  if (B == 0 || T == 0) return 0;  // empty batch: nothing to launch, the data pointers may be NULL
  SBK_REQUIRE(h && pe && w1_fc1_w && w1_fc1_b && w1_fc2_w && w1_fc2_b && w2_fc1_w && w2_fc1_b && w2_fc2_w && w2_fc2_b && ln_w &&
                  ln_b && out && workspace,
              "hypermix: null operand");
  SBK_REQUIRE(out != h, "hypermix: out must not alias h (it may alias residual)");
  const size_t need = workspace_floats(B, T, H, Dh) * sizeof(float);
  SBK_REQUIRE(workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
              "hypermix: workspace of %zu bytes, sbk_hypermix_workspace_bytes asks for %zu", workspace_bytes, need);
  HmArgs a;
  a.h = h; a.key_len = key_len; a.pe = pe;
  a.fc1w[0] = w1_fc1_w; a.fc1b[0] = w1_fc1_b; a.fc2w[0] = w1_fc2_w; a.fc2b[0] = w1_fc2_b;
  a.fc1w[1] = w2_fc1_w; a.fc1b[1] = w2_fc1_b; a.fc2w[1] = w2_fc2_w; a.fc2b[1] = w2_fc2_b;
  a.gamma = ln_w; a.beta = ln_b; a.residual = residual; a.out = out;
  a.G = static_cast<float*>(workspace);
  a.part = a.G + (size_t)B * H * Dh * (Dh + 1);
  a.B = B; a.T = T; a.H = H; a.Dh = Dh; a.k = k; a.splits = splits_of(T);
  a.eps = eps;
  const hipStream_t st = sbk::as_stream(stream);
  const int na = (Dh + 15) / 16, nc = (Dh + 1 + 15) / 16;
  switch (na * 8 + nc) {
    case 1 * 8 + 1: return launch_hypermix<1, 1>(a, st);
    case 1 * 8 + 2: return launch_hypermix<1, 2>(a, st);
    case 2 * 8 + 2: return launch_hypermix<2, 2>(a, st);
    case 2 * 8 + 3: return launch_hypermix<2, 3>(a, st);
    case 3 * 8 + 3: return launch_hypermix<3, 3>(a, st);
    case 3 * 8 + 4: return launch_hypermix<3, 4>(a, st);
    case 4 * 8 + 4: return launch_hypermix<4, 4>(a, st);
    default: return launch_hypermix<4, 5>(a, st);
  }
}
