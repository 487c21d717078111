// Auto-encoder baseline (reference auto_encoder.py:20-115, restated): per
// side of the incidence one Keras model
//   x (C) -> Dense(d, relu) [W1 C x d, b1] -> Dense(C, softmax) [W2 d x C, b2]
// trained by train_on_batch with kullback_leibler_divergence and Adagrad on
// one MI355X (gfx950).
//
// A sample is a pair (row, drop) over the resident CSR: the target is
// 1_S / n on the row's support S, the input 1_S / n (drop = -1) or
// 1_{S \ drop} / (n - 1). Neither is ever materialised: the first layer is a
// gather-sum of W1 rows, the target is read from the CSR row where the loss
// needs it.
//
// One batch (M samples):
//   ae_encode     H = relu(v (sum_{c in S, c != drop} W1[c]) + b1)   M x dp
//   per chunk of at most `chunk` rows (the M x C logit block is never whole):
//     ae_logits   Z = H W2                      32x32 tiles, f32 MFMA
//     ae_softmax  P = softmax(Z + b2), the row's loss, dZ in place
//     ae_wgrad2   gW2 (+)= H^T dZ               32x32 tiles, f32 MFMA
//     colsum      gb2 (+)= sum_m dZ
//     ae_dh       dH = (dZ W2^T) * [H > 0]      32x32 tiles, f32 MFMA, the
//                 reduction over C in pieces of kSplit columns summed in order
//   colsum        gb1 = sum_m dH
//   ae_w1_update  gW1[c] = sum of v_m dH_m over the batch's samples that hold
//                 column c, a segmented sum along the transposed CSR row of c
//                 in a fixed order (no float atomics: a popular column is in
//                 most samples of a batch), and Adagrad on that row
//   ae_adagrad    b1, W2, b2
// Adagrad runs once per batch whatever the chunk size; its arithmetic is the
// trainer's (a += g g; p -= lr g / (sqrt(a) + eps), no contraction).
//
// Every GEMM is v_mfma_f32_32x32x2_f32 (exact f32 products, f32
// accumulation), one wave per 32x32 output tile, operands read straight from
// global memory in the instruction's lane order (the stored-P form; whether
// recomputing logit tiles in the backward GEMMs beats storing them is
// unmeasured).
//
// Layout: d is padded to dp (64, 128, 256 or 512), C to Cp (multiple of 32), a
// chunk's rows to a multiple of 32. Padded weights start at 0 and stay 0
// (their gradients are exactly 0), padded activations and deltas are written
// as 0, so padding changes no result.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hgx_internal.h"

// a + g*g must stay two roundings (see hgx_mlp.hip)
#pragma clang fp contract(off)

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kMaxD = 512;
constexpr int kSplit = 2048;    // columns per partial of the dH reduction
constexpr int kSeg = 256;       // rows per partial of a column sum
constexpr int kMaxChunk = 8192; // chunk rows when memory does not bound them
constexpr float kKeps = 1e-7f;  // Keras' epsilon in its float32 graph

__host__ __device__ inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- sample draw ----------------------------------------------------------
// One thread per listed row: the unperturbed sample, then min(n, spi) distinct
// columns of the row. n <= spi: every column once, in CSR order. n > spi:
// selection sampling (Knuth's algorithm S) over the CSR row, column j taken
// when bounded(u_j, n - j) < spi - taken with u_j = mix64(key(seed, epoch,
// row) + j): every spi-subset is equally likely, and the draw depends on
// (seed, row, epoch) alone.
__global__ void ae_draw(const int *rows, int n_idx, const int *soff, const int *rp,
                        const int *col, int spi, uint64_t seed, uint32_t epoch, int *s_row,
                        int *s_drop, int *s_ord, int2 *grp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_idx) return;
  const int r = rows[i], base = soff[i], b = rp[r], n = rp[r + 1] - b;
  s_row[base] = r;
  s_drop[base] = -1;
  s_ord[base] = base;
  int cnt = 1;
  if (n > 1) {
    const int k = n < spi ? n : spi;
    const uint64_t key = hgx::rand64_key(seed, ((uint64_t)epoch << 32) | (uint32_t)r);
    int taken = 0;
    for (int j = 0; j < n && taken < k; j++) {
      bool take = true;
      if (n > k)
        take = hgx::bounded(hgx::mix64(key + (uint64_t)j), (uint32_t)(n - j)) <
               (uint32_t)(k - taken);
      if (take) {
        s_row[base + cnt] = r;
        s_drop[base + cnt] = col[b + j];
        s_ord[base + cnt] = base + cnt;
        cnt++;
        taken++;
      }
    }
  }
  if (grp) grp[r] = make_int2(base, cnt);
}

__global__ void ae_grp_set(const int *urow, const int *ustart, const int *ucnt, int n,
                           int2 *grp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) grp[urow[i]] = make_int2(ustart[i], ucnt[i]);
}
__global__ void ae_grp_clear(const int *s_row, int M, int2 *grp) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < M) grp[s_row[m]] = make_int2(-1, 0);
}

// the input's value on its support
__device__ __forceinline__ float sample_v(int n, int drop) {
  return 1.0f / (float)(drop >= 0 ? n - 1 : n);
}

// ---- encode ---------------------------------------------------------------
// One wave per sample; lane l holds columns l + 64 q of the row. Rows m >= M
// (the tile padding) are written as 0.
template <int NPL>
__global__ __launch_bounds__(256) void ae_encode(int M, int Mp, const int *s_row,
                                                 const int *s_drop, const int *rp,
                                                 const int *col, const float *W1,
                                                 const float *b1, float *H, int dp) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= Mp) return;
  float acc[NPL];
#pragma unroll
  for (int q = 0; q < NPL; q++) acc[q] = 0.f;
  if (m < M) {
    const int r = s_row[m], drop = s_drop ? s_drop[m] : -1;
    const int b = rp[r], n = rp[r + 1] - b;
    for (int j = 0; j < n; j++) {
      const int c = col[b + j];
      if (c == drop) continue;
      const float *w = W1 + (size_t)c * dp;
#pragma unroll
      for (int q = 0; q < NPL; q++) acc[q] += w[lane + 64 * q];
    }
    const float v = sample_v(n, drop);
#pragma unroll
    for (int q = 0; q < NPL; q++) {
      const float z = v * acc[q] + b1[lane + 64 * q];
      acc[q] = z > 0.f ? z : 0.f;
    }
  }
#pragma unroll
  for (int q = 0; q < NPL; q++) H[(size_t)m * dp + lane + 64 * q] = acc[q];
}

// ---- the 32x32 tile on v_mfma_f32_32x32x2_f32 -----------------------------
// Lane l = 32 h + i supplies A[i][h] and B[h][i] of one 32x2 by 2x32 product;
// value r of the accumulator is D[8 (r / 4) + 4 h + r % 4][i]. The loops below
// read four reduction indices per lane half at once (index 4 h + q of a
// group of eight goes to product q), which pairs A and B consistently, and
// keep one accumulator per product q: four independent MFMA chains, summed
// (0 + 1) + (2 + 3) at the end.
__device__ __forceinline__ void tile_store(const f32x16 &acc, float *D, size_t ld, int lane) {
  const int h = lane >> 5, j = lane & 31;
#pragma unroll
  for (int r = 0; r < 16; r++)
    D[(size_t)(8 * (r >> 2) + 4 * h + (r & 3)) * ld + j] = acc[r];
}

// Z (rows_p x Cp) = H (rows_p x dp) W2 (dp x Cp); 4 waves = 4 column tiles.
__global__ __launch_bounds__(256) void ae_logits(const float *H, const float *W2, float *Z,
                                                 int dp, int Cp) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
  const int n0 = (blockIdx.x * 4 + w) * 32, m0 = blockIdx.y * 32;
  if (n0 >= Cp) return;
  const float *a = H + (size_t)(m0 + i) * dp + 4 * h;
  const float *b = W2 + (size_t)(4 * h) * Cp + n0 + i;
  f32x16 c0 = {}, c1 = {}, c2 = {}, c3 = {};
  for (int k0 = 0; k0 < dp; k0 += 8) {
    const float4 a4 = *reinterpret_cast<const float4 *>(a + k0);
    const float *bk = b + (size_t)k0 * Cp;
    const float b0 = bk[0], b1 = bk[Cp], b2 = bk[2 * (size_t)Cp], b3 = bk[3 * (size_t)Cp];
    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b0, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b1, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b2, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b3, c3, 0, 0, 0);
  }
  tile_store((c0 + c1) + (c2 + c3), Z + (size_t)m0 * Cp + n0, Cp, lane);
}

// gW2 (dp x Cp) (+)= H^T (dp x rows_p) dZ (rows_p x Cp); 4 waves = 4 column
// tiles of one 32-row band of gW2. first: start from 0 (the batch's first
// chunk), else from the stored sum.
__global__ __launch_bounds__(256) void ae_wgrad2(const float *H, const float *Z, float *gW2,
                                                 int rows_p, int dp, int Cp, int first) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
  const int n0 = (blockIdx.x * 4 + w) * 32, k0 = blockIdx.y * 32;
  if (n0 >= Cp) return;
  float *G = gW2 + (size_t)k0 * Cp + n0;
  f32x16 c0 = {}, c1 = {}, c2 = {}, c3 = {};
  if (!first) {
#pragma unroll
    for (int r = 0; r < 16; r++)
      c0[r] = G[(size_t)(8 * (r >> 2) + 4 * h + (r & 3)) * Cp + i];
  }
  const float *a = H + (size_t)(4 * h) * dp + k0 + i;
  const float *b = Z + (size_t)(4 * h) * Cp + n0 + i;
  for (int m = 0; m < rows_p; m += 8) {
    const float *am = a + (size_t)m * dp, *bm = b + (size_t)m * Cp;
    const float a0 = am[0], a1 = am[dp], a2 = am[2 * dp], a3 = am[3 * dp];
    const float b0 = bm[0], b1 = bm[Cp], b2 = bm[2 * (size_t)Cp], b3 = bm[3 * (size_t)Cp];
    c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, c3, 0, 0, 0);
  }
  tile_store((c0 + c1) + (c2 + c3), G, Cp, lane);
}

// part[z] (rows_p x dp) = dZ[:, piece z] W2[:, piece z]^T, piece z = columns
// [z kSplit, min(Cp, (z + 1) kSplit)); one wave per tile and piece.
__global__ __launch_bounds__(64) void ae_dh(const float *Z, const float *W2, float *part,
                                            int rows_p, int dp, int Cp) {
  const int lane = threadIdx.x, h = lane >> 5, i = lane & 31;
  const int m0 = blockIdx.x * 32, k0 = blockIdx.y * 32, z = blockIdx.z;
  const int c0 = z * kSplit, c1 = min(Cp, c0 + kSplit);
  const float *a = Z + (size_t)(m0 + i) * Cp + 4 * h;
  const float *b = W2 + (size_t)(k0 + i) * Cp + 4 * h;
  f32x16 s0 = {}, s1 = {}, s2 = {}, s3 = {};
  for (int c = c0; c < c1; c += 8) {
    const float4 a4 = *reinterpret_cast<const float4 *>(a + c);
    const float4 b4 = *reinterpret_cast<const float4 *>(b + c);
    s0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.x, b4.x, s0, 0, 0, 0);
    s1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.y, b4.y, s1, 0, 0, 0);
    s2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.z, b4.z, s2, 0, 0, 0);
    s3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a4.w, b4.w, s3, 0, 0, 0);
  }
  tile_store((s0 + s1) + (s2 + s3), part + ((size_t)z * rows_p + m0) * dp + k0, dp, lane);
}

// dH = (sum_z part[z], in order) where H > 0, else 0
__global__ void ae_dh_finish(const float *part, int nsplit, size_t n, const float *H,
                             float *dH) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = part[e];
  for (int z = 1; z < nsplit; z++) s += part[(size_t)z * n + e];
  dH[e] = H[e] > 0.f ? s : 0.f;
}

// ---- bias, softmax, loss and dZ of one row, in place ----------------------
__device__ __forceinline__ float block_sum(float x, float *sh) {
  x = hgx::group_allreduce_sum<64>(x);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = x;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ float block_max(float x, float *sh) {
  x = hgx::wave_max(x);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = x;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
// One workgroup per row of the chunk, four passes over its columns (float4
// per thread). With yt the clipped target (1 / n on the row's support, 1e-7
// elsewhere), pc = max(p, 1e-7), u = [p >= 1e-7] and T = sum_c u_c yt_c:
//   loss = sum_c yt log(yt / pc),
//   dZ_c = (p_c T - u_c yt_c) / M  (the softmax Jacobian applied to
//   dL/dp_c = -u_c yt_c / pc_c, with p_c / pc_c = 1 wherever u_c = 1).
// The third pass stores p and treats every column as off the support; the
// threads then walk the CSR row, move the row's n columns to the support's
// side of the loss and of the two counts T is made of (T = 1e-7 #{u, off} +
// #{u, on} / n: exact counts, no long sum), and mark them by the sign of the
// stored p (p >= 0, and -0 keeps the mark), which the last pass reads: the
// target is never looked up per column.
__global__ __launch_bounds__(256) void ae_softmax(float *Z, int rows, int C, int Cp,
                                                  const float *b2, const int *s_row,
                                                  const int *rp, const int *col, float invM,
                                                  float *lossrow) {
  __shared__ float sh[4];
  __shared__ int cnt[2];
  const int m = blockIdx.x, t = threadIdx.x;
  float *z = Z + (size_t)m * Cp;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (m >= rows) {
    for (int c = 4 * t; c < Cp; c += 1024) *reinterpret_cast<float4 *>(z + c) = zero4;
    return;
  }
  if (t < 2) cnt[t] = 0;
  const int r = s_row[m], b = rp[r], n = rp[r + 1] - b;
  const int *cs = col + b;
  const float yon = 1.0f / (float)n;
  float mx = -INFINITY;
  for (int c = 4 * t; c < Cp; c += 1024) {
    const float4 v = *reinterpret_cast<const float4 *>(z + c);
    const float4 bb = *reinterpret_cast<const float4 *>(b2 + c);
    const float x[4] = {v.x + bb.x, v.y + bb.y, v.z + bb.z, v.w + bb.w};
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (c + e < C) mx = fmaxf(mx, x[e]);
  }
  mx = block_max(mx, sh);
  float sm = 0.f;
  for (int c = 4 * t; c < Cp; c += 1024) {
    const float4 v = *reinterpret_cast<const float4 *>(z + c);
    const float4 bb = *reinterpret_cast<const float4 *>(b2 + c);
    const float x[4] = {v.x + bb.x, v.y + bb.y, v.z + bb.z, v.w + bb.w};
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (c + e < C) sm += expf(x[e] - mx);
  }
  sm = block_sum(sm, sh);
  const float lk = logf(kKeps);
  float ls = 0.f;
  int ca = 0, co = 0;
  for (int c = 4 * t; c < Cp; c += 1024) {
    const float4 v = *reinterpret_cast<const float4 *>(z + c);
    const float4 bb = *reinterpret_cast<const float4 *>(b2 + c);
    const float x[4] = {v.x + bb.x, v.y + bb.y, v.z + bb.z, v.w + bb.w};
    float p[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      p[e] = 0.f;
      if (c + e < C) {
        p[e] = expf(x[e] - mx) / sm;
        if (p[e] >= kKeps) {
          ca++;
          ls += kKeps * (lk - logf(p[e]));
        }  // else pc = 1e-7: the term is 1e-7 log(1) = 0
      }
    }
    *reinterpret_cast<float4 *>(z + c) = make_float4(p[0], p[1], p[2], p[3]);
  }
  __syncthreads();  // every p of the row is stored
  for (int j = t; j < n; j += 256) {
    const int c = cs[j];
    const float p = z[c];
    const float pc = p < kKeps ? kKeps : p;
    if (p >= kKeps) {
      co++;
      ls -= kKeps * (lk - logf(p));
    }
    ls += yon * logf(yon / pc);
    z[c] = -p;
  }
  atomicAdd(&cnt[0], ca);
  atomicAdd(&cnt[1], co);
  ls = block_sum(ls, sh);  // its barriers also order the marks and the counts
  if (t == 0) lossrow[m] = ls;
  const int con = cnt[1], coff = cnt[0] - con;
  const float T = kKeps * (float)coff + yon * (float)con;
  for (int c = 4 * t; c < Cp; c += 1024) {
    const float4 v = *reinterpret_cast<const float4 *>(z + c);
    const float x[4] = {v.x, v.y, v.z, v.w};
    float dz[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const float p = fabsf(x[e]);
      const float yt = (__float_as_uint(x[e]) >> 31) ? yon : kKeps;
      dz[e] = c + e < C ? (p * T - (p >= kKeps ? yt : 0.f)) * invM : 0.f;
    }
    *reinterpret_cast<float4 *>(z + c) = make_float4(dz[0], dz[1], dz[2], dz[3]);
  }
}

// ---- column sums in two fixed-order levels --------------------------------
__global__ void ae_colsum_part(const float *X, int rows, size_t ld, int cols, float *part) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, sg = blockIdx.y;
  if (c >= cols) return;
  const int r1 = min(rows, (sg + 1) * kSeg);
  float s = 0.f;
  for (int r = sg * kSeg; r < r1; r++) s += X[(size_t)r * ld + c];
  part[(size_t)sg * cols + c] = s;
}
__global__ void ae_colsum_fin(const float *part, int nseg, int cols, float *out, int first) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float s = part[c];
  for (int sg = 1; sg < nseg; sg++) s += part[(size_t)sg * cols + c];
  out[c] = first ? s : out[c] + s;
}

// ---- Adagrad --------------------------------------------------------------
__device__ __forceinline__ void adagrad1(float &p, float &a, float g, float lr, float eps) {
  a = a + g * g;
  p = p - lr * g / (sqrtf(a) + eps);
}
__global__ void ae_adagrad(float *p, float *a, const float *g, size_t n, float lr,
                           float eps) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float pv = p[e], av = a[e];
  adagrad1(pv, av, g[e], lr, eps);
  p[e] = pv;
  a[e] = av;
}

// One wave per column c of the model's input: gW1[c] = sum over the rows r of
// the transposed CSR row of c that are in the batch (grp[r].x >= 0), in that
// order, over r's samples in list order, drop != c, of v_m dH_m; then Adagrad
// on row c. A column no batch row holds is left alone (its gradient is 0).
template <int NPL>
__global__ __launch_bounds__(256) void ae_w1_update(int C, const int *rpT, const int *colT,
                                                    const int *rp, const int2 *grp,
                                                    const int *s_ord, const int *s_drop,
                                                    const float *dH, float *W1, float *aW1,
                                                    int dp, float lr, float eps) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;
  float g[NPL];
#pragma unroll
  for (int q = 0; q < NPL; q++) g[q] = 0.f;
  bool touched = false;
  const int e1 = rpT[c + 1];
  for (int e = rpT[c]; e < e1; e++) {
    const int r = colT[e];
    const int2 gr = grp[r];
    if (gr.x < 0) continue;
    touched = true;
    const int n = rp[r + 1] - rp[r];
    for (int s = 0; s < gr.y; s++) {
      const int m = s_ord[gr.x + s], drop = s_drop[m];
      if (drop == c) continue;
      const float v = sample_v(n, drop);
      const float *dh = dH + (size_t)m * dp;
#pragma unroll
      for (int q = 0; q < NPL; q++) g[q] += v * dh[lane + 64 * q];
    }
  }
  if (!touched) return;
#pragma unroll
  for (int q = 0; q < NPL; q++) {
    const size_t e = (size_t)c * dp + lane + 64 * q;
    float pv = W1[e], av = aW1[e];
    adagrad1(pv, av, g[q], lr, eps);
    W1[e] = pv;
    aW1[e] = av;
  }
}

// batch loss = (sum of the row losses, fixed order, float64) / M
__global__ __launch_bounds__(256) void ae_loss_fin(const float *lossrow, int M, float *out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) s += (double)lossrow[m];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = (float)(sh[0] / (double)M);
}

}  // namespace

struct hgx_ae {
  hgx_ctx *ctx = nullptr;
  int side = 0, R = 0, C = 0, d = 0, dp = 0, Cp = 0;
  uint64_t inc_gen = 0;
  const int *rp = nullptr, *col = nullptr, *rpT = nullptr, *colT = nullptr;
  std::vector<int32_t> h_rp, h_col;  // host copy: preconditions, batch sizes
  DevBuf W1, b1, W2, b2, aW1, ab1, aW2, ab2, gW2, gb2, gb1;
  DevBuf s_row, s_drop, s_ord, grp, urow, ustart, ucnt;
  DevBuf H, dH, Z, part, lossrow, cpart, bloss, perm, soff, rows_d;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double ms = 0, flops = 0;
  int64_t samples = 0, batches = 0;
};

namespace {

size_t w1_n(const hgx_ae *a) { return (size_t)a->C * a->dp; }
size_t w2_n(const hgx_ae *a) { return (size_t)a->dp * a->Cp; }

int ae_live(hgx_ae *a) {
  hgx_ctx *ctx = a->ctx;
  HGX_CHECK(ctx, a->inc_gen == ctx->inc_gen, HGX_ESTATE,
            "the incidence changed after hgx_ae_create");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  return HGX_OK;
}

// samples of a row: the unperturbed one and min(n, spi) drops when n > 1
inline int row_samples(const hgx_ae *a, int r, int spi) {
  const int n = a->h_rp[r + 1] - a->h_rp[r];
  return 1 + (n > 1 ? std::min(n, spi) : 0);
}

// rows per chunk: the tuning value, else what half of the free memory holds
int chunk_rows(hgx_ae *a, int M, int *out) {
  hgx_ctx *ctx = a->ctx;
  const int Mp = round_up(M, 32);
  int ch = ctx->tune.ae_chunk_rows;
  if (ch > 0) {
    *out = std::min(round_up(ch, 32), Mp);
    return HGX_OK;
  }
  ch = std::min(Mp, kMaxChunk);
  const size_t nsplit = (size_t)(a->Cp + kSplit - 1) / kSplit;
  const size_t per_row = sizeof(float) * ((size_t)a->Cp + nsplit * a->dp);
  if (a->Z.bytes < per_row * ch) {  // the buffers have to grow: ask the device
    size_t fr = 0, tot = 0;
    HGX_HIP(ctx, hipMemGetInfo(&fr, &tot));
    fr += a->Z.bytes + a->part.bytes;
    const size_t fit = fr / 2 / per_row / 32 * 32;
    HGX_CHECK(ctx, fit >= 32, HGX_EUNSUP,
              "auto-encoder: a chunk of 32 rows (%zu bytes) does not fit into half of the "
              "%zu free bytes", per_row * 32, fr);
    ch = (int)std::min<size_t>(ch, fit);
  }
  *out = ch;
  return HGX_OK;
}

int launch_encode(hgx_ae *a, int M, int Mp, const int *s_row, const int *s_drop, float *H) {
  hgx_ctx *ctx = a->ctx;
  const dim3 g((Mp + 3) / 4), b(256);
#define HGX_AE_ENC(N)                                                              \
  hipLaunchKernelGGL(ae_encode<N>, g, b, 0, ctx->stream, M, Mp, s_row, s_drop, a->rp, \
                     a->col, a->W1.as<float>(), a->b1.as<float>(), H, a->dp)
  switch (a->dp / 64) {
    case 1: HGX_AE_ENC(1); break;
    case 2: HGX_AE_ENC(2); break;
    case 4: HGX_AE_ENC(4); break;
    default: HGX_AE_ENC(8); break;
  }
#undef HGX_AE_ENC
  HGX_LAUNCH_CHECK(ctx);
  return HGX_OK;
}

int launch_w1(hgx_ae *a, float lr, float eps) {
  hgx_ctx *ctx = a->ctx;
  const dim3 g((a->C + 3) / 4), b(256);
#define HGX_AE_W1(N)                                                                 \
  hipLaunchKernelGGL(ae_w1_update<N>, g, b, 0, ctx->stream, a->C, a->rpT, a->colT, a->rp, \
                     a->grp.as<int2>(), a->s_ord.as<int>(), a->s_drop.as<int>(),       \
                     a->dH.as<float>(), a->W1.as<float>(), a->aW1.as<float>(), a->dp, lr, eps)
  switch (a->dp / 64) {
    case 1: HGX_AE_W1(1); break;
    case 2: HGX_AE_W1(2); break;
    case 4: HGX_AE_W1(4); break;
    default: HGX_AE_W1(8); break;
  }
#undef HGX_AE_W1
  HGX_LAUNCH_CHECK(ctx);
  return HGX_OK;
}

int colsum(hgx_ae *a, const float *X, int rows, size_t ld, int cols, float *out, int first) {
  hgx_ctx *ctx = a->ctx;
  const int nseg = (rows + kSeg - 1) / kSeg;
  HGX_TRY(hgx_ensure(ctx, a->cpart, sizeof(float) * (size_t)nseg * cols));
  hipLaunchKernelGGL(ae_colsum_part, dim3((cols + 255) / 256, nseg), dim3(256), 0, ctx->stream,
                     X, rows, ld, cols, a->cpart.as<float>());
  HGX_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(ae_colsum_fin, dim3((cols + 255) / 256), dim3(256), 0, ctx->stream,
                     a->cpart.as<float>(), nseg, cols, out, first);
  HGX_LAUNCH_CHECK(ctx);
  return HGX_OK;
}

int adagrad(hgx_ae *a, DevBuf &p, DevBuf &acc, DevBuf &g, size_t n, float lr, float eps) {
  hipLaunchKernelGGL(ae_adagrad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     a->ctx->stream, p.as<float>(), acc.as<float>(), g.as<float>(), n, lr, eps);
  HGX_LAUNCH_CHECK(a->ctx);
  return HGX_OK;
}

// sample-list buffers for M samples; activations for their padded rows
int ensure_batch(hgx_ae *a, int M) {
  hgx_ctx *ctx = a->ctx;
  const size_t Mp = round_up(M, 32);
  for (DevBuf *b : {&a->s_row, &a->s_drop, &a->s_ord})
    HGX_TRY(hgx_ensure(ctx, *b, sizeof(int) * Mp));
  HGX_TRY(hgx_ensure(ctx, a->H, sizeof(float) * Mp * a->dp));
  HGX_TRY(hgx_ensure(ctx, a->dH, sizeof(float) * Mp * a->dp));
  HGX_TRY(hgx_ensure(ctx, a->lossrow, sizeof(float) * Mp));
  return HGX_OK;
}

// One train_on_batch on the M samples in s_row / s_drop / s_ord with grp set
// for their rows; the batch loss goes to *loss_dev. Every launch is queued on
// the context's stream; grp is cleared again at the end.
int run_batch(hgx_ae *a, int M, int chunk, float lr, float eps, float *loss_dev) {
  hgx_ctx *ctx = a->ctx;
  const int Mp = round_up(M, 32), dp = a->dp, Cp = a->Cp;
  const int nsplit = (Cp + kSplit - 1) / kSplit;
  HGX_TRY(hgx_ensure(ctx, a->Z, sizeof(float) * (size_t)chunk * Cp));
  HGX_TRY(hgx_ensure(ctx, a->part, sizeof(float) * (size_t)nsplit * chunk * dp));
  float *H = a->H.as<float>(), *dH = a->dH.as<float>(), *Z = a->Z.as<float>();
  const int *s_row = a->s_row.as<int>();
  HGX_TRY(launch_encode(a, M, Mp, s_row, a->s_drop.as<int>(), H));
  const float invM = 1.0f / (float)M;
  for (int m0 = 0; m0 < M; m0 += chunk) {
    const int rows = std::min(chunk, M - m0), rows_p = round_up(rows, 32);
    const int first = m0 == 0;
    const float *Hc = H + (size_t)m0 * dp;
    hipLaunchKernelGGL(ae_logits, dim3((Cp / 32 + 3) / 4, rows_p / 32), dim3(256), 0,
                       ctx->stream, Hc, a->W2.as<float>(), Z, dp, Cp);
    HGX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(ae_softmax, dim3(rows_p), dim3(256), 0, ctx->stream, Z, rows, a->C, Cp,
                       a->b2.as<float>(), s_row + m0, a->rp, a->col, invM,
                       a->lossrow.as<float>() + m0);
    HGX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(ae_wgrad2, dim3((Cp / 32 + 3) / 4, dp / 32), dim3(256), 0, ctx->stream,
                       Hc, Z, a->gW2.as<float>(), rows_p, dp, Cp, first);
    HGX_LAUNCH_CHECK(ctx);
    HGX_TRY(colsum(a, Z, rows_p, (size_t)Cp, Cp, a->gb2.as<float>(), first));
    hipLaunchKernelGGL(ae_dh, dim3(rows_p / 32, dp / 32, nsplit), dim3(64), 0, ctx->stream, Z,
                       a->W2.as<float>(), a->part.as<float>(), rows_p, dp, Cp);
    HGX_LAUNCH_CHECK(ctx);
    const size_t ne = (size_t)rows_p * dp;
    hipLaunchKernelGGL(ae_dh_finish, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                       ctx->stream, a->part.as<float>(), nsplit, ne, Hc, dH + (size_t)m0 * dp);
    HGX_LAUNCH_CHECK(ctx);
  }
  HGX_TRY(colsum(a, dH, Mp, (size_t)dp, dp, a->gb1.as<float>(), 1));
  HGX_TRY(launch_w1(a, lr, eps));
  HGX_TRY(adagrad(a, a->b1, a->ab1, a->gb1, (size_t)dp, lr, eps));
  HGX_TRY(adagrad(a, a->W2, a->aW2, a->gW2, w2_n(a), lr, eps));
  HGX_TRY(adagrad(a, a->b2, a->ab2, a->gb2, (size_t)Cp, lr, eps));
  hipLaunchKernelGGL(ae_loss_fin, dim3(1), dim3(256), 0, ctx->stream, a->lossrow.as<float>(), M,
                     loss_dev);
  HGX_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(ae_grp_clear, dim3((M + 255) / 256), dim3(256), 0, ctx->stream, s_row, M,
                     a->grp.as<int2>());
  HGX_LAUNCH_CHECK(ctx);
  a->samples += M;
  a->batches += 1;
  a->flops += 6.0 * (double)M * (double)a->C * (double)a->d;
  return HGX_OK;
}

int time_end(hgx_ae *a) {
  hgx_ctx *ctx = a->ctx;
  HGX_HIP(ctx, hipEventRecord(a->e1, ctx->stream));
  HGX_HIP(ctx, hipEventSynchronize(a->e1));
  float ms = 0.f;
  HGX_HIP(ctx, hipEventElapsedTime(&ms, a->e0, a->e1));
  a->ms += ms;
  return HGX_OK;
}

int upload_ints(hgx_ae *a, DevBuf &b, const std::vector<int32_t> &v) {
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(hgx_ensure(ctx, b, sizeof(int32_t) * std::max<size_t>(v.size(), 1)));
  if (!v.empty())
    HGX_HIP(ctx, hipMemcpyAsync(b.p, v.data(), sizeof(int32_t) * v.size(),
                                hipMemcpyHostToDevice, ctx->stream));
  return HGX_OK;
}

int check_rows(hgx_ae *a, int64_t n, const int32_t *rows, const char *what) {
  for (int64_t i = 0; i < n; i++) {
    HGX_CHECK(a->ctx, rows[i] >= 0 && rows[i] < a->R, HGX_EINVAL,
              "%s: row %d at position %lld outside [0, %d)", what, rows[i], (long long)i, a->R);
    HGX_CHECK(a->ctx, a->h_rp[rows[i] + 1] > a->h_rp[rows[i]], HGX_EINVAL,
              "%s: row %d has no column", what, rows[i]);
  }
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_ae_destroy(hgx_ae *a) {
  if (!a) return HGX_OK;
  if (a->ctx) hipStreamSynchronize(a->ctx->stream);
  for (DevBuf *b : {&a->W1, &a->b1, &a->W2, &a->b2, &a->aW1, &a->ab1, &a->aW2, &a->ab2,
                    &a->gW2, &a->gb2, &a->gb1, &a->s_row, &a->s_drop, &a->s_ord, &a->grp,
                    &a->urow, &a->ustart, &a->ucnt, &a->H, &a->dH, &a->Z, &a->part,
                    &a->lossrow, &a->cpart, &a->bloss, &a->perm, &a->soff, &a->rows_d})
    hgx_release(*b);
  for (hipEvent_t e : {a->e0, a->e1})
    if (e) hipEventDestroy(e);
  delete a;
  return HGX_OK;
}

static int ae_alloc(hgx_ae *a) {
  hgx_ctx *ctx = a->ctx;
  const size_t n1 = w1_n(a), n2 = w2_n(a);
  // W1 and W2 with their accumulators, gW2, the biases, the row groups
  const size_t fixed = sizeof(float) * (2 * n1 + 3 * n2 + 3 * (size_t)a->Cp + 3 * (size_t)a->dp) +
                       sizeof(int2) * (size_t)a->R;
  const size_t nsplit = (size_t)(a->Cp + kSplit - 1) / kSplit;
  const size_t chunk32 = sizeof(float) * 32 * ((size_t)a->Cp + nsplit * a->dp);
  size_t fr = 0, tot = 0;
  HGX_HIP(ctx, hipMemGetInfo(&fr, &tot));
  HGX_CHECK(ctx, fixed + 2 * chunk32 <= fr, HGX_EUNSUP,
            "auto-encoder %d x %d at d = %d: weights, accumulators and gradients (%zu bytes) "
            "with the smallest chunk (%zu bytes) exceed the %zu free bytes",
            a->R, a->C, a->d, fixed, chunk32, fr);
  for (DevBuf *b : {&a->W1, &a->aW1}) HGX_TRY(hgx_ensure(ctx, *b, sizeof(float) * n1));
  for (DevBuf *b : {&a->W2, &a->aW2, &a->gW2}) HGX_TRY(hgx_ensure(ctx, *b, sizeof(float) * n2));
  for (DevBuf *b : {&a->b2, &a->ab2, &a->gb2})
    HGX_TRY(hgx_ensure(ctx, *b, sizeof(float) * (size_t)a->Cp));
  for (DevBuf *b : {&a->b1, &a->ab1, &a->gb1})
    HGX_TRY(hgx_ensure(ctx, *b, sizeof(float) * (size_t)a->dp));
  HGX_TRY(hgx_ensure(ctx, a->grp, sizeof(int2) * (size_t)a->R));
  for (DevBuf *b : {&a->W1, &a->aW1, &a->W2, &a->aW2, &a->gW2, &a->b2, &a->ab2, &a->gb2, &a->b1,
                    &a->ab1, &a->gb1})
    HGX_HIP(ctx, hipMemsetAsync(b->p, 0, b->bytes, ctx->stream));
  HGX_HIP(ctx, hipMemsetAsync(a->grp.p, 0xFF, a->grp.bytes, ctx->stream));  // {-1, -1}
  HGX_HIP(ctx, hipEventCreate(&a->e0));
  HGX_HIP(ctx, hipEventCreate(&a->e1));
  const int64_t nnz = ctx->nnz;
  a->h_rp.resize((size_t)a->R + 1);
  a->h_col.resize((size_t)nnz);
  HGX_HIP(ctx, hipMemcpyAsync(a->h_rp.data(), a->rp, sizeof(int32_t) * a->h_rp.size(),
                              hipMemcpyDeviceToHost, ctx->stream));
  if (nnz)
    HGX_HIP(ctx, hipMemcpyAsync(a->h_col.data(), a->col, sizeof(int32_t) * (size_t)nnz,
                                hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_ae_create(hgx_ctx *ctx, int side, int dim, hgx_ae **out) {
  if (!ctx || !out) return HGX_EINVAL;
  *out = nullptr;
  HGX_CHECK(ctx, ctx->N > 0 && ctx->E > 0 && ctx->rp_n.p && ctx->rp_e.p, HGX_ESTATE,
            "hgx_ae_create before hgx_upload_incidence");
  HGX_CHECK(ctx, side == 0 || side == 1, HGX_EINVAL, "side %d is not 0 (node rows) or 1 "
            "(edge rows)", side);
  HGX_CHECK(ctx, dim >= 1, HGX_EINVAL, "dimension %d < 1", dim);
  HGX_CHECK(ctx, dim <= kMaxD, HGX_EUNSUP, "auto-encoder dimension %d above %d", dim, kMaxD);
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  hgx_ae *a = new hgx_ae();
  a->ctx = ctx;
  a->side = side;
  a->R = side ? ctx->E : ctx->N;
  a->C = side ? ctx->N : ctx->E;
  a->d = dim;
  a->dp = 64;  // 64, 128, 256 or 512: 1, 2, 4 or 8 columns per lane
  while (a->dp < dim) a->dp *= 2;
  a->Cp = round_up(a->C, 32);
  a->inc_gen = ctx->inc_gen;
  a->rp = (side ? ctx->rp_e : ctx->rp_n).as<int>();
  a->col = (side ? ctx->col_e : ctx->col_n).as<int>();
  a->rpT = (side ? ctx->rp_n : ctx->rp_e).as<int>();
  a->colT = (side ? ctx->col_n : ctx->col_e).as<int>();
  const int rc = ae_alloc(a);
  if (rc) {
    hgx_ae_destroy(a);
    return rc;
  }
  *out = a;
  return HGX_OK;
}

// flat host layout: W1 (C x d), b1 (d), W2 (d x C), b2 (C)
static int ae_weights_io(hgx_ae *a, float *flat, bool set) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(ae_live(a));
  HGX_CHECK(ctx, flat, HGX_EINVAL, "null weight array");
  const size_t d = a->d, C = a->C, fs = sizeof(float);
  float *hW1 = flat, *hb1 = hW1 + C * d, *hW2 = hb1 + d, *hb2 = hW2 + d * C;
  const hipMemcpyKind kind = set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
  struct { float *dev; size_t ldd; float *host; size_t w, h; } v[4] = {
      {a->W1.as<float>(), (size_t)a->dp, hW1, d, C},
      {a->b1.as<float>(), (size_t)a->dp, hb1, d, 1},
      {a->W2.as<float>(), (size_t)a->Cp, hW2, C, d},
      {a->b2.as<float>(), (size_t)a->Cp, hb2, C, 1}};
  if (set) {
    for (DevBuf *b : {&a->W1, &a->aW1, &a->W2, &a->aW2, &a->b2, &a->ab2, &a->b1, &a->ab1})
      HGX_HIP(ctx, hipMemsetAsync(b->p, 0, b->bytes, ctx->stream));
  }
  for (auto &t : v) {
    if (set)
      HGX_HIP(ctx, hipMemcpy2DAsync(t.dev, fs * t.ldd, t.host, fs * t.w, fs * t.w, t.h, kind,
                                    ctx->stream));
    else
      HGX_HIP(ctx, hipMemcpy2DAsync(t.host, fs * t.w, t.dev, fs * t.ldd, fs * t.w, t.h, kind,
                                    ctx->stream));
  }
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_ae_set_weights(hgx_ae *a, const float *flat) {
  return ae_weights_io(a, const_cast<float *>(flat), true);
}
extern "C" int hgx_ae_get_weights(hgx_ae *a, float *flat) {
  return ae_weights_io(a, flat, false);
}

extern "C" int hgx_ae_draw(hgx_ae *a, int64_t n_idx, const int32_t *rows, int samples_per_idx,
                           uint64_t seed, int epoch, int64_t *n, int32_t *row_out,
                           int32_t *drop_out) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(ae_live(a));
  HGX_CHECK(ctx, n_idx >= 0 && (n_idx == 0 || rows) && n, HGX_EINVAL, "hgx_ae_draw: null list");
  HGX_CHECK(ctx, samples_per_idx >= 0 && epoch >= 0, HGX_EINVAL,
            "hgx_ae_draw: samples_per_idx %d or epoch %d negative", samples_per_idx, epoch);
  HGX_TRY(check_rows(a, n_idx, rows, "hgx_ae_draw"));
  std::vector<int32_t> soff((size_t)n_idx), rv(rows, rows + n_idx);
  int64_t tot = 0;
  for (int64_t i = 0; i < n_idx; i++) {
    soff[i] = (int32_t)tot;
    tot += row_samples(a, rows[i], samples_per_idx);
    HGX_CHECK(ctx, tot < (1ll << 31), HGX_EUNSUP, "hgx_ae_draw: more than 2^31 samples");
  }
  *n = tot;
  if (!row_out || !drop_out || tot == 0) return HGX_OK;
  HGX_TRY(ensure_batch(a, (int)tot));
  HGX_TRY(upload_ints(a, a->rows_d, rv));
  HGX_TRY(upload_ints(a, a->soff, soff));
  hipLaunchKernelGGL(ae_draw, dim3((unsigned)((n_idx + 63) / 64)), dim3(64), 0, ctx->stream,
                     a->rows_d.as<int>(), (int)n_idx, a->soff.as<int>(), a->rp, a->col,
                     samples_per_idx, seed, (uint32_t)epoch, a->s_row.as<int>(),
                     a->s_drop.as<int>(), a->s_ord.as<int>(), (int2 *)nullptr);
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipMemcpyAsync(row_out, a->s_row.p, sizeof(int32_t) * (size_t)tot,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(drop_out, a->s_drop.p, sizeof(int32_t) * (size_t)tot,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_ae_step(hgx_ae *a, int64_t n, const int32_t *row, const int32_t *drop,
                           float lr, float eps, float *loss) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(ae_live(a));
  HGX_CHECK(ctx, n >= 1 && n < (1ll << 31) && row && drop, HGX_EINVAL,
            "hgx_ae_step: empty or null sample list");
  HGX_TRY(check_rows(a, n, row, "hgx_ae_step"));
  for (int64_t m = 0; m < n; m++) {
    if (drop[m] < 0) {
      HGX_CHECK(ctx, drop[m] == -1, HGX_EINVAL, "hgx_ae_step: drop %d at sample %lld", drop[m],
                (long long)m);
      continue;
    }
    const int32_t *b = a->h_col.data() + a->h_rp[row[m]], *e = a->h_col.data() + a->h_rp[row[m] + 1];
    HGX_CHECK(ctx, e - b > 1, HGX_EINVAL,
              "hgx_ae_step: sample %lld drops a column of row %d, which has one column",
              (long long)m, row[m]);
    HGX_CHECK(ctx, std::binary_search(b, e, drop[m]), HGX_EINVAL,
              "hgx_ae_step: sample %lld drops column %d, which row %d does not hold",
              (long long)m, drop[m], row[m]);
  }
  const int M = (int)n;
  // the samples of one row form one group (list order kept inside it)
  std::vector<int32_t> ord((size_t)M), urow, ustart, ucnt;
  for (int m = 0; m < M; m++) ord[m] = m;
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return row[x] < row[y]; });
  for (int i = 0; i < M; i++) {
    if (i == 0 || row[ord[i]] != row[ord[i - 1]]) {
      urow.push_back(row[ord[i]]);
      ustart.push_back(i);
      ucnt.push_back(0);
    }
    ucnt.back()++;
  }
  int chunk = 0;
  HGX_TRY(chunk_rows(a, M, &chunk));
  HGX_TRY(ensure_batch(a, M));
  HGX_TRY(hgx_ensure(ctx, a->bloss, sizeof(float)));
  HGX_HIP(ctx, hipMemcpyAsync(a->s_row.p, row, sizeof(int32_t) * (size_t)M, hipMemcpyHostToDevice,
                              ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(a->s_drop.p, drop, sizeof(int32_t) * (size_t)M,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_TRY(upload_ints(a, a->s_ord, ord));
  HGX_TRY(upload_ints(a, a->urow, urow));
  HGX_TRY(upload_ints(a, a->ustart, ustart));
  HGX_TRY(upload_ints(a, a->ucnt, ucnt));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  const int nu = (int)urow.size();
  hipLaunchKernelGGL(ae_grp_set, dim3((nu + 255) / 256), dim3(256), 0, ctx->stream,
                     a->urow.as<int>(), a->ustart.as<int>(), a->ucnt.as<int>(), nu,
                     a->grp.as<int2>());
  HGX_LAUNCH_CHECK(ctx);
  a->ms = a->flops = 0;
  a->samples = a->batches = 0;
  HGX_TRY(run_batch(a, M, chunk, lr, eps, a->bloss.as<float>()));
  HGX_TRY(time_end(a));
  float l = 0.f;
  HGX_HIP(ctx, hipMemcpy(&l, a->bloss.p, sizeof(float), hipMemcpyDeviceToHost));
  if (loss) *loss = l;
  return HGX_OK;
}

extern "C" int hgx_ae_fit(hgx_ae *a, int epochs, int idx_per_batch, int samples_per_idx,
                          float lr, float eps, uint64_t seed, const int64_t *perms,
                          float *batch_loss, int *n_batches) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(ae_live(a));
  HGX_CHECK(ctx, epochs >= 0 && idx_per_batch >= 1 && samples_per_idx >= 0, HGX_EINVAL,
            "hgx_ae_fit: epochs %d, idx_per_batch %d or samples_per_idx %d out of range",
            epochs, idx_per_batch, samples_per_idx);
  const int R = a->R;
  for (int r = 0; r < R; r++)
    HGX_CHECK(ctx, a->h_rp[r + 1] > a->h_rp[r], HGX_EINVAL, "hgx_ae_fit: row %d has no column",
              r);
  // np.array_split(perm, s): the first R mod s sections hold one row more
  const int s = std::max(1, R / idx_per_batch), base = R / s, extra = R % s;
  if (n_batches) *n_batches = epochs * s;
  if (epochs == 0) return HGX_OK;
  HGX_CHECK(ctx, batch_loss, HGX_EINVAL, "hgx_ae_fit: null batch_loss");
  std::vector<int32_t> perm((size_t)epochs * R), soff((size_t)epochs * R);
  std::vector<int32_t> bM((size_t)epochs * s);
  std::vector<char> seen;
  int maxM = 0;
  for (int ep = 0; ep < epochs; ep++) {
    int32_t *p = perm.data() + (size_t)ep * R;
    if (perms) {
      seen.assign((size_t)R, 0);
      for (int i = 0; i < R; i++) {
        const int64_t r = perms[(size_t)ep * R + i];
        HGX_CHECK(ctx, r >= 0 && r < R && !seen[(size_t)r], HGX_EINVAL,
                  "hgx_ae_fit: perms row %d is not a permutation of [0, %d) at position %d",
                  ep, R, i);
        seen[(size_t)r] = 1;
        p[i] = (int32_t)r;
      }
    } else {
      // the library's shuffle: rows ordered by their counter-based keys
      std::vector<std::pair<uint64_t, int32_t>> kv((size_t)R);
      const uint64_t key = hgx::rand64_key(seed, 0x5aeull << 32 | (uint32_t)ep);
      for (int i = 0; i < R; i++) kv[i] = {hgx::mix64(key + (uint64_t)i), i};
      std::sort(kv.begin(), kv.end());
      for (int i = 0; i < R; i++) p[i] = kv[i].second;
    }
    int i = 0;
    for (int b = 0; b < s; b++) {
      const int len = base + (b < extra ? 1 : 0);
      int64_t tot = 0;
      for (int j = 0; j < len; j++, i++) {
        soff[(size_t)ep * R + i] = (int32_t)tot;
        tot += row_samples(a, p[i], samples_per_idx);
        HGX_CHECK(ctx, tot < (1ll << 31), HGX_EUNSUP, "hgx_ae_fit: a batch of 2^31 samples");
      }
      bM[(size_t)ep * s + b] = (int32_t)tot;
      maxM = std::max(maxM, (int)tot);
    }
  }
  int chunk = 0;
  HGX_TRY(chunk_rows(a, maxM, &chunk));
  HGX_TRY(ensure_batch(a, maxM));
  {  // every buffer at its largest now: no allocation between the batches
    const size_t nsplit = (size_t)(a->Cp + kSplit - 1) / kSplit;
    const size_t seg_c = (size_t)(chunk + kSeg - 1) / kSeg * a->Cp;
    const size_t seg_m = (size_t)(round_up(maxM, 32) + kSeg - 1) / kSeg * a->dp;
    HGX_TRY(hgx_ensure(ctx, a->Z, sizeof(float) * (size_t)chunk * a->Cp));
    HGX_TRY(hgx_ensure(ctx, a->part, sizeof(float) * nsplit * chunk * a->dp));
    HGX_TRY(hgx_ensure(ctx, a->cpart, sizeof(float) * std::max(seg_c, seg_m)));
  }
  HGX_TRY(hgx_ensure(ctx, a->bloss, sizeof(float) * (size_t)epochs * s));
  HGX_TRY(upload_ints(a, a->perm, perm));
  HGX_TRY(upload_ints(a, a->soff, soff));
  a->ms = a->flops = 0;
  a->samples = a->batches = 0;
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  for (int ep = 0; ep < epochs; ep++) {
    int i = 0;
    for (int b = 0; b < s; b++) {
      const int len = base + (b < extra ? 1 : 0);
      const size_t o = (size_t)ep * R + i;
      const int M = bM[(size_t)ep * s + b];
      i += len;
      if (len == 0) {  // R < s cannot happen (s <= R), kept for a zero-row side
        continue;
      }
      hipLaunchKernelGGL(ae_draw, dim3((len + 63) / 64), dim3(64), 0, ctx->stream,
                         a->perm.as<int>() + o, len, a->soff.as<int>() + o, a->rp, a->col,
                         samples_per_idx, seed, (uint32_t)ep, a->s_row.as<int>(),
                         a->s_drop.as<int>(), a->s_ord.as<int>(), a->grp.as<int2>());
      HGX_LAUNCH_CHECK(ctx);
      HGX_TRY(run_batch(a, M, std::min(chunk, round_up(M, 32)), lr, eps,
                        a->bloss.as<float>() + (size_t)ep * s + b));
    }
  }
  HGX_TRY(time_end(a));
  HGX_HIP(ctx, hipMemcpy(batch_loss, a->bloss.p, sizeof(float) * (size_t)epochs * s,
                         hipMemcpyDeviceToHost));
  return HGX_OK;
}

extern "C" int hgx_ae_encode(hgx_ae *a, int64_t n, const int32_t *rows, float *out) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(ae_live(a));
  HGX_CHECK(ctx, n >= 0 && n < (1ll << 31) && (n == 0 || (rows && out)), HGX_EINVAL,
            "hgx_ae_encode: null list or output");
  HGX_TRY(check_rows(a, n, rows, "hgx_ae_encode"));
  if (n == 0) return HGX_OK;
  const std::vector<int32_t> rv(rows, rows + n);
  HGX_TRY(upload_ints(a, a->rows_d, rv));
  const int M = (int)n;
  HGX_TRY(hgx_ensure(ctx, a->H, sizeof(float) * (size_t)round_up(M, 32) * a->dp));
  HGX_TRY(launch_encode(a, M, M, a->rows_d.as<int>(), nullptr, a->H.as<float>()));
  HGX_HIP(ctx, hipMemcpy2DAsync(out, sizeof(float) * a->d, a->H.p, sizeof(float) * a->dp,
                                sizeof(float) * a->d, (size_t)M, hipMemcpyDeviceToHost,
                                ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_ae_last_stats(const hgx_ae *a, double *ms, int64_t *samples,
                                 int64_t *batches, double *flops) {
  if (!a) return HGX_EINVAL;
  if (ms) *ms = a->ms;
  if (samples) *samples = a->samples;
  if (batches) *batches = a->batches;
  if (flops) *flops = a->flops;
  return HGX_OK;
}
