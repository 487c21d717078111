// Batched small-problem C-SVC (RBF) for the per-edge / per-node link
// prediction classifiers (reference evaluation_util.py:286-449): many
// independent dual problems per launch, solved with libsvm's SMO (gradient
// kept incrementally, second-order working-set selection, box clipping,
// stop at m(alpha) - M(alpha) < eps), and a batched decision function.
//
// A problem is a list of rows of one float32 table with a 0/1 label each;
// s = +1 for label 1 and -1 for label 0, K(x, y) = exp(-gamma |x - y|^2)
// with |x - y|^2 summed as (x_k - y_k)^2 (the expanded form cancels in
// float32 when an edge's members sit close together). Tiers by problem size:
//   m <= 32, m <= 64  one wave per problem, four problems per workgroup; a
//                     lane owns one sample (alpha, G, s in registers), the
//                     m x m kernel matrix of the wave is in LDS (4 / 16 KiB),
//                     reductions are cross-lane, no block barrier
//   m <= 128          one workgroup per problem, kernel matrix in LDS
//                     (64 KiB: two workgroups per CU), alpha / G in LDS;
//                     tuning svc_lds_m = 192 moves the cut (144 KiB, one
//                     workgroup per CU)
//   larger            one workgroup per problem, the two kernel columns of
//                     an iteration recomputed from the table rows, alpha / G
//                     / the columns in global scratch; no cap on m
// Ties in both argmax steps resolve to the lowest sample index and every
// reduction has a fixed shape, so a problem's result does not depend on
// what else is in the launch.
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>

#include "hgx_internal.h"

struct hgx_svc {
  hgx_ctx *ctx = nullptr;
  int dim = 0, ld = 0, lanes = 1;  // ld: row stride (dim rounded up to 4)
  int64_t n_rows = 0;
  DevBuf tab;
  // the last fit
  bool fitted = false;
  int64_t n_prob = 0, n_samp = 0;
  float gamma = 0;
  std::vector<int64_t> off;
  DevBuf d_off, d_row, d_lab, d_order, d_coef, d_rho, d_iters, d_status;
  DevBuf st_alpha, st_G, st_K0, st_K1;  // recompute-tier state, one float per sample
  // decision scratch
  DevBuf q_prob, q_row, q_idx, q_out, q_vec;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double fit_ms = 0, dec_ms = 0;
};

namespace {

constexpr int kTB = 256;     // threads per workgroup
constexpr int kWaveM = 64;   // largest problem solved by one wave
constexpr int kLdsMax = 192;  // largest kernel matrix the LDS holds (144 KiB)
constexpr float kTau = 1e-12f;  // libsvm's TAU

struct FitArgs {
  const float *tab;
  int ld, lanes;
  const int64_t *off;
  const int32_t *row;
  const uint8_t *lab;
  const int32_t *order;  // problems of this launch
  int n;
  float C, gamma, eps;
  int max_iter;  // <= 0: max(10000, 100 m)
  float *coef, *rho;
  int32_t *iters, *status;
  float *st_alpha, *st_G, *st_K0, *st_K1;
};

__device__ __forceinline__ int iter_cap(int max_iter, int m) {
  if (max_iter > 0) return max_iter;
  const long long c = 100ll * m;
  return c > 10000 ? (c > INT_MAX ? INT_MAX : (int)c) : 10000;
}

// |a - b|^2 of two rows of ld floats (ld a multiple of 4, both 16-byte
// aligned) by an aligned group of L lanes (a power of two <= 16), `sub` the
// lane's place in the group; every lane of the group returns the sum.
__device__ __forceinline__ float row_dist2(const float *a, const float *b,
                                           int ld, int L, int sub) {
  float acc = 0.f;
  for (int k = sub * 4; k < ld; k += L * 4) {
    const float4 x = *reinterpret_cast<const float4 *>(a + k);
    const float4 y = *reinterpret_cast<const float4 *>(b + k);
    const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
    acc = fmaf(d0, d0, acc);
    acc = fmaf(d1, d1, acc);
    acc = fmaf(d2, d2, acc);
    acc = fmaf(d3, d3, acc);
  }
  for (int o = L >> 1; o; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// libsvm's Solver::Solve step on the pair (i, j) with C_i = C_j = C and
// Q_ii = Q_jj = 1: the new alpha_i, alpha_j clipped to the box.
__device__ __forceinline__ void smo_pair(float si, float sj, float Gi, float Gj,
                                         float Kij, float C, float &ai,
                                         float &aj) {
  float quad = 2.f - 2.f * Kij;
  if (quad <= 0.f) quad = kTau;
  if (si != sj) {
    const float delta = (-Gi - Gj) / quad, diff = ai - aj;
    ai += delta;
    aj += delta;
    if (diff > 0.f) {
      if (aj < 0.f) { aj = 0.f; ai = diff; }
    } else {
      if (ai < 0.f) { ai = 0.f; aj = -diff; }
    }
    if (diff > 0.f) {
      if (ai > C) { ai = C; aj = C - diff; }
    } else {
      if (aj > C) { aj = C; ai = C + diff; }
    }
  } else {
    const float delta = (Gi - Gj) / quad, sum = ai + aj;
    ai -= delta;
    aj += delta;
    if (sum > C) {
      if (ai > C) { ai = C; aj = sum - C; }
    } else {
      if (aj < 0.f) { aj = 0.f; ai = sum; }
    }
    if (sum > C) {
      if (aj > C) { aj = C; ai = sum - C; }
    } else {
      if (ai < 0.f) { ai = 0.f; aj = sum; }
    }
  }
}

__device__ __forceinline__ float wave_sum(float x) {
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// lowest lane whose predicate holds (64 if none)
__device__ __forceinline__ int first_lane(bool pred) {
  const unsigned long long b = __ballot(pred);
  return b ? __ffsll((long long)b) - 1 : 64;
}

// ---- m <= MP: one wave per problem ----------------------------------------
template <int MP>
__global__ __launch_bounds__(kTB) void svc_fit_wave(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = blockIdx.x * (kTB / 64) + wave;
  if (slot >= a.n) return;  // whole wave; the kernel has no block barrier
  const int p = a.order[slot];
  const int64_t o = a.off[p];
  const int m = (int)(a.off[p + 1] - o);
  float *K = smem + wave * MP * MP;

  {  // kernel matrix, upper triangle computed once and mirrored
    const int L = a.lanes, ngrp = 64 / L, grp = lane / L, sub = lane % L;
    for (int idx = grp; idx < m * m; idx += ngrp) {
      const int r = idx / m, c = idx - r * m;
      if (c < r) continue;
      const float d2 = row_dist2(a.tab + (int64_t)a.row[o + r] * a.ld,
                                 a.tab + (int64_t)a.row[o + c] * a.ld, a.ld, L, sub);
      if (sub == 0) {
        const float k = expf(-a.gamma * d2);
        K[r * MP + c] = k;
        K[c * MP + r] = k;
      }
    }
  }
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();

  const bool valid = lane < m;
  const int t = valid ? lane : 0;
  const float s = valid ? (a.lab[o + t] ? 1.f : -1.f) : 1.f;
  const float C = a.C;
  float alpha = 0.f, G = -1.f;
  const int cap = iter_cap(a.max_iter, m);
  int it = 0, status = 0;
  for (;;) {
    const float u = -s * G;
    const bool up = valid && (s > 0.f ? alpha < C : alpha > 0.f);
    const float uv = up ? u : -INFINITY;
    const float gmax = hgx::wave_max(uv);
    const int i = first_lane(up && uv == gmax);
    if (i == 64) break;
    const float Ki = K[i * MP + t];
    const bool low = valid && (s > 0.f ? alpha > 0.f : alpha < C);
    const float gmax2 = hgx::wave_max(low ? -u : -INFINITY);
    if (gmax + gmax2 < a.eps) break;
    const float b = gmax - u;
    float quad = 2.f - 2.f * Ki;
    if (quad <= 0.f) quad = kTau;
    const bool cand = low && b > 0.f;
    const float score = cand ? b * b / quad : -INFINITY;
    const float best = hgx::wave_max(score);
    const int j = first_lane(cand && score == best);
    if (j == 64) break;
    if (it >= cap) {
      status = 1;
      break;
    }
    const float Kj = K[j * MP + t];
    const float si = __shfl(s, i), sj = __shfl(s, j);
    const float ai0 = __shfl(alpha, i), aj0 = __shfl(alpha, j);
    float ai = ai0, aj = aj0;
    smo_pair(si, sj, __shfl(G, i), __shfl(G, j), K[i * MP + j], C, ai, aj);
    const float dai = ai - ai0, daj = aj - aj0;
    G += s * (si * Ki * dai + sj * Kj * daj);
    if (lane == i) alpha = ai;
    if (lane == j) alpha = aj;
    it++;
  }

  // rho (libsvm calculate_rho): mean of s G over the free vectors, else the
  // midpoint of the two bounds
  const float yG = s * G;
  const bool at_ub = alpha >= C, at_lb = alpha <= 0.f;
  const bool fre = valid && !at_ub && !at_lb;
  const int nfree = __popcll(__ballot(fre));
  const float sum_free = wave_sum(fre ? yG : 0.f);
  const bool for_ub = valid && ((at_ub && s < 0.f) || (at_lb && !at_ub && s > 0.f));
  const bool for_lb = valid && ((at_ub && s > 0.f) || (at_lb && !at_ub && s < 0.f));
  const float ub = hgx::wave_min(for_ub ? yG : INFINITY);
  const float lb = hgx::wave_max(for_lb ? yG : -INFINITY);
  if (valid) a.coef[o + t] = s * alpha;
  if (lane == 0) {
    a.rho[p] = nfree > 0 ? sum_free / (float)nfree : (ub + lb) * 0.5f;
    a.iters[p] = it;
    a.status[p] = status;
  }
}

// ---- one workgroup per problem --------------------------------------------
struct BlockRed {
  float v[4];
  int i[4];
  float g[4];
  float pad[4];
};

// (largest v, the lowest index that has it, largest g) over the workgroup
__device__ __forceinline__ void block_argmax(BlockRed *red, float &v, int &idx,
                                             float &g) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float wv = hgx::wave_max(v);
  const int wi = -hgx::wave_max_i(-(v == wv ? idx : INT_MAX));
  const float wg = hgx::wave_max(g);
  if (lane == 0) {
    red->v[wave] = wv;
    red->i[wave] = wi;
    red->g[wave] = wg;
  }
  __syncthreads();
  v = red->v[0];
  idx = red->i[0];
  g = red->g[0];
  for (int w = 1; w < 4; w++) {
    const float ov = red->v[w];
    const int oi = red->i[w];
    if (ov > v || (ov == v && oi < idx)) {
      v = ov;
      idx = oi;
    }
    g = fmaxf(g, red->g[w]);
  }
  __syncthreads();
}

__device__ __forceinline__ float block_sum(BlockRed *red, float x) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  x = wave_sum(x);
  if (lane == 0) red->v[wave] = x;
  __syncthreads();
  const float r = ((red->v[0] + red->v[1]) + red->v[2]) + red->v[3];
  __syncthreads();
  return r;
}

// column i of the kernel matrix from the table rows: col[t] = K(x_i, x_t)
__device__ __forceinline__ void kernel_column(const FitArgs &a, int64_t o, int m,
                                              int i, float *xi, float *col) {
  const float *src = a.tab + (int64_t)a.row[o + i] * a.ld;
  for (int k = threadIdx.x; k < a.ld; k += kTB) xi[k] = src[k];
  __syncthreads();
  const int L = a.lanes, ngrp = kTB / L, grp = threadIdx.x / L, sub = threadIdx.x % L;
  for (int t = grp; t < m; t += ngrp) {
    const float d2 = row_dist2(xi, a.tab + (int64_t)a.row[o + t] * a.ld, a.ld, L, sub);
    if (sub == 0) col[t] = expf(-a.gamma * d2);
  }
  __syncthreads();
}

// LDM > 0: problems of up to LDM samples, kernel matrix in LDS; 0: any size,
// columns recomputed
template <int LDM>
__global__ __launch_bounds__(kTB) void svc_fit_block(FitArgs a) {
  constexpr bool LDSK = LDM > 0;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  BlockRed *red = reinterpret_cast<BlockRed *>(smem);
  float *lds = smem + sizeof(BlockRed) / sizeof(float);
  const int tid = threadIdx.x;
  const int p = a.order[blockIdx.x];
  const int64_t o = a.off[p];
  const int m = (int)(a.off[p + 1] - o);
  const uint8_t *lab = a.lab + o;
  // LDSK: [K m x m, row stride LDM | alpha | G]; else [x_i] and the state
  // in global scratch
  float *Kmat = lds, *xi = lds;
  float *alpha = LDSK ? lds + LDM * LDM : a.st_alpha + o;
  float *G = LDSK ? alpha + LDM : a.st_G + o;
  float *col_i = LDSK ? nullptr : a.st_K0 + o;
  float *col_j = LDSK ? nullptr : a.st_K1 + o;

  if (LDSK) {
    const int L = a.lanes, ngrp = kTB / L, grp = tid / L, sub = tid % L;
    for (int idx = grp; idx < m * m; idx += ngrp) {
      const int r = idx / m, c = idx - r * m;
      if (c < r) continue;
      const float d2 = row_dist2(a.tab + (int64_t)a.row[o + r] * a.ld,
                                 a.tab + (int64_t)a.row[o + c] * a.ld, a.ld, L, sub);
      if (sub == 0) {
        const float k = expf(-a.gamma * d2);
        Kmat[r * LDM + c] = k;
        Kmat[c * LDM + r] = k;
      }
    }
  }
  for (int t = tid; t < m; t += kTB) {
    alpha[t] = 0.f;
    G[t] = -1.f;
  }
  __syncthreads();

  const float C = a.C;
  const int cap = iter_cap(a.max_iter, m);
  int it = 0, status = 0;
  for (;;) {
    float bv = -INFINITY, unused = -INFINITY;
    int bi = INT_MAX;
    for (int t = tid; t < m; t += kTB) {
      const bool pos = lab[t] != 0;
      const float al = alpha[t], u = pos ? -G[t] : G[t];
      if ((pos ? al < C : al > 0.f) && u > bv) {
        bv = u;
        bi = t;
      }
    }
    block_argmax(red, bv, bi, unused);
    const int i = bi;
    if (i == INT_MAX) break;
    const float gmax = bv;
    const float *Ki;
    if (LDSK) {
      Ki = Kmat + i * LDM;
    } else {
      kernel_column(a, o, m, i, xi, col_i);
      Ki = col_i;
    }
    float g2 = -INFINITY;
    bv = -INFINITY;
    bi = INT_MAX;
    for (int t = tid; t < m; t += kTB) {
      const bool pos = lab[t] != 0;
      const float al = alpha[t], u = pos ? -G[t] : G[t];
      if (pos ? al > 0.f : al < C) {
        g2 = fmaxf(g2, -u);
        const float b = gmax - u;
        if (b > 0.f) {
          float quad = 2.f - 2.f * Ki[t];
          if (quad <= 0.f) quad = kTau;
          const float sc = b * b / quad;
          if (sc > bv) {
            bv = sc;
            bi = t;
          }
        }
      }
    }
    block_argmax(red, bv, bi, g2);
    const int j = bi;
    if (gmax + g2 < a.eps || j == INT_MAX) break;
    if (it >= cap) {
      status = 1;
      break;
    }
    const float *Kj;
    if (LDSK) {
      Kj = Kmat + j * LDM;
    } else {
      kernel_column(a, o, m, j, xi, col_j);
      Kj = col_j;
    }
    const float si = lab[i] ? 1.f : -1.f, sj = lab[j] ? 1.f : -1.f;
    const float ai0 = alpha[i], aj0 = alpha[j];
    float ai = ai0, aj = aj0;
    smo_pair(si, sj, G[i], G[j], Ki[j], C, ai, aj);
    __syncthreads();  // every thread has read the pair's state
    const float ci = si * (ai - ai0), cj = sj * (aj - aj0);
    for (int t = tid; t < m; t += kTB) {
      const float s = lab[t] ? 1.f : -1.f;
      G[t] += s * (Ki[t] * ci + Kj[t] * cj);
      if (t == i) alpha[t] = ai;
      if (t == j) alpha[t] = aj;
    }
    __syncthreads();
    it++;
  }

  float sum_free = 0.f, nfree = 0.f, ub = INFINITY, lb = -INFINITY;
  for (int t = tid; t < m; t += kTB) {
    const bool pos = lab[t] != 0;
    const float al = alpha[t], yG = pos ? G[t] : -G[t];
    if (al >= C) {
      if (pos) lb = fmaxf(lb, yG); else ub = fminf(ub, yG);
    } else if (al <= 0.f) {
      if (pos) ub = fminf(ub, yG); else lb = fmaxf(lb, yG);
    } else {
      sum_free += yG;
      nfree += 1.f;
    }
    a.coef[o + t] = pos ? al : -al;
  }
  sum_free = block_sum(red, sum_free);
  nfree = block_sum(red, nfree);
  float nub = -ub;
  int di = INT_MAX;
  block_argmax(red, nub, di, lb);  // nub := max(-ub), lb := max(lb)
  if (tid == 0) {
    a.rho[p] = nfree > 0.f ? sum_free / nfree : (-nub + lb) * 0.5f;
    a.iters[p] = it;
    a.status[p] = status;
  }
}

// ---- decision function ------------------------------------------------------
// One wave per (problem, query row); queries arrive sorted by problem so the
// waves of a workgroup read the same support rows. Zero coefficients are
// skipped. out[qidx[q]] = sum_j coef_j K(x_j, q) - rho.
__global__ __launch_bounds__(kTB) void svc_decision(
    const float *tab, int ld, int lanes, const int64_t *off, const int32_t *row,
    const float *coef, const float *rho, const float *qtab, const int32_t *qprob,
    const int32_t *qrow, const int32_t *qidx, int64_t nq, float gamma, float *out) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * (kTB / 64) + (threadIdx.x >> 6);
  if (q >= nq) return;
  const int p = qprob[q];
  const int64_t o = off[p];
  const int m = (int)(off[p + 1] - o);
  const float *xq = qtab + (int64_t)qrow[q] * ld;
  const int L = lanes, ngrp = 64 / L, grp = lane / L, sub = lane % L;
  float acc = 0.f;
  for (int v = grp; v < m; v += ngrp) {
    const float c = coef[o + v];
    if (c == 0.f) continue;
    const float d2 = row_dist2(tab + (int64_t)row[o + v] * ld, xq, ld, L, sub);
    acc = fmaf(c, expf(-gamma * d2), acc);
  }
  const float f = wave_sum(sub == 0 ? acc : 0.f);
  if (lane == 0) out[qidx[q]] = f - rho[p];
}

int upload(hgx_svc *s, DevBuf &b, const void *src, size_t bytes) {
  HGX_TRY(hgx_ensure(s->ctx, b, bytes));
  if (bytes)
    HGX_HIP(s->ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice,
                                   s->ctx->stream));
  return HGX_OK;
}

template <class Kern>
int launch_fit(hgx_svc *s, Kern kern, FitArgs a, const std::vector<int32_t> &list,
               size_t order_at, int per_block, size_t lds) {
  if (list.empty()) return HGX_OK;
  a.order = s->d_order.as<int32_t>() + order_at;
  a.n = (int)list.size();
  if (lds > 64 * 1024)
    HGX_HIP(s->ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
  const unsigned grid = (unsigned)((list.size() + per_block - 1) / per_block);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(kTB), lds, s->ctx->stream, a);
  HGX_LAUNCH_CHECK(s->ctx);
  return HGX_OK;
}

int run_decision(hgx_svc *s, int64_t n_q, const int32_t *prob, const int32_t *row,
                 const float *qtab, int64_t q_rows, float *f_out) {
  hgx_ctx *ctx = s->ctx;
  HGX_CHECK(ctx, s->fitted, HGX_ESTATE, "hgx_svc_decision before hgx_svc_fit");
  HGX_CHECK(ctx, n_q >= 0 && n_q < INT32_MAX, HGX_EINVAL, "query count out of range");
  if (n_q == 0) return HGX_OK;
  HGX_CHECK(ctx, prob && row && f_out, HGX_EINVAL, "null query array");
  for (int64_t q = 0; q < n_q; q++) {
    HGX_CHECK(ctx, prob[q] >= 0 && prob[q] < s->n_prob, HGX_EVALUE,
              "query %lld: problem %d out of range [0, %lld)", (long long)q, prob[q],
              (long long)s->n_prob);
    HGX_CHECK(ctx, row[q] >= 0 && row[q] < q_rows, HGX_EVALUE,
              "query %lld: row %d out of range [0, %lld)", (long long)q, row[q],
              (long long)q_rows);
  }
  std::vector<int32_t> idx(n_q), sp(n_q), sr(n_q);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(),
                   [&](int32_t x, int32_t y) { return prob[x] < prob[y]; });
  for (int64_t q = 0; q < n_q; q++) {
    sp[q] = prob[idx[q]];
    sr[q] = row[idx[q]];
  }
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_TRY(upload(s, s->q_prob, sp.data(), sizeof(int32_t) * n_q));
  HGX_TRY(upload(s, s->q_row, sr.data(), sizeof(int32_t) * n_q));
  HGX_TRY(upload(s, s->q_idx, idx.data(), sizeof(int32_t) * n_q));
  HGX_TRY(hgx_ensure(ctx, s->q_out, sizeof(float) * n_q));
  HGX_HIP(ctx, hipEventRecord(s->e0, ctx->stream));
  const unsigned grid = (unsigned)((n_q + kTB / 64 - 1) / (kTB / 64));
  hipLaunchKernelGGL(svc_decision, dim3(grid), dim3(kTB), 0, ctx->stream,
                     s->tab.as<float>(), s->ld, s->lanes, s->d_off.as<int64_t>(),
                     s->d_row.as<int32_t>(), s->d_coef.as<float>(),
                     s->d_rho.as<float>(), qtab, s->q_prob.as<int32_t>(),
                     s->q_row.as<int32_t>(), s->q_idx.as<int32_t>(), n_q, s->gamma,
                     s->q_out.as<float>());
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipEventRecord(s->e1, ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(f_out, s->q_out.p, sizeof(float) * n_q,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HGX_HIP(ctx, hipEventElapsedTime(&ms, s->e0, s->e1));
  s->dec_ms = ms;
  return HGX_OK;
}

// rows x dim host floats -> rows x ld device floats (zero padded)
int upload_rows(hgx_svc *s, DevBuf &b, int64_t rows, const float *src) {
  const size_t bytes = sizeof(float) * (size_t)rows * s->ld;
  HGX_TRY(hgx_ensure(s->ctx, b, bytes));
  HGX_HIP(s->ctx, hipMemsetAsync(b.p, 0, bytes ? bytes : 16, s->ctx->stream));
  if (rows)
    HGX_HIP(s->ctx, hipMemcpy2DAsync(b.p, sizeof(float) * s->ld, src,
                                     sizeof(float) * s->dim, sizeof(float) * s->dim,
                                     (size_t)rows, hipMemcpyHostToDevice,
                                     s->ctx->stream));
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_svc_create(hgx_ctx *ctx, int dim, int64_t n_rows,
                              const float *rows, hgx_svc **out) {
  if (!ctx || !out) return HGX_EINVAL;
  *out = nullptr;
  HGX_CHECK(ctx, dim > 0, HGX_EINVAL, "dimension must be positive");
  HGX_CHECK(ctx, dim <= 16384, HGX_EUNSUP, "dimensions above 16384 are not supported");
  HGX_CHECK(ctx, n_rows > 0 && n_rows < INT32_MAX && rows, HGX_EINVAL,
            "the table needs at least one row");
  for (int64_t k = 0; k < n_rows * dim; k++)
    HGX_CHECK(ctx, std::isfinite(rows[k]), HGX_EVALUE,
              "table row %lld holds a non-finite value", (long long)(k / dim));
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  hgx_svc *s = new hgx_svc();
  s->ctx = ctx;
  s->dim = dim;
  s->ld = (dim + 3) / 4 * 4;
  s->n_rows = n_rows;
  while (s->lanes < 16 && s->lanes * 4 < s->ld) s->lanes <<= 1;
  int rc = upload_rows(s, s->tab, n_rows, rows);
  if (!rc && hipEventCreate(&s->e0) != hipSuccess) rc = hgx_fail(ctx, HGX_EHIP, "event");
  if (!rc && hipEventCreate(&s->e1) != hipSuccess) rc = hgx_fail(ctx, HGX_EHIP, "event");
  if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess)
    rc = hgx_fail(ctx, HGX_EHIP, "stream synchronize failed");
  if (rc) {
    hgx_svc_destroy(s);
    return rc;
  }
  *out = s;
  return HGX_OK;
}

extern "C" int hgx_svc_destroy(hgx_svc *s) {
  if (!s) return HGX_OK;
  if (s->ctx) hipStreamSynchronize(s->ctx->stream);
  DevBuf *bufs[] = {&s->tab, &s->d_off, &s->d_row, &s->d_lab, &s->d_order,
                    &s->d_coef, &s->d_rho, &s->d_iters, &s->d_status, &s->st_alpha,
                    &s->st_G, &s->st_K0, &s->st_K1, &s->q_prob, &s->q_row,
                    &s->q_idx, &s->q_out, &s->q_vec};
  for (DevBuf *b : bufs) hgx_release(*b);
  if (s->e0) hipEventDestroy(s->e0);
  if (s->e1) hipEventDestroy(s->e1);
  delete s;
  return HGX_OK;
}

extern "C" int hgx_svc_fit(hgx_svc *s, int64_t n_prob, const int64_t *off,
                           const int32_t *row, const uint8_t *label, float C,
                           float gamma, float eps, int max_iter,
                           int32_t *iters_out, int32_t *status_out) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  HGX_CHECK(ctx, n_prob > 0 && n_prob < INT32_MAX && off, HGX_EINVAL,
            "at least one problem is needed");
  HGX_CHECK(ctx, C > 0.f && std::isfinite(C), HGX_EVALUE, "C must be positive");
  HGX_CHECK(ctx, gamma > 0.f && std::isfinite(gamma), HGX_EVALUE,
            "gamma must be positive");
  HGX_CHECK(ctx, eps > 0.f && std::isfinite(eps), HGX_EVALUE, "eps must be positive");
  HGX_CHECK(ctx, off[0] == 0, HGX_EINVAL, "off[0] must be 0");
  std::vector<int32_t> tier[4];
  const int lds_m = ctx->tune.svc_lds_m;
  for (int64_t p = 0; p < n_prob; p++) {
    const int64_t m = off[p + 1] - off[p];
    HGX_CHECK(ctx, m > 0, HGX_EVALUE, "problem %lld has no samples", (long long)p);
    HGX_CHECK(ctx, m < (1 << 24), HGX_EUNSUP, "problem %lld: more than 2^24 samples",
              (long long)p);
    HGX_CHECK(ctx, row && label, HGX_EINVAL, "null sample array");
    int64_t npos = 0;
    for (int64_t k = off[p]; k < off[p + 1]; k++) {
      HGX_CHECK(ctx, row[k] >= 0 && row[k] < s->n_rows, HGX_EVALUE,
                "problem %lld: row %d out of range [0, %lld)", (long long)p, row[k],
                (long long)s->n_rows);
      HGX_CHECK(ctx, label[k] <= 1, HGX_EVALUE, "problem %lld: label %d is not 0 / 1",
                (long long)p, (int)label[k]);
      npos += label[k];
    }
    HGX_CHECK(ctx, npos > 0 && npos < m, HGX_EVALUE,
              "problem %lld has only one class", (long long)p);
    tier[m <= 32 ? 0 : m <= kWaveM ? 1 : m <= lds_m ? 2 : 3].push_back((int32_t)p);
  }
  const int64_t n_samp = off[n_prob];
  s->fitted = false;
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<int32_t> order;
  size_t at[4];
  for (int k = 0; k < 4; k++) {
    at[k] = order.size();
    order.insert(order.end(), tier[k].begin(), tier[k].end());
  }
  HGX_TRY(upload(s, s->d_off, off, sizeof(int64_t) * (n_prob + 1)));
  HGX_TRY(upload(s, s->d_row, row, sizeof(int32_t) * n_samp));
  HGX_TRY(upload(s, s->d_lab, label, (size_t)n_samp));
  HGX_TRY(upload(s, s->d_order, order.data(), sizeof(int32_t) * n_prob));
  HGX_TRY(hgx_ensure(ctx, s->d_coef, sizeof(float) * n_samp));
  HGX_TRY(hgx_ensure(ctx, s->d_rho, sizeof(float) * n_prob));
  HGX_TRY(hgx_ensure(ctx, s->d_iters, sizeof(int32_t) * n_prob));
  HGX_TRY(hgx_ensure(ctx, s->d_status, sizeof(int32_t) * n_prob));
  if (!tier[3].empty())
    for (DevBuf *b : {&s->st_alpha, &s->st_G, &s->st_K0, &s->st_K1})
      HGX_TRY(hgx_ensure(ctx, *b, sizeof(float) * n_samp));
  FitArgs a{};
  a.tab = s->tab.as<float>();
  a.ld = s->ld;
  a.lanes = s->lanes;
  a.off = s->d_off.as<int64_t>();
  a.row = s->d_row.as<int32_t>();
  a.lab = s->d_lab.as<uint8_t>();
  a.C = C;
  a.gamma = gamma;
  a.eps = eps;
  a.max_iter = max_iter;
  a.coef = s->d_coef.as<float>();
  a.rho = s->d_rho.as<float>();
  a.iters = s->d_iters.as<int32_t>();
  a.status = s->d_status.as<int32_t>();
  a.st_alpha = s->st_alpha.as<float>();
  a.st_G = s->st_G.as<float>();
  a.st_K0 = s->st_K0.as<float>();
  a.st_K1 = s->st_K1.as<float>();
  const int wpb = kTB / 64;
  HGX_HIP(ctx, hipEventRecord(s->e0, ctx->stream));
  HGX_TRY(launch_fit(s, svc_fit_wave<32>, a, tier[0], at[0], wpb,
                     sizeof(float) * wpb * 32 * 32));
  HGX_TRY(launch_fit(s, svc_fit_wave<kWaveM>, a, tier[1], at[1], wpb,
                     sizeof(float) * wpb * kWaveM * kWaveM));
  const size_t lds_b = sizeof(BlockRed) + sizeof(float) * (lds_m * lds_m + 2 * lds_m);
  if (lds_m == kLdsMax)
    HGX_TRY(launch_fit(s, svc_fit_block<kLdsMax>, a, tier[2], at[2], 1, lds_b));
  else
    HGX_TRY(launch_fit(s, svc_fit_block<128>, a, tier[2], at[2], 1, lds_b));
  HGX_TRY(launch_fit(s, svc_fit_block<0>, a, tier[3], at[3], 1,
                     sizeof(BlockRed) + sizeof(float) * s->ld));
  HGX_HIP(ctx, hipEventRecord(s->e1, ctx->stream));
  if (iters_out)
    HGX_HIP(ctx, hipMemcpyAsync(iters_out, s->d_iters.p, sizeof(int32_t) * n_prob,
                                hipMemcpyDeviceToHost, ctx->stream));
  if (status_out)
    HGX_HIP(ctx, hipMemcpyAsync(status_out, s->d_status.p, sizeof(int32_t) * n_prob,
                                hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  float ms = 0;
  HGX_HIP(ctx, hipEventElapsedTime(&ms, s->e0, s->e1));
  s->fit_ms = ms;
  s->n_prob = n_prob;
  s->n_samp = n_samp;
  s->gamma = gamma;
  s->off.assign(off, off + n_prob + 1);
  s->fitted = true;
  return HGX_OK;
}

extern "C" int hgx_svc_decision(hgx_svc *s, int64_t n_q, const int32_t *prob,
                                const int32_t *row, float *f_out) {
  if (!s) return HGX_EINVAL;
  return run_decision(s, n_q, prob, row, s->tab.as<float>(), s->n_rows, f_out);
}

extern "C" int hgx_svc_decision_vec(hgx_svc *s, int64_t n_q, const int32_t *prob,
                                    const float *vecs, float *f_out) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  HGX_CHECK(ctx, n_q >= 0 && n_q < INT32_MAX, HGX_EINVAL, "query count out of range");
  if (n_q == 0) return HGX_OK;
  HGX_CHECK(ctx, vecs, HGX_EINVAL, "null query vectors");
  for (int64_t k = 0; k < n_q * s->dim; k++)
    HGX_CHECK(ctx, std::isfinite(vecs[k]), HGX_EVALUE,
              "query vector %lld holds a non-finite value", (long long)(k / s->dim));
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_TRY(upload_rows(s, s->q_vec, n_q, vecs));
  std::vector<int32_t> rows(n_q);
  std::iota(rows.begin(), rows.end(), 0);
  return run_decision(s, n_q, prob, rows.data(), s->q_vec.as<float>(), n_q, f_out);
}

extern "C" int hgx_svc_get(hgx_svc *s, float *coef_out, float *rho_out) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  HGX_CHECK(ctx, s->fitted, HGX_ESTATE, "hgx_svc_get before hgx_svc_fit");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  if (coef_out)
    HGX_HIP(ctx, hipMemcpyAsync(coef_out, s->d_coef.p, sizeof(float) * s->n_samp,
                                hipMemcpyDeviceToHost, ctx->stream));
  if (rho_out)
    HGX_HIP(ctx, hipMemcpyAsync(rho_out, s->d_rho.p, sizeof(float) * s->n_prob,
                                hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_svc_last_stats(const hgx_svc *s, double *fit_ms,
                                  double *decision_ms) {
  if (!s) return HGX_EINVAL;
  if (fit_ms) *fit_ms = s->fit_ms;
  if (decision_ms) *decision_ms = s->dec_ms;
  return HGX_OK;
}
