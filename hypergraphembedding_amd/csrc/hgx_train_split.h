// Trainer kernels, two-kernel step: K1 train_fwd_bwd, K2 train_update and the
// Adagrad / no-contraction helpers the deferred-row step shares with them.
#pragma once
#include "hgx_train_common.h"

namespace {

// MODE: 0 = activation and loss read from the arguments; 1 = FOBE (sigmoid,
// KLD); 2 = HOBE (relu, MSE). KEXACT: K == KMAX at compile time. The
// specialised forms drop the per-record branches, exp and log of the other
// head types: each wave runs its record chain alone on its SIMD, so its
// instruction count is its latency.
template <int L, int VPL, int KMAX, bool KEXACT, int MODE, int TB>
__global__ __launch_bounds__(TB) void train_fwd_bwd(TrainArgs a, int cb) {
  constexpr int RPB = TB / L;
  __shared__ float4 s_z[2][RPB][L * VPL];
  __shared__ float s_loss[RPB];
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int grp = threadIdx.x / L, lane = threadIdx.x % L;
  const int rib = blockIdx.x * RPB + grp;
  const int K = KEXACT ? KMAX : a.K, R = KEXACT ? 4 + 2 * KMAX : a.R;
  const int dp = a.dp;
  // everything below depends only on (cb, rib): the batch metadata and the
  // record's ids / slot positions load together (buffers are padded)
  const int2 bm = a.bmeta[cb];
  const int *ri = a.bidx + ((size_t)cb * a.B + rib) * R;
  const float *yt = a.btgt + ((size_t)cb * a.B + rib) * 3;
  const int *pos = a.inv + (size_t)cb * a.SB + (size_t)rib * R;
  int ln = ri[0], le = ri[1], rn = ri[2], re = ri[3];
  int nnk[KMAX], nek[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; k++) {
    nnk[k] = k < K ? ri[4 + k] : 0;
    nek[k] = k < K ? ri[4 + K + k] : 0;
  }
  const int nb = bm.x;
  HGX_STAMP(ts[1]);
  if (nb == 0 || (g_tab & 1)) return;
  const float inv_b = 1.0f / (float)nb;
  float4 zN[VPL], zE[VPL];
#pragma unroll
  for (int v = 0; v < VPL; v++) zN[v] = zE[v] = f4(0.f);
  float lrec = 0.f;
  if (rib < nb) {
    if (g_tab & 4) {
      ln = le = rn = re = 0;
#pragma unroll
      for (int k = 0; k < KMAX; k++) nnk[k] = nek[k] = 0;
    }
    float4 Nl[VPL], Nr[VPL], El[VPL], Er[VPL], Nk[KMAX][VPL], Ek[KMAX][VPL];
    load_row<L, VPL>(a.ntab, ln, dp, lane, Nl);
    load_row<L, VPL>(a.ntab, rn, dp, lane, Nr);
    load_row<L, VPL>(a.etab, le, dp, lane, El);
    load_row<L, VPL>(a.etab, re, dp, lane, Er);
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      if (k < K) {
        load_row<L, VPL>(a.ntab, nnk[k], dp, lane, Nk[k]);
        load_row<L, VPL>(a.etab, nek[k], dp, lane, Ek[k]);
      }
    }
    HGX_STAMP(ts[2]);
    float z1 = 0.f, z2 = 0.f, za[KMAX], zb[KMAX];
#pragma unroll
    for (int v = 0; v < VPL; v++) {
      z1 += dot4(Nl[v], Nr[v]);
      z2 += dot4(El[v], Er[v]);
    }
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      za[k] = zb[k] = 0.f;
      if (k < K) {
#pragma unroll
        for (int v = 0; v < VPL; v++) {
          za[k] += dot4(Nk[k][v], Nl[v]);
          zb[k] += dot4(Ek[k][v], Er[v]);
        }
      }
    }
    z1 = group_sum<L>(z1);
    z2 = group_sum<L>(z2);
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      if (k < K) {
        za[k] = group_sum<L>(za[k]);
        zb[k] = group_sum<L>(zb[k]);
      }
    }
    const int act = MODE == 1 ? 0 : MODE == 2 ? 1 : a.act;
    const int lossk = MODE == 1 ? 0 : MODE == 2 ? 1 : a.loss;
    const float y1 = act_f(act, z1), y2 = act_f(act, z2);
    float sa[KMAX], sb[KMAX], P = 0.f, Q = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      if (k < K) {
        sa[k] = act_f(act, za[k]);
        sb[k] = act_f(act, zb[k]);
        P += sa[k];
        Q += sb[k];
      }
    }
    P = P / (float)K;
    Q = Q / (float)K;
    const float y3 = P * Q;
    float l1, l2, l3, g1, g2, g3;
    head_loss(lossk, y1, yt[0], l1, g1);
    head_loss(lossk, y2, yt[1], l2, g2);
    head_loss(lossk, y3, yt[2], l3, g3);
    lrec = l1 + l2 + l3;
    HGX_STAMP(ts[3]);
    g1 *= inv_b;
    g2 *= inv_b;
    g3 *= inv_b;
    const float dz1 = g1 * act_d(act, z1, y1);
    const float dz2 = g2 * act_d(act, z2, y2);
    const float dP = g3 * Q / (float)K, dQ = g3 * P / (float)K;
    auto emit = [&](int s, int row, bool edge, const float4(&g)[VPL]) {
      if (row == 0) {
#pragma unroll
        for (int v = 0; v < VPL; v++) {
          if (edge) zE[v] = zE[v] + g[v];
          else zN[v] = zN[v] + g[v];
        }
      } else if (!(g_tab & 8)) {
        float4 *p = reinterpret_cast<float4 *>(a.gslot + (size_t)pos[s] * dp);
#pragma unroll
        for (int v = 0; v < VPL; v++) p[v * L + lane] = g[v];
      }
    };
    float4 gln[VPL], gre[VPL], tmp[VPL];
#pragma unroll
    for (int v = 0; v < VPL; v++) {
      gln[v] = fma4(dz1, Nr[v], f4(0.f));
      gre[v] = fma4(dz2, El[v], f4(0.f));
    }
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
      if (k < K) {
        const float da = dP * act_d(act, za[k], sa[k]);
        const float db = dQ * act_d(act, zb[k], sb[k]);
#pragma unroll
        for (int v = 0; v < VPL; v++) {
          gln[v] = fma4(da, Nk[k][v], gln[v]);
          gre[v] = fma4(db, Ek[k][v], gre[v]);
          tmp[v] = fma4(da, Nl[v], f4(0.f));
        }
        emit(4 + k, nnk[k], false, tmp);
#pragma unroll
        for (int v = 0; v < VPL; v++) tmp[v] = fma4(db, Er[v], f4(0.f));
        emit(4 + K + k, nek[k], true, tmp);
      }
    }
    emit(0, ln, false, gln);
    emit(3, re, true, gre);
#pragma unroll
    for (int v = 0; v < VPL; v++) tmp[v] = fma4(dz1, Nl[v], f4(0.f));
    emit(2, rn, false, tmp);
#pragma unroll
    for (int v = 0; v < VPL; v++) tmp[v] = fma4(dz2, Er[v], f4(0.f));
    emit(1, le, true, tmp);
    HGX_STAMP(ts[4]);
  }
  // padding-row partials and loss: reduce over the record groups
#pragma unroll
  for (int v = 0; v < VPL; v++) {
    s_z[0][grp][v * L + lane] = zN[v];
    s_z[1][grp][v * L + lane] = zE[v];
  }
  if (lane == 0) s_loss[grp] = lrec;
  __syncthreads();
  for (int t = threadIdx.x; t < 2 * L * VPL; t += TB) {
    const int tab = t / (L * VPL), j = t % (L * VPL);
    float4 s = f4(0.f);
    for (int g = 0; g < RPB; g++) s = s + s_z[tab][g][j];
    reinterpret_cast<float4 *>(a.gzero + ((size_t)blockIdx.x * 2 + tab) * dp)[j] = s;
  }
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int g = 0; g < RPB; g++) s += s_loss[g];
    a.lossbuf[(size_t)bm.y * a.lstride + blockIdx.x] = s;
  }
  HGX_STAMP(ts[5]);
  trace_put(bm.y, 0, 6, ts);
}

// The step's scalar head math, its float2 dot and its Adagrad updates (in the
// step and in train_flush, which must agree: a streamed run ends every chunk
// with a flush where a resident run goes on stepping) with every product that
// feeds a sum, and the sums of products, compiled with contraction off
// (these operations carry no `contract` flag, so no fma is formed from them;
// the __f*_rn functions are plain operators and do contract). The compiler pairs up and contracts these
// few scalar operations differently in every instantiation (y3 - yt3 was an
// fma at float4 rows and a packed subtraction at float2 rows; the paired-wave
// form, with half the heads per wave, chose differently again), and the
// step's forms must agree bit for bit (tests/test_gpu_train_pair.py). The
// oracle rounds each operation too.
__device__ __forceinline__ float mul_nc(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}
__device__ __forceinline__ float add_nc(float x, float y) {
#pragma clang fp contract(off)
  return x + y;
}
__device__ __forceinline__ float sub_nc(float x, float y) {
#pragma clang fp contract(off)
  return x - y;
}

// Adagrad on one float4 of a row (Keras 2.x formulas, round-to-nearest ops
// so the device matches the oracle's rounding)
__device__ __forceinline__ void adagrad4(float4 &p, float4 &ac, float4 g,
                                         float lr, float eps) {
  float *pp = &p.x, *aa = &ac.x;
  const float *gv = &g.x;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const float na = __fadd_rn(aa[c], __fmul_rn(gv[c], gv[c]));
    aa[c] = na;
    pp[c] = __fsub_rn(pp[c], __fdiv_rn(__fmul_rn(lr, gv[c]),
                                       __fadd_rn(sqrtf(na), eps)));
  }
}

// The same update with the hardware square root and reciprocal (<= 1 ulp
// each; the fused step runs every row update of a record on one wave, where
// the correctly rounded sequences cost ~30 instructions per element).
__device__ __forceinline__ void adagrad4_hw(float4 &p, float4 &ac, float4 g,
                                            float lr, float eps) {
  float *pp = &p.x, *aa = &ac.x;
  const float *gv = &g.x;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const float na = add_nc(aa[c], mul_nc(gv[c], gv[c]));
    aa[c] = na;
    const float den = add_nc(__builtin_amdgcn_sqrtf(na), eps);
    pp[c] = sub_nc(pp[c], mul_nc(mul_nc(lr, gv[c]), __builtin_amdgcn_rcpf(den)));
  }
}

// K2. Workgroups [0, gridDim-2): one L-lane group per unique touched row.
// The last two workgroups: the padding row 0 of the node / edge table, its
// gradient = the sum of the nblk1 per-K1-workgroup partials, loaded by all
// 256 threads at once and tree-summed in LDS (fixed order: deterministic).
template <int L, int VPL, int TB>
__global__ __launch_bounds__(TB) void train_update(TrainArgs a, int cb) {
  constexpr int GPB = TB / L;
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int dp = a.dp, SB = a.SB;
  const int2 bm = a.bmeta[cb];
  if (blockIdx.x >= gridDim.x - 2) {
    __shared__ float4 s_part[TB];
    const int table = blockIdx.x - (gridDim.x - 2);
    const int NC = dp / 4;                  // float4 columns, <= 256
    const int TPC = TB / NC;               // threads per column (>= 1)
    const int col = threadIdx.x % NC, sub = threadIdx.x / NC;
    float4 *P = reinterpret_cast<float4 *>(table ? a.etab : a.ntab);
    float4 *A = reinterpret_cast<float4 *>(table ? a.eacc : a.nacc);
    const bool own = sub == 0;
    float4 pv = f4(0.f), av = f4(0.f);
    if (own && threadIdx.x < NC * TPC) {
      pv = P[col];
      av = A[col];
    }
    HGX_STAMP(ts[1]);
    if (bm.x == 0 || (g_tab & 2)) return;
    float4 g = f4(0.f);
    if (sub < TPC && !(g_tab & 16)) {
      const float4 *base = reinterpret_cast<const float4 *>(a.gzero) +
                           (size_t)table * NC + col;
      const size_t bstride = (size_t)2 * NC;
      for (int b = sub; b < a.nblk1; b += TPC) g = g + base[b * bstride];
    }
    s_part[threadIdx.x] = g;
    __syncthreads();
    for (int w = TPC / 2; w > 0; w >>= 1) {  // TPC is a power of two
      if (sub < w) s_part[threadIdx.x] = s_part[threadIdx.x] + s_part[threadIdx.x + w * NC];
      __syncthreads();
    }
    HGX_STAMP(ts[2]);
    if (own && !(g_tab & 32)) {
      adagrad4(pv, av, s_part[col], a.lr, a.eps);
      P[col] = pv;
      A[col] = av;
    }
    HGX_STAMP(ts[3]);
    trace_put(bm.y, 1, 4, ts);
    return;
  }
  const int grp = threadIdx.x / L, lane = threadIdx.x % L;
  const int it = blockIdx.x * GPB + grp;
  // the task's key and slot range load beside the batch metadata
  const int *ukey = a.ukey + (size_t)cb * SB;
  const int *uoff = a.uoff + (size_t)cb * (SB + 1);
  const int itc = min(it, SB - 1);
  const int key = ukey[itc], j0 = uoff[itc], j1 = uoff[min(it + 1, SB)];
  const int U = a.ucount[cb];
  HGX_STAMP(ts[1]);
  if (bm.x == 0 || (g_tab & 2) || it >= U) {
    ts[2] = ts[3] = ts[1];
    trace_put(bm.y, 1, 4, ts);
    return;
  }
  const int table = key >> 30, row = key & 0x3fffffff;
  float4 *P = reinterpret_cast<float4 *>((table ? a.etab : a.ntab) + (size_t)row * dp);
  float4 *A = reinterpret_cast<float4 *>((table ? a.eacc : a.nacc) + (size_t)row * dp);
  // table row and accumulator first: their latency hides under the sums
  float4 pv[VPL], av[VPL];
  if (!(g_tab & 32)) {
#pragma unroll
    for (int v = 0; v < VPL; v++) {
      pv[v] = P[v * L + lane];
      av[v] = A[v * L + lane];
    }
  }
  float4 g[VPL];
#pragma unroll
  for (int v = 0; v < VPL; v++) g[v] = f4(0.f);
  if (!(g_tab & 16)) {
    // this row's slot gradients are contiguous (prep sorted them)
    for (int j = j0; j < j1; j++) {
      const float4 *p = reinterpret_cast<const float4 *>(a.gslot + (size_t)j * dp);
#pragma unroll
      for (int v = 0; v < VPL; v++) g[v] = g[v] + p[v * L + lane];
    }
  }
  HGX_STAMP(ts[2]);
  if (g_tab & 32) return;
#pragma unroll
  for (int v = 0; v < VPL; v++) {
    adagrad4(pv[v], av[v], g[v], a.lr, a.eps);
    P[v * L + lane] = pv[v];
    A[v * L + lane] = av[v];
  }
  HGX_STAMP(ts[3]);
  trace_put(bm.y, 1, 4, ts);
}

}  // namespace
