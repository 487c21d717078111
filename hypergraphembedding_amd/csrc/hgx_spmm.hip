// Block primitives of the truncated SVD of the resident 0/1 incidence
// (hypergraphembedding_amd/svd.py drives them): a wide sparse x tall-skinny
// product in both orientations, and tall-skinny dense block algebra (Gram,
// small-matrix apply, column scaling) on device panels.
//
// A panel is a row-major fp32 matrix with one row per edge (side 0) or per
// node (side 1), row stride rounded up to 4 floats; every primitive works on
// a column range [col0, col0 + ncols) of a panel slot.
//
//   spmm   Y = A X (X on the edge side) or X' = A^T Y (Y on the node side).
//          Both CSR orientations are resident, so either product is a row
//          gather without atomics. A group of G lanes (a power of two, the
//          float4 column groups of the view rounded up, at most 64) owns a
//          row and a lane owns float4 column groups: every source row is
//          read as whole 16-byte pieces, 64 bytes or more per row from b =
//          16 on. A row is summed in CSR column order in float64 and rounded
//          once (the gather is bound by memory, and with fp32 sums the edge
//          rows of thousands of incidences put the solver's residual floor
//          above 1e-5); rows longer than the long-row threshold are cut into
//          pieces of that many incidences, each summed the same way into a
//          float64 partial row, and the partial rows are added in piece
//          order. No step depends on the launch shape, so a result is
//          bitwise reproducible.
//   gram   G = P^T Q in float64: products of two floats are exact in double,
//          64 x 64 output tiles with a 4 x 4 register tile per thread, the
//          rows cut into chunks whose partial tiles are added in chunk order.
//   apply  P = beta P + Q M with M a small float64 matrix from the host,
//          accumulated in float64 and rounded once to fp32.
//   scale  Y = Y diag(s).
//   cd_sweep  one non-negative coordinate-descent sweep of the NMF solver
//          (nmf.py) over the rows of a panel: see the kernel below.
#include <algorithm>
#include <cmath>

#include "hgx_internal.h"

namespace {

constexpr int kSlots = 8;
constexpr int kMaxSmall = 1056;  // largest p, q of gram / apply
constexpr int kTB = 256;
constexpr int kCdTB = 1024;      // cd_sweep workgroup: 16 waves share one Q
constexpr int kCdMaxR = 8;       // coordinates of a row per lane
constexpr int kCdMaxK = 64 * kCdMaxR;  // the sweep's limit (include/hgx.h)
constexpr size_t kCdLds = 160 * 1024;  // a CU's LDS

struct Panel {
  DevBuf buf;
  int side = -1;  // 0: one row per edge, 1: one row per node
  int width = 0, ld = 0;
  int64_t rows = 0;
};

// long rows of one CSR orientation at the engine's threshold
struct SvdLong {
  DevBuf seg, off, rows;  // int2 {row, piece} per piece; first piece; row ids
  int nlong = 0, nseg = 0;
};

}  // namespace

struct hgx_svd {
  hgx_ctx *ctx = nullptr;
  int thresh = 0;
  int32_t N = 0, E = 0;
  int64_t nnz = 0;
  uint64_t inc_gen = 0;  // the upload the long-row tables were built from
  Panel panel[kSlots];
  SvdLong lg[2];  // [0]: edge rows (rp_e), [1]: node rows (rp_n)
  DevBuf part;    // long-row partial rows (float64)
  DevBuf gpart, gout, mdev;  // gram chunk partials / result, apply's M
  DevBuf cdq, cdviol;        // cd_sweep: Q^T, per-row violations and their sum
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipEvent_t c0 = nullptr, c1 = nullptr;  // around a cd_sweep
  int ncu = 0;
  double cd_ms = 0;
  int64_t cd_sweeps = 0;
  bool spmm_pending = false;
  double spmm_pending_bytes = 0;
  double spmm_ms = 0, spmm_bytes = 0;
  int64_t spmm_calls = 0, spmm_cols = 0, dense_calls = 0;
};

namespace {

// VEC floats of a source row, and the float64 sums of VEC columns
template <int VEC> struct Vec;
template <> struct Vec<4> {
  float4 v;
  __device__ __forceinline__ void load(const float *p) {
    v = *reinterpret_cast<const float4 *>(p);
  }
};
template <> struct Vec<1> {
  float v;
  __device__ __forceinline__ void load(const float *p) { v = *p; }
};
template <int VEC> struct Acc;
template <> struct Acc<4> {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  __device__ __forceinline__ void add(const Vec<4> &o) {
    a[0] += (double)o.v.x;
    a[1] += (double)o.v.y;
    a[2] += (double)o.v.z;
    a[3] += (double)o.v.w;
  }
};
template <> struct Acc<1> {
  double a[1] = {0.0};
  __device__ __forceinline__ void add(const Vec<1> &o) { a[0] += (double)o.v; }
};
// the sums rounded to fp32 (an output row) or kept (a long row's piece)
template <int VEC>
__device__ __forceinline__ void store_sums(float *p, const Acc<VEC> &s, int valid) {
  if (VEC == 4 && valid >= 4) {
    *reinterpret_cast<float4 *>(p) =
        make_float4((float)s.a[0], (float)s.a[1], (float)s.a[2], (float)s.a[3]);
  } else {
    for (int k = 0; k < VEC && k < valid; k++) p[k] = (float)s.a[k];
  }
}
template <int VEC>
__device__ __forceinline__ void store_sums(double *p, const Acc<VEC> &s, int valid) {
  for (int k = 0; k < VEC && k < valid; k++) p[k] = s.a[k];
}

// One group of G lanes per output row (SEG: per piece of a long row, OUT =
// double). X points at the view's first column of source row 0, Y at the
// view's first column of output row 0 (SEG: at the partial rows).
template <int VEC, bool SEG, class OUT>
__global__ __launch_bounds__(kTB) void spmm_rows(
    const int32_t *__restrict__ rp, const int32_t *__restrict__ col, int n_out,
    const int2 *__restrict__ seg, int thresh, const float *__restrict__ X,
    int64_t ldx, OUT *__restrict__ Y, int64_t ldy, int ncols, int G) {
  const int lane = threadIdx.x & 63;
  const int sub = lane & (G - 1), grp = lane / G;
  const int64_t wave = (int64_t)blockIdx.x * (kTB / 64) + (threadIdx.x >> 6);
  const int64_t o = wave * (64 / G) + grp;
  if (o >= n_out) return;  // no barrier in this kernel
  int beg, end;
  if (SEG) {
    const int2 s = seg[o];
    beg = rp[s.x] + s.y * thresh;
    end = min(rp[s.x + 1], beg + thresh);
  } else {
    beg = rp[o];
    end = rp[o + 1];
    if (end - beg > thresh) return;  // a long row: its pieces and spmm_long_finish
  }
  const int ncg = (ncols + VEC - 1) / VEC;
  OUT *y = Y + o * ldy;
  for (int cg = sub; cg < ncg; cg += G) {
    const float *xb = X + cg * VEC;
    Acc<VEC> acc;
    Vec<VEC> v0, v1, v2, v3;
    int t = beg;
    for (; t + 4 <= end; t += 4) {  // four rows in flight, added in order
      const int c0 = col[t], c1 = col[t + 1], c2 = col[t + 2], c3 = col[t + 3];
      v0.load(xb + c0 * ldx);
      v1.load(xb + c1 * ldx);
      v2.load(xb + c2 * ldx);
      v3.load(xb + c3 * ldx);
      acc.add(v0);
      acc.add(v1);
      acc.add(v2);
      acc.add(v3);
    }
    for (; t < end; t++) {
      v0.load(xb + col[t] * ldx);
      acc.add(v0);
    }
    store_sums<VEC>(y + cg * VEC, acc, ncols - cg * VEC);
  }
}

// one workgroup per long row: its partial rows added in piece order
__global__ __launch_bounds__(kTB) void spmm_long_finish(
    const int32_t *__restrict__ rows, const int32_t *__restrict__ off,
    const double *__restrict__ part, int64_t ldp, float *__restrict__ Y,
    int64_t ldy, int ncols) {
  const int l = blockIdx.x;
  const int p0 = off[l], p1 = off[l + 1];
  float *y = Y + (int64_t)rows[l] * ldy;
  for (int c = threadIdx.x; c < ncols; c += kTB) {
    double s = 0.0;
    for (int p = p0; p < p1; p++) s += part[p * ldp + c];
    y[c] = (float)s;
  }
}

// ---- gram ------------------------------------------------------------------
constexpr int kGT = 64;   // output tile edge
constexpr int kGR = 32;   // rows staged per step

// partial[z][i][j] = sum over the rows of chunk z of P[r][i] Q[r][j]
__global__ __launch_bounds__(kTB) void gram_partial(
    const float *__restrict__ P, int64_t ldp, int p, const float *__restrict__ Q,
    int64_t ldq, int q, int64_t n, int64_t chunk, double *__restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float Ps[kGR][kGT];
  __shared__ __attribute__((aligned(16))) float Qs[kGR][kGT];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int i0 = blockIdx.x * kGT, j0 = blockIdx.y * kGT;
  const int64_t r_beg = (int64_t)blockIdx.z * chunk;
  const int64_t r_end = r_beg + chunk < n ? r_beg + chunk : n;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
  for (int64_t r0 = r_beg; r0 < r_end; r0 += kGR) {
#pragma unroll
    for (int k = 0; k < kGR * kGT / kTB; k++) {
      const int idx = tid + k * kTB, r = idx / kGT, c = idx % kGT;
      const int64_t row = r0 + r;
      const bool in = row < r_end;
      Ps[r][c] = in && i0 + c < p ? P[row * ldp + i0 + c] : 0.f;
      Qs[r][c] = in && j0 + c < q ? Q[row * ldq + j0 + c] : 0.f;
    }
    __syncthreads();
#pragma unroll 8
    for (int r = 0; r < kGR; r++) {
      const float4 a = *reinterpret_cast<const float4 *>(&Ps[r][ty * 4]);
      const float4 b = *reinterpret_cast<const float4 *>(&Qs[r][tx * 4]);
      const double av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = fma(av[x], bv[y], acc[x][y]);
    }
    __syncthreads();
  }
  double *out = partial + (int64_t)blockIdx.z * p * q;
#pragma unroll
  for (int x = 0; x < 4; x++)
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int i = i0 + ty * 4 + x, j = j0 + tx * 4 + y;
      if (i < p && j < q) out[(int64_t)i * q + j] = acc[x][y];
    }
}

__global__ __launch_bounds__(kTB) void gram_reduce(const double *__restrict__ partial,
                                                   int nz, int64_t pq,
                                                   double *__restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (k >= pq) return;
  double s = 0.0;
  for (int z = 0; z < nz; z++) s += partial[z * pq + k];
  out[k] = s;
}

// ---- apply -----------------------------------------------------------------
constexpr int kAK = 16;  // inner dimension staged per step

// D[r][j] = beta D[r][j] + sum_k S[r][k] M[k][j], M row-major q x p
__global__ __launch_bounds__(kTB) void apply_small(
    float *__restrict__ D, int64_t ldd, int p, const float *__restrict__ S,
    int64_t lds, int q, const double *__restrict__ M, double beta, int64_t n) {
  __shared__ float Ss[kGT][kAK + 1];
  __shared__ __attribute__((aligned(16))) double Ms[kAK][kGT];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * kGT;
  const int j0 = blockIdx.y * kGT;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
  for (int k0 = 0; k0 < q; k0 += kAK) {
#pragma unroll
    for (int k = 0; k < kGT * kAK / kTB; k++) {
      const int idx = tid + k * kTB;
      const int r = idx / kAK, c = idx % kAK;
      Ss[r][c] = r0 + r < n && k0 + c < q ? S[(r0 + r) * lds + k0 + c] : 0.f;
      const int mr = idx / kGT, mc = idx % kGT;
      Ms[mr][mc] = k0 + mr < q && j0 + mc < p ? M[(int64_t)(k0 + mr) * p + j0 + mc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kAK; k++) {
      double sv[4], mv[4];
#pragma unroll
      for (int x = 0; x < 4; x++) sv[x] = Ss[ty * 4 + x][k];
#pragma unroll
      for (int y = 0; y < 4; y++) mv[y] = Ms[k][tx * 4 + y];
#pragma unroll
      for (int x = 0; x < 4; x++)
#pragma unroll
        for (int y = 0; y < 4; y++) acc[x][y] = fma(sv[x], mv[y], acc[x][y]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int x = 0; x < 4; x++) {
    const int64_t r = r0 + ty * 4 + x;
    if (r >= n) continue;
#pragma unroll
    for (int y = 0; y < 4; y++) {
      const int j = j0 + tx * 4 + y;
      if (j >= p) continue;
      float *d = D + r * ldd + j;
      *d = (float)(beta != 0.0 ? fma(beta, (double)*d, acc[x][y]) : acc[x][y]);
    }
  }
}

__global__ __launch_bounds__(kTB) void scale_cols(float *__restrict__ Y, int64_t ld,
                                                  int ncols, int64_t n,
                                                  const double *__restrict__ s) {
  const int64_t k = (int64_t)blockIdx.x * kTB + threadIdx.x;
  if (k >= n * ncols) return;
  const int64_t r = k / ncols;
  const int c = (int)(k - r * ncols);
  Y[r * ld + c] = (float)((double)Y[r * ld + c] * s[c]);
}

// ---- cd_sweep --------------------------------------------------------------
// One sweep of the coordinate-descent NMF solver (sklearn's
// _update_cdnmf_fast, no regularisation, no shuffle) over the rows of the
// n x k view P, with B the matching rows of the sparse product and Q the
// k x k Gram of the other factor:
//   for t = 0..k-1:  g = sum_r Q[t][r] P[i][r] - B[i][t]
//                    viol += |P[i][t] == 0 ? min(g, 0) : g|
//                    if Q[t][t] != 0: P[i][t] = fp32(max(P[i][t] - g / Q[t][t], 0))
// all in float64, later coordinates seeing the rounded value.
//
// A group of G lanes (a power of two, k rounded up, at most 64) owns a row
// and lane `sub` of it holds the coordinates r = j G + sub (j < R) with their
// gradient entries g_r = (P_i Q - B_i)_r in float64 registers. The gradient
// is built coordinate by coordinate (g += P[i][t] Q^T[t][:] for the non-zero
// P[i][t]) and then kept up to date: step t's owner lane forms the new value
// and the change delta, one 64-bit shuffle hands delta to the group, and
// every lane adds delta Q^T[t][r] to its entries. A coordinate that stays
// clamped at zero (delta = 0) costs no row of Q. There is no cross-lane sum
// in the chain. QT is Q transposed, so that the entries a group reads at step
// t are consecutive; with LDSQ it is staged once per workgroup in LDS (16
// waves share it, consecutive float64 per lane: no bank conflict), above 160
// KiB (k > 143) it is read through L2. The row's violation is summed over
// the group by a fixed xor tree and written per row; cd_violation adds the
// rows in a fixed order. Rows are handed out grid-stride, and nothing a row
// computes depends on which group got it.
//
// Fused form (rp != nullptr): B is not read from a panel but formed here, row
// i of A X (or A^T X) summed in CSR column order in float64 from the other
// side's panel X (B, ldb then point at X), and never rounded to fp32. The
// gradient of a badly scaled component cancels B against the Gram terms, and
// there the fp32 rounding of a stored product is the solver's largest error
// (DESIGN §4.8). A row is gathered by its own group, however long it is.
template <int R, bool LDSQ>
__global__ __launch_bounds__(kCdTB) void cd_sweep_rows(
    float *__restrict__ P, int64_t ldp, const float *__restrict__ B, int64_t ldb, int k,
    const double *__restrict__ QT, int64_t n, int G, double *__restrict__ viol,
    const int32_t *__restrict__ rp, const int32_t *__restrict__ col) {
  extern __shared__ __attribute__((aligned(16))) double cd_q[];
  if (LDSQ) {
    for (int i = threadIdx.x; i < k * k; i += kCdTB) cd_q[i] = QT[i];
    __syncthreads();
  }
  auto qt = [&](int t, int r) -> double {
    return LDSQ ? cd_q[t * k + r] : QT[(int64_t)t * k + r];
  };
  const int lane = threadIdx.x & 63, sub = lane & (G - 1);
  const int rpw = 64 / G;
  const int64_t wave = (int64_t)blockIdx.x * (kCdTB / 64) + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * (kCdTB / 64) * rpw;
  // a group leaves as a whole: the shuffles below read lanes of the own group
  for (int64_t row = wave * rpw + lane / G; row < n; row += stride) {
    float *p = P + row * ldp;
    double g[R];
    float pv[R];
    if (rp) {
#pragma unroll
      for (int j = 0; j < R; j++) {
        const int r = j * G + sub;
        pv[j] = r < k ? p[r] : 0.f;
        g[j] = 0.0;
      }
      const int beg = rp[row], end = rp[row + 1];
      int e = beg;
      for (; e + 2 <= end; e += 2) {  // two source rows in flight, added in order
        const float *x0 = B + (int64_t)col[e] * ldb;
        const float *x1 = B + (int64_t)col[e + 1] * ldb;
        float a0[R], a1[R];
#pragma unroll
        for (int j = 0; j < R; j++) {
          const int r = j * G + sub;
          a0[j] = r < k ? x0[r] : 0.f;
          a1[j] = r < k ? x1[r] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < R; j++) g[j] = (g[j] - (double)a0[j]) - (double)a1[j];
      }
      if (e < end) {
        const float *x0 = B + (int64_t)col[e] * ldb;
#pragma unroll
        for (int j = 0; j < R; j++) {
          const int r = j * G + sub;
          if (r < k) g[j] -= (double)x0[r];
        }
      }
    } else {
      const float *b = B + row * ldb;
#pragma unroll
      for (int j = 0; j < R; j++) {
        const int r = j * G + sub;
        pv[j] = r < k ? p[r] : 0.f;
        g[j] = r < k ? -(double)b[r] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
      const int lim = min(G, k - j * G);
      for (int l = 0; l < lim; l++) {
        const float pt = __shfl(pv[j], l, G);
        if (pt != 0.f) {
          const int t = j * G + l;
          const double d = pt;
#pragma unroll
          for (int jj = 0; jj < R; jj++) {
            const int r = jj * G + sub;
            if (r < k) g[jj] = fma(d, qt(t, r), g[jj]);
          }
        }
      }
    }
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < R; j++) {
      const int lim = min(G, k - j * G);
      for (int l = 0; l < lim; l++) {
        const int t = j * G + l;
        double delta = 0.0;
        if (sub == l) {
          const double gt = g[j];
          const float pt = pv[j];
          v += fabs(pt == 0.f ? fmin(gt, 0.0) : gt);
          const double qtt = qt(t, t);
          if (qtt != 0.0) {
            const float nw = (float)fmax((double)pt - gt / qtt, 0.0);
            delta = (double)nw - (double)pt;
            pv[j] = nw;
          }
        }
        delta = __shfl(delta, l, G);
        if (delta != 0.0) {
#pragma unroll
          for (int jj = 0; jj < R; jj++) {
            const int r = jj * G + sub;
            if (r < k) g[jj] = fma(delta, qt(t, r), g[jj]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < R; j++) {
      const int r = j * G + sub;
      if (r < k) p[r] = pv[j];
    }
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
    if (sub == 0) viol[row] = v;
  }
}

// out[0] = the n per-row violations added in a fixed order: thread i adds the
// rows i, i + 1024, ... in turn, then a tree over the threads
__global__ __launch_bounds__(kCdTB) void cd_violation(const double *__restrict__ viol,
                                                      int64_t n, double *__restrict__ out) {
  __shared__ double red[kCdTB];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kCdTB) s += viol[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kCdTB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// ---- host side -------------------------------------------------------------
int make_long(hgx_svd *s, const DevBuf &rp_dev, int32_t nrows, SvdLong &out) {
  hgx_ctx *ctx = s->ctx;
  std::vector<int32_t> rp((size_t)nrows + 1);
  HGX_HIP(ctx, hipMemcpy(rp.data(), rp_dev.p, sizeof(int32_t) * rp.size(),
                         hipMemcpyDeviceToHost));
  std::vector<int32_t> rows, off(1, 0), seg;
  for (int32_t r = 0; r < nrows; r++) {
    const int64_t len = rp[r + 1] - rp[r];
    if (len <= s->thresh) continue;
    const int pieces = (int)((len + s->thresh - 1) / s->thresh);
    rows.push_back(r);
    for (int p = 0; p < pieces; p++) {
      seg.push_back(r);
      seg.push_back(p);
    }
    off.push_back(off.back() + pieces);
  }
  out.nlong = (int)rows.size();
  out.nseg = off.back();
  if (!out.nlong) return HGX_OK;
  HGX_TRY(hgx_ensure(ctx, out.rows, sizeof(int32_t) * rows.size()));
  HGX_TRY(hgx_ensure(ctx, out.off, sizeof(int32_t) * off.size()));
  HGX_TRY(hgx_ensure(ctx, out.seg, sizeof(int32_t) * seg.size()));
  HGX_HIP(ctx, hipMemcpy(out.rows.p, rows.data(), sizeof(int32_t) * rows.size(),
                         hipMemcpyHostToDevice));
  HGX_HIP(ctx, hipMemcpy(out.off.p, off.data(), sizeof(int32_t) * off.size(),
                         hipMemcpyHostToDevice));
  HGX_HIP(ctx, hipMemcpy(out.seg.p, seg.data(), sizeof(int32_t) * seg.size(),
                         hipMemcpyHostToDevice));
  return HGX_OK;
}

// the column range [col0, col0 + ncols) of a slot, checked
int view(hgx_svd *s, int slot, int col0, int ncols, Panel **out) {
  hgx_ctx *ctx = s->ctx;
  HGX_CHECK(ctx, slot >= 0 && slot < kSlots, HGX_EINVAL, "panel slot %d out of range",
            slot);
  Panel *p = &s->panel[slot];
  HGX_CHECK(ctx, p->side >= 0, HGX_ESTATE, "panel slot %d is not allocated", slot);
  HGX_CHECK(ctx, col0 >= 0 && ncols > 0 && (int64_t)col0 + ncols <= p->width,
            HGX_EINVAL, "columns [%d, %d + %d) outside panel %d of width %d", col0,
            col0, ncols, slot, p->width);
  *out = p;
  return HGX_OK;
}

bool overlap(int sa, int a0, int na, int sb, int b0, int nb) {
  return sa == sb && a0 < b0 + nb && b0 < a0 + na;
}

int settle_spmm(hgx_svd *s) {
  if (!s->spmm_pending) return HGX_OK;
  float ms = 0;
  HGX_HIP(s->ctx, hipEventSynchronize(s->e1));
  HGX_HIP(s->ctx, hipEventElapsedTime(&ms, s->e0, s->e1));
  s->spmm_ms += ms;
  s->spmm_bytes += s->spmm_pending_bytes;
  s->spmm_pending = false;
  return HGX_OK;
}

template <int VEC>
int launch_spmm(hgx_svd *s, int dside, const float *X, int64_t ldx, float *Y,
                int64_t ldy, int ncols) {
  hgx_ctx *ctx = s->ctx;
  const int32_t *rp = (dside ? ctx->rp_n : ctx->rp_e).as<int32_t>();
  const int32_t *col = (dside ? ctx->col_n : ctx->col_e).as<int32_t>();
  const int nrows = dside ? s->N : s->E;
  const SvdLong &lg = s->lg[dside];
  const int ncg = (ncols + VEC - 1) / VEC;
  int G = 1;
  while (G < 64 && G < ncg) G <<= 1;
  const int rpw = 64 / G, wpb = kTB / 64;
  auto blocks = [&](int64_t n_out) {
    const int64_t waves = (n_out + rpw - 1) / rpw;
    return (unsigned)((waves + wpb - 1) / wpb);
  };
  hipLaunchKernelGGL((spmm_rows<VEC, false, float>), dim3(blocks(nrows)), dim3(kTB), 0,
                     ctx->stream, rp, col, nrows, (const int2 *)nullptr, s->thresh, X,
                     ldx, Y, ldy, ncols, G);
  HGX_LAUNCH_CHECK(ctx);
  if (lg.nseg) {
    const int64_t ldp = (ncols + 3) / 4 * 4;
    HGX_TRY(hgx_ensure(ctx, s->part, sizeof(double) * (size_t)lg.nseg * ldp));
    hipLaunchKernelGGL((spmm_rows<VEC, true, double>), dim3(blocks(lg.nseg)), dim3(kTB),
                       0, ctx->stream, rp, col, lg.nseg, lg.seg.as<int2>(), s->thresh,
                       X, ldx, s->part.as<double>(), ldp, ncols, G);
    HGX_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(spmm_long_finish, dim3(lg.nlong), dim3(kTB), 0, ctx->stream,
                       lg.rows.as<int32_t>(), lg.off.as<int32_t>(),
                       s->part.as<double>(), ldp, Y, ldy, ncols);
    HGX_LAUNCH_CHECK(ctx);
  }
  return HGX_OK;
}

template <int R, bool LDSQ>
int launch_cd(hgx_svd *s, float *P, int64_t ldp, const float *B, int64_t ldb, int k,
              int64_t n, int G, const int32_t *rp, const int32_t *col) {
  hgx_ctx *ctx = s->ctx;
  const size_t lds = LDSQ ? sizeof(double) * (size_t)k * k : 0;
  auto kern = cd_sweep_rows<R, LDSQ>;
  if (lds > 64 * 1024)
    HGX_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
  // resident workgroups only (two of 1024 threads fit a CU when their LDS
  // does): a workgroup stages Q once and walks its rows grid-stride
  const int64_t per_block = (int64_t)(kCdTB / 64) * (64 / G);
  const int64_t need = (n + per_block - 1) / per_block;
  const int64_t cap = (int64_t)std::max(s->ncu, 1) * (lds <= kCdLds / 2 ? 2 : 1);
  hipLaunchKernelGGL(kern, dim3((unsigned)std::min(need, cap)), dim3(kCdTB), lds,
                     ctx->stream, P, ldp, B, ldb, k, s->cdq.as<double>(), n, G,
                     s->cdviol.as<double>(), rp, col);
  HGX_LAUNCH_CHECK(ctx);
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_svd_create(hgx_ctx *ctx, int long_row, hgx_svd **out) {
  if (!ctx || !out) return HGX_EINVAL;
  *out = nullptr;
  HGX_CHECK(ctx, ctx->N > 0 && ctx->E > 0 && ctx->rp_n.p && ctx->rp_e.p, HGX_ESTATE,
            "hgx_svd_create before hgx_upload_incidence");
  HGX_CHECK(ctx, long_row == 0 || (long_row >= 4 && long_row <= (1 << 20)), HGX_EINVAL,
            "long-row threshold %d outside [4, 2^20]", long_row);
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  hgx_svd *s = new hgx_svd();
  s->ctx = ctx;
  s->thresh = long_row ? long_row : kLongRow;
  s->N = ctx->N;
  s->E = ctx->E;
  s->nnz = ctx->nnz;
  s->inc_gen = ctx->inc_gen;
  int rc = make_long(s, ctx->rp_e, ctx->E, s->lg[0]);
  if (!rc) rc = make_long(s, ctx->rp_n, ctx->N, s->lg[1]);
  if (!rc && hipEventCreate(&s->e0) != hipSuccess) rc = hgx_fail(ctx, HGX_EHIP, "event");
  if (!rc && hipEventCreate(&s->e1) != hipSuccess) rc = hgx_fail(ctx, HGX_EHIP, "event");
  if (!rc && hipEventCreate(&s->c0) != hipSuccess) rc = hgx_fail(ctx, HGX_EHIP, "event");
  if (!rc && hipEventCreate(&s->c1) != hipSuccess) rc = hgx_fail(ctx, HGX_EHIP, "event");
  if (!rc && hipDeviceGetAttribute(&s->ncu, hipDeviceAttributeMultiprocessorCount,
                                   ctx->device) != hipSuccess)
    rc = hgx_fail(ctx, HGX_EHIP, "multiprocessor count");
  if (rc) {
    hgx_svd_destroy(s);
    return rc;
  }
  *out = s;
  return HGX_OK;
}

extern "C" int hgx_svd_destroy(hgx_svd *s) {
  if (!s) return HGX_OK;
  if (s->ctx) hipStreamSynchronize(s->ctx->stream);
  for (Panel &p : s->panel) hgx_release(p.buf);
  for (SvdLong &l : s->lg) {
    hgx_release(l.seg);
    hgx_release(l.off);
    hgx_release(l.rows);
  }
  for (DevBuf *b : {&s->part, &s->gpart, &s->gout, &s->mdev, &s->cdq, &s->cdviol})
    hgx_release(*b);
  for (hipEvent_t e : {s->e0, s->e1, s->c0, s->c1})
    if (e) hipEventDestroy(e);
  delete s;
  return HGX_OK;
}

extern "C" int hgx_svd_panel(hgx_svd *s, int slot, int side, int width) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  HGX_CHECK(ctx, slot >= 0 && slot < kSlots, HGX_EINVAL, "panel slot %d out of range",
            slot);
  HGX_CHECK(ctx, side == 0 || side == 1, HGX_EINVAL, "side must be 0 (edges) or 1 (nodes)");
  HGX_CHECK(ctx, width > 0 && width <= (1 << 16), HGX_EINVAL, "panel width %d", width);
  HGX_CHECK(ctx, s->inc_gen == ctx->inc_gen, HGX_ESTATE,
            "the incidence changed after hgx_svd_create");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  Panel &p = s->panel[slot];
  const int ld = (width + 3) / 4 * 4;
  const int64_t rows = side ? s->N : s->E;
  const size_t bytes = sizeof(float) * (size_t)rows * ld;
  HGX_TRY(hgx_ensure(ctx, p.buf, bytes));
  HGX_HIP(ctx, hipMemsetAsync(p.buf.p, 0, bytes, ctx->stream));
  p.side = side;
  p.width = width;
  p.ld = ld;
  p.rows = rows;
  return HGX_OK;
}

extern "C" int hgx_svd_set(hgx_svd *s, int slot, int col0, int ncols,
                           const float *host) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *p;
  HGX_TRY(view(s, slot, col0, ncols, &p));
  HGX_CHECK(ctx, host, HGX_EINVAL, "null host matrix");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_HIP(ctx, hipMemcpy2DAsync(p->buf.as<float>() + col0, sizeof(float) * p->ld, host,
                                sizeof(float) * ncols, sizeof(float) * ncols,
                                (size_t)p->rows, hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_svd_get(hgx_svd *s, int slot, int col0, int ncols, float *host) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *p;
  HGX_TRY(view(s, slot, col0, ncols, &p));
  HGX_CHECK(ctx, host, HGX_EINVAL, "null host matrix");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_HIP(ctx, hipMemcpy2DAsync(host, sizeof(float) * ncols,
                                p->buf.as<float>() + col0, sizeof(float) * p->ld,
                                sizeof(float) * ncols, (size_t)p->rows,
                                hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_svd_copy(hgx_svd *s, int dst, int dcol0, int src, int scol0,
                            int ncols) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *d, *q;
  HGX_TRY(view(s, dst, dcol0, ncols, &d));
  HGX_TRY(view(s, src, scol0, ncols, &q));
  HGX_CHECK(ctx, d->side == q->side, HGX_EINVAL, "copy between panels of two sides");
  HGX_CHECK(ctx, !overlap(dst, dcol0, ncols, src, scol0, ncols), HGX_EINVAL,
            "copy onto overlapping columns of one panel");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_HIP(ctx, hipMemcpy2DAsync(d->buf.as<float>() + dcol0, sizeof(float) * d->ld,
                                q->buf.as<float>() + scol0, sizeof(float) * q->ld,
                                sizeof(float) * ncols, (size_t)d->rows,
                                hipMemcpyDeviceToDevice, ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_svd_spmm(hgx_svd *s, int dst, int dcol0, int src, int scol0,
                            int ncols) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *d, *x;
  HGX_TRY(view(s, dst, dcol0, ncols, &d));
  HGX_TRY(view(s, src, scol0, ncols, &x));
  HGX_CHECK(ctx, d->side != x->side, HGX_EINVAL,
            "the product maps one side's panel to the other side's");
  HGX_CHECK(ctx, s->inc_gen == ctx->inc_gen, HGX_ESTATE,
            "the incidence changed after hgx_svd_create");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_TRY(settle_spmm(s));
  const float *X = x->buf.as<float>() + scol0;
  float *Y = d->buf.as<float>() + dcol0;
  HGX_HIP(ctx, hipEventRecord(s->e0, ctx->stream));
  if (dcol0 % 4 == 0 && scol0 % 4 == 0)
    HGX_TRY(launch_spmm<4>(s, d->side, X, x->ld, Y, d->ld, ncols));
  else
    HGX_TRY(launch_spmm<1>(s, d->side, X, x->ld, Y, d->ld, ncols));
  HGX_HIP(ctx, hipEventRecord(s->e1, ctx->stream));
  s->spmm_pending = true;
  // algorithmic bytes: the column indices, one source row per incidence, one
  // output row per row
  s->spmm_pending_bytes = 4.0 * s->nnz + 4.0 * ncols * s->nnz + 4.0 * ncols * d->rows;
  s->spmm_calls++;
  s->spmm_cols += ncols;
  return HGX_OK;
}

extern "C" int hgx_svd_gram(hgx_svd *s, int pslot, int pcol0, int p, int qslot,
                            int qcol0, int q, double *out) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *P, *Q;
  HGX_TRY(view(s, pslot, pcol0, p, &P));
  HGX_TRY(view(s, qslot, qcol0, q, &Q));
  HGX_CHECK(ctx, P->side == Q->side, HGX_EINVAL, "Gram of panels of two sides");
  HGX_CHECK(ctx, p <= kMaxSmall && q <= kMaxSmall, HGX_EUNSUP,
            "Gram of more than %d columns", kMaxSmall);
  HGX_CHECK(ctx, out, HGX_EINVAL, "null result matrix");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t n = P->rows, pq = (int64_t)p * q;
  const int tp = (p + kGT - 1) / kGT, tq = (q + kGT - 1) / kGT;
  // row chunks: a fixed function of the shape, so the sum has a fixed order
  int64_t nz = std::min<int64_t>((n + 511) / 512, std::max(1, 1024 / (tp * tq)));
  nz = std::max<int64_t>(nz, 1);
  int64_t chunk = ((n + nz - 1) / nz + kGR - 1) / kGR * kGR;
  nz = (n + chunk - 1) / chunk;
  HGX_TRY(hgx_ensure(ctx, s->gpart, sizeof(double) * (size_t)(nz * pq)));
  HGX_TRY(hgx_ensure(ctx, s->gout, sizeof(double) * (size_t)pq));
  hipLaunchKernelGGL(gram_partial, dim3(tp, tq, (unsigned)nz), dim3(kTB), 0, ctx->stream,
                     P->buf.as<float>() + pcol0, (int64_t)P->ld, p,
                     Q->buf.as<float>() + qcol0, (int64_t)Q->ld, q, n, chunk,
                     s->gpart.as<double>());
  HGX_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(gram_reduce, dim3((unsigned)((pq + kTB - 1) / kTB)), dim3(kTB), 0,
                     ctx->stream, s->gpart.as<double>(), (int)nz, pq,
                     s->gout.as<double>());
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipMemcpyAsync(out, s->gout.p, sizeof(double) * pq,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  s->dense_calls++;
  return HGX_OK;
}

extern "C" int hgx_svd_apply(hgx_svd *s, int dst, int dcol0, int p, int src,
                             int scol0, int q, const double *M, double beta) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *D, *S;
  HGX_TRY(view(s, dst, dcol0, p, &D));
  HGX_TRY(view(s, src, scol0, q, &S));
  HGX_CHECK(ctx, D->side == S->side, HGX_EINVAL, "apply between panels of two sides");
  HGX_CHECK(ctx, p <= kMaxSmall && q <= kMaxSmall, HGX_EUNSUP,
            "apply of a matrix with more than %d rows or columns", kMaxSmall);
  HGX_CHECK(ctx, !overlap(dst, dcol0, p, src, scol0, q), HGX_EINVAL,
            "apply onto its own source columns");
  HGX_CHECK(ctx, M, HGX_EINVAL, "null matrix");
  for (int64_t k = 0; k < (int64_t)p * q; k++)
    HGX_CHECK(ctx, std::isfinite(M[k]), HGX_EVALUE, "the matrix holds a non-finite value");
  HGX_CHECK(ctx, std::isfinite(beta), HGX_EVALUE, "beta is not finite");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)p * q;
  HGX_TRY(hgx_ensure(ctx, s->mdev, bytes));
  // on the stream, so behind the previous apply that still reads the buffer
  HGX_HIP(ctx, hipMemcpyAsync(s->mdev.p, M, bytes, hipMemcpyHostToDevice,
                              ctx->stream));
  const int64_t n = D->rows;
  hipLaunchKernelGGL(apply_small, dim3((unsigned)((n + kGT - 1) / kGT), (p + kGT - 1) / kGT),
                     dim3(kTB), 0, ctx->stream, D->buf.as<float>() + dcol0,
                     (int64_t)D->ld, p, S->buf.as<float>() + scol0, (int64_t)S->ld, q,
                     s->mdev.as<double>(), beta, n);
  HGX_LAUNCH_CHECK(ctx);
  s->dense_calls++;
  return HGX_OK;
}

extern "C" int hgx_svd_scale(hgx_svd *s, int slot, int col0, int ncols,
                             const double *scale) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *P;
  HGX_TRY(view(s, slot, col0, ncols, &P));
  HGX_CHECK(ctx, scale, HGX_EINVAL, "null scale vector");
  HGX_CHECK(ctx, ncols <= kMaxSmall, HGX_EUNSUP, "scale of more than %d columns",
            kMaxSmall);
  for (int k = 0; k < ncols; k++)
    HGX_CHECK(ctx, std::isfinite(scale[k]), HGX_EVALUE, "scale %d is not finite", k);
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bytes = sizeof(double) * (size_t)ncols;
  HGX_TRY(hgx_ensure(ctx, s->mdev, bytes));
  HGX_HIP(ctx, hipMemcpyAsync(s->mdev.p, scale, bytes, hipMemcpyHostToDevice,
                              ctx->stream));
  const int64_t total = P->rows * ncols;
  hipLaunchKernelGGL(scale_cols, dim3((unsigned)((total + kTB - 1) / kTB)), dim3(kTB), 0,
                     ctx->stream, P->buf.as<float>() + col0, (int64_t)P->ld, ncols,
                     P->rows, s->mdev.as<double>());
  HGX_LAUNCH_CHECK(ctx);
  s->dense_calls++;
  return HGX_OK;
}

extern "C" int hgx_svd_last_stats(hgx_svd *s, double *spmm_ms, double *spmm_bytes,
                                  int64_t *spmm_calls, int64_t *spmm_cols,
                                  int64_t *dense_calls) {
  if (!s) return HGX_EINVAL;
  HGX_TRY(settle_spmm(s));
  if (spmm_ms) *spmm_ms = s->spmm_ms;
  if (spmm_bytes) *spmm_bytes = s->spmm_bytes;
  if (spmm_calls) *spmm_calls = s->spmm_calls;
  if (spmm_cols) *spmm_cols = s->spmm_cols;
  if (dense_calls) *dense_calls = s->dense_calls;
  return HGX_OK;
}

namespace {

// fused: bslot is the other side's panel X and B = A X (A^T X) is formed in
// the kernel
int cd_sweep(hgx_svd *s, int pslot, int pcol0, int bslot, int bcol0, int k,
             const double *Q, double *violation, bool fused) {
  if (!s) return HGX_EINVAL;
  hgx_ctx *ctx = s->ctx;
  Panel *P, *B;
  HGX_TRY(view(s, pslot, pcol0, k, &P));
  HGX_TRY(view(s, bslot, bcol0, k, &B));
  const int32_t *rp = nullptr, *col = nullptr;
  if (fused) {
    HGX_CHECK(ctx, P->side != B->side, HGX_EINVAL,
              "the fused sweep takes the other side's panel as its source");
    HGX_CHECK(ctx, s->inc_gen == ctx->inc_gen, HGX_ESTATE,
              "the incidence changed after hgx_svd_create");
    rp = (P->side ? ctx->rp_n : ctx->rp_e).as<int32_t>();
    col = (P->side ? ctx->col_n : ctx->col_e).as<int32_t>();
  } else {
    HGX_CHECK(ctx, P->side == B->side, HGX_EINVAL, "sweep over panels of two sides");
    HGX_CHECK(ctx, !overlap(pslot, pcol0, k, bslot, bcol0, k), HGX_EINVAL,
              "sweep whose factor and product share columns of one panel");
  }
  HGX_CHECK(ctx, k <= kCdMaxK, HGX_EUNSUP, "sweep of more than %d columns", kCdMaxK);
  HGX_CHECK(ctx, Q && violation, HGX_EINVAL, "null matrix or result");
  for (int64_t i = 0; i < (int64_t)k * k; i++)
    HGX_CHECK(ctx, std::isfinite(Q[i]), HGX_EVALUE, "the matrix holds a non-finite value");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t n = P->rows;
  std::vector<double> qt((size_t)k * k);
  for (int t = 0; t < k; t++)
    for (int r = 0; r < k; r++) qt[(size_t)r * k + t] = Q[(size_t)t * k + r];
  HGX_TRY(hgx_ensure(ctx, s->cdq, sizeof(double) * qt.size()));
  HGX_TRY(hgx_ensure(ctx, s->cdviol, sizeof(double) * (size_t)(n + 1)));
  HGX_HIP(ctx, hipMemcpyAsync(s->cdq.p, qt.data(), sizeof(double) * qt.size(),
                              hipMemcpyHostToDevice, ctx->stream));
  int G = 1;
  while (G < 64 && G < k) G <<= 1;
  const int R = (k + G - 1) / G;
  const bool ldsq = sizeof(double) * qt.size() <= kCdLds;
  float *p = P->buf.as<float>() + pcol0;
  const float *b = B->buf.as<float>() + bcol0;
  const int64_t ldp = P->ld, ldb = B->ld;
  HGX_HIP(ctx, hipEventRecord(s->c0, ctx->stream));
  if (ldsq) {  // k <= 143: R <= 3
    if (R == 1) HGX_TRY((launch_cd<1, true>(s, p, ldp, b, ldb, k, n, G, rp, col)));
    else if (R == 2) HGX_TRY((launch_cd<2, true>(s, p, ldp, b, ldb, k, n, G, rp, col)));
    else HGX_TRY((launch_cd<3, true>(s, p, ldp, b, ldb, k, n, G, rp, col)));
  } else {
    if (R <= 3) HGX_TRY((launch_cd<3, false>(s, p, ldp, b, ldb, k, n, G, rp, col)));
    else if (R == 4) HGX_TRY((launch_cd<4, false>(s, p, ldp, b, ldb, k, n, G, rp, col)));
    else if (R <= 6) HGX_TRY((launch_cd<6, false>(s, p, ldp, b, ldb, k, n, G, rp, col)));
    else HGX_TRY((launch_cd<kCdMaxR, false>(s, p, ldp, b, ldb, k, n, G, rp, col)));
  }
  double *sum = s->cdviol.as<double>() + n;
  hipLaunchKernelGGL(cd_violation, dim3(1), dim3(kCdTB), 0, ctx->stream,
                     s->cdviol.as<double>(), n, sum);
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipEventRecord(s->c1, ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(violation, sum, sizeof(double), hipMemcpyDeviceToHost,
                              ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // qt is read until here
  float ms = 0;
  HGX_HIP(ctx, hipEventElapsedTime(&ms, s->c0, s->c1));
  s->cd_ms += ms;
  s->cd_sweeps++;
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_svd_cd_sweep(hgx_svd *s, int pslot, int pcol0, int bslot, int bcol0,
                                int k, const double *Q, double *violation) {
  return cd_sweep(s, pslot, pcol0, bslot, bcol0, k, Q, violation, false);
}

extern "C" int hgx_svd_cd_sweep_fused(hgx_svd *s, int pslot, int pcol0, int xslot,
                                      int xcol0, int k, const double *Q,
                                      double *violation) {
  return cd_sweep(s, pslot, pcol0, xslot, xcol0, k, Q, violation, true);
}

extern "C" int hgx_svd_cd_last_stats(hgx_svd *s, double *sweep_ms, int64_t *sweeps) {
  if (!s) return HGX_EINVAL;
  if (sweep_ms) *sweep_ms = s->cd_ms;
  if (sweeps) *sweeps = s->cd_sweeps;
  return HGX_OK;
}
