// Trainer kernels, deferred-row step: fixed point, SV<>, the row-0 helpers,
// train_step, train_step_pair, train_step_quad and train_flush.
#pragma once
#include "hgx_divk.h"
#include "hgx_fix.h"
#include "hgx_train_split.h"

namespace {

// Padding-row (row 0) state for the fused path, computed by every workgroup
// of a batch (identical inputs and order, so identical values): mode 0 ->
// the tables hold it; mode 1 -> it is pending from the previous fused batch:
// (p, acc) = Adagrad(r0src, sum of that batch's np per-workgroup partials).
// row0_issue starts every load unconditionally (a load under a branch is
// waited for at the join), first thing in the kernel; row0_finish sums in a
// fixed order (thread `sub` of a column: partials sub, sub+TPC, ...; then
// the TPC sums in order) and returns the column's (p, acc) on sub == 0.
// col < 2L covers both tables (table = col / L, float4 column col % L).

// ---------------------------------------------------------------------------
// Deferred-row batch step (train_step): one launch per batch, no packing
// constraint on which workgroup holds which record.
//
// Keras applies one Adagrad update per batch with the gradients of a row's
// slots summed (hg2v_model.py:51-203 through TF's dense IndexedSlices sum).
//  - A row with ONE slot in batch b (most rows) is updated in place by the
//    lane group of its record, right after the backward pass.
//  - A row with several slots in b ("deferred" row, entry m of b) cannot be
//    summed in one place without a grid-wide barrier. Each slot adds its
//    gradient to gacc[b % 3][m] as 2^44 fixed point with integer atomics:
//    the sum is exact and independent of arrival order, so the step stays
//    bitwise reproducible. The row's owner slot writes the row's state as b
//    read it, (p, a), to shadow[b % 3][m]. The update itself is applied by
//    launch b + 1: every slot of b + 1 that touches the row ("pending" slot,
//    code kSPend, entry m') reads shadow + gacc and folds the Adagrad step
//    of b in registers (all readers compute the same bits); a deferred row of
//    b that b + 1 does not touch is written back by a "flush slot" of b + 1.
//  - The padding row 0 of both tables (nearly every record) goes the same
//    way without atomics: each workgroup stores its fixed-order LDS partial
//    (plain stores: an atomic add's completion at the kernel tail measured
//    0.7 us), every workgroup of b + 1 sums the partials in a fixed order and
//    folds the step; workgroup 0 keeps the base in shadow entry 0 / 1.
// Nothing of batch b + 1 reads a location batch b + 1 writes: the table rows
// it writes are single-slot rows of b + 1 (read only by their own group) or
// flushed rows (not read by b + 1); shadow and gacc are triple-buffered by
// batch parity, gp double-buffered. train_flush applies the last batch's
// deferred rows at the end of every epoch. A parity's gacc entries are zeroed
// two launches after their use (the count rides in the record words).
// ---------------------------------------------------------------------------

// Kernel arguments of the step. Round trip 1 (the record words) is addressed
// from scalars alone, placed ahead of the by-value TrainArgs so that the
// translation unit's kernel-argument preloading (build.py) delivers them in
// SGPRs at wave start: the chunk-local batch's bases into the placed buffers
// (pidx / pcode / ptgt + cb NBF RPB words, computed by the driver), RW, the
// batch's record count, q, and 1 / records (IEEE single division is
// correctly rounded on the host as on the device: the same bits). A by-value
// struct ends preloading, so it comes last. HGX_TRAIN_PRELOAD=0 (A/B
// builds): TrainArgs first, the bases formed in the kernel from a.pidx and
// cb, two dependent scalar round trips ahead of the record-word loads.
// HGX_TRAIN_HOSTINVB=0 (A/B builds): 1 / records divided on every wave.
#ifndef HGX_TRAIN_PRELOAD
#define HGX_TRAIN_PRELOAD 1
#endif
#ifndef HGX_TRAIN_HOSTINVB
#define HGX_TRAIN_HOSTINVB HGX_TRAIN_PRELOAD
#endif
struct StepWords {
  const int *pidx;  // this batch's record words, workgroup 0's first group
  const unsigned *pcode;
  const float *ptgt;
  int RW;
  float inv_b;
};
#if HGX_TRAIN_PRELOAD
#define HGX_STEP_PARAMS                                                              \
  const int *w_pidx, const unsigned *w_pcode, const float *w_ptgt, int w_rw, int nb, \
      int q, float w_inv_b, int gb, int cb, TrainArgs a
#define HGX_STEP_WORDS(RPB)                                \
  const StepWords w = {w_pidx, w_pcode, w_ptgt, w_rw,      \
                       HGX_TRAIN_HOSTINVB ? w_inv_b : 1.0f / (float)nb}
#else
#define HGX_STEP_PARAMS TrainArgs a, int cb, int gb, int nb, int q
#define HGX_STEP_WORDS(RPB)                                                       \
  const size_t w_g0 = (size_t)cb * gridDim.x * (RPB);                             \
  const StepWords w = {a.pidx + w_g0 * a.RW, a.pcode + w_g0 * a.RW, a.ptgt + w_g0 * 3, \
                       a.RW, 1.0f / (float)nb}
#endif

// fixed point of the deferred-row gradient sums: kFixScale, kFixLimit and
// to_fix in hgx_fix.h (shared with the host check). from_fix keeps its
// int64 -> double step: it rounds for sums above 2^53, and that rounding is
// part of the step's bits.
__device__ __forceinline__ float from_fix(long long v) {
  return (float)((double)v * kFixInv);
}
// The head math's divisions by the neighbour count (the two means and the
// mean's gradient, on every wave of a record between the exchange barrier
// and the first store): div_const of hgx_divk.h for the K it is proven
// bit-equal to the division for, the division otherwise. Every form of the
// step goes through here (train_flush divides nothing by K).
// HGX_TRAIN_DIVK=0 (A/B builds): the IEEE division.
#ifndef HGX_TRAIN_DIVK
#define HGX_TRAIN_DIVK 1
#endif
template <int K>
__device__ __forceinline__ float div_k(float x) {
  if constexpr (HGX_TRAIN_DIVK && K == 5) return div_const<K>(x);
  else return x / (float)K;
}
// The step's scalar head math (contraction off, see mul_nc)
__device__ __forceinline__ float act_d_nc(int act, float z, float y) {
  return act == 0 ? mul_nc(y, sub_nc(1.0f, y)) : (z > 0.f ? 1.f : 0.f);
}
__device__ __forceinline__ void head_loss_nc(int loss, float y, float yt,
                                             float &lv, float &g) {
  const float eps = 1e-7f;
  if (loss == 0) {  // KLD with Keras clipping
    const float ytc = fminf(fmaxf(yt, eps), 1.f);
    const float ypc = fminf(fmaxf(y, eps), 1.f);
    lv = mul_nc(ytc, logf(ytc / ypc));
    g = (y >= eps && y <= 1.f) ? -ytc / ypc : 0.f;
  } else {  // MSE
    const float df = sub_nc(y, yt);
    lv = mul_nc(df, df);
    g = 2.f * df;
  }
}

// The step's per-lane vector: VW floats of a row (float4: dp = 4L, float2:
// dp = 2L), the fixed-point view of this lane's part of a gacc entry, and the
// ops on them
template <int VW>
struct SV;
template <>
struct SV<4> {
  using T = float4;
  struct Fx {
    longlong2 a, b;
  };
  static __device__ __forceinline__ T zero() { return f4(0.f); }
  static __device__ __forceinline__ T add(T x, T y) { return x + y; }
  static __device__ __forceinline__ T mul(T x, float m) {
    return make_float4(x.x * m, x.y * m, x.z * m, x.w * m);
  }
  static __device__ __forceinline__ T fma(float s, T v, T c) { return fma4(s, v, c); }
  static __device__ __forceinline__ float dot(T x, T y) { return dot4(x, y); }
  static __device__ __forceinline__ void adagrad(T &p, T &ac, T g, float lr, float eps) {
    adagrad4_hw(p, ac, g, lr, eps);
  }
  static __device__ __forceinline__ void pin(T &v) {
    asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
  }
  static __device__ __forceinline__ Fx ldfix(const long long *e, int lane) {
    const longlong2 *g = reinterpret_cast<const longlong2 *>(e) + 2 * lane;
    return {g[0], g[1]};
  }
  static __device__ __forceinline__ T unfix(const Fx &g) {
    return make_float4(from_fix(g.a.x), from_fix(g.a.y), from_fix(g.b.x), from_fix(g.b.y));
  }
  static __device__ __forceinline__ void addfix(long long *e, int lane, T v, int &bad) {
    bad |= !(fabsf(v.x) < kFixLimit) | !(fabsf(v.y) < kFixLimit) |
           !(fabsf(v.z) < kFixLimit) | !(fabsf(v.w) < kFixLimit);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(e) + 4 * lane;
    atomicAdd(d + 0, to_fix<4>(v.x));
    atomicAdd(d + 1, to_fix<4>(v.y));
    atomicAdd(d + 2, to_fix<4>(v.z));
    atomicAdd(d + 3, to_fix<4>(v.w));
  }
  static __device__ __forceinline__ void zerofix(long long *e, int lane) {
    longlong2 *g = reinterpret_cast<longlong2 *>(e) + 2 * lane;
    g[0] = g[1] = make_longlong2(0, 0);
  }
  static __device__ __forceinline__ Fx fxadd(const Fx &x, const Fx &y) {
    return {make_longlong2(x.a.x + y.a.x, x.a.y + y.a.y),
            make_longlong2(x.b.x + y.b.x, x.b.y + y.b.y)};
  }
  static __device__ __forceinline__ Fx fxzero() {
    return {make_longlong2(0, 0), make_longlong2(0, 0)};
  }
};
template <>
struct SV<2> {
  using T = float2;
  struct Fx {
    longlong2 a;
  };
  static __device__ __forceinline__ T zero() { return make_float2(0.f, 0.f); }
  static __device__ __forceinline__ T add(T x, T y) { return make_float2(x.x + y.x, x.y + y.y); }
  static __device__ __forceinline__ T mul(T x, float m) { return make_float2(x.x * m, x.y * m); }
  static __device__ __forceinline__ T fma(float s, T v, T c) {
    return make_float2(fmaf(s, v.x, c.x), fmaf(s, v.y, c.y));
  }
  // (contraction off: two products and their sum, each rounded, in every
  // form of the step; see mul_nc)
  static __device__ __forceinline__ float dot(T x, T y) {
    return add_nc(mul_nc(x.x, y.x), mul_nc(x.y, y.y));
  }
  static __device__ __forceinline__ void adagrad(T &p, T &ac, T g, float lr, float eps) {
    const float *gv = &g.x;
    float *pp = &p.x, *aa = &ac.x;
#pragma unroll
    for (int c = 0; c < 2; c++) {
      const float na = add_nc(aa[c], mul_nc(gv[c], gv[c]));
      aa[c] = na;
      const float den = add_nc(__builtin_amdgcn_sqrtf(na), eps);
      pp[c] = sub_nc(pp[c], mul_nc(mul_nc(lr, gv[c]), __builtin_amdgcn_rcpf(den)));
    }
  }
  static __device__ __forceinline__ void pin(T &v) { asm volatile("" : "+v"(v.x), "+v"(v.y)); }
  static __device__ __forceinline__ Fx ldfix(const long long *e, int lane) {
    return {reinterpret_cast<const longlong2 *>(e)[lane]};
  }
  static __device__ __forceinline__ T unfix(const Fx &g) {
    return make_float2(from_fix(g.a.x), from_fix(g.a.y));
  }
  static __device__ __forceinline__ void addfix(long long *e, int lane, T v, int &bad) {
    bad |= !(fabsf(v.x) < kFixLimit) | !(fabsf(v.y) < kFixLimit);
    unsigned long long *d = reinterpret_cast<unsigned long long *>(e) + 2 * lane;
    atomicAdd(d + 0, to_fix<2>(v.x));
    atomicAdd(d + 1, to_fix<2>(v.y));
  }
  static __device__ __forceinline__ void zerofix(long long *e, int lane) {
    reinterpret_cast<longlong2 *>(e)[lane] = make_longlong2(0, 0);
  }
  static __device__ __forceinline__ Fx fxadd(const Fx &x, const Fx &y) {
    return {make_longlong2(x.a.x + y.a.x, x.a.y + y.a.y)};
  }
  static __device__ __forceinline__ Fx fxzero() { return {make_longlong2(0, 0)}; }
};
// the deferred Adagrad step of the previous batch: (p, a) += sum
template <int VW>
__device__ __forceinline__ void fold(typename SV<VW>::T &p, typename SV<VW>::T &ac,
                                     const typename SV<VW>::Fx &g, float lr, float eps) {
  SV<VW>::adagrad(p, ac, SV<VW>::unfix(g), lr, eps);
}

// views of the deferred-row buffers (L lanes x VW floats per row: dp = VW L)
template <int L, int VW>
__device__ __forceinline__ typename SV<VW>::T *sh_row(const TrainArgs &a, int par, int m,
                                                      int which) {
  return reinterpret_cast<typename SV<VW>::T *>(a.shadow) +
         (((size_t)par * a.MX + m) * 2 + which) * L;
}
// the dp int64 of gacc entry m
template <int L, int VW>
__device__ __forceinline__ long long *gacc_row(const TrainArgs &a, int par, int m) {
  return a.gacc + ((size_t)par * a.MX + m) * (VW * L);
}
template <int L, int VW>
__device__ __forceinline__ typename SV<VW>::T *tab_row(const TrainArgs &a, bool edge, int acc,
                                                       int row) {
  float *t = acc ? (edge ? a.eacc : a.nacc) : (edge ? a.etab : a.ntab);
  return reinterpret_cast<typename SV<VW>::T *>(t) + (size_t)row * L;
}

// The step's row stores are write-through (`global_store … sc1`), so the
// ~57 KB a workgroup writes per batch leaves no dirty lines in its XCD's L2
// for the kernel-end release to write back. Interleaved A/B against plain
// stores (profiles/r03/trainer/ab_wt_*.log): d = 128 (float2 rows) 6.88 ->
// 6.68 us per batch, d = 256 (float4 rows) 8.70 -> 8.49.
// float2: an agent-scope relaxed atomic store, which is exactly that store.
__device__ __forceinline__ void st_row(float2 *p, float2 v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long *>(p),
                     __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
// float4: there is no 16-byte atomic store, so the instruction is written
// out. s_nop 1: the wait states a >8-byte store's data registers need
// before a VALU may overwrite them (the compiler's hazard check does not see
// into asm; without it d = 256 training diverged). The "memory" clobber keeps
// the compiler's memory operations in program order around it; its vmcnt
// waits only get stricter for an extra store in flight (loads still return
// in order). HGX_TRAIN_WT4=0 (A/B builds): a plain store.
// r04: the compiler-visible form -- a raw buffer store with the sc1 policy
// bit, its base the first lane's row address (two readfirstlanes) -- is
// correct but measured 8.62 -> 8.93 us per batch at d = 256 (interleaved
// A/B, C3 HOBE records, profiles/r04/trainer/ab_wt4_builtin.log), so the
// asm stays. Every d = 256 trainer test checks the stored rows against the
// oracle (test_gpu_train.py, the C4 window in test_gpu_c4.py): a toolchain
// that broke the hazard would fail them.
#ifndef HGX_TRAIN_WT4
#define HGX_TRAIN_WT4 1
#endif
__device__ __forceinline__ void st_row(float4 *p, float4 v) {
  if (HGX_TRAIN_WT4) {
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(x) : "memory");
  } else {
    *p = v;
  }
}

// one flush entry: the deferred row (table bit 30 | row) of entry m of the
// previous batch folded and written back
template <int L, int VW>
__device__ __forceinline__ void flush_row(const TrainArgs &a, int par, int key, int m,
                                          int lane) {
  const bool edge = key >> 30;
  const int row = key & 0x3fffffff;
  typename SV<VW>::T p = sh_row<L, VW>(a, par, m, 0)[lane], ac = sh_row<L, VW>(a, par, m, 1)[lane];
  fold<VW>(p, ac, SV<VW>::ldfix(gacc_row<L, VW>(a, par, m), lane), a.lr, a.eps);
  st_row(&tab_row<L, VW>(a, edge, 0, row)[lane], p);
  st_row(&tab_row<L, VW>(a, edge, 1, row)[lane], ac);
}

// the same for a record group's flush slot words (row, code)
template <int L, int VW>
__device__ __forceinline__ void flush_slot(const TrainArgs &a, int par, int frow,
                                           unsigned fcode, int lane) {
  flush_row<L, VW>(a, par, (fcode & kFEdge ? 1 << 30 : 0) | frow, (fcode >> kDefBits) & kDefMask,
                   lane);
}

// The padding row (row 0 of both tables) of the previous batch. Its
// gradient sum arrives in kR0Slots fixed-point accumulators r0acc[q % 3]:
// every workgroup of batch q adds its records' row-0 gradients (a
// fixed-order float sum over its records, then one 2^44 fixed-point
// integer atomic per element) to slot blockIdx % kR0Slots, so the sum is
// exact and independent of arrival order. Batch q + 1 reads the kR0Slots
// slots (the owner thread of each column: kR0Slots x VW int64), adds them
// as integers and applies the Adagrad step to the base (the previous
// batch's shadow, or the table for the first batch of an epoch); batch q
// zeroes set (q + 1) % 3 for the next batch. r02/r03a instead had every
// workgroup store a float partial and every workgroup of the next batch
// read all 64 of them: 64 KB per workgroup from the Infinity Cache, about
// 0.9 us per batch at its per-CU rate (tools/ablate_train.py); now 16 KB.
// Slots per row width (interleaved A/B, profiles/r03/trainer/ab_slots_*.txt):
// 128-float rows (each record adds its own sums, 256 adders per batch) 8
// slots: 6.68 us per batch vs 7.77 at 4 and 6.81 at 16; 256-float rows (one
// add per workgroup, 64 adders) 4 slots: 8.36 vs 8.50 at 8 and 9.12 at 16.
constexpr int kR0Slots = 8;  // the most any width uses (buffer sizing)
template <int DP>
struct R0S {
  static constexpr int n = DP >= 256 ? 4 : kR0Slots;
};
template <int L, int VW>
__device__ __forceinline__ long long *r0_row(const TrainArgs &a, int par, int slot,
                                             int tab) {
  return a.r0acc + (((size_t)par * R0S<VW * L>::n + slot) * 2 + tab) * (VW * L);
}
template <int L, int VW>
struct Row0Loads {
  static constexpr int NC = 2 * L;  // V columns (both tables)
  typename SV<VW>::Fx g[R0S<VW * L>::n];
  typename SV<VW>::T rp, ra;
};
// every load issued unconditionally, first thing in the kernel (a load
// under a branch is waited for at the join); threads >= NC load column
// col - NC's words too (unused), q == 0 loads set 2 (not read)
template <int L, int VW>
__device__ __forceinline__ void row0_issue(const TrainArgs &a, int q,
                                           Row0Loads<L, VW> &ld) {
  using RL = Row0Loads<L, VW>;
  const int col = threadIdx.x % RL::NC;
  const int tab = col / L, c = col % L, ppar = (q + 2) % 3;
  // the address is selected (q is uniform), not the loaded value
  ld.rp = (q ? sh_row<L, VW>(a, ppar, tab, 0) : tab_row<L, VW>(a, tab, 0, 0))[c];
  ld.ra = (q ? sh_row<L, VW>(a, ppar, tab, 1) : tab_row<L, VW>(a, tab, 1, 0))[c];
#pragma unroll
  for (int j = 0; j < R0S<VW * L>::n; j++)
    ld.g[j] = SV<VW>::ldfix(r0_row<L, VW>(a, ppar, j, tab), c);
}
// column owners (threads < NC): the slots' exact integer sum, the previous
// batch's row-0 step (zero gradient for the first batch of an epoch)
template <int L, int VW>
__device__ __forceinline__ void row0_finish(const TrainArgs &a, int q,
                                            const Row0Loads<L, VW> &ld,
                                            typename SV<VW>::T &p0, typename SV<VW>::T &a0) {
  using S = SV<VW>;
  typename S::Fx t = ld.g[0];
#pragma unroll
  for (int j = 1; j < R0S<VW * L>::n; j++) t = S::fxadd(t, ld.g[j]);
  if (g_tab & 2048) t = S::fxzero();  // (debug ablation)
  if (q) S::adagrad(p0, a0, S::unfix(t), a.lr, a.eps);
}

// One launch = one batch. q = the batch's index in the epoch (parities
// q % 3 and q & 1). One L-lane group per record (dp == 4L), RPB = TB / L
// records per workgroup, ceil(B / RPB) workgroups; records placed by
// train_place, those without neighbour lists first (whole waves skip the list
// gathers).
// Early row-0 sums (float2 rows, d = 128): every record group adds its own
// row-0 gradients (the same float adds in emit order) to the fixed-point
// slot right after its forward pass, before its row stores, and stores its
// own loss word: no end-of-batch workgroup barrier. Interleaved A/B on C3
// HOBE records: 6.69 -> 6.65 us per batch, epoch 36.85M -> 37.09M records/s
// (profiles/r03/trainer/prep2/ab_diet_128.txt). HGX_TRAIN_R0EARLY=0 (A/B
// builds): the workgroup's fixed-order float sum, one atomic per column.
#ifndef HGX_TRAIN_R0EARLY
#define HGX_TRAIN_R0EARLY 1
#endif

// MULTI = true: after the first fold pass a wave that still has pending slots
// (pm != 0, a scalar) takes a second pass and then the slot-by-slot
// remainder; MULTI = false ends after the first pass and is correct only for
// batches in which train_place found at most one pending entry per record,
// so the host reads train_place's flags before it queues a chunk's launches
// (one stream drain per chunk). A form built as MULTI = true alone (merged)
// needs nothing from the device inside an epoch. Registers are the same
// either way (gfx950: quad 80 / 80 VGPRs, paired 86 / 86 at float2 rows and
// 124 / 124 at float4 rows, no scratch), the time is not (interleaved,
// us per batch): the paired form at float4 rows (d = 256, C4
// slice, where most batches are MULTI) 8.361 -> 8.319 merged; the quad form
// (d = 128, C3) 5.607 -> 5.804 at 2 records per workgroup and 5.314 -> 5.545
// at 1, of which 0.09 is the kernel and the rest the launch queue kept full.
// HGX_TRAIN_ONEKERNEL: 1 (default) merges the paired form at float4 rows; 0 /
// 2 (A/B builds): no form / the paired and the quad form at every width. The
// one-wave forms keep the two instantiations.
#ifndef HGX_TRAIN_ONEKERNEL
#define HGX_TRAIN_ONEKERNEL 1
#endif

// The paired-wave form of the step (PAIR, 64 lanes per record, 512 threads):
// one record on two waves of the workgroup, wave 2g the node half of record
// g and wave 2g + 1 its edge half, still 4 records per workgroup and the same
// placed buffers. The two halves of a record are the same program on
// different tables: a hub row H (Nl / Er), the other head row O (Nr / El) and
// K list rows Tk, with z = H.O, zk = Tk.H, the gradients gH = dz O + sum dk
// Tk, gO = dz H, gk = dk H, emitted lists first, then H, then O (the
// unpaired emit order restricted to one table). They meet in three scalars
// exchanged through LDS across one workgroup barrier: P = mean act(za) from
// the node wave, Q = mean act(zb) and y2 from the edge wave (y2, not l2: the
// node wave has the target and forms l2 and l1 + l2 + l3 as the one-wave form
// does). Repeated rows (s_gl, indexed by the owner's slot number), deferred
// rows, pending slots and the padding-row sums are all per table, so no other
// state crosses the pair. Own slots are j = 0 (H), 1 (O), 2 + k (Tk).
template <int VW, int K, int MODE, bool MULTI>
__device__ __forceinline__ void train_step_pair(const TrainArgs &a, const StepWords &w,
                                                int cb, int gb, int nb, int q) {
  constexpr int L = 64, RPB = 4, NW = 2 * RPB, TB = NW * L, R = 4 + 2 * K, J = 2 + K;
  constexpr int NZ = 1 + K;  // head dots of one half
  using S = SV<VW>;
  using V = typename S::T;
  static_assert(R + kWX <= 32, "slot and batch words fit the first 32 lanes");
  static_assert(NZ % 2 == 0, "the head dots reduce in groups of four, then two");
  constexpr bool kR0E = HGX_TRAIN_R0EARLY && VW == 2;
  __shared__ V s_z[2][RPB][L];
  __shared__ V s_gl[RPB][R][L];  // gradients of local (one-record) rows
  __shared__ V s_r0[2][L];
  __shared__ float s_loss[RPB];
  __shared__ float s_x[RPB][4];  // P, Q, y2 of each record
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / L), lane = threadIdx.x % L;
  const int grp = wave >> 1, half = wave & 1;  // half 1: the edge wave
  const bool edge = half;
  const int NBF = gridDim.x, RW = w.RW;
  const int par = q % 3, ppar = (q + 2) % 3, zpar = (q + 1) % 3;
  // round trip 1: as the unpaired form, both waves of a pair loading their
  // record's words; the padding-row loads by the column owners only (waves
  // 0 and 1: the node and the edge table's row 0)
  const unsigned gi = blockIdx.x * RPB + grp;  // (32-bit: at most kPackB groups of RW words)
  const int *ri = w.pidx + gi * RW;
  const unsigned *rc = w.pcode + gi * RW;
  const float *yt = w.ptgt + gi * 3;
  const int sl = lane < RW ? lane : 0;
  const int rv = ri[sl];
  const int cv = (int)rc[sl];
  const int tv = __float_as_int(yt[lane < 3 ? lane : 0]);
  // (no default values, see flush slot 0 below)
  Row0Loads<L, VW> r0l;
  if (wave < 2) row0_issue<L, VW>(a, q, r0l);
  int row[J], frow[kFX];
  unsigned code[J], fcode[kFX];
  const int sH = edge ? 3 : 0, sO = edge ? 1 : 2, sT = 4 + half * K;
  auto slot_of = [&](int j) { return j == 0 ? sH : j == 1 ? sO : sT + j - 2; };
#pragma unroll
  for (int j = 0; j < J; j++) {
    row[j] = __builtin_amdgcn_readlane(rv, slot_of(j));
    code[j] = (unsigned)__builtin_amdgcn_readlane(cv, slot_of(j));
  }
#pragma unroll
  for (int f = 0; f < kFX; f++) {
    frow[f] = __builtin_amdgcn_readlane(rv, R + f);
    fcode[f] = (unsigned)__builtin_amdgcn_readlane(cv, R + f);
  }
  const int nfo = __builtin_amdgcn_readlane(rv, R + kFX);
  const int zc = __builtin_amdgcn_readlane(rv, R + kFX + 1);
  const float yt0 = __int_as_float(__builtin_amdgcn_readlane(tv, 0));
  const float yt1 = __int_as_float(__builtin_amdgcn_readlane(tv, 1));
  const float yt2 = __int_as_float(__builtin_amdgcn_readlane(tv, 2));
  HGX_STAMP(ts[1]);
  const int nval = min(max(nb - (int)blockIdx.x + NBF - 1, 0) / NBF, RPB);
  const bool has = grp < nval;
  int bad = 0;
  if (nval > 0) {
    // round trip 2: this wave's table only
    // (the table picked once: tab_row's four-way select on a runtime table
    // bit became a pointer table in scratch)
    V *Tw = reinterpret_cast<V *>(edge ? a.etab : a.ntab);
    V *Aw = reinterpret_cast<V *>(edge ? a.eacc : a.nacc);
    const V *T = Tw, *Ac = Aw;
    V Pv[J], Av[J];
    bool lists = false;
#pragma unroll
    for (int j = 2; j < J; j++) lists |= row[j] != 0;
    auto gather = [&](int j) {
      const int arow = (code[j] & kSOwn) ? row[j] : 0;
      Pv[j] = T[(size_t)row[j] * L + lane];
      Av[j] = Ac[(size_t)arow * L + lane];
    };
#pragma unroll
    for (int j = 0; j < 2; j++) {
      if (row[j] == 0) {  // a padding slot: its value comes from s_r0 below
        Pv[j] = Av[j] = S::zero();
        continue;
      }
      gather(j);
    }
    if (lists) {
#pragma unroll
      for (int j = 2; j < J; j++) gather(j);
    }
    // flush slot 0 rides on the same round trip, on the wave of its table
    const bool fmine = frow[0] != 0 && (bool)(fcode[0] & kFEdge) == edge;
    V fp, fa;
    typename S::Fx fg;
    if (fmine) {
      const int mf = (fcode[0] >> kDefBits) & kDefMask;
      fp = sh_row<L, VW>(a, ppar, mf, 0)[lane];
      fa = sh_row<L, VW>(a, ppar, mf, 1)[lane];
      fg = S::ldfix(gacc_row<L, VW>(a, ppar, mf), lane);
    }
    if (wave < 2) {
      V p0 = r0l.rp, a0 = r0l.ra;
      S::pin(p0);
      S::pin(a0);
      row0_finish<L, VW>(a, q, r0l, p0, a0);
      s_r0[wave][lane] = p0;
      if (blockIdx.x == 0) {
        st_row(&sh_row<L, VW>(a, par, wave, 0)[lane], p0);
        st_row(&sh_row<L, VW>(a, par, wave, 1)[lane], a0);
      }
    }
    __syncthreads();  // s_r0
    HGX_STAMP(ts[2]);
    if (has && fmine) {
      fold<VW>(fp, fa, fg, a.lr, a.eps);
      st_row(&Tw[(size_t)frow[0] * L + lane], fp);
      st_row(&Aw[(size_t)frow[0] * L + lane], fa);
    }
    // pending slots of this wave's table (entries are rows of one table)
    unsigned pm = 0;
#pragma unroll
    for (int j = 0; j < J; j++)
      if (code[j] & kSPend) pm |= 1u << j;
    if (!has) pm = 0;
    auto fold_pass = [&]() {
      if (pm == 0) return;
      const int ps = __builtin_ctz(pm);
      unsigned cd = 0;
#pragma unroll
      for (int j = 0; j < J; j++)
        if (j == ps) cd = code[j];
      const unsigned mp = (cd >> kDefBits) & kDefMask;
      const typename S::Fx gg = S::ldfix(gacc_row<L, VW>(a, ppar, mp), lane);
      V pp = sh_row<L, VW>(a, ppar, mp, 0)[lane], aa = sh_row<L, VW>(a, ppar, mp, 1)[lane];
      unsigned wm = 0;
#pragma unroll
      for (int j = 0; j < J; j++)
        if (((code[j] >> kDefBits) & kDefMask) == mp) wm |= 1u << j;
      wm &= pm;
      fold<VW>(pp, aa, gg, a.lr, a.eps);
#pragma unroll
      for (int j = 0; j < J; j++)
        if ((wm >> j) & 1u) {
          Pv[j] = pp;
          Av[j] = aa;
        }
      pm &= ~wm;
    };
    fold_pass();
    // (wave-uniform: pm sits in scalar registers; a light batch pays one
    // scalar compare for the merged kernel)
    if (MULTI && pm != 0) {
      fold_pass();
      if (pm != 0) {
#pragma unroll
        for (int j = 0; j < J; j++) {
          if (!((pm >> j) & 1u)) continue;
          const int mp = (code[j] >> kDefBits) & kDefMask;
          const typename S::Fx gg = S::ldfix(gacc_row<L, VW>(a, ppar, mp), lane);
          V pp = sh_row<L, VW>(a, ppar, mp, 0)[lane], aa = sh_row<L, VW>(a, ppar, mp, 1)[lane];
          fold<VW>(pp, aa, gg, a.lr, a.eps);
          Pv[j] = pp;
          Av[j] = aa;
        }
      }
    }
    // forward, this wave's 1 + K head dots reduced together
    const int act = MODE == 1 ? 0 : 1;
    const int lossk = MODE == 1 ? 0 : 1;
    float zh = 0.f, yh = 0.f, zk[K], sk[K];
    if (has) {
#pragma unroll
      for (int j = 0; j < J; j++)
        if (row[j] == 0) Pv[j] = s_r0[half][lane];
      float zz[NZ];
      zz[0] = S::dot(Pv[0], Pv[1]);
#pragma unroll
      for (int k = 0; k < K; k++) zz[1 + k] = S::dot(Pv[2 + k], Pv[0]);
      hgx::wave_allreduce_sum_n<NZ>(zz);
      zh = zz[0];
      yh = act_f(act, zh);
      float PQ = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) {
        zk[k] = zz[1 + k];
        sk[k] = act_f(act, zk[k]);
        PQ += sk[k];
      }
      PQ = div_k<K>(PQ);
      if (lane == 0) {
        s_x[grp][half] = PQ;
        if (edge) s_x[grp][2] = yh;
      }
    }
    __syncthreads();  // s_x (reached by every wave, with a record or not)
    V zT = S::zero();  // this table's padding-row gradient sum
    float lrec = 0.f;
    if (has) {
      const float inv_b = w.inv_b;
      const V &H = Pv[0], &O = Pv[1];
      const float P = s_x[grp][0], Q = s_x[grp][1];
      const float y3 = mul_nc(P, Q);
      float lh, l3, gh, g3;
      head_loss_nc(lossk, yh, edge ? yt1 : yt0, lh, gh);
      head_loss_nc(lossk, y3, yt2, l3, g3);
      if (!edge) {
        const float y1 = yh, y2 = s_x[grp][2];
        float l1, l2, g1, g2;
        head_loss_nc(lossk, y1, yt0, l1, g1);
        head_loss_nc(lossk, y2, yt1, l2, g2);
        lrec = add_nc(add_nc(l1, l2), l3);
      }
      HGX_STAMP(ts[3]);
      gh *= inv_b;
      g3 *= inv_b;
      const float dz = gh * act_d_nc(act, zh, yh);
      // dP = g3 Q / K on the node wave, dQ = g3 P / K on the edge wave
      const float dk = div_k<K>(g3 * (edge ? P : Q));
      auto emit = [&](int j, V g) {
        const unsigned cd = code[j];
        if (row[j] == 0) {
          if (!kR0E) zT = S::add(zT, g);
        } else if (cd & kSLocal) {
          V *acc = &s_gl[grp][cd & 15u][lane];
          if (cd & kSOwn) {
            V pv = Pv[j], av = Av[j];
            S::adagrad(pv, av, S::add(*acc, g), a.lr, a.eps);
            st_row(&Tw[(size_t)row[j] * L + lane], pv);
            st_row(&Aw[(size_t)row[j] * L + lane], av);
          } else {
            *acc = (cd & kSFirst) ? g : S::add(*acc, g);
          }
        } else if (cd & kSShared) {
          const int m = cd & kDefMask;
          S::addfix(gacc_row<L, VW>(a, par, m), lane, g, bad);
          if (cd & kSOwn) {
            st_row(&sh_row<L, VW>(a, par, m, 0)[lane], Pv[j]);
            st_row(&sh_row<L, VW>(a, par, m, 1)[lane], Av[j]);
          }
        } else {
          V pv = Pv[j], av = Av[j];
          S::adagrad(pv, av, g, a.lr, a.eps);
          st_row(&Tw[(size_t)row[j] * L + lane], pv);
          st_row(&Aw[(size_t)row[j] * L + lane], av);
        }
      };
      V gH = S::fma(dz, O, S::zero());
      if (kR0E) {
        float d[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
          d[k] = dk * act_d_nc(act, zk[k], sk[k]);
          gH = S::fma(d[k], Pv[2 + k], gH);
          if (row[2 + k] == 0) zT = S::add(zT, S::fma(d[k], H, S::zero()));
        }
        if (row[0] == 0) zT = S::add(zT, gH);
        if (row[1] == 0) zT = S::add(zT, S::fma(dz, H, S::zero()));
        const int slot = (blockIdx.x * RPB + grp) % R0S<VW * L>::n;
        S::addfix(r0_row<L, VW>(a, par, slot, half), lane, zT, bad);
        if (!edge && lane == 0)
          a.lossbuf[(size_t)gb * a.lstride + blockIdx.x * RPB + grp] = lrec;
#pragma unroll
        for (int k = 0; k < K; k++) emit(2 + k, S::fma(d[k], H, S::zero()));
      } else {
#pragma unroll
        for (int k = 0; k < K; k++) {
          const float d = dk * act_d_nc(act, zk[k], sk[k]);
          gH = S::fma(d, Pv[2 + k], gH);
          emit(2 + k, S::fma(d, H, S::zero()));
        }
      }
      emit(0, gH);
      emit(1, S::fma(dz, H, S::zero()));
      HGX_STAMP(ts[4]);
    }
    if (!kR0E) {
      s_z[half][grp][lane] = zT;
      if (!edge && lane == 0) s_loss[grp] = lrec;
      __syncthreads();
      // the workgroup's fixed-order sum over its records, as the unpaired form
      if (wave < 2) {
        V sz = S::zero();
        for (int g = 0; g < RPB; g++) sz = S::add(sz, s_z[wave][g][lane]);
        S::addfix(r0_row<L, VW>(a, par, blockIdx.x % R0S<VW * L>::n, wave), lane, sz, bad);
      }
      if (threadIdx.x == 0) {
        float sl = 0.f;
        for (int g = 0; g < RPB; g++) sl += s_loss[g];
        a.lossbuf[(size_t)gb * a.lstride + blockIdx.x] = sl;
      }
    }
    // flush slots 1.., dealt over the two waves of the record
#pragma unroll
    for (int f = 1; f < kFX; f++)
      if (frow[f] != 0 && (f & 1) == half) flush_slot<L, VW>(a, ppar, frow[f], fcode[f], lane);
  }
  HGX_STAMP(ts[5]);
  // flush overflow list and the zeroing loops, over all waves
  for (int e = blockIdx.x * NW + wave; e < nfo; e += NBF * NW) {
    const int2 en = a.pfo[(size_t)cb * a.Mmax + e];
    flush_row<L, VW>(a, ppar, en.x, en.y, lane);
  }
  {
    longlong2 *z = reinterpret_cast<longlong2 *>(gacc_row<L, VW>(a, zpar, 2));
    const int tot = zc * (VW / 2) * L;
    for (int i = blockIdx.x * TB + threadIdx.x; i < tot; i += NBF * TB)
      z[i] = make_longlong2(0, 0);
    longlong2 *zr = reinterpret_cast<longlong2 *>(r0_row<L, VW>(a, zpar, 0, 0));
    for (int i = blockIdx.x * TB + threadIdx.x; i < R0S<VW * L>::n * VW * L; i += NBF * TB)
      zr[i] = make_longlong2(0, 0);
  }
  if (__any(bad) && !g_tab && lane == 0) atomicOr(a.ovf, 1);
  HGX_STAMP(ts[6]);
  trace_put(gb, 0, 7, ts, threadIdx.x == (NW - 2) * L);
}

// The quad form of the step (64 lanes per record, 256 RPB threads): each table
// half of the paired form on two waves, waves 4g .. 4g + 3 of the workgroup
// the node head, node list, edge head and edge list wave of record g. Of the
// half's own slots j = 0 (H), 1 (O), 2 + k (Tk) the head wave has H, O and
// T0 .. T(KH-1), the list wave the other KL list rows, and H's table row to
// dot them with. Both fold pending slots of what they read (every reader of
// a deferred row computes the same bits), reduce their dots (the reduction
// tree is per value), and meet at ONE workgroup barrier: the 1 + K dots of
// both halves (s_zx) and the list wave's post-fold rows (s_t) go through LDS,
// then every wave of the record runs the paired form's scalar head math from
// the twelve dots itself. The head wave runs the whole hub chain and the
// whole row-0 sum of its table in emit order (lists, H, O; a list slot's term
// is d[k] H), adds it and (node head) stores the loss word; each wave emits
// its own slots with the paired form's emit classes.
// A row repeated within the record (kSLocal) sums in LDS in emit order, so a
// half with such a slot among the list wave's is not split: its head wave runs
// the paired form's whole 7-slot program (role kQFull) and its list wave only
// reaches the barriers (kQIdle); a wave-uniform test on the codes both waves
// hold. Flush slot 0 rides on the list wave of its table, flush slots 1..
// on waves 1..3 of the record. Same placed buffers, placed for RPB records
// per workgroup. RPB = 1 (the default at d = 128): 256 workgroups of 256
// threads, a batch of 256 on every CU, 4 waves at each barrier; RPB = 2: 128
// workgroups of 512 threads (interleaved on C3 HOBE records: 5.607 us per
// batch at 2, 5.314 at 1). Float2 rows (padded d = 128) only: the
// 4-record, 1024-thread geometry measured slower than the paired form at
// both row widths, and at float4 rows the padding row's gradient is a
// float sum over the workgroup's records, bit-identical to the other forms
// only over their four.
enum { kQFull = 0, kQHead = 1, kQList = 2, kQIdle = 3 };
template <int ROLE, int J, int JH>
struct QRole {
  static constexpr unsigned all = (1u << J) - 1, head = (1u << JH) - 1;
  // slots whose table row the wave reads / slots it emits
  static constexpr unsigned pm = ROLE == kQFull   ? all
                                 : ROLE == kQHead ? head
                                 : ROLE == kQList ? ((all & ~head) | 1u)
                                                  : 0u;
  static constexpr unsigned om = ROLE == kQList ? (all & ~head) : pm;
};
template <int V>
struct QC {
  static constexpr int value = V;
};
template <int VW, int K, int MODE, bool MULTI, int RPB>
__device__ __forceinline__ void train_step_quad(const TrainArgs &a, const StepWords &w,
                                                int cb, int gb, int nb, int q) {
  constexpr int L = 64, NW = 4 * RPB, TB = NW * L, R = 4 + 2 * K, J = 2 + K;
  constexpr int KH = 1, JH = 2 + KH, KL = K - KH;  // list rows of the head / list wave
  constexpr int NZ = 1 + K;                        // head dots of one half
  using S = SV<VW>;
  using V = typename S::T;
  static_assert(R + kWX <= 32, "slot and batch words fit the first 32 lanes");
  static_assert((1 + KH) % 2 == 0 && KL % 2 == 0 && NZ % 2 == 0,
                "the head dots reduce in groups of four, then two");
  static_assert(kFX <= 4, "flush slots 1.. on waves 1..3 of the record");
  // (every record adds its own row-0 sums: no per-workgroup float sum)
  static_assert(HGX_TRAIN_R0EARLY && VW == 2, "the quad form is built for early row-0 sums");
  __shared__ V s_gl[RPB][R][L];  // gradients of local (one-record) rows
  __shared__ V s_r0[2][L];
  __shared__ V s_t[RPB][2][KL][L];  // the list waves' rows, for the hub chains
  __shared__ __attribute__((aligned(16))) float s_zx[RPB][2][8];  // z, z0 .. z(K-1) per half
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / L), lane = threadIdx.x % L;
  const int grp = wave >> 2, half = (wave >> 1) & 1, sub = wave & 1;  // sub 1: the list wave
  const bool edge = half;
  const int NBF = gridDim.x, RW = w.RW;
  const int par = q % 3, ppar = (q + 2) % 3, zpar = (q + 1) % 3;
  // round trip 1: as the paired form, all four waves loading their record's
  // words; the padding-row loads by waves 0 and 1 (node / edge table's row 0)
  const unsigned gi = blockIdx.x * RPB + grp;  // (32-bit: at most kPackB groups of RW words)
  const int *ri = w.pidx + gi * RW;
  const unsigned *rc = w.pcode + gi * RW;
  const float *yt = w.ptgt + gi * 3;
  const int sl = lane < RW ? lane : 0;
  const int rv = ri[sl];
  const int cv = (int)rc[sl];
  const int tv = __float_as_int(yt[lane < 3 ? lane : 0]);
  Row0Loads<L, VW> r0l;
  if (wave < 2) row0_issue<L, VW>(a, q, r0l);
  int row[J], frow[kFX];
  unsigned code[J], fcode[kFX];
  const int sH = edge ? 3 : 0, sO = edge ? 1 : 2, sT = 4 + half * K;
  auto slot_of = [&](int j) { return j == 0 ? sH : j == 1 ? sO : sT + j - 2; };
#pragma unroll
  for (int j = 0; j < J; j++) {
    row[j] = __builtin_amdgcn_readlane(rv, slot_of(j));
    code[j] = (unsigned)__builtin_amdgcn_readlane(cv, slot_of(j));
  }
#pragma unroll
  for (int f = 0; f < kFX; f++) {
    frow[f] = __builtin_amdgcn_readlane(rv, R + f);
    fcode[f] = (unsigned)__builtin_amdgcn_readlane(cv, R + f);
  }
  const int nfo = __builtin_amdgcn_readlane(rv, R + kFX);
  const int zc = __builtin_amdgcn_readlane(rv, R + kFX + 1);
  const float yt0 = __int_as_float(__builtin_amdgcn_readlane(tv, 0));
  const float yt1 = __int_as_float(__builtin_amdgcn_readlane(tv, 1));
  const float yt2 = __int_as_float(__builtin_amdgcn_readlane(tv, 2));
  HGX_STAMP(ts[1]);
  const int nval = min(max(nb - (int)blockIdx.x + NBF - 1, 0) / NBF, RPB);
  const bool has = grp < nval;
  // the half is split unless a list-wave slot repeats a row of the record
  unsigned lc = 0;
#pragma unroll
  for (int j = JH; j < J; j++) lc |= code[j];
  const bool split = !(lc & kSLocal);
  const int role = !has ? kQIdle : sub == 0 ? (split ? kQHead : kQFull) : (split ? kQList : kQIdle);
  // (always_inline: a role body left out of line keeps the rows in scratch)
  auto by_role = [&](auto &&f) __attribute__((always_inline)) {
    if (role == kQHead) f(QC<kQHead>{});
    else if (role == kQList) f(QC<kQList>{});
    else if (role == kQFull) f(QC<kQFull>{});
  };
  int bad = 0;
  if (nval > 0) {
    // round trip 2: this wave's rows of its table
    V *Tw = reinterpret_cast<V *>(edge ? a.etab : a.ntab);
    V *Aw = reinterpret_cast<V *>(edge ? a.eacc : a.nacc);
    const V *T = Tw, *Ac = Aw;
    V Pv[J], Av[J];
    by_role([&](auto rl) __attribute__((always_inline)) {
      using QR = QRole<decltype(rl)::value, J, JH>;
      bool lists = false;
#pragma unroll
      for (int j = 2; j < J; j++)
        if ((QR::pm >> j) & 1u) lists |= row[j] != 0;
#pragma unroll
      for (int j = 0; j < J; j++) {
        if (!((QR::pm >> j) & 1u)) continue;
        // a padding head slot (its value comes from s_r0 below) / no list
        // gathers; accumulator rows only where the wave owns the update
        if (j < 2 ? row[j] != 0 : lists) {
          const int arow = (code[j] & kSOwn) ? row[j] : 0;
          Pv[j] = T[(size_t)row[j] * L + lane];
          if ((QR::om >> j) & 1u) Av[j] = Ac[(size_t)arow * L + lane];
        } else if (j < 2) {
          Pv[j] = S::zero();
          Av[j] = S::zero();
        }
      }
    });
    // flush slot 0 rides on the same round trip, on the list wave of its table
    const bool fmine = sub == 1 && frow[0] != 0 && (bool)(fcode[0] & kFEdge) == edge;
    V fp, fa;
    typename S::Fx fg;
    if (fmine) {
      const int mf = (fcode[0] >> kDefBits) & kDefMask;
      fp = sh_row<L, VW>(a, ppar, mf, 0)[lane];
      fa = sh_row<L, VW>(a, ppar, mf, 1)[lane];
      fg = S::ldfix(gacc_row<L, VW>(a, ppar, mf), lane);
    }
    if (wave < 2) {
      V p0 = r0l.rp, a0 = r0l.ra;
      S::pin(p0);
      S::pin(a0);
      row0_finish<L, VW>(a, q, r0l, p0, a0);
      s_r0[wave][lane] = p0;
      if (blockIdx.x == 0) {
        st_row(&sh_row<L, VW>(a, par, wave, 0)[lane], p0);
        st_row(&sh_row<L, VW>(a, par, wave, 1)[lane], a0);
      }
    }
    __syncthreads();  // s_r0
    HGX_STAMP(ts[2]);
    if (has && fmine) {
      fold<VW>(fp, fa, fg, a.lr, a.eps);
      st_row(&Tw[(size_t)frow[0] * L + lane], fp);
      st_row(&Aw[(size_t)frow[0] * L + lane], fa);
    }
    const int act = MODE == 1 ? 0 : 1;
    const int lossk = MODE == 1 ? 0 : 1;
    by_role([&](auto rl) __attribute__((always_inline)) {
      using QR = QRole<decltype(rl)::value, J, JH>;
      constexpr int ROLE = decltype(rl)::value;
      // pending slots among the rows this wave read
      unsigned pm = 0;
#pragma unroll
      for (int j = 0; j < J; j++)
        if (((QR::pm >> j) & 1u) && (code[j] & kSPend)) pm |= 1u << j;
      auto fold_pass = [&]() __attribute__((always_inline)) {
        if (pm == 0) return;
        const int ps = __builtin_ctz(pm);
        unsigned cd = 0;
#pragma unroll
        for (int j = 0; j < J; j++)
          if (j == ps) cd = code[j];
        const unsigned mp = (cd >> kDefBits) & kDefMask;
        const typename S::Fx gg = S::ldfix(gacc_row<L, VW>(a, ppar, mp), lane);
        V pp = sh_row<L, VW>(a, ppar, mp, 0)[lane], aa = sh_row<L, VW>(a, ppar, mp, 1)[lane];
        unsigned wm = 0;
#pragma unroll
        for (int j = 0; j < J; j++)
          if (((code[j] >> kDefBits) & kDefMask) == mp) wm |= 1u << j;
        wm &= pm;
        fold<VW>(pp, aa, gg, a.lr, a.eps);
#pragma unroll
        for (int j = 0; j < J; j++)
          if (((QR::pm >> j) & 1u) && ((wm >> j) & 1u)) {
            Pv[j] = pp;
            Av[j] = aa;
          }
        pm &= ~wm;
      };
      fold_pass();
      if (MULTI && pm != 0) {  // (wave-uniform, as in the paired form)
        fold_pass();
        if (pm != 0) {
#pragma unroll
          for (int j = 0; j < J; j++) {
            if (!((QR::pm >> j) & 1u) || !((pm >> j) & 1u)) continue;
            const int mp = (code[j] >> kDefBits) & kDefMask;
            const typename S::Fx gg = S::ldfix(gacc_row<L, VW>(a, ppar, mp), lane);
            V pp = sh_row<L, VW>(a, ppar, mp, 0)[lane], aa = sh_row<L, VW>(a, ppar, mp, 1)[lane];
            fold<VW>(pp, aa, gg, a.lr, a.eps);
            Pv[j] = pp;
            Av[j] = aa;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < J; j++)
        if (((QR::pm >> j) & 1u) && row[j] == 0) Pv[j] = s_r0[half][lane];
      // forward: this wave's dots reduced together, to s_zx[.][0] (z = H.O)
      // and s_zx[.][1 + k] (zk = Tk.H)
      constexpr int K0 = ROLE == kQList ? KH : 0, K1 = ROLE == kQHead ? KH : K;
      constexpr int Z0 = ROLE == kQList ? 0 : 1, NQ = Z0 + K1 - K0;
      float zz[NQ];
      if (Z0) zz[0] = S::dot(Pv[0], Pv[1]);
#pragma unroll
      for (int k = K0; k < K1; k++) zz[Z0 + k - K0] = S::dot(Pv[2 + k], Pv[0]);
      hgx::wave_allreduce_sum_n<NQ>(zz);
      if (lane == 0) {
        if (Z0) s_zx[grp][half][0] = zz[0];
#pragma unroll
        for (int k = K0; k < K1; k++) s_zx[grp][half][1 + k] = zz[Z0 + k - K0];
      }
      if (ROLE == kQList) {
#pragma unroll
        for (int k = KH; k < K; k++) s_t[grp][half][k - KH][lane] = Pv[2 + k];
      }
    });
    __syncthreads();  // s_zx, s_t (reached by every wave, with a record or not)
    by_role([&](auto rl) __attribute__((always_inline)) {
      using QR = QRole<decltype(rl)::value, J, JH>;
      constexpr int ROLE = decltype(rl)::value;
      // the paired form's head math, on every wave of the record
      const float inv_b = w.inv_b;
      const float *zo = s_zx[grp][half], *zp = s_zx[grp][half ^ 1];
      const float zh = zo[0], yh = act_f(act, zh);
      float zk[K], sk[K], PQo = 0.f, PQp = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) {
        zk[k] = zo[1 + k];
        sk[k] = act_f(act, zk[k]);
        PQo += sk[k];
      }
      PQo = div_k<K>(PQo);
#pragma unroll
      for (int k = 0; k < K; k++) PQp += act_f(act, zp[1 + k]);
      PQp = div_k<K>(PQp);
      const float P = edge ? PQp : PQo, Q = edge ? PQo : PQp;
      const float y3 = mul_nc(P, Q);
      float lh, l3, gh, g3, lrec = 0.f;
      head_loss_nc(lossk, yh, edge ? yt1 : yt0, lh, gh);
      head_loss_nc(lossk, y3, yt2, l3, g3);
      if (!edge && ROLE != kQList) {
        const float y1 = yh, y2 = act_f(act, zp[0]);
        float l1, l2, g1, g2;
        head_loss_nc(lossk, y1, yt0, l1, g1);
        head_loss_nc(lossk, y2, yt1, l2, g2);
        lrec = add_nc(add_nc(l1, l2), l3);
      }
      HGX_STAMP(ts[3]);
      gh *= inv_b;
      g3 *= inv_b;
      const float dz = gh * act_d_nc(act, zh, yh);
      // dP = g3 Q / K on the node waves, dQ = g3 P / K on the edge waves
      const float dk = div_k<K>(g3 * (edge ? P : Q));
      const V &H = Pv[0], &O = Pv[1];
      auto emit = [&](int j, V g) __attribute__((always_inline)) {
        const unsigned cd = code[j];
        if (row[j] == 0) {
          // (in the head wave's row-0 sum)
        } else if (cd & kSLocal) {
          V *acc = &s_gl[grp][cd & 15u][lane];
          if (cd & kSOwn) {
            V pv = Pv[j], av = Av[j];
            S::adagrad(pv, av, S::add(*acc, g), a.lr, a.eps);
            st_row(&Tw[(size_t)row[j] * L + lane], pv);
            st_row(&Aw[(size_t)row[j] * L + lane], av);
          } else {
            *acc = (cd & kSFirst) ? g : S::add(*acc, g);
          }
        } else if (cd & kSShared) {
          const int m = cd & kDefMask;
          S::addfix(gacc_row<L, VW>(a, par, m), lane, g, bad);
          if (cd & kSOwn) {
            st_row(&sh_row<L, VW>(a, par, m, 0)[lane], Pv[j]);
            st_row(&sh_row<L, VW>(a, par, m, 1)[lane], Av[j]);
          }
        } else {
          V pv = Pv[j], av = Av[j];
          S::adagrad(pv, av, g, a.lr, a.eps);
          st_row(&Tw[(size_t)row[j] * L + lane], pv);
          st_row(&Aw[(size_t)row[j] * L + lane], av);
        }
      };
      float d[K];
#pragma unroll
      for (int k = 0; k < K; k++) d[k] = dk * act_d_nc(act, zk[k], sk[k]);
      if (ROLE != kQList) {
        if (ROLE == kQHead) {
#pragma unroll
          for (int k = KH; k < K; k++) Pv[2 + k] = s_t[grp][half][k - KH][lane];
        }
        // the hub chain and the table's row-0 sum, in emit order
        V gH = S::fma(dz, O, S::zero()), zT = S::zero();
#pragma unroll
        for (int k = 0; k < K; k++) {
          gH = S::fma(d[k], Pv[2 + k], gH);
          if (row[2 + k] == 0) zT = S::add(zT, S::fma(d[k], H, S::zero()));
        }
        if (row[0] == 0) zT = S::add(zT, gH);
        if (row[1] == 0) zT = S::add(zT, S::fma(dz, H, S::zero()));
        const int slot = (blockIdx.x * RPB + grp) % R0S<VW * L>::n;
        S::addfix(r0_row<L, VW>(a, par, slot, half), lane, zT, bad);
        if (!edge && lane == 0)
          a.lossbuf[(size_t)gb * a.lstride + blockIdx.x * RPB + grp] = lrec;
#pragma unroll
        for (int k = 0; k < K; k++)
          if ((QR::om >> (2 + k)) & 1u) emit(2 + k, S::fma(d[k], H, S::zero()));
        emit(0, gH);
        emit(1, S::fma(dz, H, S::zero()));
      } else {
#pragma unroll
        for (int k = KH; k < K; k++) emit(2 + k, S::fma(d[k], H, S::zero()));
      }
      HGX_STAMP(ts[4]);
    });
    // flush slots 1.., on waves 1..3 of the record
#pragma unroll
    for (int f = 1; f < kFX; f++)
      if (frow[f] != 0 && f == (wave & 3)) flush_slot<L, VW>(a, ppar, frow[f], fcode[f], lane);
  }
  HGX_STAMP(ts[5]);
  // flush overflow list and the zeroing loops, over all waves
  for (int e = blockIdx.x * NW + wave; e < nfo; e += NBF * NW) {
    const int2 en = a.pfo[(size_t)cb * a.Mmax + e];
    flush_row<L, VW>(a, ppar, en.x, en.y, lane);
  }
  {
    longlong2 *z = reinterpret_cast<longlong2 *>(gacc_row<L, VW>(a, zpar, 2));
    const int tot = zc * (VW / 2) * L;
    for (int i = blockIdx.x * TB + threadIdx.x; i < tot; i += NBF * TB)
      z[i] = make_longlong2(0, 0);
    longlong2 *zr = reinterpret_cast<longlong2 *>(r0_row<L, VW>(a, zpar, 0, 0));
    for (int i = blockIdx.x * TB + threadIdx.x; i < R0S<VW * L>::n * VW * L; i += NBF * TB)
      zr[i] = make_longlong2(0, 0);
  }
  if (__any(bad) && !g_tab && lane == 0) atomicOr(a.ovf, 1);
  HGX_STAMP(ts[6]);
  trace_put(gb, 0, 7, ts, threadIdx.x == (NW - 4) * L);
}

template <int VW, int KMAX, int MODE, bool MULTI, int RPB>
__global__ __launch_bounds__(256 * RPB) void train_step_q(HGX_STEP_PARAMS) {
  HGX_STEP_WORDS(RPB);
  train_step_quad<VW, KMAX, MODE, MULTI, RPB>(a, w, cb, gb, nb, q);
}

// PAIR: the paired-wave form above (L = 64, TB = 512, 4 records per workgroup)
template <int L, int VW, int KMAX, int MODE, int TB, bool MULTI, bool PAIR = false>
__global__ __launch_bounds__(TB) void train_step(HGX_STEP_PARAMS) {
  HGX_STEP_WORDS(PAIR ? 4 : TB / L);
  if constexpr (PAIR) {
    static_assert(!PAIR || (L == 64 && TB == 512), "paired geometry");
    train_step_pair<VW, KMAX, MODE, MULTI>(a, w, cb, gb, nb, q);
    return;
  }
  constexpr int RPB = TB / L, R = 4 + 2 * KMAX, K = KMAX, NC = 2 * L;
  using S = SV<VW>;
  using V = typename S::T;
  static_assert(L == 32 || L == 64, "step geometry");
  static_assert(R + kWX <= 32, "slot and batch words fit the first 32 lanes");
  // early row-0 sums at float2 rows only (at float4 rows, d = 256, the 4x
  // integer atomics cost more than the barrier: 8.49 -> 10.42 us per batch)
  constexpr bool kR0E = HGX_TRAIN_R0EARLY && VW == 2;
  __shared__ V s_z[2][RPB][L];
  __shared__ V s_gl[RPB][R][L];  // gradients of local (one-record) rows
  __shared__ V s_r0[2][L];
  __shared__ float s_loss[RPB];
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int grp = threadIdx.x / L, lane = threadIdx.x % L;
  const int NBF = gridDim.x, RW = w.RW;
  const int par = q % 3, ppar = (q + 2) % 3, zpar = (q + 1) % 3;
  // round trip 1 (kernel arguments only): record ids and slot codes (one
  // load per lane, readlane broadcast), flush slots, the batch words,
  // targets, the row-0 base and the previous batch's row-0 partials
  const unsigned gi = blockIdx.x * RPB + grp;  // (32-bit: at most kPackB groups of RW words)
  const int *ri = w.pidx + gi * RW;
  const unsigned *rc = w.pcode + gi * RW;
  const float *yt = w.ptgt + gi * 3;
  int row[R], frow[kFX];
  unsigned code[R], fcode[kFX];
  int nfo, zc;  // batch words: overflow flushes, gacc entries to zero
  // every round-trip-1 load is issued before the first use of any of them
  // (the readlane broadcasts below wait for the id words)
  const int sl = lane < RW ? lane : 0;
  const int rv = ri[sl];
  const int cv = (int)rc[sl];
  const int tv = __float_as_int(yt[L == 64 ? (lane < 3 ? lane : 0) : 0]);
  float yt1 = 0.f, yt2 = 0.f;
  if (L == 32) {
    yt1 = yt[1];
    yt2 = yt[2];
  }
  // the previous batch's row-0 gradient slots (none for the first batch of
  // an epoch: row 0 from the table)
  Row0Loads<L, VW> r0l;
  row0_issue<L, VW>(a, q, r0l);
  {
#pragma unroll
    for (int s = 0; s < R + kFX; s++) {
      int r, c;
      if (L == 64) {
        r = __builtin_amdgcn_readlane(rv, s);
        c = __builtin_amdgcn_readlane(cv, s);
      } else {
        const bool hi = threadIdx.x & 32;
        const int r0 = __builtin_amdgcn_readlane(rv, s), r1 = __builtin_amdgcn_readlane(rv, 32 + s);
        const int c0 = __builtin_amdgcn_readlane(cv, s), c1 = __builtin_amdgcn_readlane(cv, 32 + s);
        r = hi ? r1 : r0;
        c = hi ? c1 : c0;
      }
      if (s < R) {
        row[s] = r;
        code[s] = (unsigned)c;
      } else {
        frow[s - R] = r;
        fcode[s - R] = (unsigned)c;
      }
    }
    // the same in every group of the batch: lane R + kFX + i of the low half
    nfo = __builtin_amdgcn_readlane(rv, R + kFX);
    zc = __builtin_amdgcn_readlane(rv, R + kFX + 1);
  }
  float yt0 = __int_as_float(tv);
  if (L == 64) {
    // lane c < 3 loaded target c: readlanes broadcast them (scalar)
    yt0 = __int_as_float(__builtin_amdgcn_readlane(tv, 0));
    yt1 = __int_as_float(__builtin_amdgcn_readlane(tv, 1));
    yt2 = __int_as_float(__builtin_amdgcn_readlane(tv, 2));
  }
  HGX_STAMP(ts[1]);
  // records were dealt round robin over the workgroups (train_place)
  const int nval = min(max(nb - (int)blockIdx.x + NBF - 1, 0) / NBF, RPB);
  const bool has = grp < nval;
  const int col = threadIdx.x % NC, sub = threadIdx.x / NC, tab0 = col / L, c0 = col % L;
  int bad = 0;
  if (nval > 0) {
    V p0 = r0l.rp, a0 = r0l.ra;
    S::pin(p0);
    S::pin(a0);
    // round trip 2: every slot's table row and the accumulator row where
    // this slot owns the row's update (else the hot row 0; a pending slot's
    // rows are replaced by the previous batch's shadow below). List slots
    // are skipped by a WAVE-uniform branch when no record of the wave has a
    // list.
    V Pv[R], Av[R];
    bool lists = false;
#pragma unroll
    for (int s = 4; s < R; s++) lists |= row[s] != 0;
    const bool wave_lists = __any(lists);
    // (table rows only: a per-lane select between the table and the shadow
    // as the load base made the gathers 64-bit per-lane addresses and cost
    // 0.6 us per batch)
    auto gather = [&](int s) {
      const bool edge = slot_is_edge(s, K);
      const V *T = reinterpret_cast<const V *>(edge ? a.etab : a.ntab);
      const V *Ac = reinterpret_cast<const V *>(edge ? a.eacc : a.nacc);
      const int arow = (code[s] & kSOwn) ? row[s] : 0;
      Pv[s] = T[(size_t)row[s] * L + lane];
      Av[s] = Ac[(size_t)arow * L + lane];
    };
#pragma unroll
    for (int s = 0; s < 4; s++) {
      // at L = 64 (one record per wave, scalar ids) the two padding slots of
      // the first four are skipped: their value comes from s_r0 below
      if (L == 64 && row[s] == 0) {
        Pv[s] = Av[s] = S::zero();
        continue;
      }
      gather(s);
    }
    if (wave_lists && !(g_tab & 32768)) {  // (debug ablation: no list gathers)
#pragma unroll
      for (int s = 4; s < R; s++) gather(s);
    } else if (wave_lists) {
#pragma unroll
      for (int s = 4; s < R; s++) Pv[s] = Av[s] = S::zero();
    }
    // flush slot 0 (one deferred row per group in the common case) rides on
    // the same round trip
    // (no default values: a conditional assignment over a default makes the
    // compiler copy the loaded registers at the join, i.e. wait for them and
    // drain every gather before the barrier)
    V fp, fa;
    typename S::Fx fg;
    if (__any(frow[0] != 0)) {
      const int mf = (fcode[0] >> kDefBits) & kDefMask;
      fp = sh_row<L, VW>(a, ppar, mf, 0)[lane];
      fa = sh_row<L, VW>(a, ppar, mf, 1)[lane];
      fg = S::ldfix(gacc_row<L, VW>(a, ppar, mf), lane);
    }
    if (sub == 0) {
      row0_finish<L, VW>(a, q, r0l, p0, a0);
      s_r0[tab0][c0] = p0;
      if (blockIdx.x == 0) {
        st_row(&sh_row<L, VW>(a, par, tab0, 0)[c0], p0);
        st_row(&sh_row<L, VW>(a, par, tab0, 1)[c0], a0);
      }
    }
    __syncthreads();  // s_r0
    HGX_STAMP(ts[2]);
    // flush slot 0: folded and written back now (its registers are free
    // for the forward pass; nothing of this batch reads the row)
    if (has && frow[0] != 0) {
      fold<VW>(fp, fa, fg, a.lr, a.eps);
      const bool fe = fcode[0] & kFEdge;
      st_row(&tab_row<L, VW>(a, fe, 0, frow[0])[lane], fp);
      st_row(&tab_row<L, VW>(a, fe, 1, frow[0])[lane], fa);
    }
    // pending slots (rows deferred by the previous batch): base row from the
    // previous batch's shadow, folded with its gacc sum, written to every
    // slot of the record that names the same entry. A select pass handles
    // one entry per record (picked by v_cndmask: no dynamic register index,
    // no loop-carried copies of the rows). MULTI = 0: train_place found at
    // most one entry per record in this batch, one pass (normally not
    // taken); MULTI = 1: two passes, then slot by slot.
    unsigned pm = 0;
#pragma unroll
    for (int s = 0; s < R; s++)
      if (code[s] & kSPend) pm |= 1u << s;
    if (!has) pm = 0;
    auto fold_pass = [&]() {
      if (!__any(pm != 0)) return;
      const int ps = pm ? __builtin_ctz(pm) : 0;
      unsigned cd = 0;
#pragma unroll
      for (int s = 0; s < R; s++)
        if (s == ps) cd = code[s];
      const unsigned mp = (cd >> kDefBits) & kDefMask;
      const typename S::Fx gg = S::ldfix(gacc_row<L, VW>(a, ppar, mp), lane);
      V pp = sh_row<L, VW>(a, ppar, mp, 0)[lane], aa = sh_row<L, VW>(a, ppar, mp, 1)[lane];
      // the record's slots naming the same entry (a mask: the write-back
      // below is one bit test per slot)
      unsigned wm = 0;
#pragma unroll
      for (int s = 0; s < R; s++)
        if (((code[s] >> kDefBits) & kDefMask) == mp) wm |= 1u << s;
      wm &= pm;
      fold<VW>(pp, aa, gg, a.lr, a.eps);
#pragma unroll
      for (int s = 0; s < R; s++)
        if ((wm >> s) & 1u) {
          Pv[s] = pp;
          Av[s] = aa;
        }
      pm &= ~wm;
    };
    fold_pass();
    if (MULTI) {
      fold_pass();
      if (__any(pm != 0)) {
#pragma unroll
        for (int s = 0; s < R; s++) {
          if (!__any((pm >> s) & 1u)) continue;
          const int mp = (code[s] >> kDefBits) & kDefMask;
          const typename S::Fx gg = S::ldfix(gacc_row<L, VW>(a, ppar, mp), lane);
          V pp = sh_row<L, VW>(a, ppar, mp, 0)[lane], aa = sh_row<L, VW>(a, ppar, mp, 1)[lane];
          fold<VW>(pp, aa, gg, a.lr, a.eps);
          if ((pm >> s) & 1u) {
            Pv[s] = pp;
            Av[s] = aa;
          }
        }
      }
    }
    V zN = S::zero(), zE = S::zero();
    float lrec = 0.f;
    if (has) {
#pragma unroll
      for (int s = 0; s < R; s++)
        if (row[s] == 0) Pv[s] = s_r0[slot_is_edge(s, K) ? 1 : 0][lane];
      const float inv_b = w.inv_b;
      const V &Nl = Pv[0], &El = Pv[1], &Nr = Pv[2], &Er = Pv[3];
      float z1, z2, za[K], zb[K];
      if (g_tab & 4096) {  // (debug ablation: no reductions)
        z1 = S::dot(Nl, Nr);
        z2 = S::dot(El, Er);
#pragma unroll
        for (int k = 0; k < K; k++) {
          za[k] = S::dot(Pv[4 + k], Nl);
          zb[k] = S::dot(Pv[4 + K + k], Er);
        }
      } else if constexpr (L == 64 && (2 + 2 * K) % 4 == 0) {
        // the 2 + 2K head dots reduced together (same sums, no serial chain)
        float zz[2 + 2 * K];
        zz[0] = S::dot(Nl, Nr);
        zz[1] = S::dot(El, Er);
#pragma unroll
        for (int k = 0; k < K; k++) {
          zz[2 + k] = S::dot(Pv[4 + k], Nl);
          zz[2 + K + k] = S::dot(Pv[4 + K + k], Er);
        }
        hgx::wave_allreduce_sum_n<2 + 2 * K>(zz);
        z1 = zz[0];
        z2 = zz[1];
#pragma unroll
        for (int k = 0; k < K; k++) {
          za[k] = zz[2 + k];
          zb[k] = zz[2 + K + k];
        }
      } else {
        z1 = group_sum<L>(S::dot(Nl, Nr));
        z2 = group_sum<L>(S::dot(El, Er));
#pragma unroll
        for (int k = 0; k < K; k++) {
          za[k] = group_sum<L>(S::dot(Pv[4 + k], Nl));
          zb[k] = group_sum<L>(S::dot(Pv[4 + K + k], Er));
        }
      }
      const int act = MODE == 1 ? 0 : 1;
      const int lossk = MODE == 1 ? 0 : 1;
      const float y1 = act_f(act, z1), y2 = act_f(act, z2);
      float sa[K], sb[K], P = 0.f, Q = 0.f;
#pragma unroll
      for (int k = 0; k < K; k++) {
        sa[k] = act_f(act, za[k]);
        sb[k] = act_f(act, zb[k]);
        P += sa[k];
        Q += sb[k];
      }
      P = div_k<K>(P);
      Q = div_k<K>(Q);
      const float y3 = mul_nc(P, Q);
      float l1, l2, l3, g1, g2, g3;
      head_loss_nc(lossk, y1, yt0, l1, g1);
      head_loss_nc(lossk, y2, yt1, l2, g2);
      head_loss_nc(lossk, y3, yt2, l3, g3);
      lrec = add_nc(add_nc(l1, l2), l3);
      HGX_STAMP(ts[3]);
      g1 *= inv_b;
      g2 *= inv_b;
      g3 *= inv_b;
      const float dz1 = g1 * act_d_nc(act, z1, y1);
      const float dz2 = g2 * act_d_nc(act, z2, y2);
      const float dP = div_k<K>(g3 * Q), dQ = div_k<K>(g3 * P);
      auto emit = [&](int s, V g) {
        const unsigned cd = code[s];
        const bool edge = slot_is_edge(s, K);
        if (row[s] == 0) {
          if (!kR0E) {
            if (edge) zE = S::add(zE, g);
            else zN = S::add(zN, g);
          }
        } else if (cd & kSLocal) {
          // one record's slots of a row, summed in emit order in LDS (the
          // wave's own accesses, in order); the last one (owner) updates
          V *acc = &s_gl[grp][cd & 15u][lane];
          if (cd & kSOwn) {
            V pv = Pv[s], av = Av[s];
            S::adagrad(pv, av, S::add(*acc, g), a.lr, a.eps);
            st_row(&tab_row<L, VW>(a, edge, 0, row[s])[lane], pv);
            st_row(&tab_row<L, VW>(a, edge, 1, row[s])[lane], av);
          } else {
            *acc = (cd & kSFirst) ? g : S::add(*acc, g);
          }
        } else if (cd & kSShared) {
          const int m = cd & kDefMask;
          if (g_tab & 1024)  // (debug ablation: plain stores, wrong sums)
            reinterpret_cast<V *>(gacc_row<L, VW>(a, par, m))[lane] = g;
          else
            S::addfix(gacc_row<L, VW>(a, par, m), lane, g, bad);
          if (cd & kSOwn) {
            st_row(&sh_row<L, VW>(a, par, m, 0)[lane], Pv[s]);
            st_row(&sh_row<L, VW>(a, par, m, 1)[lane], Av[s]);
          }
        } else {
          V pv = Pv[s], av = Av[s];
          if (g_tab & 8192) {  // (debug ablation: no Adagrad arithmetic)
            pv = S::add(pv, g);
            av = S::add(av, g);
          } else {
            S::adagrad(pv, av, g, a.lr, a.eps);
          }
          st_row(&tab_row<L, VW>(a, edge, 0, row[s])[lane], pv);
          st_row(&tab_row<L, VW>(a, edge, 1, row[s])[lane], av);
        }
      };
      V gln = S::fma(dz1, Nr, S::zero()), gre = S::fma(dz2, El, S::zero());
      if (kR0E) {
        // the row-0 sums in emit order first (the same adds as below), added
        // to this record's slot before any row store
        float da[K], db[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
          da[k] = dP * act_d_nc(act, za[k], sa[k]);
          db[k] = dQ * act_d_nc(act, zb[k], sb[k]);
          gln = S::fma(da[k], Pv[4 + k], gln);
          gre = S::fma(db[k], Pv[4 + K + k], gre);
          if (row[4 + k] == 0) zN = S::add(zN, S::fma(da[k], Nl, S::zero()));
          if (row[4 + K + k] == 0) zE = S::add(zE, S::fma(db[k], Er, S::zero()));
        }
        if (row[0] == 0) zN = S::add(zN, gln);
        if (row[3] == 0) zE = S::add(zE, gre);
        if (row[2] == 0) zN = S::add(zN, S::fma(dz1, Nl, S::zero()));
        if (row[1] == 0) zE = S::add(zE, S::fma(dz2, Er, S::zero()));
        const int slot = (blockIdx.x * RPB + grp) % R0S<VW * L>::n;
        S::addfix(r0_row<L, VW>(a, par, slot, 0), lane, zN, bad);
        S::addfix(r0_row<L, VW>(a, par, slot, 1), lane, zE, bad);
        if (lane == 0) a.lossbuf[(size_t)gb * a.lstride + blockIdx.x * RPB + grp] = lrec;
#pragma unroll
        for (int k = 0; k < K; k++) {
          emit(4 + k, S::fma(da[k], Nl, S::zero()));
          emit(4 + K + k, S::fma(db[k], Er, S::zero()));
        }
      } else {
#pragma unroll
        for (int k = 0; k < K; k++) {
          const float da = dP * act_d_nc(act, za[k], sa[k]);
          const float db = dQ * act_d_nc(act, zb[k], sb[k]);
          gln = S::fma(da, Pv[4 + k], gln);
          gre = S::fma(db, Pv[4 + K + k], gre);
          emit(4 + k, S::fma(da, Nl, S::zero()));
          emit(4 + K + k, S::fma(db, Er, S::zero()));
        }
      }
      emit(0, gln);
      emit(3, gre);
      emit(2, S::fma(dz1, Nl, S::zero()));
      emit(1, S::fma(dz2, Er, S::zero()));
      HGX_STAMP(ts[4]);
    }
    if (!kR0E) {
      s_z[0][grp][lane] = zN;
      s_z[1][grp][lane] = zE;
      if (lane == 0) s_loss[grp] = lrec;
      if (!(g_tab & 16384)) __syncthreads();  // (debug ablation: no barrier)
      // this batch's row-0 gradients: the workgroup's fixed-order sum, added
      // to its slot of r0acc[q % 3] in fixed point
      if (threadIdx.x < NC && !(g_tab & 16384)) {
        V sz = S::zero();
        for (int g = 0; g < RPB; g++) sz = S::add(sz, s_z[tab0][g][c0]);
        S::addfix(r0_row<L, VW>(a, par, blockIdx.x % R0S<VW * L>::n, tab0), c0, sz, bad);
      }
      if (threadIdx.x == 0) {
        float sl = 0.f;
        for (int g = 0; g < RPB; g++) sl += s_loss[g];
        a.lossbuf[(size_t)gb * a.lstride + blockIdx.x] = sl;
      }
    }
    // flush slots 1.. (more deferred rows than records in the batch)
    bool more = false;
#pragma unroll
    for (int f = 1; f < kFX; f++) more |= frow[f] != 0;
    if (__any(more)) {
#pragma unroll
      for (int f = 1; f < kFX; f++)
        if (frow[f] != 0) flush_slot<L, VW>(a, ppar, frow[f], fcode[f], lane);
    }
  }
  HGX_STAMP(ts[5]);
  // flush overflow list (rare: more deferred rows than kFX per record)
  for (int e = blockIdx.x * RPB + grp; e < nfo; e += NBF * RPB) {
    const int2 en = a.pfo[(size_t)cb * a.Mmax + e];
    flush_row<L, VW>(a, ppar, en.x, en.y, lane);
  }
  // zero the gacc parity the next batch adds into (its deferred entries
  // [2, 2 + zc) were used two batches ago) and the row-0 slots it adds into
  {
    longlong2 *z = reinterpret_cast<longlong2 *>(gacc_row<L, VW>(a, zpar, 2));
    const int tot = zc * (VW / 2) * L;
    for (int i = blockIdx.x * TB + threadIdx.x; i < tot; i += NBF * TB)
      z[i] = make_longlong2(0, 0);
    longlong2 *zr = reinterpret_cast<longlong2 *>(r0_row<L, VW>(a, zpar, 0, 0));
    for (int i = blockIdx.x * TB + threadIdx.x; i < R0S<VW * L>::n * VW * L; i += NBF * TB)
      zr[i] = make_longlong2(0, 0);
  }
  // (timing ablations compute wrong values: no overflow verdict for them)
  if (__any(bad) && !g_tab && (threadIdx.x & 63) == 0) atomicOr(a.ovf, 1);
  HGX_STAMP(ts[6]);
  trace_put(gb, 0, 7, ts, threadIdx.x == (RPB - 1) * L);
}

// End of an epoch: the last batch's deferred rows folded into the tables
// (row 0 of both tables from its np partials, its shared rows from gacc;
// keys from train_prep), and every gacc entry still in use zeroed (the last
// batch's and the one before it, Ml and Mp entries). One L-lane group per
// entry.
template <int L>
__global__ __launch_bounds__(256) void train_flush(TrainArgs a, const int *keys,
                                                   const int *Ml, const int *Mp,
                                                   int q, int np) {
  constexpr int GPB = 256 / L;
  const int grp = threadIdx.x / L, lane = threadIdx.x % L;
  const int par = q % 3, opar = (q + 2) % 3;
  const int M = 2 + *Ml, zc = Mp ? *Mp : 0;
  for (int e = blockIdx.x * GPB + grp; e < M; e += gridDim.x * GPB) {
    if (e < 2) {  // row 0: the last batch's slots, summed as train_step sums
      SV<4>::Fx t = SV<4>::ldfix(r0_row<L, 4>(a, par, 0, e), lane);
      for (int j = 1; j < R0S<4 * L>::n; j++)
        t = SV<4>::fxadd(t, SV<4>::ldfix(r0_row<L, 4>(a, par, j, e), lane));
      const float4 g = SV<4>::unfix(t);
      float4 p = sh_row<L, 4>(a, par, e, 0)[lane], ac = sh_row<L, 4>(a, par, e, 1)[lane];
      adagrad4_hw(p, ac, g, a.lr, a.eps);
      tab_row<L, 4>(a, e, 0, 0)[lane] = p;
      tab_row<L, 4>(a, e, 1, 0)[lane] = ac;
      continue;
    }
    flush_row<L, 4>(a, par, keys[e - 2], e, lane);
    SV<4>::zerofix(gacc_row<L, 4>(a, par, e), lane);
  }

  longlong2 *z = reinterpret_cast<longlong2 *>(gacc_row<L, 4>(a, opar, 2));
  for (int i = blockIdx.x * 256 + threadIdx.x; i < zc * 2 * L; i += gridDim.x * 256)
    z[i] = make_longlong2(0, 0);
}

}  // namespace
