// Trainer kernels, chunk preparation: defer_codes, prep_runs_regs, train_place,
// train_prep, and the small utility kernels of the driver and the model API.
#pragma once
#include <rocprim/block/block_radix_sort.hpp>

#include "hgx_train_step.h"

namespace {

// Block-wide exclusive scan of one int per thread.
__device__ int block_exclusive_scan(int v, int *total, int *s_ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  if (lane == 63) s_ws[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < kTB / 64; w++) {
    if (w < wave) base += s_ws[w];
    tot += s_ws[w];
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// Slot codes of one batch (tail of train_prep, the batch's (row, slot) keys
// sorted in LDS). Per run of equal rows:
//  - one slot: kSOwn (in-place update by its group);
//  - several slots of ONE record: kSLocal; its group sums the slots'
//    gradients in LDS in emit order, the last slot in that order owns the
//    update (no deferral, no atomics);
//  - slots in several records: deferred entry m = 2 + its rank among the
//    batch's deferred rows (sorted key order), kSShared, the first slot owns
//    the shadow write.
// Writes per-slot codes (batch slot order), the deferred rows' keys
// (ascending) and their count. u0 = the unique-run index of this thread's
// first sorted position.
// position of slot s in train_step's emit order: 4 + k, 4 + K + k for
// k = 0..K-1, then 0, 3, 2, 1
__device__ __forceinline__ int emit_pos(int s, int K) {
  if (s >= 4 + K) return 2 * (s - 4 - K) + 1;
  if (s >= 4) return 2 * (s - 4);
  return 2 * K + (s == 0 ? 0 : s == 3 ? 1 : s == 2 ? 2 : 3);
}

__device__ void defer_codes(const TrainArgs &a, int cb, int V, int P, int u0,
                            const unsigned long long *s_key, int *s_ws, int *s_runm,
                            int *skey, int *sM) {
  const int per = P / kTB, t0 = threadIdx.x * per, t1 = min(t0 + per, V);
  const int R = a.R;
  constexpr int kDefer = 1 << 30;  // run class: deferred (m assigned below)
  auto k32 = [&](int t) { return (unsigned)(s_key[t] >> 32); };
  auto slot = [&](int t) { return (int)(unsigned)(s_key[t] & 0xffffffffu); };
  auto starts = [&](int t) { return t == 0 || k32(t - 1) != k32(t); };
  // classify the runs starting in this thread's chunk: 0 single, a slot mask
  // (local), or kDefer
  int ns = 0;
  int u = u0;
  for (int t = t0; t < t1; t++) {
    if (!starts(t)) continue;
    int e = t + 1;
    while (e < V && k32(e) == k32(t)) e++;
    int cls = 0;
    if (e - t > 1) {
      if (slot(t) / R == slot(e - 1) / R) {
        cls = 1;  // local
      } else {
        cls = kDefer;
        ns++;
      }
    }
    s_runm[u++] = cls;
  }
  int S = 0;
  int m = block_exclusive_scan(ns, &S, s_ws);
  int *keys = skey + (size_t)cb * a.Mmax;
  u = u0;
  for (int t = t0; t < t1; t++) {
    if (!starts(t)) continue;
    if (s_runm[u] == kDefer) {
      s_runm[u] = kDefer | (2 + m);
      keys[m++] = (int)k32(t);
    }
    u++;
  }
  __syncthreads();
  unsigned *sc = a.scode + (size_t)cb * a.SB;
  u = u0;
  for (int t = t0; t < t1; t++) {
    const bool st = starts(t);
    u += st;
    const int cls = s_runm[u - 1];
    unsigned code = kSOwn;
    if (cls & kDefer) {
      code = kSShared | (st ? kSOwn : 0u) | (unsigned)(cls & (kDefer - 1));
    } else if (cls) {
      // local: the run's slots in train_step's emit order; the last owns the
      // update, the first writes the LDS sum, bits 0..3 = the owner's slot
      int rs = t;  // the run start
      while (rs > 0 && k32(rs - 1) == k32(t)) rs--;
      int re = t + 1;
      while (re < V && k32(re) == k32(t)) re++;
      const int me = emit_pos(slot(t) % R, a.K);
      int first = 1, last = 1, own = slot(t) % R;
      for (int j = rs; j < re; j++) {
        const int e2 = emit_pos(slot(j) % R, a.K);
        first &= e2 >= me;
        last &= e2 <= me;
        if (e2 > emit_pos(own, a.K)) own = slot(j) % R;
      }
      code = kSLocal | (last ? kSOwn : 0u) | (first ? kSFirst : 0u) | (unsigned)own;
    }
    sc[slot(t)] = code;
  }
  if (threadIdx.x == 0) sM[cb] = S;
}

// The unique-key and slot-code phases of train_prep for the radix-sorted
// batch (P == kSortP), from the sort's registers: thread t holds sorted
// positions [t * PER, t * PER + PER) (keys kk, slots vv), the same chunk the
// generic path scans in LDS. Run starts, run ends (the last slot of the run
// by a backward pass over the chunk; a run leaving the chunk is followed in
// LDS) and the run classes stay in registers, every array indexed at compile
// time; local runs (rare) use the generic LDS scan. Same outputs as the
// generic unique phase + defer_codes, bit for bit.
template <int PER>
__device__ void prep_runs_regs(const TrainArgs &a, int cb, int P, const unsigned (&kk)[PER],
                               const int (&vv)[PER], const unsigned long long *s_key, int *s_ws,
                               unsigned short *s_runm, int *skey, int *sM) {
  const int R = a.R, t0 = threadIdx.x * PER;
  constexpr int kDefer = 1 << 30;
  const bool split = !a.fused;
  const unsigned kprev = t0 > 0 ? (unsigned)(s_key[t0 - 1] >> 32) : 0xffffffffu;
  const unsigned knext = t0 + PER < P ? (unsigned)(s_key[t0 + PER] >> 32) : 0xffffffffu;
  bool vld[PER], st[PER], eq[PER];
  int cnt = 0, valid = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    vld[i] = kk[i] != 0xffffffffu;
    st[i] = vld[i] && kk[i] != (i ? kk[i - 1] : kprev);
    eq[i] = vld[i] && kk[i] == (i + 1 < PER ? kk[i + 1] : knext);
    cnt += st[i];
    valid += vld[i];
  }
  int U = 0, V = 0;
  const int u0 = block_exclusive_scan(cnt, &U, s_ws);
  block_exclusive_scan(valid, &V, s_ws);
  {
    int *ukey = a.ukey + (size_t)cb * a.SB;
    int *uoff = a.uoff + (size_t)cb * (a.SB + 1);
    int *inv = a.inv + (size_t)cb * a.SB;
    int u = u0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
      if (!vld[i]) continue;
      if (split) inv[vv[i]] = t0 + i;
      if (st[i]) {
        ukey[u] = (int)kk[i];
        if (split) uoff[u] = t0 + i;
        u++;
      }
    }
    if (threadIdx.x == 0) {
      if (split) uoff[U] = V;
      a.ucount[cb] = U;
    }
  }
  if (!a.fused) return;
  // the last slot of the run through position i (a run leaving the chunk:
  // followed in LDS)
  int lastsl[PER];
  {
    int ls = vv[PER - 1];
    if (eq[PER - 1]) {
      int pos = t0 + PER;
      while (pos < V && (unsigned)(s_key[pos] >> 32) == kk[PER - 1]) pos++;
      ls = (int)(unsigned)s_key[pos - 1];
    }
    lastsl[PER - 1] = ls;
  }
#pragma unroll
  for (int i = PER - 2; i >= 0; i--) lastsl[i] = eq[i] ? lastsl[i + 1] : vv[i];
  // classes of the runs starting here: 0 single, 1 local, kDefer (+ 2 + m)
  int cls[PER];
  int ns = 0;
#pragma unroll
  for (int i = 0; i < PER; i++) {
    cls[i] = 0;
    if (st[i] && eq[i]) {
      cls[i] = (vv[i] / R == lastsl[i] / R) ? 1 : kDefer;
      ns += cls[i] == kDefer;
    }
  }
  int S = 0;
  int m = block_exclusive_scan(ns, &S, s_ws);
  int *keys = skey + (size_t)cb * a.Mmax;
  {
    int u = u0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
      if (!st[i]) continue;
      if (cls[i] == kDefer) {
        cls[i] = kDefer | (2 + m);
        keys[m++] = (int)kk[i];
      }
      // 16-bit in LDS: 0, 1 or 0x8000 | (2 + m) (2 + m <= SB / 2 + 2 < 2^15)
      s_runm[u++] = (unsigned short)(cls[i] & kDefer ? 0x8000 | (cls[i] & 0x7fff) : cls[i]);
    }
  }
  __syncthreads();
  auto k32 = [&](int t) { return (unsigned)(s_key[t] >> 32); };
  auto slot = [&](int t) { return (int)(unsigned)(s_key[t] & 0xffffffffu); };
  unsigned *sc = a.scode + (size_t)cb * a.SB;
  // the run through the chunk's first position began before it: its class
  int cur = 0;
  if (u0 > 0 && vld[0] && !st[0]) {
    const int v = s_runm[u0 - 1];
    cur = v & 0x8000 ? kDefer | (v & 0x7fff) : v;
  }
#pragma unroll
  for (int i = 0; i < PER; i++) {
    if (!vld[i]) continue;
    if (st[i]) cur = cls[i];
    const int t = t0 + i;
    unsigned code = kSOwn;
    if (cur & kDefer) {
      code = kSShared | (st[i] ? kSOwn : 0u) | (unsigned)(cur & (kDefer - 1));
    } else if (cur) {
      // local: as defer_codes
      int rs = t;
      while (rs > 0 && k32(rs - 1) == kk[i]) rs--;
      int re = t + 1;
      while (re < V && k32(re) == kk[i]) re++;
      const int me = emit_pos(vv[i] % R, a.K);
      int first = 1, last = 1, own = vv[i] % R;
      for (int j = rs; j < re; j++) {
        const int e2 = emit_pos(slot(j) % R, a.K);
        first &= e2 >= me;
        last &= e2 <= me;
        if (e2 > emit_pos(own, a.K)) own = slot(j) % R;
      }
      code = kSLocal | (last ? kSOwn : 0u) | (first ? kSFirst : 0u) | (unsigned)own;
    }
    sc[vv[i]] = code;
  }
  if (threadIdx.x == 0) sM[cb] = S;
}

__device__ __forceinline__ int bsearch_lds(const int *v, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (v[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && v[lo] == key ? lo : -1;
}

// Record placement of one batch for train_step (one workgroup per batch of
// the chunk, after train_prep): records without neighbour lists first
// (stable; position p to workgroup p % NBF), RW words per group (R slot ids / codes, kFX flush slots, the
// batch words: overflow flushes and the gacc entries train_step zeroes,
// i.e. the deferred rows of the batch two before this one). Slot
// codes get kSPend | m' << 12 where the row is deferred entry m' of the
// previous batch (that batch's keys: skey_cur[cb - 1], or the previous
// chunk's last batch). The previous batch's deferred rows this batch does not
// touch become flush slots (the group of record position f % nb, slot f / nb), past kFX * nb the
// overflow list.
__global__ __launch_bounds__(kTB) void train_place(TrainArgs a, int nbc, int CB,
                                                   const int *skey_cur, const int *sM_cur,
                                                   const int *skey_pc, const int *sM_pc,
                                                   int has_prev) {
  extern __shared__ int s_dyn[];
  __shared__ int s_pos[kPackB];
  __shared__ int s_ws[kTB / 64];
  const int cb = blockIdx.x;
  if (cb >= nbc) return;
  const int nb = a.bmeta[cb].x;
  const int R = a.R, K = a.K, RW = a.RW, RPB = a.prpb, SB = a.SB;
  const int G = (a.B + RPB - 1) / RPB * RPB;
  const int *prev = nullptr;
  int Mp = 0, Mpp = 0;  // deferred rows of the batches one and two before
  if (cb > 0) {
    prev = skey_cur + (size_t)(cb - 1) * a.Mmax;
    Mp = sM_cur[cb - 1];
  } else if (has_prev) {
    prev = skey_pc + (size_t)(CB - 1) * a.Mmax;
    Mp = sM_pc[CB - 1];
  }
  if (cb > 1) Mpp = sM_cur[cb - 2];
  else if (has_prev) Mpp = sM_pc[CB - 2 + cb];
  const int U = a.ucount[cb];
  int *s_prev = s_dyn, *s_u = s_dyn + a.Mmax;
  __shared__ int s_brk;
  if (threadIdx.x == 0) s_brk = 0;
  for (int j = threadIdx.x; j < Mp; j += kTB) s_prev[j] = prev[j];
  for (int j = threadIdx.x; j < U; j += kTB) s_u[j] = a.ukey[(size_t)cb * SB + j];
  const int *bidx = a.bidx + (size_t)cb * a.B * R;
  const float *btgt = a.btgt + (size_t)cb * a.B * 3;
  __syncthreads();
  // a record naming two of the previous batch's deferred rows: the batch
  // takes train_step's MULTI form (the light form folds one per record)
  for (int i = threadIdx.x; i < nb && Mp; i += kTB) {
    int e0 = -1;
    for (int s2 = 0; s2 < R; s2++) {
      const int row = bidx[i * R + s2];
      if (row == 0) continue;
      const int j = bsearch_lds(s_prev, Mp, ((int)slot_is_edge(s2, K) << 30) | row);
      if (j < 0) continue;
      if (e0 >= 0 && j != e0) s_brk = 1;
      e0 = j;
    }
  }
  __syncthreads();
  // the flag for the forms with a light kernel; the call's count of flagged
  // batches in ovf[kOvfMulti] (zeroed with the step buffer, read with every
  // epoch's loss)
  if (threadIdx.x == 0) {
    a.pbrk[cb] = s_brk;
    if (s_brk) atomicAdd(a.ovf + kOvfMulti, 1);
  }
  // stable partition: records without lists first
  {
    const int per = (nb + kTB - 1) / kTB, i0 = threadIdx.x * per, i1 = min(i0 + per, nb);
    int cs = 0;
    for (int i = i0; i < i1; i++) {
      int any = 0;
      for (int s = 4; s < R; s++) any |= bidx[i * R + s];
      s_pos[i] = any;  // temporarily: has a list
      cs += any == 0;
    }
    int NS = 0;
    int bs = block_exclusive_scan(cs, &NS, s_ws);
    // position p of the partitioned order -> workgroup p % NBF, group p / NBF:
    // every workgroup gets its share of the list records (the step's slowest
    // workgroup sets the batch time), its list-less records first
    const int NBF = G / RPB;
    for (int i = i0; i < i1; i++) {
      const bool sh = s_pos[i] == 0;
      const int p = sh ? bs : NS + (i - bs);
      s_pos[i] = (p % NBF) * RPB + p / NBF;
      bs += sh;
    }
  }
  int *pidx = a.pidx + (size_t)cb * G * RW;
  unsigned *pcode = a.pcode + (size_t)cb * G * RW;
  float *ptgt = a.ptgt + (size_t)cb * G * 3;
  for (int t = threadIdx.x; t < G * RW; t += kTB) {
    pidx[t] = 0;
    pcode[t] = 0u;
  }
  for (int t = threadIdx.x; t < G * 3; t += kTB) ptgt[t] = 0.f;
  __syncthreads();  // s_pos, s_prev, s_u; zero fill before the scattered writes
  const unsigned *sc = a.scode + (size_t)cb * SB;
  for (int t = threadIdx.x; t < nb * R; t += kTB) {
    const int i = t / R, s = t - i * R;
    const int row = bidx[t];
    unsigned code = 0;
    if (row != 0) {
      code = sc[t];
      if (Mp) {
        const int j = bsearch_lds(s_prev, Mp, ((int)slot_is_edge(s, K) << 30) | row);
        if (j >= 0) code |= kSPend | ((unsigned)(2 + j) << kDefBits);
      }
    }
    pidx[s_pos[i] * RW + s] = row;
    pcode[s_pos[i] * RW + s] = code;
  }
  for (int t = threadIdx.x; t < nb * 3; t += kTB) {
    const int i = t / 3;
    ptgt[s_pos[i] * 3 + (t - 3 * i)] = btgt[t];
  }
  // flush entries, in the previous batch's entry order
  const int per = (Mp + kTB - 1) / kTB, j0 = threadIdx.x * per, j1 = min(j0 + per, Mp);
  int cf = 0;
  for (int j = j0; j < j1; j++) cf += bsearch_lds(s_u, U, s_prev[j]) < 0;
  int F = 0;
  int f = block_exclusive_scan(cf, &F, s_ws);
  const int cap = kFX * nb;
  for (int j = j0; j < j1; j++) {
    const int key = s_prev[j];
    if (bsearch_lds(s_u, U, key) >= 0) continue;
    if (f < cap) {
      const int p = f % nb, k = f / nb, g = (p % (G / RPB)) * RPB + p / (G / RPB);
      pidx[g * RW + R + k] = key & 0x3fffffff;
      pcode[g * RW + R + k] = ((key >> 30) ? kFEdge : 0u) | ((unsigned)(2 + j) << kDefBits);
    } else {
      a.pfo[(size_t)cb * a.Mmax + (f - cap)] = make_int2(key, 2 + j);
    }
    f++;
  }
  const int nfo = max(F - cap, 0);
  for (int g = threadIdx.x; g < G; g += kTB) {
    pidx[g * RW + R + kFX] = nfo;
    pidx[g * RW + R + kFX + 1] = Mpp;
  }
}

// One workgroup per batch of the chunk: sorted unique (table,row) keys of
// the non-padding slots and, per key, its slot ids in ascending order.
__global__ __launch_bounds__(kTB) void train_prep(TrainArgs a, int64_t base,
                                                  int nbc, int P, int *skey, int *sM) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_key[];
  __shared__ int s_ws[kTB / 64];
  const int cb = blockIdx.x;
  if (cb >= nbc) {  // graph nodes past the last batch find no work
    if (threadIdx.x == 0) a.bmeta[cb] = make_int2(0, 0);
    return;
  }
  // (diagnostic phase trace: the first chunk's workgroups in trace slot
  // [batch 0][kernel 1][cb], stamps: start, ids, slot gathers, sort, unique
  // runs, codes)
  unsigned long long ts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (g_trace) ts[0] = __builtin_amdgcn_s_memrealtime();
  const int64_t r0 = (base + cb) * a.B;
  const int nb = (int)min((int64_t)a.B, a.n - r0);
  if (threadIdx.x == 0) a.bmeta[cb] = make_int2(nb, (int)(base + cb));
  const int R = a.R, K = a.K;
  const int S = nb * R;
  int *bidx = a.bidx + (size_t)cb * a.B * R;
  float *btgt = a.btgt + (size_t)cb * a.B * 3;
  // the batch's record ids once into LDS, then every gather below has one
  // round trip; slot rows 8 per thread in flight before the stores
  // the batch's record ids, in the dynamic region behind the keys: where the
  // run classes go later (radix path: 16-bit classes, so 4 workgroups fit a
  // CU's LDS) or behind them (bitonic path)
  int *s_perm = reinterpret_cast<int *>(s_key + P) + (P == kSortP ? 0 : P);
  for (int i = threadIdx.x; i < nb; i += kTB) s_perm[i] = a.perm[r0 + i];
  __syncthreads();
  HGX_STAMP(ts[1]);
  for (int t = threadIdx.x; t < nb * 3; t += kTB) {
    const int i = t / 3;
    btgt[t] = a.tgt[(int64_t)s_perm[i] * 3 + (t - 3 * i)];
  }
  for (int t0 = threadIdx.x; t0 < P; t0 += 8 * kTB) {
    int rv[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int t = t0 + u * kTB, i = t / R;
      rv[u] = t < S ? a.idx[(int64_t)s_perm[i] * R + (t - i * R)] : 0;
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int t = t0 + u * kTB;
      if (t >= P) break;
      unsigned long long key = ~0ull;
      if (t < S) {
        const int s = t % R, row = rv[u];
        bidx[t] = row;
        if (row != 0) {
          const unsigned k32 = ((unsigned)slot_is_edge(s, K) << 30) | (unsigned)row;
          key = ((unsigned long long)k32 << 32) | (unsigned)t;
        }
      }
      s_key[t] = key;
    }
  }
  __syncthreads();
  HGX_STAMP(ts[2]);
  constexpr int IPT = kSortP / kTB;
  unsigned kk[IPT];
  int vv[IPT];
  if (P == kSortP) {
    // the common batch (256 records x 14 slots): a block radix sort of the
    // 32-bit (table, row) keys with the slot as value, 8-bit digits, 4
    // passes, stable (equal keys keep slot order: the same order as the
    // 64-bit (key, slot) keys below); its storage aliases s_key. 4.5x faster
    // than the bitonic network (73 -> 16 us per batch).
    using BRS = rocprim::block_radix_sort<unsigned, kTB, kSortP / kTB, int>;
    static_assert(sizeof(typename BRS::storage_type) <= kSortP * 8 + kPrepB * 4,
                  "sort storage fits the radix path's dynamic LDS");
#pragma unroll
    for (int i = 0; i < IPT; i++) {
      const unsigned long long x = s_key[threadIdx.x * IPT + i];
      kk[i] = (unsigned)(x >> 32);  // padding: 0xffffffff, after every key
      vv[i] = (int)(unsigned)x;
    }
    __syncthreads();
    BRS().sort(kk, vv, *reinterpret_cast<typename BRS::storage_type *>(s_key));
    __syncthreads();
#pragma unroll
    for (int i = 0; i < IPT; i++)
      s_key[threadIdx.x * IPT + i] =
          kk[i] == 0xffffffffu ? ~0ull : ((unsigned long long)kk[i] << 32) | (unsigned)vv[i];
    __syncthreads();
  } else {
    for (int size = 2; size <= P; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = threadIdx.x; t < P / 2; t += kTB) {
          const int lo = 2 * t - (t & (stride - 1));
          const int hi = lo + stride;
          const bool up = ((lo & size) == 0);
          const unsigned long long x = s_key[lo], y = s_key[hi];
          if ((x > y) == up) {
            s_key[lo] = y;
            s_key[hi] = x;
          }
        }
        __syncthreads();
      }
    }
  }
  HGX_STAMP(ts[3]);
  if (P == kSortP) {
    prep_runs_regs<IPT>(a, cb, P, kk, vv, s_key, s_ws,
                        reinterpret_cast<unsigned short *>(s_key + P), skey, sM);
    HGX_STAMP(ts[5]);
    ts[4] = ts[5];
    if (g_trace && base == 0) trace_put(0, 1, 6, ts);
    return;
  }
  // unique starts over a contiguous chunk per thread, then one block scan
  const int per = P / kTB;
  const int t0 = threadIdx.x * per;
  int cnt = 0, valid = 0;
  for (int t = t0; t < t0 + per; t++) {
    const unsigned long long x = s_key[t];
    if (x == ~0ull) break;
    valid++;
    if (t == 0 || (unsigned)(s_key[t - 1] >> 32) != (unsigned)(x >> 32)) cnt++;
  }
  int U = 0, V = 0;
  int u = block_exclusive_scan(cnt, &U, s_ws);
  const int u0 = u;
  block_exclusive_scan(valid, &V, s_ws);
  int *ukey = a.ukey + (size_t)cb * a.SB;
  int *uoff = a.uoff + (size_t)cb * (a.SB + 1);
  int *inv = a.inv + (size_t)cb * a.SB;
  // (slot positions and run offsets feed the two-kernel step only)
  const bool split = !a.fused;
  for (int t = t0; t < t0 + per; t++) {
    const unsigned long long x = s_key[t];
    if (x == ~0ull) break;
    if (split) inv[x & 0xffffffffu] = t;
    if (t == 0 || (unsigned)(s_key[t - 1] >> 32) != (unsigned)(x >> 32)) {
      ukey[u] = (int)(x >> 32);
      if (split) uoff[u] = t;
      u++;
    }
  }
  if (threadIdx.x == 0) {
    if (split) uoff[U] = V;
    a.ucount[cb] = U;
  }
  HGX_STAMP(ts[4]);
  if (a.fused)
    defer_codes(a, cb, V, P, u0, s_key, s_ws, reinterpret_cast<int *>(s_key + P), skey, sM);
  HGX_STAMP(ts[5]);
  if (g_trace && base == 0) trace_put(0, 1, 6, ts);
}

// deterministic two-level sum of the chunk's per-block losses:
// loss_partial (kLossBlocks blocks) then loss_final (one block)
constexpr int kLossBlocks = 256;
__global__ void loss_partial(const float *lossbuf, int64_t m, double *part) {
  __shared__ double s[kTB];
  double v = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)kTB + threadIdx.x; i < m;
       i += (int64_t)kLossBlocks * kTB)
    v += (double)lossbuf[i];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int o = kTB / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = s[0];
}
__global__ void loss_final(const double *part, double *acc) {
  __shared__ double s[kLossBlocks];
  s[threadIdx.x] = part[threadIdx.x];
  __syncthreads();
  for (int o = kLossBlocks / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *acc += s[0];
}

// the identity order (records already in epoch order, ctx->rec_in_order)
__global__ void iota_perm(int64_t n, int *perm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    perm[i] = (int)i;
}

__global__ void shuffle_keys(uint64_t seed, int epoch, int64_t n,
                             unsigned long long *keys, int *vals) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    keys[i] = hgx::rand64(seed, 0x5348554646ull + epoch, (uint64_t)i);
    vals[i] = (int)i;
  }
}

__global__ void max_index(const int *idx, int64_t n, int R, int K, int *out) {
  int mn = 0, me = 0, neg = 0;
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int *p = idx + r * R;
    for (int s = 0; s < R; s++) {
      const int v = p[s];
      neg |= v < 0;
      if (slot_is_edge(s, K)) me = max(me, v);
      else mn = max(mn, v);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = max(mn, __shfl_xor(mn, off));
    me = max(me, __shfl_xor(me, off));
    neg |= __shfl_xor(neg, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&out[0], mn);
    atomicMax(&out[1], me);
    atomicOr(&out[2], neg);
  }
}

__global__ void init_uniform(float *tab, int64_t rows, int d, int dp,
                             uint64_t seed, uint64_t stream) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       i < rows * dp; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % dp);
    float v = 0.f;
    if (c < d) {
      const uint64_t r = hgx::rand64(seed, stream, (uint64_t)i);
      v = -0.05f + 0.1f * (float)(r >> 40) * (1.0f / 16777216.0f);
    }
    tab[i] = v;
  }
}

__global__ void pad_rows(const float *src, float *dst, int64_t rows, int d,
                         int dp) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       i < rows * dp; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / dp;
    const int c = (int)(i % dp);
    dst[i] = c < d ? src[r * d + c] : 0.f;
  }
}

__global__ void unpad_rows(const float *src, float *dst, int64_t rows, int d,
                           int dp) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       i < rows * d; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / d;
    const int c = (int)(i % d);
    dst[i] = src[r * dp + c];
  }
}

}  // namespace
