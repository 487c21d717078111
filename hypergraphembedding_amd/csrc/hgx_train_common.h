// Trainer kernels, shared part: TrainArgs, the slot codes and size limits,
// the debug ablation / phase-trace hooks and the small row helpers.
// Included by hgx_train.hip only (one translation unit, see there).
#pragma once
#include "hgx_internal.h"

namespace {

constexpr int kTB = 256;
constexpr int kChunkRound = 64;  // a chunk buffer holds a multiple of this many batches

// diagnostic ablation bits (HGX_TRAIN_ABLATE, timing experiments only;
// results are wrong when set): 1 empty K1, 2 empty K2, 4 K1 gathers hit
// row 0, 8 K1 skips gradient stores, 16 K2 skips slot sums, 32 K2 skips
// the table read-modify-write; train_step: 1024 shared-row gradients by
// plain stores, 2048 no row-0 partial loads, 4096 no forward reductions,
// 8192 no Adagrad arithmetic, 16384 no end-of-batch barrier / partial
// stores, 32768 no neighbour-list gathers (timing ablations: wrong sums).
#ifdef HGX_DEBUG_KNOBS
__constant__ int g_tab = 0;  // ablation bits (diagnostic builds only)
#else
static constexpr int g_tab = 0;
#endif

// diagnostic phase trace (HGX_TRAIN_TRACE=<file>, timing experiments only):
// one wave of every workgroup stamps s_memrealtime (100 MHz) at phase ends
// for the first g_trace_nb batches; slots [batch][kernel][block < 1024][8].
// Diagnostic builds only: in a release build the trace pointer is a
// compile-time null, so the step's prologue has no dependent scalar load of a
// device global (GOT entry, then the value) ahead of its kernel-argument
// loads.
#ifdef HGX_DEBUG_KNOBS
__constant__ unsigned long long *g_trace = nullptr;
__constant__ int g_trace_nb = 0;
#else
static constexpr unsigned long long *g_trace = nullptr;
static constexpr int g_trace_nb = 0;
#endif
#define HGX_STAMP(var)                                              \
  do {                                                              \
    if (g_trace) {                                                  \
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   \
      var = __builtin_amdgcn_s_memrealtime();                       \
    }                                                               \
  } while (0)
// `who`: the one thread of the workgroup whose stamps are kept. The step
// passes the first lane of its last record group's (head) wave: placement
// deals the records without neighbour lists first, so wave 0 always holds one
// of those and its stamps under-report the waves that set the batch time.
__device__ __forceinline__ void trace_put(int gb, int kern, int nst,
                                          const unsigned long long *t, bool who) {
  if (g_trace && who && gb < g_trace_nb && blockIdx.x < 1024) {
    unsigned long long *q = g_trace + (((size_t)gb * 2 + kern) * 1024 + blockIdx.x) * 8;
    for (int i = 0; i < nst; i++) q[i] = t[i];
  }
}
__device__ __forceinline__ void trace_put(int gb, int kern, int nst,
                                          const unsigned long long *t) {
  trace_put(gb, kern, nst, t, threadIdx.x == 0);
}

struct TrainArgs {
  const int *idx;
  const float *tgt;
  const int *perm;
  int64_t n;
  int B, R, K, dp;
  float *ntab, *etab, *nacc, *eacc;
  float *gslot, *gzero, *lossbuf;
  // chunk buffers written by train_prep: batch-ordered records, each
  // slot's position in its batch's sorted (row, slot) order, unique keys
  int *bidx;
  float *btgt;
  int *inv, *ukey, *uoff, *ucount;
  int2 *bmeta;  // per chunk-local batch: {records (0 = no batch), global batch}
  int SB, nblk1;
  int lstride;  // per-batch stride of lossbuf (>= the blocks of either path)
  float lr, eps;
  int loss, act;
  // deferred-row step (train_step, train_place): per chunk-local batch
  // ceil(B / prpb) workgroups x prpb groups of RW words (R slot ids / codes
  // + kFX flush slots) and 3 targets; per-slot codes and the deferred rows'
  // keys from train_prep; deferred entries per batch (pM), flush overflow
  // list (pfo). gacc [3][MX][dp] fixed-point sums and shadow [3][MX][2][dp]
  // base rows of deferred entries by batch parity (entries 0 / 1: row 0 of
  // the node / edge table, shadow only); r0acc the padding row's gradient
  // sums, kR0Slots fixed-point accumulators per batch parity; ovf[0] the
  // fixed-point range flag, ovf[kOvfMulti] the call's count of batches
  // train_place flagged MULTI.
  int fused, prpb, RW, MX, Mmax;
  int *pidx, *pbrk;
  unsigned *pcode, *scode;
  float *ptgt;
  int2 *pfo;
  long long *gacc;
  float *shadow;
  long long *r0acc;  // [3][kR0Slots][2][dp] fixed point, see Row0Loads
  int *ovf;
};

// slot codes of the deferred-row step (train_prep / train_place -> train_step)
constexpr unsigned kSShared = 0x80000000u;  // row in several records: deferred entry m
constexpr unsigned kSOwn = 0x40000000u;     // this slot writes the row (or its shadow)
constexpr unsigned kSPend = 0x20000000u;    // row deferred by the previous batch: entry m'
constexpr unsigned kSLocal = 0x10000000u;   // row in several slots of ONE record
constexpr unsigned kSFirst = 0x08000000u;   // local: first slot in emit order (no read)
                                            // local: bits 0..3 the owner slot
constexpr unsigned kFEdge = 0x10000000u;    // flush slot words: edge table
constexpr int kDefBits = 14;                // m / slot mask in bits 0..13, m' in 14..25
constexpr unsigned kDefMask = 0xfffu;
constexpr unsigned kSlotMask = 0x3fffu;
constexpr int kFX = 4;                      // flush slots per record group
constexpr int kWX = kFX + 2;                // + batch words: overflow flushes,
                                            //   gacc entries to zero
constexpr int kOvfMulti = 1;                // word of TrainArgs::ovf, see there
constexpr int kPackB = 512;                 // max records per step batch
constexpr int kPrepB = 1366;  // max records per prepared batch: 8192 slots / R >= 6
constexpr int kSortP = 4096;  // prepared-batch slot count sorted by block radix sort

__device__ __forceinline__ bool slot_is_edge(int s, int K) {
  return s == 1 || s == 3 || s >= 4 + K;
}

__device__ __forceinline__ float act_f(int act, float z) {
  return act == 0 ? 1.0f / (1.0f + expf(-z)) : (z > 0.f ? z : 0.f);
}
__device__ __forceinline__ float act_d(int act, float z, float y) {
  return act == 0 ? y * (1.0f - y) : (z > 0.f ? 1.f : 0.f);
}
// per-sample loss value and dL/dyhat (before the 1/batch factor)
__device__ __forceinline__ void head_loss(int loss, float y, float yt,
                                          float &lv, float &g) {
  const float eps = 1e-7f;
  if (loss == 0) {  // KLD with Keras clipping
    const float ytc = fminf(fmaxf(yt, eps), 1.f);
    const float ypc = fminf(fmaxf(y, eps), 1.f);
    lv = ytc * logf(ytc / ypc);
    g = (y >= eps && y <= 1.f) ? -ytc / ypc : 0.f;
  } else {  // MSE
    const float df = y - yt;
    lv = df * df;
    g = 2.f * df;
  }
}

__device__ __forceinline__ float4 f4(float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float4 operator+(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
__device__ __forceinline__ float4 fma4(float s, float4 v, float4 a) {
  return make_float4(fmaf(s, v.x, a.x), fmaf(s, v.y, a.y), fmaf(s, v.z, a.z),
                     fmaf(s, v.w, a.w));
}
__device__ __forceinline__ float dot4(float4 a, float4 b) {
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

template <int L>
__device__ __forceinline__ float group_sum(float v) {
  return hgx::group_allreduce_sum<L>(v);
}

template <int L, int VPL>
__device__ __forceinline__ void load_row(const float *tab, int row, int dp,
                                         int lane, float4 (&out)[VPL]) {
  const float4 *p = reinterpret_cast<const float4 *>(tab + (size_t)row * dp);
#pragma unroll
  for (int v = 0; v < VPL; v++) out[v] = p[v * L + lane];
}

}  // namespace
