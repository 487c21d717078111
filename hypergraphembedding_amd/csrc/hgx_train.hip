// FOBE/HOBE trainer on MI355X: Keras-semantics Adagrad over the record
// stream, one synchronous batch at a time.
//
// Reference: hg2v_model.py:51-125 (BooleanModel: sigmoid heads, KLD),
// 129-203 (UnweightedFloatModel: relu heads, MSE); embedding.py:269-305
// (fit: batch 256, shuffle per epoch, EarlyStopping(loss, min_delta 1e-3,
// patience 0)); KerasModelToEmbedding hg2v_model.py:31-48 (row idx+1).
//   nn = act(N[ln].N[rn]), ee = act(E[le].E[re]),
//   ne = mean_k act(N[nn_k].N[ln]) * mean_k act(E[ne_k].E[re]);
//   loss = sum over heads of the batch mean; Adagrad a += g^2,
//   p -= lr*g/(sqrt(a)+eps) with the gradients of duplicate rows summed
//   (TF densifies the IndexedSlices before the update).
//
// Per batch (strictly sequential, like Keras):
//   K1 train_fwd_bwd  -- one L-lane group per record (L*VPL*4 = padded d):
//      gather the 4+2K rows, 2+2K dots (xor-shuffle reductions), heads,
//      loss, and the per-slot gradient rows -> gslot[B*R][dp]. Gradients of
//      the padding row 0 (touched by almost every record) are pre-summed
//      per workgroup -> gzero[blk][2][dp], so no row sees >~B/RPB addends.
//   K2 train_update   -- one group per unique touched row of the batch:
//      sum its slot rows in sorted slot order (deterministic) and apply
//      Adagrad in place.
// The unique-row lists come from train_prep, run for a whole chunk of
// batches in parallel (one workgroup per batch: block radix sort of the
// batch's (row, slot) keys; an LDS bitonic network for other batch shapes).
// K1/K2 of a chunk's batches are direct launches, the chunk-local batch index
// passed as a kernel argument (no device counters, no dependent index load).
// Preparation runs once per chunk of up to 1024 batches, by default on the
// same stream before the chunk's batches; tuning train_prep_overlap runs
// chunk c + 1's on a second stream while chunk c trains (train_prep_cus:
// disjoint CU masks for the two streams).
//
// One translation unit: the kernels live in hgx_train_*.h, included below in
// dependency order (the debug symbols g_tab / g_trace stay with the kernels
// that read them); this file keeps the kernel pickers, the hgx_records_* /
// hgx_model_* API and the driver hgx_train.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hgx_internal.h"
#include "hgx_train_common.h"
#include "hgx_train_split.h"
#include "hgx_train_step.h"
#include "hgx_train_prep.h"
#include "hgx_train_layout.h"

namespace {

int grid_for(int64_t work, int per_block) {
  int64_t g = (work + per_block - 1) / per_block;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, 4096));
}

// lanes per record L (power of two <= 64) and float4 per lane VPL
void geometry(int d, int &L, int &VPL) {
  const int nv = (d + 3) / 4;
  L = 1;
  while (L < nv && L < 64) L *= 2;
  VPL = (nv + L - 1) / L;
  if (VPL == 3) VPL = 4;
}

// slots of a batch rounded up for train_prep's sort (a power of two >= kTB)
int sort_slots(int SB) {
  int P = 1;
  while (P < SB) P <<= 1;
  return std::max(P, kTB);
}

using KFn = void (*)(TrainArgs, int);

int env_int(const char *name, int dflt) { return hgx_debug_env(name, dflt); }

template <int L, int VPL, int TB>
KFn fwd_spec(int K, int loss, int act) {
  if (K == 5 && loss == 0 && act == 0) return train_fwd_bwd<L, VPL, 5, true, 1, TB>;
  if (K == 5 && loss == 1 && act == 1) return train_fwd_bwd<L, VPL, 5, true, 2, TB>;
  return nullptr;
}

template <int L, int VPL>
KFn fwd_for(int K, int loss, int act, int tb1) {
  KFn f = tb1 == 512 ? fwd_spec<L, VPL, 512>(K, loss, act)
                     : fwd_spec<L, VPL, kTB>(K, loss, act);
  if (f) return f;
  if (K <= 2) return train_fwd_bwd<L, VPL, 2, false, 0, kTB>;
  if (K <= 5) return train_fwd_bwd<L, VPL, 5, false, 0, kTB>;
  if (K <= 8) return train_fwd_bwd<L, VPL, 8, false, 0, kTB>;
  return train_fwd_bwd<L, VPL, 16, false, 0, kTB>;
}

// (the step's parameter list: HGX_STEP_PARAMS in hgx_train_step.h)
#if HGX_TRAIN_PRELOAD
using KStepFn = void (*)(const int *, const unsigned *, const float *, int, int, int, float, int,
                         int, TrainArgs);
#else
using KStepFn = void (*)(TrainArgs, int, int, int, int);
#endif
using KFlushFn = void (*)(TrainArgs, const int *, const int *, const int *, int, int);

// deferred-row step: d in (64, 256], K = 5 with the FOBE (sigmoid/KLD) or
// HOBE (relu/MSE) heads. One SL-lane group per record with VW floats per lane
// (dp = SL VW): float4 x 32 lanes or float2 x 64 lanes for dp = 128, float4 x
// 64 lanes for dp = 256. tb = the workgroup size (records per workgroup =
// tb / SL, ceil(batch / (tb / SL)) workgroups). The flush kernel views rows
// as float4.
template <int SL, int VW, int TB>
void step_fns(int loss, KStepFn *kf, KFlushFn &kfl) {
  kf[0] = loss == 0 ? train_step<SL, VW, 5, 1, TB, false>
                    : train_step<SL, VW, 5, 2, TB, false>;
  kf[1] = loss == 0 ? train_step<SL, VW, 5, 1, TB, true>
                    : train_step<SL, VW, 5, 2, TB, true>;
  kfl = train_flush<SL * VW / 4>;
}
// A merged form (HGX_TRAIN_ONEKERNEL, see hgx_train_step.h) is one kernel:
// kf[0] == kf[1], which is what tells the driver that it needs no MULTI flags
// on the host.
// HGX_TRAIN_CHUNKWAIT=1 (A/B builds): the flag copy and the per-chunk host
// wait kept for a merged form too (the kernel's cost apart from the driver's)
#ifndef HGX_TRAIN_CHUNKWAIT
#define HGX_TRAIN_CHUNKWAIT 0
#endif
constexpr bool kMergePair4 = HGX_TRAIN_ONEKERNEL >= 1;  // paired form, float4 rows
constexpr bool kMergeAll = HGX_TRAIN_ONEKERNEL == 2;    // paired and quad, every width
template <int VW>
void step_fns_pair(int loss, KStepFn *kf, KFlushFn &kfl) {
  constexpr bool M0 = kMergeAll || (kMergePair4 && VW == 4);  // MULTI of kf[0]
  kf[0] = loss == 0 ? train_step<64, VW, 5, 1, 512, M0, true>
                    : train_step<64, VW, 5, 2, 512, M0, true>;
  kf[1] = loss == 0 ? train_step<64, VW, 5, 1, 512, true, true>
                    : train_step<64, VW, 5, 2, 512, true, true>;
  kfl = train_flush<64 * VW / 4>;
}
// the quad form: one record on four waves, RPB records per 256 RPB-thread
// workgroup, float2 rows (see train_step_quad)
template <int RPB>
void step_fns_quad(int loss, KStepFn *kf, KFlushFn &kfl) {
  kf[0] = loss == 0 ? train_step_q<2, 5, 1, kMergeAll, RPB> : train_step_q<2, 5, 2, kMergeAll, RPB>;
  kf[1] = loss == 0 ? train_step_q<2, 5, 1, true, RPB> : train_step_q<2, 5, 2, true, RPB>;
  kfl = train_flush<32>;
}
// the default form per row width: 1 paired, 4 quad at one record per
// workgroup (interleaved A/B)
constexpr int kPairDefault128 = 4, kPairDefault256 = 1;
// lanes = the tuning (0 auto, 32 or 64 lanes per record where dp = 128);
// sets sl (the step's lanes per record), tb, rpb (records per workgroup) and
// the kernels. pair = the tuning (-1 per geometry): at 64 lanes per record 1
// the paired-wave form, 512 threads for 4 records; 3 the quad form, 512
// threads for 2 records, 4 the quad form, 256 threads for 1 record (float2
// rows; at float4 rows the paired form).
bool pick_step(int L, int VPL, int K, int loss, int act, int lanes, int pair, int &sl,
               int &tb, int &rpb, KStepFn *kf, KFlushFn &kfl) {
  if (VPL != 1 || K != 5 || loss != act) return false;
  if (L != 32 && L != 64) return false;
  // dp = 128, measured r02 (tools/ab_train.py, interleaved, us per batch on
  // random / C3 HOBE records): float2 x 64 lanes at 256 threads 7.63 / 7.79;
  // float4 x 32 lanes at 128 threads 8.07 / 8.42 (8.33 / 8.75 at 256)
  const int vw = L == 32 && lanes != 32 ? 2 : 4;
  sl = L * 4 / vw;
  // (an explicit train_tb keeps the one-wave form it names)
  const int pair_auto = tb != 0 ? 0 : vw == 2 ? kPairDefault128 : kPairDefault256;
  const int form = pair < 0 ? pair_auto : pair;
  if (sl == 64 && vw == 2 && form == 3) {
    tb = 512;
    rpb = 2;
    step_fns_quad<2>(loss, kf, kfl);
    return true;
  }
  if (sl == 64 && vw == 2 && form == 4) {
    tb = 256;
    rpb = 1;
    step_fns_quad<1>(loss, kf, kfl);
    return true;
  }
  if (sl == 64 && form) {
    tb = 512;
    rpb = 4;
    if (vw == 2) step_fns_pair<2>(loss, kf, kfl);
    else step_fns_pair<4>(loss, kf, kfl);
    return true;
  }
  if (sl == 32) {
    tb = tb == 256 ? 256 : 128;
    if (tb == 128) step_fns<32, 4, 128>(loss, kf, kfl);
    else step_fns<32, 4, 256>(loss, kf, kfl);
  } else if (vw == 2) {
    tb = tb == 512 || tb == 128 ? tb : 256;
    if (tb == 512) step_fns<64, 2, 512>(loss, kf, kfl);
    else if (tb == 128) step_fns<64, 2, 128>(loss, kf, kfl);
    else step_fns<64, 2, 256>(loss, kf, kfl);
  } else {
    tb = 256;
    step_fns<64, 4, 256>(loss, kf, kfl);
  }
  rpb = tb / sl;
  return true;
}

bool pick_kernels(int L, int VPL, int K, int loss, int act, int &tb1, int tb2,
                  KFn &k1, KFn &k2) {
#define HGX_CASE(LL, VV)                                                     \
  if (L == LL && VPL == VV) {                                                \
    k1 = env_int("HGX_TRAIN_GENERIC", 0) == 1                                \
             ? train_fwd_bwd<LL, VV, 16, false, 0, kTB>                      \
             : fwd_for<LL, VV>(K, loss, act, tb1);                           \
    k2 = tb2 == 512 ? train_update<LL, VV, 512> : train_update<LL, VV, kTB>; \
    return true;                                                             \
  }
  HGX_CASE(1, 1) HGX_CASE(2, 1) HGX_CASE(4, 1) HGX_CASE(8, 1)
  HGX_CASE(16, 1) HGX_CASE(32, 1) HGX_CASE(64, 1) HGX_CASE(64, 2)
  HGX_CASE(64, 4)
#undef HGX_CASE
  return false;
}


}  // namespace

// ---------------------------------------------------------------------------
// records
// ---------------------------------------------------------------------------
// n records copied into the context (from the host or the device) as one block
static int records_write(hgx_ctx *ctx, int64_t n, int K, const void *idx, const void *tgt,
                         hipMemcpyKind kind) {
  const int R = 4 + 2 * K;
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_TRY(hgx_ensure(ctx, ctx->rec_idx, sizeof(int32_t) * (n * R + 1)));
  HGX_TRY(hgx_ensure(ctx, ctx->rec_tgt, sizeof(float) * (n * 3 + 1)));
  if (n) {
    HGX_HIP(ctx, hipMemcpyAsync(ctx->rec_idx.p, idx, sizeof(int32_t) * n * R, kind, ctx->stream));
    HGX_HIP(ctx, hipMemcpyAsync(ctx->rec_tgt.p, tgt, sizeof(float) * n * 3, kind, ctx->stream));
  }
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->n_rec = n;
  ctx->K = K;
  ctx->smp_family = -1;
  ctx->rec_in_order = false;
  ctx->store_carry = 0;  // no store batch tail survives a rewrite
  ctx->rec_bounds[0] = 0;
  ctx->rec_bounds[1] = n;
  ctx->n_rec_blocks = 1;
  return HGX_OK;
}

extern "C" int hgx_records_set(hgx_ctx *ctx, int64_t n, int K,
                               const int32_t *idx, const float *tgt) {
  if (!ctx) return HGX_EINVAL;
  HGX_CHECK(ctx, n >= 0 && K >= 1 && K <= 16, HGX_EUNSUP,
            "num_neighbors K=%d outside [1,16]", K);
  HGX_CHECK(ctx, n == 0 || (idx && tgt), HGX_EINVAL, "null record buffer");
  for (int64_t i = 0; i < n * (4 + 2 * K); i++)
    HGX_CHECK(ctx, idx[i] >= 0, HGX_EINVAL, "negative record index");
  return records_write(ctx, n, K, idx, tgt, hipMemcpyHostToDevice);
}

extern "C" int hgx_records_blocks(hgx_ctx *ctx, int *nblocks, int64_t *bounds) {
  if (!ctx) return HGX_EINVAL;
  if (nblocks) *nblocks = ctx->n_rec_blocks;
  if (bounds)
    for (int i = 0; i <= ctx->n_rec_blocks; i++) bounds[i] = ctx->rec_bounds[i];
  return HGX_OK;
}

// the context's records copied out (to the host or the device); null: not wanted
static int records_read(hgx_ctx *ctx, void *idx, void *tgt, hipMemcpyKind kind) {
  const int64_t n = ctx->n_rec;
  const int R = 4 + 2 * ctx->K;
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  if (idx)
    HGX_HIP(ctx, hipMemcpyAsync(idx, ctx->rec_idx.p, sizeof(int32_t) * n * R, kind, ctx->stream));
  if (tgt)
    HGX_HIP(ctx, hipMemcpyAsync(tgt, ctx->rec_tgt.p, sizeof(float) * n * 3, kind, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_records_export(hgx_ctx *ctx, void *d_idx, void *d_tgt) {
  if (!ctx) return HGX_EINVAL;
  if (ctx->n_rec == 0) return HGX_OK;
  HGX_CHECK(ctx, d_idx || d_tgt, HGX_EINVAL, "null export buffer");
  return records_read(ctx, d_idx, d_tgt, hipMemcpyDeviceToDevice);
}

extern "C" int hgx_records_import(hgx_ctx *ctx, int64_t n, int K,
                                  const void *d_idx, const void *d_tgt,
                                  int nblocks, const int64_t *bounds) {
  if (!ctx) return HGX_EINVAL;
  HGX_CHECK(ctx, n >= 0 && K >= 1 && K <= 16, HGX_EUNSUP,
            "num_neighbors K=%d outside [1,16]", K);
  HGX_CHECK(ctx, n == 0 || (d_idx && d_tgt), HGX_EINVAL, "null record buffer");
  HGX_CHECK(ctx, nblocks >= 0 && nblocks <= hgx_ctx::kMaxRecBlocks, HGX_EINVAL,
            "%d record blocks (at most %d)", nblocks, hgx_ctx::kMaxRecBlocks);
  if (nblocks > 0) {
    HGX_CHECK(ctx, bounds && bounds[0] == 0 && bounds[nblocks] == n, HGX_EINVAL,
              "block bounds must run from 0 to n");
    for (int i = 0; i < nblocks; i++)
      HGX_CHECK(ctx, bounds[i] <= bounds[i + 1], HGX_EINVAL,
                "block bounds not ascending");
  }
  HGX_TRY(records_write(ctx, n, K, d_idx, d_tgt, hipMemcpyDeviceToDevice));
  if (nblocks > 0) {
    for (int i = 0; i <= nblocks; i++) ctx->rec_bounds[i] = bounds[i];
    ctx->n_rec_blocks = nblocks;
  }
  return HGX_OK;
}

// The records of `src` (and their kind blocks) copied device to device into
// `dst` on the same device: the hand-over of a chunk sampled on one context
// (beside the training) to the training context.
extern "C" int hgx_records_copy(hgx_ctx *dst, hgx_ctx *src) {
  if (!dst || !src) return HGX_EINVAL;
  HGX_CHECK(dst, dst->device == src->device, HGX_EINVAL,
            "contexts on devices %d and %d", dst->device, src->device);
  HGX_HIP(dst, hipSetDevice(dst->device));
  HGX_HIP(dst, hipStreamSynchronize(src->stream));
  HGX_CHECK(dst, src->n_rec_blocks >= 0 && src->n_rec_blocks <= hgx_ctx::kMaxRecBlocks,
            HGX_EINVAL, "source has %d record blocks", src->n_rec_blocks);
  // (the same one-element slack as every other record writer)
  HGX_TRY(records_write(dst, src->n_rec, src->K, src->rec_idx.p, src->rec_tgt.p,
                        hipMemcpyDeviceToDevice));
  dst->smp_family = src->smp_family;
  dst->smp_seed = src->smp_seed;
  dst->rec_in_order = src->rec_in_order;
  dst->store_carry = 0;  // the tail (if any) stays with src's buffer
  dst->n_rec_blocks = src->n_rec_blocks;
  for (int i = 0; i <= src->n_rec_blocks; i++) dst->rec_bounds[i] = src->rec_bounds[i];
  return HGX_OK;
}

extern "C" int hgx_records_info(hgx_ctx *ctx, int64_t *n, int *K) {
  if (!ctx) return HGX_EINVAL;
  if (n) *n = ctx->n_rec;
  if (K) *K = ctx->K;
  return HGX_OK;
}

extern "C" int hgx_records_get(hgx_ctx *ctx, int32_t *idx, float *tgt) {
  if (!ctx) return HGX_EINVAL;
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->n_rec == 0) return HGX_OK;
  return records_read(ctx, idx, tgt, hipMemcpyDeviceToHost);
}

// ---------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------
// host rows [rows][d] -> the padded device table [rows][dp], staged in ctx->s1
static int upload_padded(hgx_ctx *ctx, const float *src, int64_t rows, float *tab) {
  HGX_HIP(ctx, hipMemcpyAsync(ctx->s1.p, src, sizeof(float) * rows * ctx->d,
                              hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(pad_rows, dim3(grid_for(rows * ctx->dp, 256)), dim3(256), 0,
                     ctx->stream, ctx->s1.as<float>(), tab, rows, ctx->d, ctx->dp);
  return HGX_OK;
}

extern "C" int hgx_model_init(hgx_ctx *ctx, int d, int64_t node_rows,
                              int64_t edge_rows, uint64_t seed,
                              const float *node_tab, const float *edge_tab) {
  if (!ctx) return HGX_EINVAL;
  HGX_CHECK(ctx, d >= 1 && d <= 1024, HGX_EUNSUP, "dimension %d outside [1,1024]", d);
  HGX_CHECK(ctx, node_rows >= 1 && edge_rows >= 1 && node_rows < (1 << 30) &&
                     edge_rows < (1 << 30),
            HGX_EUNSUP, "table rows outside [1, 2^30)");
  HGX_CHECK(ctx, (node_tab == nullptr) == (edge_tab == nullptr), HGX_EINVAL,
            "give both initial tables or neither");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  int L, VPL;
  geometry(d, L, VPL);
  const int dp = 4 * L * VPL;
  ctx->d = d;
  ctx->dp = dp;
  ctx->node_rows = node_rows;
  ctx->edge_rows = edge_rows;
  const size_t nb = sizeof(float) * node_rows * dp, eb = sizeof(float) * edge_rows * dp;
  HGX_TRY(hgx_ensure(ctx, ctx->ntab, nb));
  HGX_TRY(hgx_ensure(ctx, ctx->etab, eb));
  HGX_TRY(hgx_ensure(ctx, ctx->nacc, nb));
  HGX_TRY(hgx_ensure(ctx, ctx->eacc, eb));
  HGX_HIP(ctx, hipMemsetAsync(ctx->nacc.p, 0, nb, ctx->stream));
  HGX_HIP(ctx, hipMemsetAsync(ctx->eacc.p, 0, eb, ctx->stream));
  if (node_tab) {
    HGX_TRY(hgx_ensure(ctx, ctx->s1, sizeof(float) * std::max(node_rows, edge_rows) * d));
    HGX_TRY(upload_padded(ctx, node_tab, node_rows, ctx->ntab.as<float>()));
    HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // s1 is reused
    HGX_TRY(upload_padded(ctx, edge_tab, edge_rows, ctx->etab.as<float>()));
  } else {
    hipLaunchKernelGGL(init_uniform, dim3(grid_for(node_rows * dp, 256)),
                       dim3(256), 0, ctx->stream, ctx->ntab.as<float>(),
                       node_rows, d, dp, seed, (uint64_t)1);
    hipLaunchKernelGGL(init_uniform, dim3(grid_for(edge_rows * dp, 256)),
                       dim3(256), 0, ctx->stream, ctx->etab.as<float>(),
                       edge_rows, d, dp, seed, (uint64_t)2);
  }
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

// the padded device table [rows][dp] -> host rows [rows][d], staged in ctx->s1
static int download_unpadded(hgx_ctx *ctx, const float *tab, int64_t rows, float *dst) {
  hipLaunchKernelGGL(unpad_rows, dim3(grid_for(rows * ctx->d, 256)), dim3(256), 0, ctx->stream,
                     tab, ctx->s1.as<float>(), rows, ctx->d, ctx->dp);
  HGX_HIP(ctx, hipMemcpyAsync(dst, ctx->s1.p, sizeof(float) * rows * ctx->d,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_model_get(hgx_ctx *ctx, float *node_tab, float *edge_tab) {
  if (!ctx) return HGX_EINVAL;
  HGX_CHECK(ctx, ctx->d > 0, HGX_ESTATE, "no model on device");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  HGX_TRY(hgx_ensure(ctx, ctx->s1,
                     sizeof(float) * std::max(ctx->node_rows, ctx->edge_rows) * ctx->d));
  if (node_tab) HGX_TRY(download_unpadded(ctx, ctx->ntab.as<float>(), ctx->node_rows, node_tab));
  if (edge_tab) HGX_TRY(download_unpadded(ctx, ctx->etab.as<float>(), ctx->edge_rows, edge_tab));
  HGX_LAUNCH_CHECK(ctx);
  return HGX_OK;
}

__global__ void gather_rows(const float *__restrict__ src,
                            const int64_t *__restrict__ rows, float *dst,
                            int64_t n, int d, int dp) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n * d;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = i / d;
    dst[i] = src[rows[q] * dp + (int)(i % d)];
  }
}

extern "C" int hgx_model_get_rows(hgx_ctx *ctx, int table, int64_t n,
                                  const int64_t *rows, float *out) {
  if (!ctx) return HGX_EINVAL;
  HGX_CHECK(ctx, ctx->d > 0, HGX_ESTATE, "no model on device");
  HGX_CHECK(ctx, table == 0 || table == 1, HGX_EINVAL, "table must be 0 or 1");
  HGX_CHECK(ctx, n >= 0, HGX_EINVAL, "negative row count");
  if (n == 0) return HGX_OK;
  HGX_CHECK(ctx, rows && out, HGX_EINVAL, "null rows / out");
  const int64_t nr = table == 0 ? ctx->node_rows : ctx->edge_rows;
  for (int64_t q = 0; q < n; q++)
    HGX_CHECK(ctx, rows[q] >= 0 && rows[q] < nr, HGX_EINVAL,
              "row %lld outside the table (%lld rows)", (long long)rows[q],
              (long long)nr);
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  const int d = ctx->d;
  HGX_TRY(hgx_ensure(ctx, ctx->s2, sizeof(int64_t) * n));
  HGX_TRY(hgx_ensure(ctx, ctx->s1, sizeof(float) * n * d));
  HGX_HIP(ctx, hipMemcpyAsync(ctx->s2.p, rows, sizeof(int64_t) * n,
                              hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(gather_rows, dim3(grid_for(n * d, 256)), dim3(256), 0,
                     ctx->stream, (table == 0 ? ctx->ntab : ctx->etab).as<float>(),
                     ctx->s2.as<int64_t>(), ctx->s1.as<float>(), n, d, ctx->dp);
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipMemcpyAsync(out, ctx->s1.p, sizeof(float) * n * d,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

// ---------------------------------------------------------------------------
// fit
// ---------------------------------------------------------------------------
// The two streams of the overlapped chunk preparation (tuning
// train_prep_overlap): tstream[0] the batch steps, tstream[1] the
// preparation. With cus > 0 they get disjoint CU masks: the first `cus`
// CU-mask bits (rounded up to a multiple of 8) for the preparation, the rest
// for the steps (which use 64 workgroups per batch): a preparation workgroup
// never shares a CU with a batch step. Mask bit i is CU i / 8 of XCD i % 8
// (probed on MI355X, tools/cumask_probe.hip); a mask that leaves an XCD
// without CUs is ignored by the runtime (the whole device), so each side
// keeps CUs on every XCD.
static int train_streams(hgx_ctx *ctx, int cus) {
  if (ctx->tstream_cus == cus && ctx->tstream[0]) return HGX_OK;
  for (hipStream_t &s : ctx->tstream) {
    if (s) {
      HGX_HIP(ctx, hipStreamSynchronize(s));
      HGX_HIP(ctx, hipStreamDestroy(s));
      s = nullptr;
    }
  }
  ctx->tstream_cus = -1;
  if (cus <= 0) {
    for (hipStream_t &s : ctx->tstream)
      HGX_HIP(ctx, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  } else {
    int ncu = 0;
    HGX_HIP(ctx, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount,
                                       ctx->device));
    HGX_CHECK(ctx, cus <= ncu / 2, HGX_EINVAL, "train_prep_cus %d above half of %d CUs",
              cus, ncu);
    const int W = (ncu + 31) / 32;
    std::vector<uint32_t> ms(W, 0u), mp(W, 0u);
    const int np = (cus + 7) / 8 * 8;
    for (int i = 0; i < ncu; i++) (i < np ? mp : ms)[i / 32] |= 1u << (i % 32);
    HGX_HIP(ctx, hipExtStreamCreateWithCUMask(&ctx->tstream[0], W, ms.data()));
    HGX_HIP(ctx, hipExtStreamCreateWithCUMask(&ctx->tstream[1], W, mp.data()));
  }
  ctx->tstream_cus = cus;
  return HGX_OK;
}

// Argument checks, then the records' indices against the tables (the kernels
// do not bounds-check): one max_index round trip.
static int train_validate(hgx_ctx *ctx, int batch, int max_epochs, int loss, int act) {
  HGX_CHECK(ctx, ctx->d > 0, HGX_ESTATE, "hgx_model_init not called");
  HGX_CHECK(ctx, ctx->n_rec > 0, HGX_ESTATE, "no records on device");
  HGX_CHECK(ctx, batch >= 1, HGX_EINVAL, "batch_size must be >= 1");
  HGX_CHECK(ctx, max_epochs >= 0, HGX_EINVAL, "epochs must be >= 0");
  HGX_CHECK(ctx, loss == 0 || loss == 1, HGX_EINVAL, "loss must be 0 or 1");
  HGX_CHECK(ctx, act == 0 || act == 1, HGX_EINVAL, "act must be 0 or 1");
  HGX_CHECK(ctx, ctx->n_rec < (int64_t)INT32_MAX, HGX_EUNSUP, "more than 2^31 records");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  const int K = ctx->K, R = 4 + 2 * K;
  HGX_CHECK(ctx, (size_t)sort_slots(batch * R) * 8 <= 64 * 1024, HGX_EUNSUP,
            "batch_size*(4+2K)=%d exceeds the 8192-slot batch limit", batch * R);
  HGX_TRY(hgx_ensure(ctx, ctx->s0, 16));
  HGX_HIP(ctx, hipMemsetAsync(ctx->s0.p, 0, 16, ctx->stream));
  hipLaunchKernelGGL(max_index, dim3(grid_for(ctx->n_rec, 256)), dim3(256), 0, ctx->stream,
                     ctx->rec_idx.as<int>(), ctx->n_rec, R, K, ctx->s0.as<int>());
  HGX_LAUNCH_CHECK(ctx);
  int mx[4] = {0, 0, 0, 0};
  HGX_HIP(ctx, hipMemcpyAsync(mx, ctx->s0.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  HGX_CHECK(ctx, mx[2] == 0, HGX_EINVAL, "negative record index");
  HGX_CHECK(ctx, mx[0] < ctx->node_rows && mx[1] < ctx->edge_rows, HGX_EINVAL,
            "record index (node %d, edge %d) outside the tables (%lld, %lld)",
            mx[0], mx[1], (long long)ctx->node_rows, (long long)ctx->edge_rows);
  return HGX_OK;
}

// The launch plan of one hgx_train call: geometry, kernels and chunking. The
// layout's Dims are the part of it that sizes the scratch buffers.
struct TrainPlan : hgx_layout::Dims {
  int64_t n, nbatches, nchunks;
  int K, SB, P, L, VPL;
  float lr, eps;
  int loss, act;
  int tb1, tb2, grid2;  // K1 / K2 workgroup sizes, K2 workgroups
  KFn k1 = nullptr, k2 = nullptr;
  // deferred-row step (fused): eligible geometry and batch <= kPackB records (every
  // batch of the run then takes it); else the two-kernel step for every batch
  KStepFn kf[2] = {nullptr, nullptr};  // light / MULTI pending-slot forms
  KFlushFn kfl = nullptr;
  int tbf, lstride;              // the step's workgroup size; lossbuf words per batch
  bool ahead;                    // overlapped on one stream (train_prep_overlap == 2)
  size_t prep_smem, place_smem;  // dynamic LDS of train_prep / train_place
  int chunk_batches(int64_t c) const { return (int)std::min<int64_t>(CB, nbatches - c * CB); }
};

// the two-kernel step's geometry and kernels
static int plan_split(hgx_ctx *ctx, TrainPlan &p) {
  // K1 workgroup size: 8 records per workgroup measured best (d=128: 256
  // threads, 10.5 us/batch vs 11.0 at 128 / 12.8 at 64 / 10.9 at 512;
  // d=256: 512 threads, 13.6 vs 14.7 at 256). Specialised FOBE/HOBE
  // kernels only; HGX_TRAIN_TB1=256|512 overrides.
  p.tb1 = env_int("HGX_TRAIN_TB1", p.L >= 64 ? 512 : kTB);
  if (p.tb1 != 512) p.tb1 = kTB;
  if (!(p.K == 5 && p.loss == p.act) || env_int("HGX_TRAIN_GENERIC", 0) == 1) p.tb1 = kTB;
  // K2 workgroup size: 512 threads measured best (d=128: 10.2 vs 10.6
  // us/batch at 256 and 10.5 at 1024; d=256: 12.6 vs 13.5 / 12.7)
  p.tb2 = env_int("HGX_TRAIN_TB2", 512);
  if (p.tb2 != 512) p.tb2 = kTB;
  HGX_CHECK(ctx, pick_kernels(p.L, p.VPL, p.K, p.loss, p.act, p.tb1, p.tb2, p.k1, p.k2),
            HGX_EUNSUP, "no kernel for d=%d", ctx->d);
  p.RPB = p.tb1 / p.L;
  p.nblk1 = (p.batch + p.RPB - 1) / p.RPB;
  // one unique-row task per group, plus the two padding-row workgroups
  const int GPB2 = p.tb2 / p.L;
  p.grid2 = (p.SB + GPB2 - 1) / GPB2 + 2;
  return HGX_OK;
}

static int train_plan(hgx_ctx *ctx, int batch, float lr, float eps, int loss, int act,
                      TrainPlan &p) {
  p.n = ctx->n_rec;
  p.batch = batch, p.K = ctx->K, p.R = 4 + 2 * p.K, p.dp = ctx->dp, p.r0slots = kR0Slots;
  p.lr = lr, p.eps = eps, p.loss = loss, p.act = act;
  p.SB = batch * p.R;
  p.P = sort_slots(p.SB);
  geometry(ctx->d, p.L, p.VPL);
  HGX_TRY(plan_split(ctx, p));
  p.tbf = ctx->tune.train_tb;  // (0: per geometry)
  int SL = 0, rpbf = 0;        // lanes per record, records per workgroup
  p.fused = ctx->tune.train_fused && env_int("HGX_TRAIN_GENERIC", 0) != 1 && batch <= kPackB &&
            pick_step(p.L, p.VPL, p.K, loss, act, ctx->tune.train_lanes,
                      ctx->tune.train_wave_pair, SL, p.tbf, rpbf, p.kf, p.kfl);
  p.prpb = p.fused ? rpbf : 0;
  p.NBF = p.fused ? (batch + p.prpb - 1) / p.prpb : 0;
  p.RW = p.R + kWX;
  p.Mmax = p.SB / 2 + 1;  // deferred rows per batch: <= SB / 2
  p.MX = p.fused ? 2 + p.Mmax : 0;
  HGX_CHECK(ctx, p.MX <= (int)kDefMask + 1, HGX_EUNSUP, "batch too large for the step");
  // (early row-0 form: one loss word per record group, float2 rows)
  const bool r0e = HGX_TRAIN_R0EARLY && p.fused && ctx->dp == 2 * SL;
  p.lstride = std::max(p.nblk1, r0e ? p.NBF * p.prpb : p.NBF);
  p.nbatches = (p.n + batch - 1) / batch;
  // prep chunk: CB batches prepared by one launch, then trained
  p.CB = (int)std::min<int64_t>(1024, (p.nbatches + kChunkRound - 1) / kChunkRound * kChunkRound);
  p.nchunks = (p.nbatches + p.CB - 1) / p.CB;
  p.overlap = p.fused && ctx->tune.train_prep_overlap >= 1;
  p.ahead = p.overlap && ctx->tune.train_prep_overlap == 2;
  // train_prep's dynamic LDS: keys + run classes + record ids (radix path:
  // the ids and the 16-bit classes share one region)
  p.prep_smem = p.P == kSortP ? ((size_t)p.P * 8 + std::max<size_t>(kPrepB * 4, (size_t)p.SB * 2) + 15) / 16 * 16
                              : (size_t)p.P * 12 + kPrepB * 4;
  p.place_smem = sizeof(int) * ((size_t)p.Mmax + p.SB);
  return HGX_OK;
}

// Diagnostic hooks of a HGX_DEBUG_KNOBS build: the ablation bits (HGX_TRAIN_ABLATE)
// and the phase-trace buffer (HGX_TRAIN_TRACE=<file>), detached and freed on every exit.
struct TrainTrace {
  static constexpr int kBatches = 256;
  static constexpr size_t kBytes = sizeof(unsigned long long) * kBatches * 2 * 1024 * 8;
  const char *path = nullptr;
  void *p = nullptr;
  int begin(hgx_ctx *ctx) {
    path = hgx_debug_env_str("HGX_TRAIN_TRACE");
    if (path && path[0]) {
      HGX_HIP(ctx, hipMalloc(&p, kBytes));
      HGX_HIP(ctx, hipMemset(p, 0, kBytes));
    }
#ifdef HGX_DEBUG_KNOBS
    const int ab = env_int("HGX_TRAIN_ABLATE", 0), tn = p ? kBatches : 0;
    HGX_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_tab), &ab, sizeof(int)));
    HGX_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &p, sizeof(p)));
    HGX_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_trace_nb), &tn, sizeof(tn)));
#endif
    return HGX_OK;
  }
  void write_out() const {
    std::vector<unsigned long long> h(p ? kBytes / 8 : 0);
    if (!p || hipMemcpy(h.data(), p, kBytes, hipMemcpyDeviceToHost) != hipSuccess) return;
    if (FILE *f = fopen(path, "wb")) {
      fwrite(h.data(), 1, kBytes, f);
      fclose(f);
    }
  }
  ~TrainTrace() {
    if (!p) return;
#ifdef HGX_DEBUG_KNOBS
    unsigned long long *z = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &z, sizeof(z));
#endif
    (void)hipFree(p);
  }
};

// The epoch's record order in ctx->s1: the caller's `perms`, the identity for
// records loaded by hgx_store_load (trained in the order they were written: the
// store drew the epoch's global permutation), or the device shuffle (random
// keys, radix sort; scratch in ctx->s7).
struct EpochPerm {
  hgx_ctx *ctx;
  int64_t n;
  const int64_t *perms;
  bool in_order;
  int *perm = nullptr;
  size_t sort_tmp = 0, sort_off = 0;  // device shuffle only
  unsigned long long *keys_in = nullptr, *keys_out = nullptr;
  int *vals_in = nullptr;
  std::vector<int> hperm;

  EpochPerm(hgx_ctx *c, const int64_t *host_perms)
      : ctx(c), n(c->n_rec), perms(host_perms), in_order(!host_perms && c->rec_in_order) {}
  int init() {
    HGX_TRY(hgx_ensure(ctx, ctx->s1, sizeof(int) * (n + 1)));
    perm = ctx->s1.as<int>();
    if (perms || in_order) return HGX_OK;
    HGX_HIP(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_tmp, keys_in, keys_out,
                                                    vals_in, perm, (int)n));
    sort_off = (sizeof(unsigned long long) * 2 * n + sizeof(int) * n + 255) / 256 * 256;
    HGX_TRY(hgx_ensure(ctx, ctx->s7, sort_off + sort_tmp + 256));
    keys_in = ctx->s7.as<unsigned long long>();
    keys_out = keys_in + n;
    vals_in = reinterpret_cast<int *>(keys_out + n);
    return HGX_OK;
  }
  // queues epoch ep's order on ctx->stream
  int draw(int ep, uint64_t seed) {
    if (perms) return upload(perms + (int64_t)ep * n);
    if (in_order) {
      hipLaunchKernelGGL(iota_perm, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, n, perm);
      return HGX_OK;
    }
    hipLaunchKernelGGL(shuffle_keys, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, seed,
                       ep, n, keys_in, vals_in);
    size_t tmp = sort_tmp;
    if (hipcub::DeviceRadixSort::SortPairs(ctx->s7.as<char>() + sort_off, tmp, keys_in, keys_out,
                                           vals_in, perm, (int)n, 0, 64, ctx->stream) != hipSuccess)
      return hgx_fail(ctx, HGX_EHIP, "shuffle sort failed");
    return HGX_OK;
  }
  int upload(const int64_t *pe) {
    hperm.resize(n);
    for (int64_t i = 0; i < n; i++) {
      if (pe[i] < 0 || pe[i] >= n)
        return hgx_fail(ctx, HGX_EINVAL, "permutation entry out of range");
      hperm[i] = (int)pe[i];
    }
    if (hipMemcpyAsync(perm, hperm.data(), sizeof(int) * n, hipMemcpyHostToDevice,
                       ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
      return hgx_fail(ctx, HGX_EHIP, "permutation upload failed");
    return HGX_OK;
  }
};

// One hgx_train call in flight: buffers, streams, events and the counters;
// host resources released on every exit path. A form with one step kernel
// (merged: kf[0] == kf[1]) needs nothing from the device inside an epoch: the
// in-line schedule queues prepare(c + 1) directly behind chunk c's launches
// (stream order protects the placed set and the skey / sM parities), and a
// failure surfaces at the epoch's final synchronise, as a step's does. The
// other forms copy each chunk's MULTI flags into the context's pinned buffer
// and wait for them, one host wait per chunk.
struct TrainRun {
  hgx_ctx *ctx;
  const TrainPlan &p;
  // kernel arguments per placed set (one set unless the preparation is
  // overlapped); the deferred rows' keys and counts by chunk parity
  TrainArgs ap[2];
  int *skey[2] = {nullptr, nullptr}, *sM[2] = {nullptr, nullptr};
  double *dloss = nullptr, *dpart = nullptr;
  // the batch-step stream and the preparation stream: ctx->stream, or with the
  // two-stream overlapped preparation ctx->tstream (disjoint CU masks when
  // train_prep_cus > 0), ordered after everything queued on ctx->stream at the
  // epoch's start and joined back into it by join()
  hipStream_t sst, spr;
  // bev: one pair per prep chunk, device time of the batch kernels only; pev
  // (overlapped preparation, timing off): chunk c prepared (pev[c]), the
  // epoch's join with ctx->stream (pev[nchunks])
  std::vector<hipEvent_t> bev, pev;
  const bool merged;    // one step kernel: no MULTI flags on the host
  int *hbrk = nullptr;  // ctx->train_hbrk: the chunk's MULTI flags (train_place) per placed set
  hipError_t flags_err = hipSuccess;  // of the last copy into hbrk
  // nmulti: train_place's count of flagged batches (ovf[kOvfMulti]) as of the
  // last finished epoch
  int64_t nfused = 0, nsplit = 0, nmulti = 0;
  double batch_ms = 0.0;

  TrainRun(hgx_ctx *c, const TrainPlan &plan)
      : ctx(c), p(plan), sst(c->stream), spr(c->stream),
        merged(plan.fused && plan.kf[0] == plan.kf[1] && !HGX_TRAIN_CHUNKWAIT) {}
  ~TrainRun() {
    for (auto e : bev) if (e) (void)hipEventDestroy(e);
    for (auto e : pev) if (e) (void)hipEventDestroy(e);
  }
  // Sizes every scratch buffer of the call and carves s5 / s3 by the one
  // layout (hgx_train_layout.h); both start the call zeroed.
  int buffers(int *perm) {
    TrainArgs &a = ap[0];
    memset(&a, 0, sizeof(a));
    const size_t s3_bytes = hgx_layout::carve_step(p, {}, a);
    const size_t s5_bytes = hgx_layout::carve_chunk(p, {}, ap, skey, sM);
    HGX_TRY(hgx_ensure(ctx, ctx->s2, sizeof(float) * (size_t)p.SB * p.dp));  // gslot
    HGX_TRY(hgx_ensure(ctx, ctx->s3, s3_bytes));
    HGX_TRY(hgx_ensure(ctx, ctx->s4, sizeof(float) * (size_t)p.nbatches * p.lstride + 16));
    HGX_TRY(hgx_ensure(ctx, ctx->s5, s5_bytes));
    HGX_TRY(hgx_ensure(ctx, ctx->s6, 64 + sizeof(double) * kLossBlocks));  // loss
    HGX_HIP(ctx, hipMemsetAsync(ctx->s5.p, 0, s5_bytes, ctx->stream));
    HGX_HIP(ctx, hipMemsetAsync(ctx->s3.p, 0, s3_bytes, ctx->stream));
    a.idx = ctx->rec_idx.as<int>(), a.tgt = ctx->rec_tgt.as<float>(), a.perm = perm;
    a.n = p.n, a.B = p.batch, a.R = p.R, a.K = p.K, a.dp = p.dp;
    a.ntab = ctx->ntab.as<float>(), a.etab = ctx->etab.as<float>();
    a.nacc = ctx->nacc.as<float>(), a.eacc = ctx->eacc.as<float>();
    a.gslot = ctx->s2.as<float>(), a.lossbuf = ctx->s4.as<float>();
    a.lr = p.lr, a.eps = p.eps, a.loss = p.loss, a.act = p.act;
    a.SB = p.SB, a.nblk1 = p.nblk1, a.lstride = p.lstride;
    a.fused = p.fused ? 1 : 0, a.prpb = p.prpb, a.RW = p.RW, a.MX = p.MX, a.Mmax = p.Mmax;
    hgx_layout::carve_step(p, {ctx->s3.as<char>()}, a);
    hgx_layout::carve_chunk(p, {ctx->s5.as<char>()}, ap, skey, sM);
    dloss = reinterpret_cast<double *>(ctx->s6.as<char>() + 32);
    dpart = reinterpret_cast<double *>(ctx->s6.as<char>() + 64);
    return HGX_OK;
  }
  int init(int *perm) {
    HGX_TRY(buffers(perm));
    if (p.fused && !merged) {
      const size_t need = (size_t)p.CB * (p.overlap ? 2 : 1);
      if (ctx->train_hbrk_n < need) {
        if (ctx->train_hbrk) (void)hipHostFree(ctx->train_hbrk);
        ctx->train_hbrk = nullptr, ctx->train_hbrk_n = 0;
        HGX_HIP(ctx, hipHostMalloc(reinterpret_cast<void **>(&ctx->train_hbrk),
                                   sizeof(int) * need));
        ctx->train_hbrk_n = need;
      }
      hbrk = ctx->train_hbrk;
    }
    if (p.overlap && !p.ahead) {
      HGX_TRY(train_streams(ctx, ctx->tune.train_prep_cus));
      sst = ctx->tstream[0];
      spr = ctx->tstream[1];
    }
    bev.assign(2 * p.nchunks, nullptr);
    pev.assign(p.overlap ? p.nchunks + 1 : 0, nullptr);
    for (auto &e : bev) HGX_HIP(ctx, hipEventCreate(&e));
    for (auto &e : pev) HGX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return HGX_OK;
  }
  int set_of(int64_t c) const { return p.overlap ? (int)(c & 1) : 0; }  // chunk c's placed set

  void begin_epoch() {
    (void)hipMemsetAsync(dloss, 0, sizeof(double), ctx->stream);
    (void)hipMemsetAsync(ap[0].lossbuf, 0, sizeof(float) * (size_t)p.nbatches * p.lstride,
                         ctx->stream);
    // row-0 slots start at zero every epoch (then each batch zeroes the set
    // the next one adds into)
    if (p.fused) (void)hipMemsetAsync(ap[0].r0acc, 0, hgx_layout::r0acc_bytes(p), ctx->stream);
    if (p.overlap && !p.ahead) {
      (void)hipEventRecord(pev[p.nchunks], ctx->stream);
      (void)hipStreamWaitEvent(sst, pev[p.nchunks], 0);
      (void)hipStreamWaitEvent(spr, pev[p.nchunks], 0);
    }
  }
  // Preparation of chunk c on spr. In line it runs right before the chunk's
  // batches (the records it writes are still in the Infinity Cache when they
  // are read). With the step it also places the chunk into set_of(c) and,
  // for a form with a light kernel, copies the chunk's MULTI flags to the host.
  void prepare(int64_t c) {
    const int nbc = p.chunk_batches(c), cp = (int)(c & 1), set = set_of(c);
    hipLaunchKernelGGL(train_prep, dim3(p.CB), dim3(kTB), p.prep_smem, spr, ap[0], c * p.CB, nbc,
                       p.P, skey[cp], sM[cp]);
    if (!p.fused) return;
    hipLaunchKernelGGL(train_place, dim3(p.CB), dim3(kTB), p.place_smem, spr, ap[set], nbc, p.CB,
                       skey[cp], sM[cp], skey[cp ^ 1], sM[cp ^ 1], c > 0 ? 1 : 0);
    if (!merged)
      flags_err = hipMemcpyAsync(hbrk + (size_t)set * p.CB, ap[set].pbrk, sizeof(int) * nbc,
                                 hipMemcpyDeviceToHost, spr);
    if (p.overlap) (void)hipEventRecord(pev[c], spr);
  }
  // Until chunk c's MULTI flags are on the host (a step with a light kernel;
  // in line: one host wait per chunk of 1024 batches) and, on two streams,
  // chunk c's steps ordered after its preparation. The two-kernel step and,
  // in line, a merged step need neither.
  int wait_prepared(int64_t c) {
    hipError_t e = hipSuccess;
    if (p.overlap) {
      e = hipEventSynchronize(pev[c]);
      if (e == hipSuccess && !p.ahead) (void)hipStreamWaitEvent(sst, pev[c], 0);
    } else if (p.fused && !merged) {
      e = flags_err != hipSuccess ? flags_err : hipStreamSynchronize(spr);
    }
    if (e == hipSuccess) return HGX_OK;
    return hgx_fail(ctx, HGX_EHIP, "batch preparation failed: %s",
                    hipGetErrorString(hipGetLastError()));
  }
  // Chunk c's batches on sst, direct launches (measured as fast as hipGraph
  // replay of the same kernels, 10.6 us per batch both ways at d=128, with
  // less host time). The step: one launch per batch, q = the batch's index in
  // the epoch.
  void run_steps(int64_t c) {
    const int nbc = p.chunk_batches(c), set = set_of(c);
    for (int bi = 0; bi < nbc; bi++) {
      if (!p.fused) {
        hipLaunchKernelGGL(p.k1, dim3(p.nblk1), dim3(p.tb1), 0, sst, ap[0], bi);
        hipLaunchKernelGGL(p.k2, dim3(p.grid2), dim3(p.tb2), 0, sst, ap[0], bi);
        continue;
      }
      const int64_t gbat = c * p.CB + bi;
      const int nrec = (int)std::min<int64_t>(p.batch, p.n - gbat * p.batch);
      const int multi = merged || (hbrk[(size_t)set * p.CB + bi] && gbat > 0);
#if HGX_TRAIN_PRELOAD
      // the batch's record words in the placed set, and 1 / records (the
      // division the step did on every wave)
      const TrainArgs &as = ap[set];
      const size_t g0 = (size_t)bi * p.NBF * p.prpb;
      hipLaunchKernelGGL(p.kf[multi], dim3(p.NBF), dim3(p.tbf), 0, sst, as.pidx + g0 * p.RW,
                         as.pcode + g0 * p.RW, as.ptgt + g0 * 3, p.RW, nrec, (int)gbat,
                         1.0f / (float)nrec, (int)gbat, bi, as);
#else
      hipLaunchKernelGGL(p.kf[multi], dim3(p.NBF), dim3(p.tbf), 0, sst, ap[set], bi, (int)gbat,
                         nrec, (int)gbat);
#endif
    }
    (p.fused ? nfused : nsplit) += nbc;
  }
  // One epoch's chunks. Overlapped, chunk c + 1 is prepared on spr while
  // chunk c trains on sst; placed set c & 1 is rewritten (chunk c + 2) only
  // after chunk c's steps are done.
  int run_chunks() {
    if (p.overlap) prepare(0);
    for (int64_t c = 0; c < p.nchunks; c++) {
      if (!p.overlap) prepare(c);
      // one stream: chunk c + 1's preparation queued ahead of chunk c's
      // batches (stream order protects placed set (c + 1) & 1, last read
      // by chunk c - 1's batches, queued before it)
      if (p.ahead && c + 1 < p.nchunks) prepare(c + 1);
      HGX_TRY(wait_prepared(c));
      (void)hipEventRecord(bev[2 * c], sst);
      run_steps(c);
      (void)hipEventRecord(bev[2 * c + 1], sst);
      // Two streams: the host enqueues chunk c + 1's preparation only once
      // chunk c - 1's steps are done (it waits for them after queueing chunk
      // c's; placed set (c + 1) & 1 is free then), so the preparation stream
      // never holds a barrier packet blocked on the step stream.
      if (p.overlap && !p.ahead && c + 1 < p.nchunks) {
        if (c >= 1 && hipEventSynchronize(bev[2 * (c - 1) + 1]) != hipSuccess)
          return hgx_fail(ctx, HGX_EHIP, "batch step failed: %s",
                          hipGetErrorString(hipGetLastError()));
        prepare(c + 1);
      }
    }
    return HGX_OK;
  }
  // the last batch's deferred rows -> tables; gacc clean for the next
  // epoch (the last batch's entries and the one before it)
  void flush() const {
    const int cp = (int)((p.nchunks - 1) & 1), last_nbc = p.chunk_batches(p.nchunks - 1);
    const int *ml = sM[cp] + (last_nbc - 1);
    const int *mp = last_nbc >= 2 ? sM[cp] + (last_nbc - 2)
                                  : (p.nchunks >= 2 ? sM[cp ^ 1] + (p.CB - 1) : nullptr);
    const int nlast = (int)(p.n - (p.nbatches - 1) * p.batch);
    hipLaunchKernelGGL(p.kfl, dim3(64), dim3(256), 0, sst, ap[0],
                       skey[cp] + (size_t)(last_nbc - 1) * p.Mmax, ml, mp,
                       (int)(p.nbatches - 1), std::min(p.NBF, nlast));
  }
  // The epoch's tail: flush, the loss sum (lsum) and the overflow verdict
  // read back, the chunks' batch-kernel times added to batch_ms.
  int finish_epoch(double &lsum) {
    if (p.fused) flush();
    hipLaunchKernelGGL(loss_partial, dim3(kLossBlocks), dim3(kTB), 0, sst, ap[0].lossbuf,
                       p.nbatches * p.lstride, dpart);
    hipLaunchKernelGGL(loss_final, dim3(1), dim3(kLossBlocks), 0, sst, dpart, dloss);
    int fl[2] = {0, 0};  // ovf[0], ovf[kOvfMulti]
    static_assert(kOvfMulti == 1, "read with the range flag");
    if (hipMemcpyAsync(&lsum, dloss, sizeof(double), hipMemcpyDeviceToHost, sst) != hipSuccess ||
        (p.fused && hipMemcpyAsync(fl, ap[0].ovf, sizeof(fl), hipMemcpyDeviceToHost, sst) !=
                        hipSuccess) ||
        hipStreamSynchronize(sst) != hipSuccess)
      return hgx_fail(ctx, HGX_EHIP, "epoch failed: %s", hipGetErrorString(hipGetLastError()));
    nmulti = fl[1];
    if (fl[0])
      return hgx_fail(ctx, HGX_ENUMERIC,
                      "a gradient left the step's fixed-point range (|g| >= %g after "
                      "the 1/batch factor, or NaN): training diverged",
                      (double)kFixLimit);
    for (int64_t c = 0; c < p.nchunks; c++) {
      float m = 0.f;
      if (hipEventElapsedTime(&m, bev[2 * c], bev[2 * c + 1]) == hipSuccess) batch_ms += m;
    }
    return HGX_OK;
  }
  // Nothing of this call is left running on the side streams (every exit
  // path of the epoch loop); returns the wall time since ev0 in ms.
  float join() {
    if (p.overlap) {
      (void)hipStreamSynchronize(spr);
      (void)hipStreamSynchronize(sst);
    }
    float ms = 0.f;
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    (void)hipEventSynchronize(ctx->ev1);
    (void)hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1);
    return ms;
  }
  void stats(int epochs, float ms) const {
    ctx->train_ms = batch_ms;
    ctx->train_epoch_ms = ms;
    ctx->train_records = (int64_t)epochs * p.n;
    ctx->train_batches = (int64_t)epochs * p.nbatches;
    ctx->train_fused = nfused;
    ctx->train_split = nsplit;
    ctx->train_multi = nmulti;
    ctx->train_step_tb = p.fused ? p.tbf : 0;
    ctx->train_step_rpb = p.prpb;
  }
};

extern "C" int hgx_train(hgx_ctx *ctx, int batch, int max_epochs, float lr, float eps, int loss,
                         int act, float min_delta, uint64_t shuffle_seed, const int64_t *perms,
                         float *epoch_loss, int *epochs_run) {
  if (!ctx) return HGX_EINVAL;
  HGX_TRY(train_validate(ctx, batch, max_epochs, loss, act));
  TrainPlan p;
  HGX_TRY(train_plan(ctx, batch, lr, eps, loss, act, p));
  TrainTrace trace;
  HGX_TRY(trace.begin(ctx));
  EpochPerm order(ctx, perms);
  HGX_TRY(order.init());
  TrainRun run(ctx, p);
  HGX_TRY(run.init(order.perm));
  double best = INFINITY;
  int ep = 0, rc = HGX_OK;
  HGX_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (ep = 0; ep < max_epochs; ep++) {
    double lsum = 0.0;
    if ((rc = order.draw(ep, shuffle_seed)) != HGX_OK) break;
    run.begin_epoch();
    if ((rc = run.run_chunks()) != HGX_OK || (rc = run.finish_epoch(lsum)) != HGX_OK) break;
    const double cur = lsum / (double)p.n;
    ctx->train_loss_sum = lsum;
    if (epoch_loss) epoch_loss[ep] = (float)cur;
    if (cur < best - (double)min_delta) {
      best = cur;
    } else {
      ep++;
      break;
    }
  }
  const float ms = run.join();
  if (rc) return rc;
  trace.write_out();
  HGX_LAUNCH_CHECK(ctx);
  run.stats(ep, ms);
  if (epochs_run) *epochs_run = ep;
  return HGX_OK;
}


extern "C" int hgx_train_last_stats(hgx_ctx *ctx, double *ms, int64_t *records,
                                    int64_t *batches) {
  if (!ctx) return HGX_EINVAL;
  if (ms) *ms = ctx->train_ms;
  if (records) *records = ctx->train_records;
  if (batches) *batches = ctx->train_batches;
  return HGX_OK;
}

extern "C" int hgx_train_last_loss(hgx_ctx *ctx, double *loss_sum) {
  if (!ctx) return HGX_EINVAL;
  if (loss_sum) *loss_sum = ctx->train_loss_sum;
  return HGX_OK;
}

extern "C" int hgx_train_multi_pending(hgx_ctx *ctx, int64_t *batches) {
  if (!ctx) return HGX_EINVAL;
  if (batches) *batches = ctx->train_multi;
  return HGX_OK;
}

extern "C" int hgx_train_step_geometry(hgx_ctx *ctx, int *threads, int *records) {
  if (!ctx) return HGX_EINVAL;
  if (threads) *threads = ctx->train_step_tb;
  if (records) *records = ctx->train_step_rpb;
  return HGX_OK;
}

extern "C" int hgx_train_path_stats(hgx_ctx *ctx, int64_t *fused_batches,
                                    int64_t *split_batches) {
  if (!ctx) return HGX_EINVAL;
  if (fused_batches) *fused_batches = ctx->train_fused;
  if (split_batches) *split_batches = ctx->train_split;
  return HGX_OK;
}
