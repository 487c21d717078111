/*
 * hgx.h -- C ABI of libhgx.so, the MI355X (gfx950) FOBE/HOBE hot path.
 *
 * Plain pointers and sizes only. The caller owns every host buffer; the
 * library owns all device memory, one HIP stream per context (a context is
 * thread-compatible: use one per thread) and no global state.
 *
 * Every call returns 0 on success or a negative HGX_E* code; the message is
 * in hgx_last_error(ctx). The Python host package (hypergraphembedding_amd,
 * _hgx._raise) maps
 *   HGX_EINVAL   -> AssertionError (the reference's precondition style,
 *                   e.g. embedding.py:83-85, hg2v_sample.py:646-647)
 *   HGX_EZERODIV -> ZeroDivisionError (algebraic_distance.py:49 on an
 *                   isolated row)
 *   HGX_EVALUE   -> ValueError (np.random.choice on an empty row,
 *                   hg2v_sample.py:49-51)
 *   HGX_ENUMERIC -> FloatingPointError (trainer fixed-point range left)
 *   the rest (EHIP, ENOMEM, ESTATE, EUNSUP) -> RuntimeError.
 *
 * Each entry point names the reference interface it replaces
 * (JSybrandt/HypergraphEmbedding, hypergraph_embedding/<file>:<line>).
 */
#ifndef HGX_H_
#define HGX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HGX_OK 0
#define HGX_EINVAL -1    /* precondition violated (AssertionError)          */
#define HGX_EHIP -2      /* HIP / RCCL runtime error                        */
#define HGX_ENOMEM -3    /* device allocation failed                        */
#define HGX_EZERODIV -4  /* isolated node/edge in algebraic distance        */
#define HGX_ESTATE -5    /* call out of order (e.g. no incidence uploaded)  */
#define HGX_EUNSUP -6    /* shape outside what this build supports          */
#define HGX_EVALUE -7    /* ValueError in the reference (np.random.choice on
                            an empty row, hg2v_sample.py:49-51)             */
#define HGX_ENUMERIC -8  /* trainer: a gradient left the batch step's fixed-
                            point range (diverged run, NaN)                 */

#define HGX_LOSS_KLD 0   /* BooleanModel: kullback_leibler_divergence       */
#define HGX_LOSS_MSE 1   /* UnweightedFloatModel: mean_squared_error        */
#define HGX_ACT_SIGMOID 0
#define HGX_ACT_RELU 1

typedef struct hgx_ctx hgx_ctx;

/* ---- context ---------------------------------------------------------- */
int hgx_create(int device, hgx_ctx **out);
int hgx_destroy(hgx_ctx *ctx);
const char *hgx_last_error(const hgx_ctx *ctx);
int hgx_version(void);
/* Run on an external stream (e.g. torch.cuda.current_stream()); NULL =
 * the context's own stream. */
int hgx_set_stream(hgx_ctx *ctx, void *hip_stream);
int hgx_synchronize(hgx_ctx *ctx);
/* HIP devices visible to this library (no context needed), and the free /
 * total device memory of a context's device (hipMemGetInfo). */
int hgx_device_count(int *n);
int hgx_mem_info(hgx_ctx *ctx, int64_t *free_bytes, int64_t *total_bytes);
/* Implementation choices of this context (none changes a result's math or
 * distribution; not a reference interface). key:
 *   "sample_reject_w"  2/3-hop sample rows with more expansion paths are
 *                      sampled by rejection (default 32768; 0 = expand all)
 *   "sample_mode3"     3-hop rejection proposal: 0 auto, 1 paths
 *                      (Karp-Luby), 2 uniform columns
 *   "sample_mode3_shift" auto rule for node rows: uniform columns when a
 *                      row's path count >= columns x 2^shift (default 1,
 *                      -10..10); "sample_mode3_shift_e" the same for edge
 *                      rows (default 1)
 *   "train_fused"      1 fused one-launch batch step (default), 0 the
 *                      two-kernel step for every batch
 *   "train_lanes"      fused step at padded d = 128: lanes per record
 *                      (0 auto = 64, 32 = float4 per lane, 64 = float2)
 *   "train_tb"         fused step workgroup size (0 auto, 128, 256, 512;
 *                      a size the geometry has no form for -> its default)
 *   "train_wave_pair"  fused step at 64 lanes per record (padded d = 128 or
 *                      256): 1 one record on two waves of a 512-thread
 *                      workgroup (the node wave owns the node-table slots,
 *                      the edge wave the edge-table slots; still 4 records
 *                      per workgroup; overrides train_tb), 3 one record on
 *                      four waves (each table half on a head and a list
 *                      wave), 2 records per 512-thread workgroup (padded
 *                      d = 128; at 256 the same as 1), 4 the same four
 *                      waves, 1 record per 256-thread workgroup (padded
 *                      d = 128; at 256 the same as 1), 0 one wave per
 *                      record, -1 per geometry where train_tb is 0
 *                      (default); bit-identical
 *   "alg_long"         alg-dist long-row threshold (0 = 512, else >= 64)
 *   "alg_ks"           alg-dist coordinate row width in floats (0 = auto:
 *                      round_up(k + 1, 4), widened from 12 to 16 floats
 *                      when the node + edge rows exceed 256 MiB)
 *   "alg_push"         alg-dist edge half: 0 gather (default), 1 push form
 *                      (the node half writes per-incidence contributions in
 *                      edge-major order, the edge half streams them; single
 *                      GPU, k <= 15; measured slower, kept for the record)
 *   "mlp_fuse_head"    combiner MLP training: 1 the label head computed in
 *                      the launch forming the joint layers' deltas (default,
 *                      bit-identical), 0 its own launch
 *   "mlp_prefetch"     combiner MLP training: 1 batch b + 1's dropped-out
 *                      input rows gathered by extra workgroups of batch b's
 *                      hidden-layer launch (default, bit-identical), 2 of its
 *                      joint-layer launch (measured 0.4% slower), 0 the
 *                      first layer and its weight gradient gather them
 *   "mlp_wgrad_split"  combiner MLP training: 0 every weight gradient in one
 *                      launch (default), 1 two launches (the layers after the
 *                      pre layers, then the pre layers; measured slower)
 *   "svc_lds_m"        batched SVC: largest problem (samples) solved with its
 *                      kernel matrix in LDS, 128 (default, two workgroups per
 *                      CU), 192 (one per CU) or 64 (only the one-wave
 *                      solvers keep one); larger ones recompute two kernel
 *                      columns per iteration (bit-identical results)
 *   "train_prep_overlap" trainer: 1 prepare chunk c + 1 (train_prep /
 *                      train_place) on a second stream while chunk c trains,
 *                      0 in line before each chunk (default); the same
 *                      batches, bit for bit
 *   "train_prep_cus"   with train_prep_overlap: CUs reserved for the
 *                      preparation stream by disjoint CU masks (0 = no masks)
 *   "ae_chunk_rows"    auto-encoder: rows of one chunk of a batch's logit
 *                      block, rounded up to a multiple of 32 (0 = sized from
 *                      the free device memory, default; at most 65536)
 *   "n2v_expand_w"     node2vec clique walks: a row with at most this many
 *                      paths draws its distinct neighbour by expansion, a
 *                      longer one by rejection (default 256; 0 = always
 *                      rejection; the same distribution)
 *   "n2v_chunk_walks"  node2vec concurrent trainer: walks per launch (0 =
 *                      about a quarter of the vertex count, in [64, 4096],
 *                      default; at most 65536)
 *   "dw_hot_levels"    DeepWalk concurrent trainer: the inner nodes at the
 *                      first T positions of a path (T tree levels from the
 *                      root, at most 2^T - 1 rows) are summed per workgroup in
 *                      LDS and added to memory once per workgroup; 0 to 6
 *                      (default 6, measured fastest at every row width), 0 =
 *                      every update is a global atomic
 *   "line_chunk_samples" LINE concurrent trainer: samples per launch, 64 to a
 *                      wave (0 = a quarter of the vertex count rounded down to
 *                      a multiple of 256, in [256, 65536], default; at most
 *                      2^20)
 *   "mp_chunk_walks"   metapath2vec: walks per chunk of the streamed corpus
 *                      (one walk-kernel launch, then one histogram or trainer
 *                      launch), rounded up to a multiple of 4 (0 =
 *                      "n2v_chunk_walks"' rule, and 64 for the sequential
 *                      trainer, default; at most 65536). The sequential
 *                      result does not depend on it
 * Unknown keys and out-of-range values -> HGX_EINVAL. */
int hgx_set_tuning(hgx_ctx *ctx, const char *key, int64_t value);

/* ---- incidence --------------------------------------------------------- *
 * Replaces ToCsrMatrix / ToEdgeCsrMatrix(CompressRange(hg))
 * (hypergraph_util.py:96-135, 223-244): the compressed N x E incidence in
 * both orientations, int32 CSR with sorted columns. */
int hgx_upload_incidence(hgx_ctx *ctx, int32_t N, int32_t E, int64_t nnz,
                         const int32_t *rowptr_n, const int32_t *col_n,
                         const int32_t *rowptr_e, const int32_t *col_e);

/* ---- algebraic distance ----------------------------------------------- *
 * Replaces EmbedAlgebraicDistance's relaxation loop
 * (algebraic_distance.py:126-175, helpers 34-123): per iteration the node
 * half, then the edge half on the NEW node coords, then the joint per-dim
 * min-max rescale to [0,1]. Coordinates are fp32 on device.
 *   hgx_alg_dist: upload node_xy (N x k) / edge_xy (E x k), run `iters`
 *   iterations, download the rescaled result into the same buffers.
 * The split calls keep the coords resident for benchmarking / HOBE:
 *   hgx_alg_set -> hgx_alg_run (repeatable) -> hgx_alg_get. */
int hgx_alg_dist(hgx_ctx *ctx, int k, int iters, float *node_xy,
                 float *edge_xy);
int hgx_alg_set(hgx_ctx *ctx, int k, const float *node_xy,
                const float *edge_xy);
int hgx_alg_run(hgx_ctx *ctx, int iters);
int hgx_alg_get(hgx_ctx *ctx, float *node_xy, float *edge_xy);
/* Device time (ms) of the last hgx_alg_run and its algorithmic bytes
 * (8*nnz + (8+12k)*(N+E) per iteration). */
int hgx_alg_last_stats(hgx_ctx *ctx, double *ms, double *bytes);

/* Multi-GPU, node-row sharded. Rank g owns node rows
 * [row0,row1); every rank holds all edge coords. The CALLER owns the two
 * exchange buffers (device memory, e.g. torch tensors) and runs the
 * collectives (torch.distributed "nccl" = RCCL over xGMI) between calls:
 *   begin(row0,row1, partial[E*KS] f32, mm[iters*M] i32, iters, &KS)
 *   for it: node(it); edge_partial(it); all_reduce(partial, SUM);
 *           edge_final(it); all_reduce(mm[it*M : (it+1)*M], MAX)
 *   end()   -> own node rows + all edge rows rescaled on device
 * with M = 2 * KS * HGX_MM_REPLICAS. min/max words are order-preserving
 * int32 (max slot f(x), min slot ~f(x)), so MAX is the only reduction. */
#define HGX_MM_REPLICAS 64
int hgx_alg_shard_begin(hgx_ctx *ctx, int32_t row0, int32_t row1,
                        void *d_partial, void *d_mm, int iters, int *ks_out);
int hgx_alg_shard_node(hgx_ctx *ctx, int it);
int hgx_alg_shard_edge_partial(hgx_ctx *ctx, int it);
int hgx_alg_shard_edge_final(hgx_ctx *ctx, int it);
int hgx_alg_shard_end(hgx_ctx *ctx);
/* Compact exchange (optional, after begin): only edges whose incidences sit
 * on two or more ranks go on the wire, as rows of k + 1 floats
 * [sum w, sum w x_1..k] (no padding slot). edge_slot[E] (host): wire row of
 * a shared edge (0..n_shared-1, the same on every rank), -1 an edge private
 * to this rank, -2 another rank's private edge (left unset here). The caller
 * then all-reduces d_wire (n_shared * (k + 1) floats, SUM) in place of
 * d_partial, which becomes this rank's local scratch. */
int hgx_alg_shard_wire(hgx_ctx *ctx, void *d_wire, int64_t n_shared,
                       const int32_t *edge_slot);
/* Exchange pipelining (optional, after begin / wire): split the edge rows
 * into n (1..16) contiguous ranges balanced by the incidences of the whole
 * graph, so every rank gets the same split; bounds[n + 1] receives the range
 * starts. Then per iteration
 * edge_partial_range(it, r) for r = 0..n-1 in place of edge_partial(it): the
 * caller may all-reduce range r's rows (of d_partial, or its wire rows) while
 * range r + 1 is computed, and calls edge_final(it) after all of them. The
 * reference has one monolithic pass (algebraic_distance.py:77-95). */
int hgx_alg_shard_ranges(hgx_ctx *ctx, int n, int32_t *bounds);
int hgx_alg_shard_edge_partial_range(hgx_ctx *ctx, int it, int r);

/* ---- HOBE probabilities ------------------------------------------------ *
 * _same_type_dist_calc (hg2v_sample.py:527-543) and DiffTypeDistanceSample
 * (:588-629) on the device-resident alg coords (after hgx_alg_run or
 * hgx_alg_set; values are used exactly as given, i.e. already rescaled).
 * kind: 0 node-node, 1 edge-edge, 2 node-edge. Bit-exact with numpy's
 * float32 norm at every k (double-accumulated float products below k = 32,
 * the blocked sdot kernel of csrc/hgx_norm32.h from there on). */
int hgx_hobe_probs(hgx_ctx *ctx, int kind, int64_t n, const int32_t *a,
                   const int32_t *b, float *out);

/* Per-incidence weights (hg2v_weighting.py): which = 0 UniformWeight
 * (195-198), 1 WeightByNeighborhood(alpha) (137-167), 2 HOBE distance weight
 * (hg2v_sample.py:540-541). Output is node-major (nnz, CSR order of col_n)
 * and edge-major (nnz, CSR order of col_e); either may be NULL. */
int hgx_incidence_weights(hgx_ctx *ctx, int which, double alpha,
                          float *node_major, float *edge_major);

/* ---- samplers ----------------------------------------------------------- *
 * Record layout = SamplesToModelInput(records, K, weighted=False)
 * (hg2v_sample.py:751-797): int32 [ln, le, rn, re, nn_0..K-1, ne_0..K-1]
 * (ids +1, 0 = absent) and float32 [nn_prob, ee_prob, ne_prob].
 * Records stay on the device for hgx_train; hgx_records_get copies out.
 *
 * BooleanSamples (hg2v_sample.py:125-242). Quotas are the reference's
 * int(weight * num_samples) (:138-146); the negative quotas may be NULL
 * (neg_samples == 0). Uniform draws come from a counter-based generator
 * keyed by `seed` (distribution-identical to the reference, not the same
 * stream). */
int hgx_sample_fobe(hgx_ctx *ctx, uint64_t seed, int K,
                    const int32_t *node_quota, const int32_t *edge_quota,
                    const int32_t *neg_node_quota,
                    const int32_t *neg_edge_quota, int64_t *n_records);
/* AlgebraicDistanceSamples (hg2v_sample.py:632-717) on the device alg
 * coords: quota S for every row, nn/ee/ne probabilities as above. */
int hgx_sample_hobe(hgx_ctx *ctx, uint64_t seed, int K, int S,
                    int64_t *n_records);
/* The same on a subset of rows: quota per node row / edge row instead of S
 * (both NULL -> S everywhere, i.e. hgx_sample_hobe). Used to sample the
 * rows one rank owns and for bounded slices of large graphs. */
int hgx_sample_hobe_rows(hgx_ctx *ctx, uint64_t seed, int K,
                         const int32_t *node_quota, const int32_t *edge_quota,
                         int S, int64_t *n_records);
/* The reference's record stream bit for bit (rng="mt19937"): the same
 * samplers drawing from numpy's global legacy RandomState, whose MT19937
 * state (np.random.get_state(): 624 key words and the position) is passed
 * in and updated in place to the state the reference leaves behind.
 * hgx_sample_fobe_mt replaces BooleanSamples (hg2v_sample.py:125-242, the
 * quotas as for hgx_sample_fobe); hgx_sample_hobe_mt replaces
 * AlgebraicDistanceSamples(run_in_parallel=False) (:632-717): its
 * neighbour draws come from the worker's copy of the stream (:604-605), so
 * the returned state is the parent's after its last pair draw. The host
 * walks the stream (the bounded draws' accepted values, in order); the
 * device orders the pattern rows (scipy's SMMP column order), runs every
 * row's Fisher-Yates and writes the records (csrc/hgx_mt.hip). Such a
 * stream is not keyed, so hgx_store_append refuses it. */
int hgx_sample_fobe_mt(hgx_ctx *ctx, uint32_t *mt_key, int32_t *mt_pos, int K,
                       const int32_t *node_quota, const int32_t *edge_quota,
                       const int32_t *neg_node_quota,
                       const int32_t *neg_edge_quota, int64_t *n_records);
int hgx_sample_hobe_mt(hgx_ctx *ctx, uint32_t *mt_key, int32_t *mt_pos, int K,
                       int S, int64_t *n_records);
/* WeightedJaccardSamples(run_in_parallel=False) (hg2v_sample.py:395-510)
 * drawing numpy's stream, the per-row quotas int(weight * S) as for
 * hgx_sample_jaccard (declared below) and its probabilities. */
int hgx_sample_jaccard_mt(hgx_ctx *ctx, uint32_t *mt_key, int32_t *mt_pos, int K,
                          const int32_t *node_quota, const int32_t *edge_quota,
                          int64_t *n_records);
/* ---- weighted-Jaccard samples (HG2V_ADJ_JAC / HG2V_NEIGH_JAC) --------- *
 * Replaces WeightedJaccardSamples (hg2v_sample.py:395-510) with
 * SparseWeightedJaccard (:250-273) and GetAllCentroids (:276-326).
 * Features: node2features / edge2features values on A's pattern (A's CSR
 * order, A^T's CSR order), e.g. UniformWeight / WeightByNeighborhood
 * (hg2v_weighting.py:137-198). Quotas are per row, int(weight * S). */
int hgx_features_set(hgx_ctx *ctx, const float *node_major,
                     const float *edge_major);
int hgx_sample_jaccard(hgx_ctx *ctx, uint64_t seed, int K,
                       const int32_t *node_quota, const int32_t *edge_quota,
                       int64_t *n_records);
/* kind 0 node-node, 1 edge-edge (SameTypeJaccardSample, :329-341), 2
 * node-edge (DiffTypeJaccardSample, :343-392) for pairs (a[i], b[i]). */
int hgx_jaccard_probs(hgx_ctx *ctx, int kind, int64_t n, const int32_t *a,
                      const int32_t *b, float *out);
/* The centroid CSR (which 0: node rows over nodes, 1: edge rows over
 * edges); any output may be NULL (sizes first). */
int hgx_jaccard_centroids(hgx_ctx *ctx, int which, int64_t *nnz,
                          int64_t *rowptr, int32_t *col, float *val);
/* Of the last hgx_sample_* call: 2-hop rows sampled from the union by
 * rejection (rows whose expansion exceeds the sample_reject_w tuning,
 * default 32768) and rows that fell back to expansion. */
int hgx_sample_last_stats(hgx_ctx *ctx, int64_t *union_rows,
                          int64_t *fallback_rows);
/* Of the last hgx_sample_* call: 3-hop rows sampled by uniform-column
 * rejection (a subset of union_rows). */
int hgx_sample_uniform_rows(hgx_ctx *ctx, int64_t *rows);
int hgx_records_set(hgx_ctx *ctx, int64_t n, int K, const int32_t *idx,
                    const float *tgt);
/* the records of `src` copied device to device into `dst` (same device) */
int hgx_records_copy(hgx_ctx *dst, hgx_ctx *src);
int hgx_records_info(hgx_ctx *ctx, int64_t *n, int *K);
int hgx_records_get(hgx_ctx *ctx, int32_t *idx, float *tgt);
/* Kind blocks of the stream in the reference's record order (hgx_sample_*:
 * nn, ee, ne node rows, ne edge rows [, the five negative blocks]; one block
 * after hgx_records_set): block i = [bounds[i], bounds[i+1]), at most 16
 * blocks (bounds holds nblocks + 1 entries). */
int hgx_records_blocks(hgx_ctx *ctx, int *nblocks, int64_t *bounds);
/* Device-to-device record copies for collectives over caller-owned device
 * buffers (e.g. RCCL all-gather of row-sharded samples):
 * export the n x (4+2K) ids and n x 3 targets; import a stream (nblocks 0 ->
 * one block). */
int hgx_records_export(hgx_ctx *ctx, void *d_idx, void *d_tgt);
int hgx_records_import(hgx_ctx *ctx, int64_t n, int K, const void *d_idx,
                       const void *d_tgt, int nblocks, const int64_t *bounds);

/* ---- compact record store: streams larger than HBM -------------------- *
 * The reference materialises every SimilarityRecord once and fits with
 * Keras' shuffle=True: each epoch a uniform permutation of the whole
 * stream in batches of 256 (embedding.py:277-302). The store keeps each
 * sampled record as 12 bytes (kind block and row, column or rank in row,
 * target); the rest of the record (neighbour lists, negatives' columns) is
 * re-derived from the sampler's keyed draws, bit for bit.
 *   hgx_store_reset(capacity)   empty the store, reserve `capacity` records
 *   hgx_store_append()          pack the records of the last
 *                               hgx_sample_fobe / hgx_sample_hobe(_rows)
 *                               call (HGX_ESTATE for any other stream; every
 *                               record is checked to reload bit for bit);
 *                               graphs of < 2^28 nodes and edges
 *   hgx_store_read / _write     raw 3 x uint32 entries to / from host or
 *                               device memory (multi-GPU: ranks exchange
 *                               what they sampled); write takes the
 *                               sampler family (0 FOBE, 1 HOBE), K, seed
 *   hgx_store_plan(epoch_seed, budget)
 *                               the epoch's order: records sorted by a
 *                               bijective mix of (identity, epoch_seed), so
 *                               the order does not depend on where records
 *                               sit in the store; the key space cut into
 *                               chunks of <= budget records, as bin ranges
 *                               of HGX_STORE_BINS bins (bin_bounds:
 *                               n_chunks + 1 entries, counts: n_chunks;
 *                               both arrays of HGX_STORE_BINS + 1)
 *   hgx_store_load(epoch_seed, bin_lo, bin_hi, batch, last)
 *                               the chunk's records as the context's record
 *                               stream, in epoch order, after the batch
 *                               tail the previous load kept (so batches
 *                               follow the global order); unless `last`,
 *                               the stream's own tail (< batch records) is
 *                               kept for the next load. hgx_train then
 *                               trains the records in that order (no
 *                               shuffle). n_records = records to train.
 *   hgx_store_release()         free the store, its load scratch and the
 *                               loaded records (the embedders call it when
 *                               fit_store returns or raises). */
#define HGX_STORE_BINS 16384
int hgx_store_reset(hgx_ctx *ctx, int64_t capacity);
int hgx_store_append(hgx_ctx *ctx);
int hgx_store_info(hgx_ctx *ctx, int64_t *n, int *family, int *K,
                   uint64_t *seed);
int hgx_store_read(hgx_ctx *ctx, int64_t start, int64_t n, void *dst,
                   int dst_device);
int hgx_store_write(hgx_ctx *ctx, int64_t n, const void *src, int src_device,
                    int family, int K, uint64_t seed);
int hgx_store_plan(hgx_ctx *ctx, uint64_t epoch_seed, int64_t budget,
                   int *n_chunks, int32_t *bin_bounds, int64_t *counts);
int hgx_store_load(hgx_ctx *ctx, uint64_t epoch_seed, int32_t bin_lo,
                   int32_t bin_hi, int batch, int last, int64_t *n_records);
int hgx_store_release(hgx_ctx *ctx);

/* ---- hg2v_weighting distance / span weights ------------------------------ *
 * hg2v_weighting.py:34-64 (WeightBySameTypeDistance), 67-103
 * (WeightByDistance), 170-192 + 236-293 (WeightByAlgebraicSpan,
 * ComputeSpans). The vectors are the alg coordinates on the context
 * (hgx_alg_set of the reference embedding's node / edge rows). `norm`:
 * np.linalg.norm (HGX_NORM_L2: numpy's float32 sdot arithmetic) or its
 * ord=inf (HGX_NORM_INF). Values are the reference's after
 * ZeroOneScaleValues -> OneMinusValues -> AlphaScaleValues, float32 (the
 * reference's arrays of protobuf float fields are float32); zeros are
 * returned (the reference's lil_matrix drops them). */
#define HGX_NORM_L2 0
#define HGX_NORM_INF 1
/* first order: per incidence, in A's (node_major) and A^T's (edge_major)
 * CSR order (either may be NULL) */
int hgx_weight_distance(hgx_ctx *ctx, int norm, double alpha, float *node_major,
                        float *edge_major);
/* second order: the A A^T (side 0, node rows) or A^T A (side 1) pattern,
 * diagonal included, as CSR over compressed ids (rows sorted, columns
 * ascending). col == val == NULL: only *nnz (and rowptr[R+1] if given);
 * HGX_EUNSUP when the pattern's expansion exceeds 2^31 paths. */
int hgx_weight_same_type(hgx_ctx *ctx, int side, int norm, double alpha,
                         int64_t *nnz, int64_t *rowptr, int32_t *col, float *val);
/* spans (ComputeSpans) and the span weights per incidence (node_major[v,e]
 * = edge e's value, edge_major[e,v] = node v's); any output may be NULL */
int hgx_weight_span(hgx_ctx *ctx, double alpha, float *node_span,
                    float *edge_span, float *node_major, float *edge_major);

/* ---- diagnostics ----------------------------------------------------------- *
 * Random-row gather rate of the device: rows of `row_floats` floats drawn
 * uniformly from a table of `table_bytes`, quads of lanes one row, in_flight
 * (4, 8, 16) rows per lane; best of `reps` launches, in rows per second.
 * The ceiling bench.py holds the C4 alg-dist gather against. */
int hgx_probe_gather(hgx_ctx *ctx, int64_t table_bytes, int row_floats,
                     int in_flight, int reps, double *rows_per_s);

/* ---- model + trainer ---------------------------------------------------- *
 * Replaces BooleanModel / UnweightedFloatModel (hg2v_model.py:51-203) and
 * the model.fit loop (embedding.py:269-305): two tables of (rows x d) fp32,
 * row 0 = padding, Keras Adagrad (a += g^2; p -= lr*g/(sqrt(a)+eps),
 * duplicate rows of a batch summed), loss = sum over the three heads of the
 * batch mean, EarlyStopping(monitor=loss, min_delta, patience=0).
 *   init_tables NULL -> uniform(-0.05, 0.05) from `seed` on device. */
int hgx_model_init(hgx_ctx *ctx, int d, int64_t node_rows, int64_t edge_rows,
                   uint64_t seed, const float *node_tab, const float *edge_tab);
int hgx_model_get(hgx_ctx *ctx, float *node_tab, float *edge_tab);
/* Rows `rows[0..n)` of the node (table 0) or edge (table 1) table into
 * out[n x d]: the touched rows of a 10M-row table without downloading it
 * (KerasModelToEmbedding reads rows idx + 1, hg2v_model.py:31-48). */
int hgx_model_get_rows(hgx_ctx *ctx, int table, int64_t n, const int64_t *rows,
                       float *out);
/* perms: NULL -> a fresh device shuffle per epoch keyed by shuffle_seed,
 * else max_epochs x n int64 permutations (Keras' np.random.shuffle order).
 * epoch_loss: max_epochs floats (may be NULL). */
int hgx_train(hgx_ctx *ctx, int batch, int max_epochs, float lr, float eps,
              int loss, int act, float min_delta, uint64_t shuffle_seed,
              const int64_t *perms, float *epoch_loss, int *epochs_run);
/* Device time (ms) of the last hgx_train spent in the per-batch kernels
 * (the K1+K2 replays, HIP events on the context stream; excludes the
 * per-epoch shuffle and batch preparation) and the records / batches they
 * processed. */
int hgx_train_last_stats(hgx_ctx *ctx, double *ms, int64_t *records,
                         int64_t *batches);
/* Of the last hgx_train: batches run by the one-launch deferred-row step
 * (train_step: rows in several records of a batch summed as fixed point and
 * applied by the next launch, the padding row likewise) and batches that
 * took the two-kernel step (train_fwd_bwd + train_update; tuning
 * "train_fused" 0 forces it). Same Keras semantics either way
 * (embedding.py:269-305, hg2v_model.py:51-203). They differ in how a row's
 * slot gradients are summed: the two-kernel step adds them in fp32, the
 * deferred-row step rounds each slot gradient (after the 1/batch factor) to
 * the nearest multiple of 2^-44 and adds them exactly as 64-bit integers
 * (order-free, bitwise reproducible): a quantisation of 2^-45 absolute per
 * slot, so values below 2^-45 (~2.8e-14) vanish. The padding row's
 * gradients are summed in fp32 per record (steps holding a float2 of the row
 * per lane, d = 128 by default) or per workgroup of records (float4 per
 * lane, d = 256) before that rounding. A slot gradient
 * of magnitude >= 32 fails the call with HGX_ENUMERIC. */
int hgx_train_path_stats(hgx_ctx *ctx, int64_t *fused_batches,
                         int64_t *split_batches);
/* Of the last hgx_train: step batches launched in the MULTI pending-slot form
 * (a record of theirs names two rows deferred by the previous batch). */
int hgx_train_multi_pending(hgx_ctx *ctx, int64_t *batches);
/* Of the last hgx_train: the deferred-row step's workgroup size and records
 * per workgroup (0, 0 if it was not eligible). The paired-wave form is 512
 * threads for 4 records; the one-wave forms have threads / records = the
 * lanes per record. */
int hgx_train_step_geometry(hgx_ctx *ctx, int *threads, int *records);
/* Sum of the per-record losses (all three heads) of the last epoch of the
 * last hgx_train, in double: epoch loss = sum / records. Consecutive
 * hgx_train calls continue the same model state (tables and Adagrad
 * accumulators persist; the padding row is written back at the end of each
 * call), so a stream too large to keep resident trains as a sequence of
 * one-epoch calls over resident chunks, the caller adding up these sums
 * (hg2v_model.Hg2vModel.fit_store over hgx_store_load's chunks). */
int hgx_train_last_loss(hgx_ctx *ctx, double *loss_sum);

/* ---- dense MLP engine (combiners + link-prediction classifier) --------- *
 * Replaces the Keras models of
 *   HGX_MLP_LP_CLASSIFIER       _TrainNodeEdgeEmbeddingClassifier +
 *                               NodeEdgeEmbeddingPrediction
 *                               (evaluation_util.py:471-552):
 *                               [node | edge] -> Dense(in, relu) -> Dense(1,
 *                               sigmoid); in = embedding.dim
 *   HGX_MLP_NE_SUPERVISED       CombineEmbeddingsViaNodeEdgeClassifier(...,
 *                               with_auto_encoder=False)
 *                               (combine_embeddings_util.py:80-174); in =
 *                               input_size, out = desired_dim
 *   HGX_MLP_NE_SEMI_SUPERVISED  the same with with_auto_encoder=True
 * Layers (Keras creation order; hgx_mlp_layers gives each kernel's K x N):
 *   classifier: hidden, label
 *   combiners:  pre_node, pre_edge, joint_node, joint_edge,
 *               [post_node, post_edge, recovered_node, recovered_edge,]
 *               hidden, label
 * Weights travel flat: per layer the kernel (K x N, row-major) then the bias
 * (N). Training = Keras fit: MSE, Adagrad(lr, eps, zero accumulators; a
 * set_weights restarts them), batches sequential, Dropout(0.5) on the
 * combiner inputs (mask from `seed`), EarlyStopping(monitor=loss,
 * min_delta, patience=0). perms: NULL -> device shuffle per epoch, else
 * max_epochs x n permutations. Samples reference table rows. */
#define HGX_MLP_LP_CLASSIFIER 0
#define HGX_MLP_NE_SUPERVISED 1
#define HGX_MLP_NE_SEMI_SUPERVISED 2
typedef struct hgx_mlp hgx_mlp;
int hgx_mlp_create(hgx_ctx *ctx, int kind, int in_dim, int out_dim,
                   hgx_mlp **out);
int hgx_mlp_destroy(hgx_mlp *m);
int hgx_mlp_layers(const hgx_mlp *m, int *n_layers, int32_t *shapes);
int hgx_mlp_set_weights(hgx_mlp *m, const float *flat);
int hgx_mlp_get_weights(hgx_mlp *m, float *flat);
/* node_tab: node_rows x in_dim, edge_tab: edge_rows x in_dim (row-major) */
int hgx_mlp_set_tables(hgx_mlp *m, int64_t node_rows, const float *node_tab,
                       int64_t edge_rows, const float *edge_tab);
/* (node row, edge row, label) per sample */
int hgx_mlp_set_samples(hgx_mlp *m, int64_t n, const int32_t *node_row,
                        const int32_t *edge_row, const float *label);
int hgx_mlp_fit(hgx_mlp *m, int batch, int max_epochs, float lr, float eps,
                float min_delta, uint64_t seed, const int64_t *perms,
                float *epoch_loss, int *epochs_run);
/* output 0: the label head per (node, edge) pair (n floats);
 * 1 / 2: JointNode of node rows / JointEdge of edge rows (n x out_dim).
 * Inference: no dropout. */
int hgx_mlp_predict(hgx_mlp *m, int output, int64_t n, const int32_t *node_row,
                    const int32_t *edge_row, float *out);
/* Device time (ms, HIP events over the batch launches) of the last fit,
 * samples and batches trained, algorithmic flops (fwd + bwd + weight
 * gradients of the unpadded layers). */
int hgx_mlp_last_stats(const hgx_mlp *m, double *ms, int64_t *samples,
                       int64_t *batches, double *flops);

/* ---- batched RBF C-SVC (per-edge / per-node link-prediction classifiers) *
 * Replaces the sklearn.svm.SVC(C=1, gamma=0.1) fits and predictions of
 * _train_personalized_classifier / PersonalizedClassifierPrediction
 * (evaluation_util.py:318-449): many small independent dual problems per
 * launch, libsvm's SMO (second-order working-set selection, stop at
 * m(alpha) - M(alpha) < eps) in float32, K(x, y) = exp(-gamma |x - y|^2).
 * A problem p is the samples [off[p], off[p + 1]): a row of the table and a
 * 0 / 1 label each; there is no limit on a problem's size. Label 1 is the
 * positive side of the decision value f = sum_j coef_j K(x_j, q) - rho,
 * coef = +-alpha. The dual coefficients and rho stay on the device
 * (hgx_svc_get copies them out, coef in sample order). max_iter <= 0 means
 * max(10000, 100 m) iterations per problem; a problem that reaches the cap
 * gets status 1 (0: converged) and keeps its current alpha and rho.
 * HGX_EVALUE before any launch: a non-finite table or query value, a row or
 * problem index out of range, a label other than 0 / 1, a problem without
 * samples or with one class only, C, gamma or eps not positive.
 * hgx_svc_decision scores rows of the table, hgx_svc_decision_vec host
 * vectors (n_q x dim), with the same kernel. hgx_svc_last_stats: device
 * time (ms, HIP events over the launches) of the last fit and decision. */
typedef struct hgx_svc hgx_svc;
int hgx_svc_create(hgx_ctx *ctx, int dim, int64_t n_rows, const float *rows,
                   hgx_svc **out);
int hgx_svc_destroy(hgx_svc *s);
int hgx_svc_fit(hgx_svc *s, int64_t n_prob, const int64_t *off,
                const int32_t *row, const uint8_t *label, float C, float gamma,
                float eps, int max_iter, int32_t *iters_out,
                int32_t *status_out);
int hgx_svc_decision(hgx_svc *s, int64_t n_q, const int32_t *prob,
                     const int32_t *row, float *f_out);
int hgx_svc_decision_vec(hgx_svc *s, int64_t n_q, const int32_t *prob,
                         const float *vecs, float *f_out);
int hgx_svc_get(hgx_svc *s, float *coef_out, float *rho_out);
int hgx_svc_last_stats(const hgx_svc *s, double *fit_ms, double *decision_ms);

/* ---- block primitives of the truncated SVD of the incidence -------------- *
 * The device half of EmbedSvd (reference embedding.py:110-126, which calls
 * scipy.sparse.linalg.svds): hypergraphembedding_amd/svd.py runs a
 * thick-restart block Lanczos through these calls, and only small matrices
 * (at most 1056 x 1056 float64) and the final vectors cross to the host.
 * The engine works on the incidence uploaded by hgx_upload_incidence before
 * hgx_svd_create (HGX_ESTATE without one, or after it was replaced).
 * long_row: rows with more incidences are summed in pieces of that many
 * (0: the library's default, 512); a result does not depend on anything
 * else, and two calls with the same operands are bitwise equal.
 *
 * A panel slot (0..7) holds a row-major fp32 matrix with one row per edge
 * (side 0) or per node (side 1); hgx_svd_panel (re)allocates it zeroed.
 * Every call below works on the columns [col0, col0 + ncols) of a slot
 * (HGX_EINVAL outside the panel):
 *   hgx_svd_set / _get  host (rows x ncols, row-major) <-> device
 *   hgx_svd_copy        dst <- src, same side, not overlapping
 *   hgx_svd_spmm        dst <- A src (src on the edge side, dst on the node
 *                       side) or dst <- A^T src (the other way round); a row
 *                       is summed in CSR column order, an empty row is zero
 *   hgx_svd_gram        out (p x q float64, row-major, host) <- P^T Q,
 *                       accumulated in float64; p, q <= 1056 (HGX_EUNSUP)
 *   hgx_svd_apply       dst (p columns) <- beta dst + src (q columns) M, M a
 *                       q x p row-major float64 host matrix, accumulated in
 *                       float64 and rounded once; dst and src must not share
 *                       columns; p, q <= 1056
 *   hgx_svd_scale       column j of the range <- column j * scale[j]
 * A non-finite entry of M, beta or scale is HGX_EVALUE before any launch.
 * hgx_svd_last_stats: device time (ms, HIP events) and algorithmic bytes
 * (4 nnz + 4 b nnz + 4 b rows per product of b columns) summed over the
 * products so far, their count and their total columns, and the count of
 * dense calls (gram, apply, scale).
 *
 * hgx_svd_cd_sweep is the one primitive the NMF baseline adds (EmbedNMF,
 * reference embedding.py:143-162, sklearn's coordinate-descent solver;
 * hypergraphembedding_amd/nmf.py drives its fused form with gram): one
 * non-negative coordinate-descent sweep over every row i of the factor view
 * P = columns [pcol0, pcol0 + k) of pslot, with B = columns [bcol0, bcol0 +
 * k) of bslot the matching rows of the sparse product and Q a k x k
 * row-major float64 host matrix (the other factor's Gram). For t = 0..k-1
 * in order, in float64:
 *   g = sum_r Q[t][r] P[i][r] - B[i][t]
 *   violation += |g|, or |min(g, 0)| where P[i][t] == 0
 *   if Q[t][t] != 0: P[i][t] <- fp32(max(P[i][t] - g / Q[t][t], 0))
 * and later coordinates of the row see the rounded value. *violation is the
 * sum over all rows, one float64 partial per row added in a fixed order (no
 * atomics). The two views are on the same side, and in one slot only with
 * disjoint column ranges (HGX_EINVAL); columns outside the factor view are
 * not touched; a non-finite entry of Q is HGX_EVALUE before any launch.
 * 1 <= k <= 512 (HGX_EUNSUP above: a lane holds at most 8 coordinates of a
 * row in registers); Q is staged in LDS up to k = 143 and read through L2
 * above. The call returns after the sweep has finished.
 * hgx_svd_cd_sweep_fused is the same sweep with B not read from a panel but
 * formed inside the kernel: xslot / xcol0 name k columns X of a panel of the
 * OTHER side (HGX_EINVAL for the same side) and row i of B = A X (factor on
 * the node side) or A^T X (edge side) is summed in CSR column order in
 * float64 and used unrounded. This is the form the solver runs: the fp32
 * rounding of a stored product is its largest error where a badly scaled
 * component cancels B against the Gram terms.
 * hgx_svd_cd_last_stats: device time (ms, HIP events) summed over the
 * sweeps so far, and their count. */
typedef struct hgx_svd hgx_svd;
int hgx_svd_create(hgx_ctx *ctx, int long_row, hgx_svd **out);
int hgx_svd_destroy(hgx_svd *s);
int hgx_svd_panel(hgx_svd *s, int slot, int side, int width);
int hgx_svd_set(hgx_svd *s, int slot, int col0, int ncols, const float *host);
int hgx_svd_get(hgx_svd *s, int slot, int col0, int ncols, float *host);
int hgx_svd_copy(hgx_svd *s, int dst, int dcol0, int src, int scol0, int ncols);
int hgx_svd_spmm(hgx_svd *s, int dst, int dcol0, int src, int scol0, int ncols);
int hgx_svd_gram(hgx_svd *s, int pslot, int pcol0, int p, int qslot, int qcol0,
                 int q, double *out);
int hgx_svd_apply(hgx_svd *s, int dst, int dcol0, int p, int src, int scol0,
                  int q, const double *M, double beta);
int hgx_svd_scale(hgx_svd *s, int slot, int col0, int ncols,
                  const double *scale);
int hgx_svd_last_stats(hgx_svd *s, double *spmm_ms, double *spmm_bytes,
                       int64_t *spmm_calls, int64_t *spmm_cols,
                       int64_t *dense_calls);
int hgx_svd_cd_sweep(hgx_svd *s, int pslot, int pcol0, int bslot, int bcol0,
                     int k, const double *Q, double *violation);
int hgx_svd_cd_sweep_fused(hgx_svd *s, int pslot, int pcol0, int xslot,
                           int xcol0, int k, const double *Q,
                           double *violation);
int hgx_svd_cd_last_stats(hgx_svd *s, double *sweep_ms, int64_t *sweeps);

/* ---- auto-encoder baseline ------------------------------------------------ *
 * The device half of EmbedAutoEncoder (reference auto_encoder.py:20-115):
 * one Keras model per side of the incidence uploaded before hgx_ae_create
 * (HGX_ESTATE without one, or after it was replaced),
 *   x (C) -> Dense(dim, relu) [W1 C x dim, b1] -> Dense(C, softmax)
 *   [W2 dim x C, b2], loss kullback_leibler_divergence (both arguments
 *   clipped to [1e-7, 1], batch mean), optimizer Adagrad (accumulators from
 *   0: a += g g; p -= lr g / (sqrt(a) + eps)).
 * side 0: one row per node, C = E columns; side 1: one row per edge, C = N.
 * 1 <= dim <= 512 (HGX_EUNSUP above); HGX_EUNSUP with a message when the
 * weights, accumulators and gradients with the smallest chunk of the logit
 * block do not fit into the free device memory.
 *
 * A sample is a pair (row, drop): the target is 1 / n on the n columns of
 * the row, the input the same (drop = -1) or 1 / (n - 1) on the row without
 * its column `drop`. hgx_ae_step runs one train_on_batch on an explicit
 * sample list (one Adagrad step, *loss = the batch mean); HGX_EINVAL for a
 * row outside the side, a drop that is not a column of its row, a drop on a
 * row of one column, or an empty list. A batch's n x C logit block is
 * processed in chunks of rows (tuning "ae_chunk_rows"), gradients summed
 * over the chunks in a fixed order.
 *
 * hgx_ae_draw: the samples of the listed rows in list order, per row the
 * unperturbed sample and then, for a row of n > 1 columns, min(n,
 * samples_per_idx) distinct columns of it in ascending order: all of them
 * when n <= samples_per_idx, else a uniform subset from the library's
 * counter-based generator keyed by (seed, row, epoch) alone. *n is the sample
 * count; row_out / drop_out (n entries each) may be NULL to ask for it.
 *
 * hgx_ae_fit: `epochs` passes over every row of the side; per epoch the rows
 * of perms[epoch] (a permutation of [0, R), HGX_EINVAL otherwise; NULL: the
 * library shuffles by sorting counter-based keys of (seed, epoch)) are split
 * into s = max(1, R / idx_per_batch) sections as numpy.array_split does (the
 * first R mod s hold one row more) and every section is one batch of the
 * samples hgx_ae_draw(seed, epoch) gives for it. Every batch is queued on
 * the context's stream without waiting for the previous one; batch_loss
 * (epochs x s floats) and *n_batches are written at the end. The weights
 * after hgx_ae_fit are bit for bit those of the same hgx_ae_draw /
 * hgx_ae_step calls made one by one.
 *
 * hgx_ae_set_weights / _get_weights: the flat float32 layout W1 (C x dim),
 * b1 (dim), W2 (dim x C), b2 (C), row-major; a set restarts the
 * accumulators (a new engine holds zeros). hgx_ae_encode: relu(x W1 + b1)
 * of the unperturbed input of every listed row, out n x dim.
 * hgx_ae_last_stats: of the last hgx_ae_step or hgx_ae_fit, the device time
 * (ms, HIP events), the samples and batches trained and the algorithmic
 * flops, 6 M C dim per batch of M samples. */
typedef struct hgx_ae hgx_ae;
int hgx_ae_create(hgx_ctx *ctx, int side, int dim, hgx_ae **out);
int hgx_ae_destroy(hgx_ae *a);
int hgx_ae_set_weights(hgx_ae *a, const float *flat);
int hgx_ae_get_weights(hgx_ae *a, float *flat);
int hgx_ae_draw(hgx_ae *a, int64_t n_idx, const int32_t *rows,
                int samples_per_idx, uint64_t seed, int epoch, int64_t *n,
                int32_t *row_out, int32_t *drop_out);
int hgx_ae_step(hgx_ae *a, int64_t n, const int32_t *row, const int32_t *drop,
                float lr, float eps, float *loss);
int hgx_ae_fit(hgx_ae *a, int epochs, int idx_per_batch, int samples_per_idx,
               float lr, float eps, uint64_t seed, const int64_t *perms,
               float *batch_loss, int *n_batches);
int hgx_ae_encode(hgx_ae *a, int64_t n, const int32_t *rows, float *out);
int hgx_ae_last_stats(const hgx_ae *a, double *ms, int64_t *samples,
                      int64_t *batches, double *flops);

/* ---- node2vec baselines ---------------------------------------------------- *
 * The device half of EmbedNode2VecBipartide / EmbedNode2VecClique (reference
 * embedding.py:165-261; the node2vec package's walks and gensim's skip-gram
 * negative-sampling trainer restated) on the incidence uploaded
 * before hgx_n2v_create (HGX_ESTATE without one, or after it was replaced).
 * graph 0, bipartite: node v is vertex v, edge e is vertex N + e, V = N + E.
 * graph 1, clique: the vertices are the nodes, V = N, u ~ v iff u != v and
 * they share an edge, every distinct neighbour with weight 1; the graph is
 * never materialised. 1 <= dim <= 512 (HGX_EUNSUP above, or when the two
 * V x dim tables do not fit).
 *
 * hgx_n2v_walks: one walk of walk_length vertices (the source included;
 * at most 128, HGX_EUNSUP above) per listed (pass, source). Step 1 is uniform
 * over the neighbours; from step 2 the previous vertex has weight 1 / p and
 * every other neighbour 1 (0 < p <= 1; p = 0 is HGX_EZERODIV, anything else
 * HGX_EINVAL; q = 1). Every draw is keyed by (seed, pass, source, step), so a
 * walk does not depend on the other entries of the list. HGX_EINVAL for a
 * source without a neighbour (a node of the clique graph that shares no edge
 * of two nodes, any zero-degree row of the bipartite graph). The walks stay
 * on the device for hgx_n2v_counts and hgx_n2v_train; walks_out (n x
 * walk_length, NULL to skip) receives a copy. The clique draw expands rows
 * of at most "n2v_expand_w" paths and samples longer ones by rejection.
 *
 * hgx_n2v_counts: occurrences of every vertex in the resident walks (V
 * entries). hgx_n2v_set_vocab: keep[w], the 32-bit threshold of word w's
 * subsampling (a word stays iff keep[w] > a uniform draw below 2^32 - 1), and
 * cum, the non-decreasing cumulative table of the negatives (a negative is
 * the first w with cum[w] >= a uniform draw below cum[V - 1]).
 *
 * hgx_n2v_train: `epochs` passes of skip-gram with `negative` (at most 8)
 * negatives over the resident walks, or over `walks` (n_walks x walk_length
 * vertices, which then become the resident ones) when it is not NULL. Per
 * kept word i of a walk and reduced window, per kept word j of the window:
 * l1 = syn0[w_j] held fixed; for t = w_i (label 1), then each negative
 * (label 0, one equal to w_i skipped), in order: x = l1 . syn1[t], skipped
 * when |x| >= 6, g = (label - 1 / (1 + exp(-x))) alpha, neu += g syn1[t],
 * syn1[t] += g l1; then syn0[w_j] += neu. alpha falls linearly from `alpha`
 * to `min_alpha` over the epochs x n_walks walks. concurrent 0: one wave
 * trains the walks in order (reproducible bit for bit). concurrent 1: the
 * walks of a chunk ("n2v_chunk_walks") train at once on a wave each, every
 * update a float atomic add; same draws, results differ in the last bits
 * from run to run.
 *
 * hgx_n2v_set_vectors / _get_vectors: V x dim float32 row-major; a NULL syn1
 * sets zeros / is not read back. hgx_n2v_last_stats: device time of the last
 * hgx_n2v_walks and hgx_n2v_train (ms, HIP events), the walks, kept words and
 * pairs of the last hgx_n2v_train, and the clique steps of the last
 * hgx_n2v_walks drawn by expansion and by rejection.
 *
 * DeepWalk is the same engine at p = 1 with a hierarchical-
 * softmax trainer. hgx_n2v_set_tree: the Huffman paths, vertex v's inner
 * nodes point[ptr[v] .. ptr[v + 1]) root first with one code bit each (V + 1,
 * ptr[V] and ptr[V] entries). Checked on the host before anything is
 * uploaded: ptr[0] == 0, ptr non-decreasing, every point in [0, V - 1), every
 * code 0 or 1, no inner node twice on a path, and the paths agree on the
 * inner node under every code prefix shorter than 6 bits (HGX_EINVAL); a path
 * longer than 64 is HGX_EUNSUP. A vertex with an empty path is never a target.
 *
 * hgx_n2v_train_hs: hgx_n2v_train's walks, keeps, reduced windows, pair order
 * and alpha schedule (of the vocabulary only keep is read), needs
 * hgx_n2v_set_vocab and hgx_n2v_set_tree (HGX_ESTATE). Per pair (input word
 * w_j, output word w_i): l1 = syn0[w_j] held fixed; for each inner node t of
 * w_i's path, root first, with code bit c: x = l1 . syn1[t], skipped when
 * |x| >= 6, g = (1 - c - 1 / (1 + exp(-x))) alpha, neu += g syn1[t] (the row
 * before its update), syn1[t] += g l1; then syn0[w_j] += neu. concurrent 0 is
 * reproducible bit for bit; concurrent 1 trains a chunk of walks per launch,
 * and the rows of the first "dw_hot_levels" tree levels are summed per
 * workgroup on chip: a wave sees its own updates to them at once, the other
 * workgroups at the next launch; no update is lost.
 * hgx_n2v_last_stats describes the last run of either trainer;
 * hgx_n2v_last_hs_stats: the sum of the path lengths over the pairs of the
 * last hgx_n2v_train_hs (0 after hgx_n2v_train).
 *
 * LINE is an edge-sampling trainer on the same engine, for the
 * bipartite graph only (HGX_ESTATE on a clique engine); it reads no walks.
 * Incidence p (position p of the node-major CSR) is the two arcs row(p) ->
 * N + col_n[p] and back, both of weight w_p. hgx_n2v_set_arcs: the alias
 * table over the incidences (draw p0 uniformly and a 32-bit value a below
 * 2^32 - 1; take p0 if a < thr[p0], else alias[p0]; nnz entries each, both
 * NULL for equal weights) and cum, the non-decreasing cumulative table of the
 * negatives over the V vertices (hgx_n2v_set_vocab's rule). HGX_EINVAL when
 * one of thr and alias is NULL and not the other, an alias is outside
 * [0, nnz), cum decreases or cum[V - 1] <= 0; a failed call sets no tables.
 *
 * Sample s (64 bits, 0 <= s < n_samples) draws with key (seed, s): counter 0
 * the position, 1 the alias decision, 2 the direction (0: u = row(p), v = N +
 * col_n[p]; 1: the reverse), 3 + k negative k; negatives are kept as drawn.
 * hgx_n2v_line_samples: the draws alone, row i of out (count x (2 +
 * negative)) = (u, v, negatives) of sample s0 + i.
 *
 * hgx_n2v_train_line: Tgt = syn0 at order 1, syn1 at order 2. Per sample:
 * l1 = syn0[u] held fixed, err = 0; for t = v (label 1), then each negative
 * (label 0), in order: x = l1 . Tgt[t] (the row as it stands, this sample's
 * earlier updates included), g = (label - s(x)) rho_s with s(x) = 1 above 6,
 * 0 below -6, else 1 / (1 + exp(-x)); err += g Tgt[t]; Tgt[t] += g l1; then
 * syn0[u] += err (to the row as it then stands). rho_s = max(rho (1 - s /
 * (n_samples + 1)), 1e-4 rho). concurrent 0: one wave trains the samples in
 * order (reproducible bit for bit). concurrent 1: "line_chunk_samples"
 * samples per launch, wave g of a launch the 64 consecutive samples from the
 * launch's start + 64 g in order, every update a float atomic add; same
 * draws, results differ in the last bits from run to run. Needs
 * hgx_n2v_set_arcs and hgx_n2v_set_vectors (HGX_ESTATE); order outside
 * {1, 2}, negative < 0 or n_samples < 0 is HGX_EINVAL, negative > 8
 * HGX_EUNSUP; n_samples = 0 trains nothing. hgx_n2v_last_stats' train_ms
 * covers the run. hgx_n2v_last_line_stats: the samples, the evaluated
 * targets and those of them with |x| > 6 of the last hgx_n2v_train_line (0
 * after the other trainers).
 *
 * metapath2vec / metapath2vec++ trains skip-gram with negative
 * sampling over a corpus that is never resident: walk g of n_walks =
 * num_walks x n_src has pass g / n_src and source sources[g % n_src], L
 * vertices (at most 256) and hgx_n2v_walks' draws at p = 1, and is generated
 * again whenever a chunk ("mp_chunk_walks") needs it. Bipartite engines only
 * (HGX_ESTATE on a clique engine). Every source is an edge vertex in [N, V)
 * with a non-empty row, so a walk never stands on a vertex without a
 * neighbour: nodes of degree 0 and empty edges are legal here. HGX_EINVAL for
 * L < 1, num_walks < 1, n_src < 1 or a bad source; HGX_EUNSUP for L > 256 or
 * n_walks >= 2^31.
 *
 * hgx_n2v_mp_walks: the walks g0 .. g0 + count - 1 alone (count x L).
 * hgx_n2v_mp_counts: occurrences of every vertex over the whole corpus (V
 * entries of 64 bits), chunk by chunk.
 *
 * hgx_n2v_set_vocab_typed: keep as hgx_n2v_set_vocab's; typed 0: cum under
 * hgx_n2v_set_vocab's rule, one segment [0, V); typed 1: two segments, [0, N)
 * and [N, V), each non-decreasing with a positive last entry. A negative for
 * an output word is the first w of the segment of the word's type with
 * cum[w] >= a uniform draw below the segment's last entry. HGX_EINVAL on a
 * violation; a failed call sets nothing. These tables are hgx_n2v_train_mp's
 * alone: hgx_n2v_set_vocab's stay as they are.
 *
 * hgx_n2v_train_mp: hgx_n2v_train's keeps, reduced windows, pair order and
 * alpha schedule over the streamed corpus, with key (train_seed, epoch << 32
 * | g) and counter ((position i << 8 | position j) << 4) | slot (slot 0 the
 * keep draw, 1 the window reduction, 2 + k negative k). Per pair: l1 =
 * syn0[w_j] held fixed; for t = w_i (label 1), then each negative (label 0,
 * one equal to w_i skipped), in order: x = l1 . syn1[t] (the row as it
 * stands), g = (label - s(x)) alpha with hgx_n2v_train_line's s; neu += g
 * syn1[t]; syn1[t] += g l1; then syn0[w_j] += neu. concurrent 0: one wave
 * trains the walks in corpus order; the result is reproducible bit for bit
 * and does not depend on the chunk size. concurrent 1: a chunk of walks per
 * launch on a wave each, every update a float atomic add. Needs
 * hgx_n2v_set_vocab_typed and hgx_n2v_set_vectors (HGX_ESTATE). window < 1,
 * negative < 0 or epochs < 0 is HGX_EINVAL; negative > 8 is HGX_EUNSUP, and so
 * is min(2 window + 1, L) x negative > 512, the negatives staged per output
 * word. hgx_n2v_last_stats' walk_ms is the device time of the run's walk
 * kernels and train_ms that of the rest of the run. hgx_n2v_last_mp_stats: the
 * walks, kept words, pairs, evaluated targets and those of them with |x| > 6
 * of the last hgx_n2v_train_mp. */
typedef struct hgx_n2v hgx_n2v;
int hgx_n2v_create(hgx_ctx *ctx, int graph, int dim, hgx_n2v **out);
int hgx_n2v_destroy(hgx_n2v *n);
int hgx_n2v_walks(hgx_n2v *n, int64_t n_src, const int32_t *pass,
                  const int32_t *source, int walk_length, double p,
                  uint64_t seed, int32_t *walks_out);
int hgx_n2v_counts(hgx_n2v *n, int32_t *counts);
int hgx_n2v_set_vocab(hgx_n2v *n, const uint32_t *keep, const int32_t *cum);
int hgx_n2v_set_vectors(hgx_n2v *n, const float *syn0, const float *syn1);
int hgx_n2v_get_vectors(hgx_n2v *n, float *syn0, float *syn1);
int hgx_n2v_train(hgx_n2v *n, int64_t n_walks, int walk_length,
                  const int32_t *walks, int window, int negative, int epochs,
                  float alpha, float min_alpha, uint64_t seed, int concurrent);
int hgx_n2v_last_stats(const hgx_n2v *n, double *walk_ms, double *train_ms,
                       int64_t *walks, int64_t *words, int64_t *pairs,
                       int64_t *expand_steps, int64_t *reject_steps);
int hgx_n2v_set_tree(hgx_n2v *n, const int32_t *ptr, const int32_t *point,
                     const uint8_t *code);
int hgx_n2v_train_hs(hgx_n2v *n, int64_t n_walks, int walk_length,
                     const int32_t *walks, int window, int epochs, float alpha,
                     float min_alpha, uint64_t seed, int concurrent);
int hgx_n2v_last_hs_stats(const hgx_n2v *n, int64_t *path_nodes);
int hgx_n2v_set_arcs(hgx_n2v *n, const uint32_t *thr, const int32_t *alias,
                     const int32_t *cum);
int hgx_n2v_line_samples(hgx_n2v *n, int64_t s0, int64_t count, int negative,
                         uint64_t seed, int32_t *out);
int hgx_n2v_train_line(hgx_n2v *n, int order, int negative, int64_t n_samples,
                       float rho, uint64_t seed, int concurrent);
int hgx_n2v_last_line_stats(const hgx_n2v *n, int64_t *samples,
                            int64_t *targets, int64_t *clamped);
int hgx_n2v_mp_walks(hgx_n2v *n, int64_t n_src, const int32_t *sources,
                     int num_walks, int L, uint64_t walk_seed, int64_t g0,
                     int64_t count, int32_t *out);
int hgx_n2v_mp_counts(hgx_n2v *n, int64_t n_src, const int32_t *sources,
                      int num_walks, int L, uint64_t walk_seed,
                      int64_t *counts_out);
int hgx_n2v_set_vocab_typed(hgx_n2v *n, const uint32_t *keep,
                            const int32_t *cum, int typed);
int hgx_n2v_train_mp(hgx_n2v *n, int64_t n_src, const int32_t *sources,
                     int num_walks, int L, int window, int negative,
                     int epochs, float alpha, float min_alpha,
                     uint64_t walk_seed, uint64_t train_seed, int concurrent);
int hgx_n2v_last_mp_stats(const hgx_n2v *n, int64_t *walks, int64_t *words,
                          int64_t *pairs, int64_t *targets, int64_t *clamped);

/* ---- host utilities (bench / test data; not reference entry points) --- *
 * Power-law synthetic incidence of SURVEY.md §8(d) (C4/C5): node degree
 * 1 + Poisson(mean_degree - 1), distinct edges per node drawn with
 * probability proportional to rank^-exponent; edges no node picked are
 * dropped and the rest renumbered (*E_out). Call with col_n == NULL to get
 * rowptr_n (N+1) and *nnz, then again with col_n (nnz) to fill the sorted
 * columns. Deterministic for `seed`. No context, no device. */
int hgx_synth_powerlaw(int32_t N, int32_t E, double mean_degree,
                       double exponent, uint64_t seed, int32_t *rowptr_n,
                       int32_t *col_n, int64_t *nnz, int32_t *E_out);
/* Native hypergraph.proto reader (Hypergraph, hypergraph.proto:6-23): the
 * serialized message -> the compressed incidence of
 * CompressRange(hg) (hypergraph_util.py:223-244) over every node's `edges`
 * list (Relabel, :208-212), duplicates dropped, plus weights (default 1).
 * Parse, read sizes, fill (rowptr_n N+1, col_n nnz, ids/weights N or E;
 * any pointer may be NULL), free. Errors: hgx_host_last_error(). */
typedef struct hgx_hg hgx_hg;
int hgx_proto_parse_hypergraph(const uint8_t *buf, int64_t len, hgx_hg **out,
                               int32_t *N, int32_t *E, int64_t *nnz);
int hgx_proto_hypergraph_fill(const hgx_hg *h, int32_t *rowptr_n,
                              int32_t *col_n, int64_t *node_ids,
                              int64_t *edge_ids, float *node_weight,
                              float *edge_weight);
void hgx_proto_hypergraph_free(hgx_hg *h);
/* Native HypergraphEmbedding writer (hypergraph.proto:26-35): rows of
 * node_tab (n_nodes x d) keyed by node_ids, likewise edges, dim, and
 * method_name (NULL = unset), entries in ascending id order. out == NULL
 * returns the size in *len; then call again with cap >= *len. */
int hgx_proto_write_embedding(int64_t n_nodes, const int64_t *node_ids,
                              const float *node_tab, int64_t n_edges,
                              const int64_t *edge_ids, const float *edge_tab,
                              int d, const char *method_name, uint8_t *out,
                              int64_t cap, int64_t *len);
/* Native HypergraphEmbedding reader (hypergraph.proto:26-35): one buffer
 * holding one message, or several shards of one embedding concatenated
 * (protobuf's wire format merges them: map entries union, a repeated key
 * keeps its last entry, the last dim / method_name wins). Any size, no
 * 2 GiB message limit. Parse -> sizes (entries per map, `width` = values per
 * entry, the same for every entry, and the dim field, 0 if unset); fill
 * (ids ascending, tables n x width row-major; any pointer may be NULL;
 * method_name NUL-terminated, cap >= hgx_proto_embedding_method_len + 1);
 * free. Replaces HypergraphEmbedding.ParseFromString for embeddings
 * written by runner.py:363-364 or by write_embedding's shards. */
typedef struct hgx_emb hgx_emb;
int hgx_proto_parse_embedding(const uint8_t *buf, int64_t len, hgx_emb **out,
                              int64_t *n_nodes, int64_t *n_edges,
                              int64_t *width, int32_t *dim);
int hgx_proto_embedding_fill(const hgx_emb *h, int64_t *node_ids,
                             float *node_tab, int64_t *edge_ids,
                             float *edge_tab, char *method_name, int64_t cap);
int64_t hgx_proto_embedding_method_len(const hgx_emb *h);
void hgx_proto_embedding_free(hgx_emb *h);
/* Hypergraph writer (test / bench data): compressed incidence + original
 * ids -> wire bytes (repeated fields unpacked, proto2's default). */
int hgx_proto_write_hypergraph(int32_t N, int32_t E, const int32_t *rowptr_n,
                               const int32_t *col_n, const int32_t *rowptr_e,
                               const int32_t *col_e, const int64_t *node_ids,
                               const int64_t *edge_ids, uint8_t *out,
                               int64_t cap, int64_t *len);
/* ---- link prediction, Python `random` semantics (host) ------------------ *
 * state: the 625 ints of random.getstate()[1] (MT19937 words + position),
 * advanced in place exactly as CPython's `random` would be.
 * SampleMissingConnections (evaluation_util.py:125-158): nodes / edges are
 * list positions (the map iteration order the caller saw); rowptr/col = each
 * node's edges as sorted edge positions. Outputs the distinct accepted
 * (node, edge) positions in insertion order (num_samples capacity). */
int hgx_pyrandom_sample_missing(uint32_t *state, int32_t n_nodes,
                                int32_t n_edges, const int64_t *rowptr,
                                const int32_t *col, int64_t num_samples,
                                int32_t *node_pos, int32_t *edge_pos,
                                int64_t *n_out);
/* RemoveRandomConnections (evaluation_util.py:84-122): pairs in the
 * reference's node_edges order, current degrees (decremented in place);
 * outputs the indices of the removed pairs in removal order. */
int hgx_pyrandom_remove_connections(uint32_t *state, int64_t n_pairs,
                                    const int32_t *pair_node,
                                    const int32_t *pair_edge,
                                    int32_t *node_deg, int32_t *edge_size,
                                    double probability, int64_t *removed,
                                    int64_t *n_removed);
const char *hgx_lp_last_error(void);
/* Message of the last failed host utility call on this thread. */
const char *hgx_host_last_error(void);
/* CSR transpose by counting sort (rows of the result sorted). */
int hgx_csr_transpose(int32_t nrow, int32_t ncol, const int32_t *rowptr,
                      const int32_t *col, int32_t *rowptr_t, int32_t *col_t);

#ifdef __cplusplus
}
#endif
#endif /* HGX_H_ */
