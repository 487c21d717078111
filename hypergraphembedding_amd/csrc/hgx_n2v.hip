// node2vec baselines (reference embedding.py:165-261, the node2vec package's
// walks and gensim's skip-gram negative-sampling trainer, restated: neither
// library is a dependency) on one MI355X (gfx950).
//
// Vertices. Bipartite graph: node v is vertex v, edge e is vertex N + e,
// adjacency = the two resident CSR orientations. Clique graph: the vertices
// are the nodes, u ~ v iff u != v and they share an edge, every distinct
// neighbour once; it is never materialised.
//
//   n2v_walk_bip     one lane per walk: an indexed CSR draw per step
//   n2v_walk_clique  one lane per walk: a uniform distinct co-member per step,
//                    by expansion of the row's paths (few paths) or by
//                    rejection with the 1 / |E(u) n E(v)| acceptance (many)
//   n2v_hist         count[w] = occurrences of vertex w in the walks
//   n2v_train        SGNS over the walks: one wave per walk, lane l holds
//                    columns l + 64 q of a row (d padded to 64, 128, 256, 512)
//
// The trainer has two modes. Sequential: one wave trains the walks in corpus
// order with plain loads and stores; this is the definition of the result.
// Concurrent: a chunk of walks per launch, one wave each; every update is a
// float atomic add without return (lossless), every row read is an
// agent-scope load (not served by a CU's L1), and the launch boundary bounds
// how stale a read can be to the walks of one chunk.
//
// Every draw is counter-based (rand64_key / mix64 of hgx_internal.h):
//   walks    key(seed, pass << 32 | source), counter step << 24 | try << 2 | slot
//   trainer  key(seed, epoch << 32 | walk),
//            counter (position i << 7 | position j) << 4 | slot
//            slot 0 the keep draw of position i, 1 its window reduction,
//            2 + k negative k of the pair (input word at j, output word at i)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "hgx_internal.h"

// g * x + y must stay two roundings: the host restatement rounds the product
#pragma clang fp contract(off)

namespace {

constexpr int kMaxD = 512;
constexpr int kMaxL = 128;    // walk length limit (the reference uses 3, 5, 7)
constexpr int kMaxNeg = 8;    // negatives per pair held in registers
constexpr int kMaxT = 1 + kMaxNeg;
constexpr int kMaxTry = 1 << 16;  // proposals per clique step before the step gives up
constexpr int kStatSlots = 64;
constexpr int kSeqWalks = 8192;  // walks per launch of the sequential trainer

__host__ __device__ inline uint64_t walk_ctr(int step, int it, int slot) {
  return ((uint64_t)step << 24) | ((uint64_t)it << 2) | (uint64_t)slot;
}
__host__ __device__ inline uint64_t train_ctr(int pi, int pj, int slot) {
  return ((((uint64_t)pi << 7) | (uint64_t)pj) << 4) | (uint64_t)slot;
}
__device__ __forceinline__ double u01(uint64_t r) {
  return (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

// ---- walks, bipartite graph ------------------------------------------------
// Step 1 (and every step at p = 1) is uniform over the current vertex's
// neighbours. Step t >= 2 at p < 1: the previous vertex has weight 1 / p, the
// deg - 1 others 1: back with probability (1 / p) / (deg - 1 + 1 / p), else a
// second draw uniform over the others.
__global__ void n2v_walk_bip(int n, const int *pass, const int *src, int L, double invp,
                             uint64_t seed, int N, const int *rp_n, const int *col_n,
                             const int *rp_e, const int *col_e, int *walks) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int cur = src[i], prev = -1;
  const uint64_t key = hgx::rand64_key(seed, ((uint64_t)(uint32_t)pass[i] << 32) | (uint32_t)cur);
  int *out = walks + (size_t)i * L;
  out[0] = cur;
  for (int t = 1; t < L; t++) {
    const bool node = cur < N;
    const int r = node ? cur : cur - N;
    const int *rp = node ? rp_n : rp_e, *col = node ? col_n : col_e;
    const int b = rp[r], deg = rp[r + 1] - b, shift = node ? N : 0;
    const uint64_t r0 = hgx::mix64(key + walk_ctr(t, 0, 0));
    int next;
    if (t == 1 || invp == 1.0) {
      next = col[b + hgx::bounded(r0, (uint32_t)deg)] + shift;
    } else if (u01(r0) * ((double)(deg - 1) + invp) < invp) {
      next = prev;
    } else {
      int k = (int)hgx::bounded(hgx::mix64(key + walk_ctr(t, 0, 1)), (uint32_t)(deg - 1));
      const int pc = prev - shift;  // the previous vertex as a column of this row
      int lo = 0, hi = deg;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[b + mid] < pc) lo = mid + 1; else hi = mid;
      }
      if (k >= lo) k++;
      next = col[b + k] + shift;
    }
    prev = cur;
    cur = next;
    out[t] = cur;
  }
}

// ---- walks, clique graph ---------------------------------------------------
__device__ __forceinline__ bool row_has(const int *col, int b, int e, int x) {
  while (b < e) {
    const int mid = (b + e) >> 1;
    const int c = col[mid];
    if (c == x) return true;
    if (c < x) b = mid + 1; else e = mid;
  }
  return false;
}

// A path of node u is (a, v): its a-th edge and a member v != u of it; the
// row has W = sum (|e| - 1) paths. A path is the representative of v when no
// earlier edge of u holds v: the representatives are the distinct neighbours.
// Expansion (W <= expand_w): D = the number of representatives, the draw is
// the bounded(r, D)-th in path order. Rejection: a uniform path, accepted
// with probability 1 / m, m = |E(u) n E(v)| the number of paths to v. Both
// are uniform over the distinct neighbours. The return weight: a proposal
// equal to the previous vertex is taken, any other with probability p
// (weights 1 : p, which is 1 / p : 1).
__global__ void n2v_walk_clique(int n, const int *pass, const int *src, int L, double p,
                                uint64_t seed, int expand_w, const int *rp_n, const int *col_n,
                                const int *rp_e, const int *col_e, int *walks,
                                unsigned long long *path_stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int cur = src[i], prev = -1;
  const uint64_t key = hgx::rand64_key(seed, ((uint64_t)(uint32_t)pass[i] << 32) | (uint32_t)cur);
  int *out = walks + (size_t)i * L;
  out[0] = cur;
  unsigned n_exp = 0, n_rej = 0;
  for (int t = 1; t < L; t++) {
    const int ub = rp_n[cur], ue = rp_n[cur + 1];
    long long W = 0;
    for (int a = ub; a < ue; a++) {
      const int e = col_n[a];
      W += rp_e[e + 1] - rp_e[e] - 1;
    }
    const bool expand = W <= (long long)expand_w;
    int D = 0;
    if (expand) {
      n_exp++;
      for (int a = ub; a < ue; a++) {
        const int e = col_n[a];
        for (int m = rp_e[e]; m < rp_e[e + 1]; m++) {
          const int v = col_e[m];
          if (v == cur) continue;
          bool first = true;
          for (int a2 = ub; a2 < a && first; a2++) {
            const int e2 = col_n[a2];
            first = !row_has(col_e, rp_e[e2], rp_e[e2 + 1], v);
          }
          D += first;
        }
      }
    } else {
      n_rej++;
    }
    int next = prev >= 0 ? prev : cur;
    for (int it = 0; it < kMaxTry; it++) {
      const uint64_t r0 = hgx::mix64(key + walk_ctr(t, it, 0));
      int cand = -1;
      if (expand) {
        int k = (int)hgx::bounded(r0, (uint32_t)D);
        for (int a = ub; a < ue && cand < 0; a++) {
          const int e = col_n[a];
          for (int m = rp_e[e]; m < rp_e[e + 1]; m++) {
            const int v = col_e[m];
            if (v == cur) continue;
            bool first = true;
            for (int a2 = ub; a2 < a && first; a2++) {
              const int e2 = col_n[a2];
              first = !row_has(col_e, rp_e[e2], rp_e[e2 + 1], v);
            }
            if (first && k-- == 0) {
              cand = v;
              break;
            }
          }
        }
      } else {
        // the path with index j: edges in row order, members in column order
        long long j = (long long)__umul64hi(r0, (uint64_t)W);
        int v = -1;
        for (int a = ub; a < ue; a++) {
          const int e = col_n[a], eb = rp_e[e], sz = rp_e[e + 1] - eb;
          if (j < sz - 1) {
            // the j-th member that is not cur (cur is a member of e)
            int lo = 0, hi = sz;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (col_e[eb + mid] < cur) lo = mid + 1; else hi = mid;
            }
            v = col_e[eb + (int)j + ((int)j >= lo ? 1 : 0)];
            break;
          }
          j -= sz - 1;
        }
        // m = |E(cur) n E(v)| by a merge of the two sorted rows
        int m = 0, x = ub, y = rp_n[v];
        const int ye = rp_n[v + 1];
        while (x < ue && y < ye) {
          const int cx = col_n[x], cy = col_n[y];
          m += cx == cy;
          x += cx <= cy;
          y += cy <= cx;
        }
        if (hgx::bounded(hgx::mix64(key + walk_ctr(t, it, 1)), (uint32_t)m) == 0) cand = v;
        if (it == kMaxTry - 1 && prev < 0) cand = v;  // first step: never stay
      }
      if (cand < 0) continue;
      if (t == 1 || p == 1.0 || cand == prev ||
          u01(hgx::mix64(key + walk_ctr(t, it, 2))) < p) {
        next = cand;
        break;
      }
    }
    prev = cur;
    cur = next;
    out[t] = cur;
  }
  if (path_stats) {
    if (n_exp) atomicAdd(path_stats, (unsigned long long)n_exp);
    if (n_rej) atomicAdd(path_stats + 1, (unsigned long long)n_rej);
  }
}

__global__ void n2v_hist(const int *walks, size_t n, int *count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(count + walks[i], 1);
}

// ---- trainer ---------------------------------------------------------------
struct TrainArgs {
  float *syn0, *syn1;
  const int *walks;
  const unsigned *keep;
  const int *cum;
  unsigned long long *stats;  // kStatSlots x {words, pairs}
  int dp, L, V, window, negative, epochs;
  int n_walks;
  uint32_t cum_last;
  uint64_t seed;
  double alpha, min_alpha;
};

template <bool CONC>
__device__ __forceinline__ float row_load(const float *p) {
  if (CONC) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return *p;
}

// One pair: input row l1 = syn0[wj] held fixed, targets t[0] = wi (label 1)
// and the negatives (label 0, one equal to wi skipped), processed in order. A
// target that repeats an earlier one reads the row as that one left it.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_pair(const TrainArgs &A, int lane, int wj, int wi,
                                           const int *negs, float alpha) {
  const int nt = 1 + A.negative;
  float *r0 = A.syn0 + (size_t)wj * A.dp + lane;
  float l1[NPL], neu[NPL], r[kMaxT][NPL];
  int tg[kMaxT];
#pragma unroll
  for (int k = 0; k < kMaxT; k++)
    tg[k] = k == 0 ? wi : (k < nt ? __builtin_amdgcn_readfirstlane(negs[k - 1]) : -1);
#pragma unroll
  for (int q = 0; q < NPL; q++) {
    l1[q] = row_load<CONC>(r0 + 64 * q);
    neu[q] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < kMaxT; k++) {
    if (k < nt) {
      const float *s = A.syn1 + (size_t)tg[k] * A.dp + lane;
#pragma unroll
      for (int q = 0; q < NPL; q++) r[k][q] = row_load<CONC>(s + 64 * q);
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxT; k++) {
    if (k < nt && (k == 0 || tg[k] != wi)) {
#pragma unroll
      for (int j = 0; j < k; j++) {
        if (tg[j] == tg[k]) {
#pragma unroll
          for (int q = 0; q < NPL; q++) r[k][q] = r[j][q];
        }
      }
      float x = 0.f;
#pragma unroll
      for (int q = 0; q < NPL; q++) x += l1[q] * r[k][q];
      x = hgx::group_allreduce_sum<64>(x);
      if (fabsf(x) < 6.0f) {  // word2vec's MAX_EXP: skipped at and above it
        const double sg = 1.0 / (1.0 + exp(-(double)x));
        const float g = (float)((k == 0 ? 1.0 : 0.0) - sg) * alpha;
        float *s = A.syn1 + (size_t)tg[k] * A.dp + lane;
#pragma unroll
        for (int q = 0; q < NPL; q++) {
          neu[q] += g * r[k][q];
          const float dlt = g * l1[q];
          r[k][q] += dlt;
          if (CONC) unsafeAtomicAdd(s + 64 * q, dlt);
          else s[64 * q] = r[k][q];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NPL; q++) {
    if (CONC) unsafeAtomicAdd(r0 + 64 * q, neu[q]);
    else r0[64 * q] = l1[q] + neu[q];
  }
}

// One walk on one wave. kw / kb: the kept words and (position | span << 8),
// span = window - b the reduced window; ng: the negatives of one output
// position's pairs, drawn by all lanes at once (a binary search of the
// cumulative table each) so that no pair waits on one.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_walk(const TrainArgs &A, int lane, int ep, int w,
                                           volatile int *kw, volatile int *kb, volatile int *ng) {
  const uint64_t key = hgx::rand64_key(A.seed, ((uint64_t)(uint32_t)ep << 32) | (uint32_t)w);
  const double gidx = (double)ep * (double)A.n_walks + (double)w;
  const double tot = (double)A.epochs * (double)A.n_walks;
  const double a = A.alpha - (A.alpha - A.min_alpha) * gidx / tot;
  const float alpha = (float)(a > A.min_alpha ? a : A.min_alpha);
  int nk = 0;
  for (int h = 0; h < 2; h++) {
    const int pos = lane + 64 * h;
    const bool valid = pos < A.L;
    const int word = valid ? A.walks[(size_t)w * A.L + pos] : 0;
    bool keep = false;
    if (valid)
      keep = A.keep[word] > hgx::bounded(hgx::mix64(key + train_ctr(pos, 0, 0)), 0xFFFFFFFFu);
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int idx = nk + __popcll(mask & ((1ull << lane) - 1ull));
      const int b = (int)hgx::bounded(hgx::mix64(key + train_ctr(pos, 0, 1)), (uint32_t)A.window);
      const int span = min(A.window - b, kMaxL);
      kw[idx] = word;
      kb[idx] = pos | (span << 8);
    }
    nk += __popcll(mask);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  long long pairs = 0;
  for (int i = 0; i < nk; i++) {
    const int wi = __builtin_amdgcn_readfirstlane(kw[i]);
    const int pbi = __builtin_amdgcn_readfirstlane(kb[i]);
    const int pi = pbi & 255, span = pbi >> 8;
    const int j0 = max(0, i - span), j1 = min(nk - 1, i + span);
    const int total = (j1 - j0 + 1) * A.negative;
    for (int s = lane; s < total; s += 64) {
      const int j = j0 + s / A.negative, k = s % A.negative;
      if (j == i) continue;
      const int pj = kb[j] & 255;
      const int x = (int)hgx::bounded(hgx::mix64(key + train_ctr(pi, pj, 2 + k)), A.cum_last);
      int lo = 0, hi = A.V - 1;  // x < cum[V - 1]: the answer is at most V - 1
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A.cum[mid] < x) lo = mid + 1; else hi = mid;
      }
      ng[s] = lo;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int j = j0; j <= j1; j++) {
      if (j == i) continue;
      const int wj = __builtin_amdgcn_readfirstlane(kw[j]);
      train_pair<NPL, CONC>(A, lane, wj, wi, (const int *)ng + (j - j0) * A.negative, alpha);
      pairs++;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    unsigned long long *st = A.stats + 2 * (w % kStatSlots);
    atomicAdd(st, (unsigned long long)nk);
    atomicAdd(st + 1, (unsigned long long)pairs);
  }
}

// Concurrent: wave g of the launch trains walk w0 + g of epoch ep. Sequential
// (one wave in all): epochs [ep, ep1), the walks [w0, w1) in order.
template <int NPL, bool CONC>
__global__ __launch_bounds__(256) void n2v_train(TrainArgs A, int ep, int ep1, int w0, int w1) {
  __shared__ int s_kw[4][kMaxL], s_kb[4][kMaxL], s_ng[4][kMaxL * kMaxNeg];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (CONC) {
    const int w = w0 + blockIdx.x * 4 + wv;
    if (w < w1) train_walk<NPL, true>(A, lane, ep, w, s_kw[wv], s_kb[wv], s_ng[wv]);
  } else {
    for (int e = ep; e < ep1; e++)
      for (int w = w0; w < w1; w++)
        train_walk<NPL, false>(A, lane, e, w, s_kw[0], s_kb[0], s_ng[0]);
  }
}

}  // namespace

struct hgx_n2v {
  hgx_ctx *ctx = nullptr;
  int graph = 0, N = 0, E = 0, V = 0, d = 0, dp = 0;
  uint64_t inc_gen = 0;
  std::vector<int32_t> h_rp_n, h_col_n, h_rp_e;  // host copy: preconditions
  DevBuf syn0, syn1, walks, pass, src, count, keep, cum, stats, pstats;
  int64_t n_walks = 0;  // resident walks
  int L = 0;
  bool vocab = false;
  uint32_t cum_last = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double walk_ms = 0, train_ms = 0;
  int64_t st_walks = 0, st_words = 0, st_pairs = 0, st_expand = 0, st_reject = 0;
};

namespace {

int n2v_live(hgx_n2v *a) {
  hgx_ctx *ctx = a->ctx;
  HGX_CHECK(ctx, a->inc_gen == ctx->inc_gen, HGX_ESTATE,
            "the incidence changed after hgx_n2v_create");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  return HGX_OK;
}

int n2v_elapsed(hgx_n2v *a, double *ms) {
  hgx_ctx *ctx = a->ctx;
  HGX_HIP(ctx, hipEventRecord(a->e1, ctx->stream));
  HGX_HIP(ctx, hipEventSynchronize(a->e1));
  float t = 0.f;
  HGX_HIP(ctx, hipEventElapsedTime(&t, a->e0, a->e1));
  *ms = t;
  return HGX_OK;
}

// walks per launch of the concurrent trainer: the tuning value, else about a
// quarter of the vertex count (a walk touches a few dozen rows: with V / 4
// walks in flight most rows a walk reads have no other writer in the launch),
// at most 4096 (16 waves on each CU)
int chunk_walks(const hgx_n2v *a) {
  int ch = a->ctx->tune.n2v_chunk_walks;
  if (ch <= 0) ch = std::min(4096, std::max(64, a->V / 4));
  return (ch + 3) / 4 * 4;
}

}  // namespace

extern "C" int hgx_n2v_destroy(hgx_n2v *a) {
  if (!a) return HGX_OK;
  if (a->ctx) hipStreamSynchronize(a->ctx->stream);
  for (DevBuf *b : {&a->syn0, &a->syn1, &a->walks, &a->pass, &a->src, &a->count, &a->keep,
                    &a->cum, &a->stats, &a->pstats})
    hgx_release(*b);
  for (hipEvent_t e : {a->e0, a->e1})
    if (e) hipEventDestroy(e);
  delete a;
  return HGX_OK;
}

static int n2v_alloc(hgx_n2v *a) {
  hgx_ctx *ctx = a->ctx;
  const size_t tab = sizeof(float) * (size_t)a->V * a->dp;
  size_t fr = 0, tot = 0;
  HGX_HIP(ctx, hipMemGetInfo(&fr, &tot));
  HGX_CHECK(ctx, 2 * tab <= fr, HGX_EUNSUP,
            "node2vec: two %d x %d tables (%zu bytes) exceed the %zu free bytes", a->V, a->dp,
            2 * tab, fr);
  HGX_TRY(hgx_ensure(ctx, a->syn0, tab));
  HGX_TRY(hgx_ensure(ctx, a->syn1, tab));
  HGX_TRY(hgx_ensure(ctx, a->count, sizeof(int) * (size_t)a->V));
  HGX_TRY(hgx_ensure(ctx, a->keep, sizeof(unsigned) * (size_t)a->V));
  HGX_TRY(hgx_ensure(ctx, a->cum, sizeof(int) * (size_t)a->V));
  HGX_TRY(hgx_ensure(ctx, a->stats, sizeof(unsigned long long) * 2 * kStatSlots));
  HGX_TRY(hgx_ensure(ctx, a->pstats, sizeof(unsigned long long) * 2));
  HGX_HIP(ctx, hipMemsetAsync(a->syn0.p, 0, a->syn0.bytes, ctx->stream));
  HGX_HIP(ctx, hipMemsetAsync(a->syn1.p, 0, a->syn1.bytes, ctx->stream));
  HGX_HIP(ctx, hipEventCreate(&a->e0));
  HGX_HIP(ctx, hipEventCreate(&a->e1));
  a->h_rp_n.resize((size_t)a->N + 1);
  a->h_rp_e.resize((size_t)a->E + 1);
  a->h_col_n.resize((size_t)ctx->nnz);
  HGX_HIP(ctx, hipMemcpyAsync(a->h_rp_n.data(), ctx->rp_n.p, sizeof(int32_t) * a->h_rp_n.size(),
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(a->h_rp_e.data(), ctx->rp_e.p, sizeof(int32_t) * a->h_rp_e.size(),
                              hipMemcpyDeviceToHost, ctx->stream));
  if (ctx->nnz)
    HGX_HIP(ctx, hipMemcpyAsync(a->h_col_n.data(), ctx->col_n.p,
                                sizeof(int32_t) * (size_t)ctx->nnz, hipMemcpyDeviceToHost,
                                ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_n2v_create(hgx_ctx *ctx, int graph, int dim, hgx_n2v **out) {
  if (!ctx || !out) return HGX_EINVAL;
  *out = nullptr;
  HGX_CHECK(ctx, ctx->N > 0 && ctx->E > 0 && ctx->rp_n.p && ctx->rp_e.p, HGX_ESTATE,
            "hgx_n2v_create before hgx_upload_incidence");
  HGX_CHECK(ctx, graph == 0 || graph == 1, HGX_EINVAL,
            "graph %d is not 0 (bipartite) or 1 (clique)", graph);
  HGX_CHECK(ctx, dim >= 1, HGX_EINVAL, "dimension %d < 1", dim);
  HGX_CHECK(ctx, dim <= kMaxD, HGX_EUNSUP, "node2vec dimension %d above %d", dim, kMaxD);
  HGX_CHECK(ctx, (int64_t)ctx->N + ctx->E < (1ll << 31), HGX_EUNSUP,
            "node2vec: N + E does not fit 31 bits");
  HGX_HIP(ctx, hipSetDevice(ctx->device));
  hgx_n2v *a = new hgx_n2v();
  a->ctx = ctx;
  a->graph = graph;
  a->N = ctx->N;
  a->E = ctx->E;
  a->V = graph == 0 ? ctx->N + ctx->E : ctx->N;
  a->d = dim;
  a->dp = 64;  // 64, 128, 256 or 512: 1, 2, 4 or 8 columns per lane
  while (a->dp < dim) a->dp *= 2;
  a->inc_gen = ctx->inc_gen;
  const int rc = n2v_alloc(a);
  if (rc) {
    hgx_n2v_destroy(a);
    return rc;
  }
  *out = a;
  return HGX_OK;
}

extern "C" int hgx_n2v_walks(hgx_n2v *a, int64_t n, const int32_t *pass, const int32_t *source,
                             int walk_length, double p, uint64_t seed, int32_t *walks_out) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, n >= 1 && pass && source, HGX_EINVAL, "hgx_n2v_walks: empty or null list");
  HGX_CHECK(ctx, walk_length >= 1, HGX_EINVAL, "hgx_n2v_walks: walk length %d < 1", walk_length);
  HGX_CHECK(ctx, walk_length <= kMaxL, HGX_EUNSUP, "hgx_n2v_walks: walk length %d above %d",
            walk_length, kMaxL);
  HGX_CHECK(ctx, p != 0.0, HGX_EZERODIV, "hgx_n2v_walks: p = 0 (the return weight is 1 / p)");
  HGX_CHECK(ctx, p > 0.0 && p <= 1.0, HGX_EINVAL, "hgx_n2v_walks: p = %g outside (0, 1]", p);
  HGX_CHECK(ctx, n * walk_length < (1ll << 31), HGX_EUNSUP,
            "hgx_n2v_walks: %lld walks of %d vertices do not fit 31 bits", (long long)n,
            walk_length);
  for (int64_t i = 0; i < n; i++) {
    const int s = source[i];
    HGX_CHECK(ctx, pass[i] >= 0, HGX_EINVAL, "hgx_n2v_walks: pass %d at position %lld", pass[i],
              (long long)i);
    HGX_CHECK(ctx, s >= 0 && s < a->V, HGX_EINVAL,
              "hgx_n2v_walks: source %d at position %lld outside [0, %d)", s, (long long)i, a->V);
    if (a->graph == 0) {
      const int deg = s < a->N ? a->h_rp_n[s + 1] - a->h_rp_n[s]
                               : a->h_rp_e[s - a->N + 1] - a->h_rp_e[s - a->N];
      HGX_CHECK(ctx, deg > 0, HGX_EINVAL, "hgx_n2v_walks: vertex %d has no neighbour", s);
    } else {
      bool ok = false;
      for (int e = a->h_rp_n[s]; e < a->h_rp_n[s + 1] && !ok; e++)
        ok = a->h_rp_e[a->h_col_n[e] + 1] - a->h_rp_e[a->h_col_n[e]] > 1;
      HGX_CHECK(ctx, ok, HGX_EINVAL,
                "hgx_n2v_walks: node %d has no distinct neighbour (it is not in the clique "
                "graph)", s);
    }
  }
  if (a->graph == 0 && walk_length > 1) {
    // a walk may reach any vertex: every row needs a neighbour
    for (int v = 0; v < a->N; v++)
      HGX_CHECK(ctx, a->h_rp_n[v + 1] > a->h_rp_n[v], HGX_EINVAL,
                "hgx_n2v_walks: node %d has no edge", v);
    for (int e = 0; e < a->E; e++)
      HGX_CHECK(ctx, a->h_rp_e[e + 1] > a->h_rp_e[e], HGX_EINVAL,
                "hgx_n2v_walks: edge %d has no node", e);
  }
  const int L = walk_length;
  HGX_TRY(hgx_ensure(ctx, a->pass, sizeof(int) * (size_t)n));
  HGX_TRY(hgx_ensure(ctx, a->src, sizeof(int) * (size_t)n));
  HGX_TRY(hgx_ensure(ctx, a->walks, sizeof(int) * (size_t)n * L));
  a->n_walks = 0;
  HGX_HIP(ctx, hipMemcpyAsync(a->pass.p, pass, sizeof(int) * (size_t)n, hipMemcpyHostToDevice,
                              ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(a->src.p, source, sizeof(int) * (size_t)n, hipMemcpyHostToDevice,
                              ctx->stream));
  HGX_HIP(ctx, hipMemsetAsync(a->pstats.p, 0, a->pstats.bytes, ctx->stream));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  const dim3 g((unsigned)((n + 63) / 64)), b(64);
  if (a->graph == 0)
    hipLaunchKernelGGL(n2v_walk_bip, g, b, 0, ctx->stream, (int)n, a->pass.as<int>(),
                       a->src.as<int>(), L, 1.0 / p, seed, a->N, ctx->rp_n.as<int>(),
                       ctx->col_n.as<int>(), ctx->rp_e.as<int>(), ctx->col_e.as<int>(),
                       a->walks.as<int>());
  else
    hipLaunchKernelGGL(n2v_walk_clique, g, b, 0, ctx->stream, (int)n, a->pass.as<int>(),
                       a->src.as<int>(), L, p, seed, ctx->tune.n2v_expand_w,
                       ctx->rp_n.as<int>(), ctx->col_n.as<int>(), ctx->rp_e.as<int>(),
                       ctx->col_e.as<int>(), a->walks.as<int>(),
                       a->pstats.as<unsigned long long>());
  HGX_LAUNCH_CHECK(ctx);
  HGX_TRY(n2v_elapsed(a, &a->walk_ms));
  unsigned long long ps[2] = {0, 0};
  HGX_HIP(ctx, hipMemcpy(ps, a->pstats.p, sizeof(ps), hipMemcpyDeviceToHost));
  a->st_expand = (int64_t)ps[0];
  a->st_reject = (int64_t)ps[1];
  a->n_walks = n;
  a->L = L;
  a->st_walks = n;
  if (walks_out)
    HGX_HIP(ctx, hipMemcpy(walks_out, a->walks.p, sizeof(int) * (size_t)n * L,
                           hipMemcpyDeviceToHost));
  return HGX_OK;
}

extern "C" int hgx_n2v_counts(hgx_n2v *a, int32_t *counts) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, counts, HGX_EINVAL, "hgx_n2v_counts: null output");
  HGX_CHECK(ctx, a->n_walks > 0, HGX_ESTATE, "hgx_n2v_counts before hgx_n2v_walks");
  const size_t n = (size_t)a->n_walks * a->L;
  HGX_HIP(ctx, hipMemsetAsync(a->count.p, 0, sizeof(int) * (size_t)a->V, ctx->stream));
  hipLaunchKernelGGL(n2v_hist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                     a->walks.as<int>(), n, a->count.as<int>());
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipMemcpyAsync(counts, a->count.p, sizeof(int) * (size_t)a->V,
                              hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_n2v_set_vocab(hgx_n2v *a, const uint32_t *keep, const int32_t *cum) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, keep && cum, HGX_EINVAL, "hgx_n2v_set_vocab: null table");
  for (int v = 0; v < a->V; v++)
    HGX_CHECK(ctx, cum[v] >= (v ? cum[v - 1] : 0), HGX_EINVAL,
              "hgx_n2v_set_vocab: the cumulative table decreases at %d", v);
  HGX_CHECK(ctx, cum[a->V - 1] > 0, HGX_EINVAL, "hgx_n2v_set_vocab: an empty cumulative table");
  HGX_HIP(ctx, hipMemcpyAsync(a->keep.p, keep, sizeof(uint32_t) * (size_t)a->V,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(a->cum.p, cum, sizeof(int32_t) * (size_t)a->V,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  a->cum_last = (uint32_t)cum[a->V - 1];
  a->vocab = true;
  return HGX_OK;
}

// host layout: V x dim, row-major
static int n2v_vectors_io(hgx_n2v *a, float *syn0, float *syn1, bool set) {
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  const size_t fs = sizeof(float), d = a->d, dp = a->dp, V = a->V;
  struct { DevBuf *dev; float *host; } v[2] = {{&a->syn0, syn0}, {&a->syn1, syn1}};
  for (auto &t : v) {
    if (set) {
      HGX_HIP(ctx, hipMemsetAsync(t.dev->p, 0, fs * V * dp, ctx->stream));
      if (t.host)
        HGX_HIP(ctx, hipMemcpy2DAsync(t.dev->p, fs * dp, t.host, fs * d, fs * d, V,
                                      hipMemcpyHostToDevice, ctx->stream));
    } else if (t.host) {
      HGX_HIP(ctx, hipMemcpy2DAsync(t.host, fs * d, t.dev->p, fs * dp, fs * d, V,
                                    hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_n2v_set_vectors(hgx_n2v *a, const float *syn0, const float *syn1) {
  if (!a) return HGX_EINVAL;
  HGX_CHECK(a->ctx, syn0, HGX_EINVAL, "hgx_n2v_set_vectors: null syn0");
  return n2v_vectors_io(a, const_cast<float *>(syn0), const_cast<float *>(syn1), true);
}
extern "C" int hgx_n2v_get_vectors(hgx_n2v *a, float *syn0, float *syn1) {
  if (!a) return HGX_EINVAL;
  return n2v_vectors_io(a, syn0, syn1, false);
}

extern "C" int hgx_n2v_train(hgx_n2v *a, int64_t n_walks, int walk_length,
                             const int32_t *walks, int window, int negative, int epochs,
                             float alpha, float min_alpha, uint64_t seed, int concurrent) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, a->vocab, HGX_ESTATE, "hgx_n2v_train before hgx_n2v_set_vocab");
  HGX_CHECK(ctx, window >= 1 && epochs >= 0 && negative >= 0, HGX_EINVAL,
            "hgx_n2v_train: window %d, epochs %d or negative %d out of range", window, epochs,
            negative);
  HGX_CHECK(ctx, negative <= kMaxNeg, HGX_EUNSUP, "hgx_n2v_train: negative %d above %d",
            negative, kMaxNeg);
  HGX_CHECK(ctx, concurrent == 0 || concurrent == 1, HGX_EINVAL,
            "hgx_n2v_train: concurrent %d is not 0 or 1", concurrent);
  if (walks) {
    HGX_CHECK(ctx, n_walks >= 1 && walk_length >= 1, HGX_EINVAL,
              "hgx_n2v_train: %lld walks of length %d", (long long)n_walks, walk_length);
    HGX_CHECK(ctx, walk_length <= kMaxL, HGX_EUNSUP, "hgx_n2v_train: walk length %d above %d",
              walk_length, kMaxL);
    HGX_CHECK(ctx, n_walks * walk_length < (1ll << 31), HGX_EUNSUP,
              "hgx_n2v_train: %lld walks of %d vertices do not fit 31 bits", (long long)n_walks,
              walk_length);
    const size_t n = (size_t)n_walks * walk_length;
    for (size_t i = 0; i < n; i++)
      HGX_CHECK(ctx, walks[i] >= 0 && walks[i] < a->V, HGX_EINVAL,
                "hgx_n2v_train: vertex %d at position %zu outside [0, %d)", walks[i], i, a->V);
    a->n_walks = 0;
    HGX_TRY(hgx_ensure(ctx, a->walks, sizeof(int) * n));
    HGX_HIP(ctx, hipMemcpyAsync(a->walks.p, walks, sizeof(int) * n, hipMemcpyHostToDevice,
                                ctx->stream));
    a->n_walks = n_walks;
    a->L = walk_length;
  }
  HGX_CHECK(ctx, a->n_walks > 0, HGX_ESTATE, "hgx_n2v_train without walks");
  const int nw = (int)a->n_walks;
  TrainArgs A;
  A.syn0 = a->syn0.as<float>();
  A.syn1 = a->syn1.as<float>();
  A.walks = a->walks.as<int>();
  A.keep = a->keep.as<unsigned>();
  A.cum = a->cum.as<int>();
  A.stats = a->stats.as<unsigned long long>();
  A.dp = a->dp;
  A.L = a->L;
  A.V = a->V;
  A.window = window;
  A.negative = negative;
  A.epochs = epochs;
  A.n_walks = nw;
  A.cum_last = a->cum_last;
  A.seed = seed;
  A.alpha = (double)alpha;
  A.min_alpha = (double)min_alpha;
  HGX_HIP(ctx, hipMemsetAsync(a->stats.p, 0, a->stats.bytes, ctx->stream));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  const int chunk = chunk_walks(a);
#define HGX_N2V_TRAIN(N, C, grid, tb, ep, ep1, w0, w1)                                     \
  hipLaunchKernelGGL((n2v_train<N, C>), dim3(grid), dim3(tb), 0, ctx->stream, A, ep, ep1, w0, w1)
#define HGX_N2V_BY_DP(C, grid, tb, ep, ep1, w0, w1)                       \
  switch (a->dp / 64) {                                                   \
    case 1: HGX_N2V_TRAIN(1, C, grid, tb, ep, ep1, w0, w1); break;        \
    case 2: HGX_N2V_TRAIN(2, C, grid, tb, ep, ep1, w0, w1); break;        \
    case 4: HGX_N2V_TRAIN(4, C, grid, tb, ep, ep1, w0, w1); break;        \
    default: HGX_N2V_TRAIN(8, C, grid, tb, ep, ep1, w0, w1); break;       \
  }
  if (epochs > 0) {
    if (!concurrent) {
      // one wave, the corpus in order; a launch per kSeqWalks walks keeps
      // every kernel short (the order, and so every bit, is the same)
      for (int ep = 0; ep < epochs; ep++)
        for (int w0 = 0; w0 < nw; w0 += kSeqWalks) {
          HGX_N2V_BY_DP(false, 1, 64, ep, ep + 1, w0, std::min(nw, w0 + kSeqWalks));
          HGX_LAUNCH_CHECK(ctx);
        }
    } else {
      for (int ep = 0; ep < epochs; ep++)
        for (int w0 = 0; w0 < nw; w0 += chunk) {
          const int w1 = std::min(nw, w0 + chunk);
          HGX_N2V_BY_DP(true, (w1 - w0 + 3) / 4, 256, ep, ep + 1, w0, w1);
          HGX_LAUNCH_CHECK(ctx);
        }
    }
  }
#undef HGX_N2V_BY_DP
#undef HGX_N2V_TRAIN
  HGX_TRY(n2v_elapsed(a, &a->train_ms));
  unsigned long long st[2 * kStatSlots];
  HGX_HIP(ctx, hipMemcpy(st, a->stats.p, sizeof(st), hipMemcpyDeviceToHost));
  a->st_words = a->st_pairs = 0;
  for (int i = 0; i < kStatSlots; i++) {
    a->st_words += (int64_t)st[2 * i];
    a->st_pairs += (int64_t)st[2 * i + 1];
  }
  a->st_walks = (int64_t)nw * epochs;
  return HGX_OK;
}

extern "C" int hgx_n2v_last_stats(const hgx_n2v *a, double *walk_ms, double *train_ms,
                                  int64_t *walks, int64_t *words, int64_t *pairs,
                                  int64_t *expand_steps, int64_t *reject_steps) {
  if (!a) return HGX_EINVAL;
  if (walk_ms) *walk_ms = a->walk_ms;
  if (train_ms) *train_ms = a->train_ms;
  if (walks) *walks = a->st_walks;
  if (words) *words = a->st_words;
  if (pairs) *pairs = a->st_pairs;
  if (expand_steps) *expand_steps = a->st_expand;
  if (reject_steps) *reject_steps = a->st_reject;
  return HGX_OK;
}
