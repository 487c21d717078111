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
//   n2v_train_hs     DeepWalk's trainer, skip-gram with hierarchical softmax
//                    over the same walks, keeps and windows: per pair the
//                    inner nodes of the output word's Huffman path, root
//                    first, their rows of syn1 loaded kHsBatch per round trip
//   n2v_train_line   LINE's edge-sampling trainer, first and second order
//                    (DESIGN §4.12): no corpus, one wave per 64 consecutive
//                    samples, the arc by alias table and the negatives drawn
//                    by all lanes at once, one update per sample
//   n2v_train_mp     metapath2vec(++)'s trainer: n2v_train over
//                    a corpus that is generated chunk by chunk and never
//                    resident, sentences of up to 256 vertices, negatives from
//                    the output word's own type, LINE's clamped sigmoid
//
// Either trainer has two modes. Sequential: one wave trains the walks in corpus
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
//
// Hot rows of the hierarchical-softmax trainer. Every pair
// updates the root's row of syn1, half of them each child's, and so on: sent
// as global atomics these adds would queue on a handful of rows. In concurrent
// mode the inner nodes at path positions below T = "dw_hot_levels" (a heap
// slot from the code bits above them: at most 2^T - 1 = 63 rows) are summed
// per workgroup in LDS: a hot row is read as its global value plus the
// workgroup's sum, its update is an LDS float add, and after a workgroup
// barrier each non-zero sum goes to memory as one atomic row add. A wave sees
// its own updates at once, the other workgroups at the next launch.
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
constexpr int kMaxCode = 64;     // longest Huffman path (word2vec's C code: 40)
constexpr int kMaxHotLevels = 6; // path positions summed in LDS: 2^6 - 1 = 63 rows
constexpr int kMaxHotRows = (1 << kMaxHotLevels) - 1;
constexpr int kHsBatch = 8;      // rows of a path loaded per round trip

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
  unsigned long long *stats;  // kStatSlots x {words, pairs}, then kStatSlots path nodes
  // hierarchical softmax: vertex v's path is point / code [ptr[v], ptr[v + 1]),
  // root first; hot_row[s] the inner node of heap slot s (-1: none)
  const int *ptr, *point, *hot_row;
  const uint8_t *code;
  int hot_levels;
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

// alpha of walk w in epoch ep: linear in the walk's global index
__device__ __forceinline__ float walk_alpha(const TrainArgs &A, int ep, int w) {
  const double gidx = (double)ep * (double)A.n_walks + (double)w;
  const double tot = (double)A.epochs * (double)A.n_walks;
  const double a = A.alpha - (A.alpha - A.min_alpha) * gidx / tot;
  return (float)(a > A.min_alpha ? a : A.min_alpha);
}

// The kept words of walk w, compacted in walk order: kw the words, kb
// (position | span << 8), span = window - b the reduced window. Returns their
// number; the wave may read kw / kb after it.
__device__ __forceinline__ int walk_keeps(const TrainArgs &A, int lane, uint64_t key, int w,
                                          volatile int *kw, volatile int *kb) {
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
  return nk;
}

// One walk on one wave. ng: the negatives of one output position's pairs,
// drawn by all lanes at once (a binary search of the cumulative table each)
// so that no pair waits on one.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_walk(const TrainArgs &A, int lane, int ep, int w,
                                           volatile int *kw, volatile int *kb, volatile int *ng) {
  const uint64_t key = hgx::rand64_key(A.seed, ((uint64_t)(uint32_t)ep << 32) | (uint32_t)w);
  const float alpha = walk_alpha(A, ep, w);
  const int nk = walk_keeps(A, lane, key, w, kw, kb);
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

// ---- trainer, hierarchical softmax ------------------------------------------
// One pair: l1 = syn0[wj] held fixed; the len inner nodes of the output
// word's path (point / code from pb on), root first, kHsBatch rows per round
// trip: the rows of a path are distinct and l1 is fixed, so they do not see
// each other. hot: the workgroup's sums of the hot rows (concurrent mode); the
// node at position k < hot_levels has heap slot 2^k - 1 + (the code bits above
// it), and only the first batch holds such positions.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_pair_hs(const TrainArgs &A, int lane, int wj, int pb,
                                              int len, float alpha, float *hot) {
  static_assert(kMaxHotLevels <= kHsBatch, "the hot positions lie in the first batch");
  float *r0 = A.syn0 + (size_t)wj * A.dp + lane;
  float l1[NPL], neu[NPL];
#pragma unroll
  for (int q = 0; q < NPL; q++) {
    l1[q] = row_load<CONC>(r0 + 64 * q);
    neu[q] = 0.f;
  }
  for (int k0 = 0; k0 < len; k0 += kHsBatch) {
    float r[kHsBatch][NPL], x[kHsBatch];
    int tg[kHsBatch], cd[kHsBatch], hs[kHsBatch];
#pragma unroll
    for (int k = 0; k < kHsBatch; k++) {
      const bool on = k0 + k < len;
      tg[k] = on ? A.point[pb + k0 + k] : -1;
      cd[k] = on ? (int)A.code[pb + k0 + k] : 0;
      hs[k] = -1;
      if (on) {
        const float *s = A.syn1 + (size_t)tg[k] * A.dp + lane;
#pragma unroll
        for (int q = 0; q < NPL; q++) r[k][q] = row_load<CONC>(s + 64 * q);
      }
    }
    if (CONC && k0 == 0) {
      int pre = 0;
#pragma unroll
      for (int k = 0; k < kMaxHotLevels; k++) {
        if (k < A.hot_levels && k < len) {
          hs[k] = ((1 << k) - 1 + pre) * A.dp + lane;
#pragma unroll
          for (int q = 0; q < NPL; q++)
            r[k][q] += __hip_atomic_load(hot + hs[k] + 64 * q, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_WORKGROUP);
          pre = 2 * pre + cd[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kHsBatch; k++) {
      x[k] = 0.f;
      if (tg[k] >= 0) {
#pragma unroll
        for (int q = 0; q < NPL; q++) x[k] += l1[q] * r[k][q];
      }
    }
    hgx::wave_allreduce_sum_n<kHsBatch>(x);
#pragma unroll
    for (int k = 0; k < kHsBatch; k++) {
      if (tg[k] >= 0 && fabsf(x[k]) < 6.0f) {  // word2vec's MAX_EXP
        const double sg = 1.0 / (1.0 + exp(-(double)x[k]));
        const float g = (float)((double)(1 - cd[k]) - sg) * alpha;
        float *s = A.syn1 + (size_t)tg[k] * A.dp + lane;
#pragma unroll
        for (int q = 0; q < NPL; q++) {
          neu[q] += g * r[k][q];
          const float dlt = g * l1[q];
          if (!CONC) s[64 * q] = r[k][q] + dlt;
          else if (hs[k] >= 0)
            __hip_atomic_fetch_add(hot + hs[k] + 64 * q, dlt, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
          else unsafeAtomicAdd(s + 64 * q, dlt);
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

// One walk on one wave: train_walk's keeps, windows and pair order, no
// negatives. A word without a path (it never occurs, or it is the only word)
// is an output word whose pairs change nothing.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_walk_hs(const TrainArgs &A, int lane, int ep, int w,
                                              volatile int *kw, volatile int *kb, float *hot) {
  const uint64_t key = hgx::rand64_key(A.seed, ((uint64_t)(uint32_t)ep << 32) | (uint32_t)w);
  const float alpha = walk_alpha(A, ep, w);
  const int nk = walk_keeps(A, lane, key, w, kw, kb);
  long long pairs = 0, nodes = 0;
  for (int i = 0; i < nk; i++) {
    const int wi = __builtin_amdgcn_readfirstlane(kw[i]);
    const int span = __builtin_amdgcn_readfirstlane(kb[i]) >> 8;
    const int j0 = max(0, i - span), j1 = min(nk - 1, i + span);
    const int pb = A.ptr[wi], len = A.ptr[wi + 1] - pb;
    for (int j = j0; j <= j1; j++) {
      if (j == i) continue;
      const int wj = __builtin_amdgcn_readfirstlane(kw[j]);
      train_pair_hs<NPL, CONC>(A, lane, wj, pb, len, alpha, hot);
      pairs++;
      nodes += len;
    }
  }
  if (lane == 0) {
    unsigned long long *st = A.stats + 2 * (w % kStatSlots);
    atomicAdd(st, (unsigned long long)nk);
    atomicAdd(st + 1, (unsigned long long)pairs);
    atomicAdd(A.stats + 2 * kStatSlots + w % kStatSlots, (unsigned long long)nodes);
  }
}

// n2v_train's geometry. Concurrent: s_hot (dynamic LDS, (2^hot_levels - 1) x
// dp floats) starts at zero, the workgroup's four waves add their hot-row
// deltas into it, and after the barrier wave wv sends the non-zero rows
// wv, wv + 4, ... to memory, one atomic row add each.
template <int NPL, bool CONC>
__global__ __launch_bounds__(256) void n2v_train_hs(TrainArgs A, int ep, int ep1, int w0,
                                                    int w1) {
  __shared__ int s_kw[4][kMaxL], s_kb[4][kMaxL];
  extern __shared__ float s_hot[];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (CONC) {
    const int n_hot = (1 << A.hot_levels) - 1;
    for (int i = threadIdx.x; i < n_hot * A.dp; i += 256) s_hot[i] = 0.f;
    __syncthreads();
    const int w = w0 + blockIdx.x * 4 + wv;
    if (w < w1) train_walk_hs<NPL, true>(A, lane, ep, w, s_kw[wv], s_kb[wv], s_hot);
    __syncthreads();
    for (int s = wv; s < n_hot; s += 4) {
      const int row = A.hot_row[s];
      if (row < 0) continue;
      float v[NPL];
      bool nz = false;
#pragma unroll
      for (int q = 0; q < NPL; q++) {
        v[q] = s_hot[s * A.dp + lane + 64 * q];
        nz |= v[q] != 0.f;
      }
      if (__ballot(nz)) {
        float *g = A.syn1 + (size_t)row * A.dp + lane;
#pragma unroll
        for (int q = 0; q < NPL; q++) unsafeAtomicAdd(g + 64 * q, v[q]);
      }
    }
  } else {
    for (int e = ep; e < ep1; e++)
      for (int w = w0; w < w1; w++)
        train_walk_hs<NPL, false>(A, lane, e, w, s_kw[0], s_kb[0], nullptr);
  }
}

using TrainFn = void (*)(TrainArgs, int, int, int, int);
template <bool HS, bool CONC>
TrainFn train_kernel(int npl) {
  switch (npl) {
    case 1: return HS ? n2v_train_hs<1, CONC> : n2v_train<1, CONC>;
    case 2: return HS ? n2v_train_hs<2, CONC> : n2v_train<2, CONC>;
    case 4: return HS ? n2v_train_hs<4, CONC> : n2v_train<4, CONC>;
    default: return HS ? n2v_train_hs<8, CONC> : n2v_train<8, CONC>;
  }
}

// ---- LINE: edge-sampling trainer ---------------------------------------------
// Sample s (64 bits) has key(seed, s) and the counters 0 the position p0 below
// nnz, 1 the alias decision (a 32-bit value against thr[p0]), 2 the direction,
// 3 + k negative k. Incidence p of the node-major CSR is the two arcs row(p) ->
// N + col_n[p] and back; row(p) is a binary search of rp_n, no arc array.
constexpr int kSeqSamples = 8192;  // samples per launch of the sequential trainer

struct LineArgs {
  float *syn0, *tgt;  // tgt: syn0 at order 1, syn1 at order 2
  const int *rp_n, *col_n;
  const unsigned *thr;  // null: equal weights, no table
  const int *alias, *cum;
  unsigned long long *stats;  // kStatSlots x {samples, targets, clamped}
  int dp, N, V, negative;
  uint32_t nnz, cum_last;
  int64_t T;
  uint64_t seed;
  double rho0;
};

// The draws of sample s: the arc u -> v and the negatives (-1 past A.negative)
__device__ __forceinline__ void line_draw(const LineArgs &A, int64_t s, int &u, int &v,
                                          int (&ng)[kMaxNeg]) {
  const uint64_t key = hgx::rand64_key(A.seed, (uint64_t)s);
  int p = (int)hgx::bounded(hgx::mix64(key), A.nnz);
  if (A.thr) {
    const uint32_t a = hgx::bounded(hgx::mix64(key + 1), 0xFFFFFFFFu);
    if (!(a < A.thr[p])) p = A.alias[p];
  }
  const bool back = hgx::bounded(hgx::mix64(key + 2), 2u) != 0;
  int lo = 0, hi = A.N;  // the first row that starts after p (rp_n[N] = nnz > p)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (A.rp_n[mid] <= p) lo = mid + 1; else hi = mid;
  }
  const int nd = lo - 1, ed = A.N + A.col_n[p];
  u = back ? ed : nd;
  v = back ? nd : ed;
#pragma unroll
  for (int k = 0; k < kMaxNeg; k++) {
    ng[k] = -1;
    if (k < A.negative) {
      const int x = (int)hgx::bounded(hgx::mix64(key + 3 + k), A.cum_last);
      int l = 0, h = A.V - 1;  // x < cum[V - 1]: the answer is at most V - 1
      while (l < h) {
        const int mid = (l + h) >> 1;
        if (A.cum[mid] < x) l = mid + 1; else h = mid;
      }
      ng[k] = l;
    }
  }
}

// rho of sample s: linear in s, never below 1e-4 rho0
__device__ __forceinline__ float line_rho(const LineArgs &A, int64_t s) {
  const double a = A.rho0 * (1.0 - (double)s / (double)(A.T + 1)), m = 1e-4 * A.rho0;
  return (float)(a > m ? a : m);
}

__global__ void n2v_line_samples(LineArgs A, int64_t s0, int64_t count, int *out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  int u, v, ng[kMaxNeg];
  line_draw(A, s0 + i, u, v, ng);
  int *o = out + i * (2 + A.negative);
  o[0] = u;
  o[1] = v;
#pragma unroll
  for (int k = 0; k < kMaxNeg; k++)
    if (k < A.negative) o[2 + k] = ng[k];
}

// One sample: l1 = syn0[u] held fixed, the targets tg[0] = v (label 1) and the
// negatives (label 0) in order, none rejected. All rows are loaded together; a
// target that repeats an earlier one takes that one's updated registers, and
// so does the closing row of u at order 1 when a target was u itself.
// Returns the number of targets with |x| > 6.
template <int NPL, bool CONC>
__device__ __forceinline__ int line_step(const LineArgs &A, int lane, int u, const int (&tg)[kMaxT],
                                         float rho) {
  const int nt = 1 + A.negative;
  float *r0 = A.syn0 + (size_t)u * A.dp + lane;
  float l1[NPL], err[NPL], r[kMaxT][NPL];
#pragma unroll
  for (int q = 0; q < NPL; q++) {
    l1[q] = row_load<CONC>(r0 + 64 * q);
    err[q] = 0.f;
  }
#pragma unroll
  for (int k = 0; k < kMaxT; k++) {
    if (k < nt) {
      const float *s = A.tgt + (size_t)tg[k] * A.dp + lane;
#pragma unroll
      for (int q = 0; q < NPL; q++) r[k][q] = row_load<CONC>(s + 64 * q);
    }
  }
  int clamped = 0;
#pragma unroll
  for (int k = 0; k < kMaxT; k++) {
    if (k < nt) {
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
      // LINE's bounded sigmoid: 1 above 6, 0 below -6, the logistic between
      double sg;
      if (x > 6.0f) sg = 1.0;
      else if (x < -6.0f) sg = 0.0;
      else sg = 1.0 / (1.0 + exp(-(double)x));
      clamped += fabsf(x) > 6.0f;
      const float g = (float)((k == 0 ? 1.0 : 0.0) - sg) * rho;
      if (g != 0.f) {
        float *s = A.tgt + (size_t)tg[k] * A.dp + lane;
#pragma unroll
        for (int q = 0; q < NPL; q++) {
          err[q] += g * r[k][q];
          const float dlt = g * l1[q];
          r[k][q] += dlt;
          if (CONC) unsafeAtomicAdd(s + 64 * q, dlt);
          else s[64 * q] = r[k][q];
        }
      }
    }
  }
  if (CONC) {
#pragma unroll
    for (int q = 0; q < NPL; q++) unsafeAtomicAdd(r0 + 64 * q, err[q]);
  } else {
    // the row of u as it now stands: at order 1 a target equal to u moved it
    if (A.tgt == A.syn0) {
#pragma unroll
      for (int k = 0; k < kMaxT; k++) {
        if (k < nt && tg[k] == u) {
#pragma unroll
          for (int q = 0; q < NPL; q++) l1[q] = r[k][q];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NPL; q++) r0[64 * q] = l1[q] + err[q];
  }
  return clamped;
}

// The n <= 64 consecutive samples from s0 on one wave: lane l draws sample
// s0 + l (all lanes at once, a binary search of rp_n and one of the cumulative
// table per negative each), then the wave trains them in order, reading lane
// i's draws by v_readlane.
template <int NPL, bool CONC>
__device__ __forceinline__ void line_run(const LineArgs &A, int lane, int64_t s0, int n) {
  int u = 0, v = 0, ng[kMaxNeg];
#pragma unroll
  for (int k = 0; k < kMaxNeg; k++) ng[k] = -1;
  float rho = 0.f;
  if (lane < n) {
    line_draw(A, s0 + lane, u, v, ng);
    rho = line_rho(A, s0 + lane);
  }
  int clamped = 0;
  for (int i = 0; i < n; i++) {
    int tg[kMaxT];
    const int ui = __builtin_amdgcn_readlane(u, i);
    tg[0] = __builtin_amdgcn_readlane(v, i);
#pragma unroll
    for (int k = 0; k < kMaxNeg; k++) tg[1 + k] = __builtin_amdgcn_readlane(ng[k], i);
    const float ri =
        __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rho), i));
    clamped += line_step<NPL, CONC>(A, lane, ui, tg, ri);
  }
  if (lane == 0) {
    unsigned long long *st = A.stats + 3 * ((s0 >> 6) % kStatSlots);
    atomicAdd(st, (unsigned long long)n);
    atomicAdd(st + 1, (unsigned long long)n * (1 + A.negative));
    atomicAdd(st + 2, (unsigned long long)clamped);
  }
}

// Concurrent: wave g of the launch trains the samples from s0 + 64 g, at most
// 64 and none at or past s1. Sequential (one wave in all): [s0, s1) in order.
template <int NPL, bool CONC>
__global__ __launch_bounds__(256) void n2v_train_line(LineArgs A, int64_t s0, int64_t s1) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (CONC) {
    const int64_t b = s0 + 64 * ((int64_t)blockIdx.x * 4 + wv);
    if (b < s1) line_run<NPL, true>(A, lane, b, (int)std::min<int64_t>(64, s1 - b));
  } else {
    for (int64_t b = s0; b < s1; b += 64)
      line_run<NPL, false>(A, lane, b, (int)std::min<int64_t>(64, s1 - b));
  }
}

using LineFn = void (*)(LineArgs, int64_t, int64_t);
template <bool CONC>
LineFn line_kernel(int npl) {
  switch (npl) {
    case 1: return n2v_train_line<1, CONC>;
    case 2: return n2v_train_line<2, CONC>;
    case 4: return n2v_train_line<4, CONC>;
    default: return n2v_train_line<8, CONC>;
  }
}

// ---- metapath2vec: streamed corpus, typed negatives ---------------------------
// Walk g of the corpus has pass g / n_src and source sources[g % n_src]; a
// chunk of walks is generated by n2v_walk_bip (p = 1) from the chunk's device-
// computed (pass, source) and trained, never the whole corpus. Positions reach
// 255, so the trainer's counter is (position i << 8 | position j) << 4 | slot.
constexpr int kMpMaxL = 256;    // vertices of a sentence
constexpr int kMpStage = 512;   // negatives staged per output word and wave
constexpr int kMpSeqWalks = 64;   // default chunk of the sequential trainer
constexpr int kMpStat = 4;      // words, pairs, targets, clamped

__host__ __device__ inline uint64_t mp_ctr(int pi, int pj, int slot) {
  return ((((uint64_t)pi << 8) | (uint64_t)pj) << 4) | (uint64_t)slot;
}

__global__ void n2v_mp_sources(int n, int g0, int n_src, const int *sources, int *pass,
                               int *src) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = g0 + i;
  pass[i] = g / n_src;
  src[i] = sources[g % n_src];
}

__global__ void n2v_hist64(const int *walks, size_t n, unsigned long long *count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(count + walks[i], 1ull);
}

struct MpArgs {
  float *syn0, *syn1;
  const int *walks;  // the chunk: walk g at row g - (the launch's first walk)
  const unsigned *keep;
  const int *cum;
  unsigned long long *stats;  // kStatSlots x {words, pairs, targets, clamped}
  int dp, L, V, N, window, negative, epochs, typed;
  int n_walks;  // of the corpus
  uint32_t last_node, last_edge;  // typed: cum[N - 1] and cum[V - 1]
  uint64_t seed;
  double alpha, min_alpha;
};

// train_pair with LINE's bounded sigmoid: no target is skipped for its x; one
// beyond +-6 whose label the clamped value equals has g = 0 and changes
// nothing. Counts the evaluated targets and those with |x| > 6.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_pair_mp(const MpArgs &A, int lane, int wj, int wi,
                                              const int *negs, float alpha, int &targets,
                                              int &clamped) {
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
      double sg;
      if (x > 6.0f) sg = 1.0;
      else if (x < -6.0f) sg = 0.0;
      else sg = 1.0 / (1.0 + exp(-(double)x));
      targets++;
      clamped += fabsf(x) > 6.0f;
      const float g = (float)((k == 0 ? 1.0 : 0.0) - sg) * alpha;
      if (g != 0.f) {
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

// walk_keeps for a sentence of up to 256 positions: four 64-lane passes
__device__ __forceinline__ int mp_keeps(const MpArgs &A, int lane, uint64_t key, const int *walk,
                                        volatile int *kw, volatile int *kb) {
  int nk = 0;
  for (int h = 0; h < kMpMaxL / 64; h++) {
    const int pos = lane + 64 * h;
    const bool valid = pos < A.L;
    const int word = valid ? walk[pos] : 0;
    bool keep = false;
    if (valid)
      keep = A.keep[word] > hgx::bounded(hgx::mix64(key + mp_ctr(pos, 0, 0)), 0xFFFFFFFFu);
    const unsigned long long mask = __ballot(keep);
    if (keep) {
      const int idx = nk + __popcll(mask & ((1ull << lane) - 1ull));
      const int b = (int)hgx::bounded(hgx::mix64(key + mp_ctr(pos, 0, 1)), (uint32_t)A.window);
      const int span = min(A.window - b, kMpMaxL);
      kw[idx] = word;
      kb[idx] = pos | (span << 8);
    }
    nk += __popcll(mask);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return nk;
}

// Walk g of epoch ep (row `row` of the chunk) on one wave. The negatives of an
// output word's pairs, at most min(2 window + 1, L) x negative <= kMpStage,
// come from the segment of the word's type and are drawn by all lanes at once.
template <int NPL, bool CONC>
__device__ __forceinline__ void train_walk_mp(const MpArgs &A, int lane, int ep, int g, int row,
                                              volatile int *kw, volatile int *kb,
                                              volatile int *ng) {
  const uint64_t key = hgx::rand64_key(A.seed, ((uint64_t)(uint32_t)ep << 32) | (uint32_t)g);
  const double gidx = (double)ep * (double)A.n_walks + (double)g;
  const double al = A.alpha - (A.alpha - A.min_alpha) * gidx /
                                  ((double)A.epochs * (double)A.n_walks);
  const float alpha = (float)(al > A.min_alpha ? al : A.min_alpha);
  const int nk = mp_keeps(A, lane, key, A.walks + (size_t)row * A.L, kw, kb);
  long long pairs = 0, targets = 0, clamped = 0;
  for (int i = 0; i < nk; i++) {
    const int wi = __builtin_amdgcn_readfirstlane(kw[i]);
    const int pbi = __builtin_amdgcn_readfirstlane(kb[i]);
    const int pi = pbi & 255, span = pbi >> 8;
    const int j0 = max(0, i - span), j1 = min(nk - 1, i + span);
    const int total = (j1 - j0 + 1) * A.negative;
    const bool edge = A.typed && wi >= A.N;
    const int seg_lo = edge ? A.N : 0;
    const int seg_hi = (A.typed && !edge ? A.N : A.V) - 1;
    const uint32_t last = edge || !A.typed ? A.last_edge : A.last_node;
    for (int s = lane; s < total; s += 64) {
      const int j = j0 + s / A.negative, k = s % A.negative;
      if (j == i) continue;
      const int pj = kb[j] & 255;
      const int x = (int)hgx::bounded(hgx::mix64(key + mp_ctr(pi, pj, 2 + k)), last);
      int lo = seg_lo, hi = seg_hi;  // x < cum[seg_hi]: the answer is at most seg_hi
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
      int nt = 0, nc = 0;
      train_pair_mp<NPL, CONC>(A, lane, wj, wi, (const int *)ng + (j - j0) * A.negative, alpha,
                               nt, nc);
      pairs++;
      targets += nt;
      clamped += nc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (lane == 0) {
    unsigned long long *st = A.stats + kMpStat * (g % kStatSlots);
    atomicAdd(st, (unsigned long long)nk);
    atomicAdd(st + 1, (unsigned long long)pairs);
    atomicAdd(st + 2, (unsigned long long)targets);
    atomicAdd(st + 3, (unsigned long long)clamped);
  }
}

// The walks [g0, g1) of epoch ep, rows 0 .. g1 - g0 - 1 of the chunk.
// Concurrent: wave w of the launch trains walk g0 + w. Sequential (one wave in
// all): the walks in order.
template <int NPL, bool CONC>
__global__ __launch_bounds__(256) void n2v_train_mp(MpArgs A, int ep, int g0, int g1) {
  __shared__ int s_kw[4][kMpMaxL], s_kb[4][kMpMaxL], s_ng[4][kMpStage];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (CONC) {
    const int g = g0 + blockIdx.x * 4 + wv;
    if (g < g1) train_walk_mp<NPL, true>(A, lane, ep, g, g - g0, s_kw[wv], s_kb[wv], s_ng[wv]);
  } else {
    for (int g = g0; g < g1; g++)
      train_walk_mp<NPL, false>(A, lane, ep, g, g - g0, s_kw[0], s_kb[0], s_ng[0]);
  }
}

using MpFn = void (*)(MpArgs, int, int, int);
template <bool CONC>
MpFn mp_kernel(int npl) {
  switch (npl) {
    case 1: return n2v_train_mp<1, CONC>;
    case 2: return n2v_train_mp<2, CONC>;
    case 4: return n2v_train_mp<4, CONC>;
    default: return n2v_train_mp<8, CONC>;
  }
}

}  // namespace

struct hgx_n2v {
  hgx_ctx *ctx = nullptr;
  int graph = 0, N = 0, E = 0, V = 0, d = 0, dp = 0;
  uint64_t inc_gen = 0;
  std::vector<int32_t> h_rp_n, h_col_n, h_rp_e;  // host copy: preconditions
  DevBuf syn0, syn1, walks, pass, src, count, keep, cum, stats, pstats;
  DevBuf ptr, point, code, hot_row;  // the Huffman tree (hgx_n2v_set_tree)
  bool tree = false;
  int64_t n_walks = 0;  // resident walks
  int L = 0;
  bool vocab = false;
  uint32_t cum_last = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double walk_ms = 0, train_ms = 0;
  int64_t st_walks = 0, st_words = 0, st_pairs = 0, st_expand = 0, st_reject = 0;
  int64_t st_path_nodes = 0;  // of the last hgx_n2v_train_hs
  // LINE (hgx_n2v_set_arcs / hgx_n2v_train_line)
  DevBuf arc_thr, arc_alias, arc_cum, arc_out;
  bool arcs = false, arc_weighted = false, vectors = false;
  uint32_t arc_cum_last = 0;
  int64_t st_line_samples = 0, st_line_targets = 0, st_line_clamped = 0;
  // metapath2vec (hgx_n2v_set_vocab_typed / hgx_n2v_train_mp): its own
  // vocabulary, the source list and one chunk of walks
  DevBuf mp_keep, mp_cum, mp_sources, mp_pass, mp_src, mp_walks, mp_count, mp_stats;
  bool mp_vocab = false;
  int mp_typed = 0;
  uint32_t mp_last_node = 0, mp_last_edge = 0;
  std::vector<hipEvent_t> mp_ev;  // a ring of event pairs round the walk kernels
  int64_t st_mp_walks = 0, st_mp_words = 0, st_mp_pairs = 0, st_mp_targets = 0,
          st_mp_clamped = 0;
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
                    &a->cum, &a->stats, &a->pstats, &a->ptr, &a->point, &a->code, &a->hot_row,
                    &a->arc_thr, &a->arc_alias, &a->arc_cum, &a->arc_out, &a->mp_keep,
                    &a->mp_cum, &a->mp_sources, &a->mp_pass, &a->mp_src, &a->mp_walks,
                    &a->mp_count, &a->mp_stats})
    hgx_release(*b);
  for (hipEvent_t e : {a->e0, a->e1})
    if (e) hipEventDestroy(e);
  for (hipEvent_t e : a->mp_ev)
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
  HGX_TRY(hgx_ensure(ctx, a->stats, sizeof(unsigned long long) * 3 * kStatSlots));
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
  HGX_TRY(n2v_vectors_io(a, const_cast<float *>(syn0), const_cast<float *>(syn1), true));
  a->vectors = true;
  return HGX_OK;
}
extern "C" int hgx_n2v_get_vectors(hgx_n2v *a, float *syn0, float *syn1) {
  if (!a) return HGX_EINVAL;
  return n2v_vectors_io(a, syn0, syn1, false);
}

extern "C" int hgx_n2v_set_tree(hgx_n2v *a, const int32_t *ptr, const int32_t *point,
                                const uint8_t *code) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, ptr, HGX_EINVAL, "hgx_n2v_set_tree: null ptr");
  const int V = a->V;
  HGX_CHECK(ctx, ptr[0] == 0, HGX_EINVAL, "hgx_n2v_set_tree: ptr[0] = %d", ptr[0]);
  for (int v = 0; v < V; v++) {
    HGX_CHECK(ctx, ptr[v + 1] >= ptr[v], HGX_EINVAL, "hgx_n2v_set_tree: ptr decreases at %d", v);
    HGX_CHECK(ctx, ptr[v + 1] - ptr[v] <= kMaxCode, HGX_EUNSUP,
              "hgx_n2v_set_tree: vertex %d has a path of %d inner nodes, above %d", v,
              ptr[v + 1] - ptr[v], kMaxCode);
  }
  const size_t total = (size_t)ptr[V];
  HGX_CHECK(ctx, total == 0 || (point && code), HGX_EINVAL, "hgx_n2v_set_tree: null table");
  // hot[s]: the inner node of heap slot s = 2^j - 1 + (the code bits above
  // position j), j < kMaxHotLevels. The kernel derives s from the code bits,
  // so the paths must agree on it; seen[t] = v + 1: t is on v's path already.
  std::vector<int32_t> hot(kMaxHotRows, -1), seen((size_t)V, 0);
  for (int v = 0; v < V; v++) {
    int pre = 0;
    for (int i = ptr[v], j = 0; i < ptr[v + 1]; i++, j++) {
      const int t = point[i];
      HGX_CHECK(ctx, t >= 0 && t < V - 1, HGX_EINVAL,
                "hgx_n2v_set_tree: inner node %d on vertex %d's path outside [0, %d)", t, v,
                V - 1);
      HGX_CHECK(ctx, code[i] <= 1, HGX_EINVAL, "hgx_n2v_set_tree: code %d on vertex %d's path",
                (int)code[i], v);
      HGX_CHECK(ctx, seen[t] != v + 1, HGX_EINVAL,
                "hgx_n2v_set_tree: inner node %d twice on vertex %d's path", t, v);
      seen[t] = v + 1;
      if (j < kMaxHotLevels) {
        const int s = (1 << j) - 1 + pre;
        HGX_CHECK(ctx, hot[s] < 0 || hot[s] == t, HGX_EINVAL,
                  "hgx_n2v_set_tree: the paths are not those of one tree (inner nodes %d and %d "
                  "at position %d under the same code bits)", hot[s], t, j);
        hot[s] = t;
        pre = 2 * pre + code[i];
      }
    }
  }
  for (int s = 0; s < kMaxHotRows; s++)
    for (int u = 0; u < s; u++)
      HGX_CHECK(ctx, hot[s] < 0 || hot[s] != hot[u], HGX_EINVAL,
                "hgx_n2v_set_tree: the paths are not those of one tree (inner node %d under two "
                "code prefixes)", hot[s]);
  a->tree = false;
  HGX_TRY(hgx_ensure(ctx, a->ptr, sizeof(int32_t) * ((size_t)V + 1)));
  HGX_TRY(hgx_ensure(ctx, a->point, sizeof(int32_t) * std::max<size_t>(total, 1)));
  HGX_TRY(hgx_ensure(ctx, a->code, std::max<size_t>(total, 1)));
  HGX_TRY(hgx_ensure(ctx, a->hot_row, sizeof(int32_t) * kMaxHotRows));
  HGX_HIP(ctx, hipMemcpyAsync(a->ptr.p, ptr, sizeof(int32_t) * ((size_t)V + 1),
                              hipMemcpyHostToDevice, ctx->stream));
  if (total) {
    HGX_HIP(ctx, hipMemcpyAsync(a->point.p, point, sizeof(int32_t) * total,
                                hipMemcpyHostToDevice, ctx->stream));
    HGX_HIP(ctx, hipMemcpyAsync(a->code.p, code, total, hipMemcpyHostToDevice, ctx->stream));
  }
  HGX_HIP(ctx, hipMemcpyAsync(a->hot_row.p, hot.data(), sizeof(int32_t) * kMaxHotRows,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  a->tree = true;
  return HGX_OK;
}

namespace {

// hgx_n2v_train (hs false) and hgx_n2v_train_hs
int n2v_train_any(hgx_n2v *a, bool hs, int64_t n_walks, int walk_length, const int32_t *walks,
                  int window, int negative, int epochs, float alpha, float min_alpha,
                  uint64_t seed, int concurrent) {
  hgx_ctx *ctx = a->ctx;
  const char *fn = hs ? "hgx_n2v_train_hs" : "hgx_n2v_train";
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, a->vocab, HGX_ESTATE, "%s before hgx_n2v_set_vocab", fn);
  HGX_CHECK(ctx, !hs || a->tree, HGX_ESTATE, "%s before hgx_n2v_set_tree", fn);
  HGX_CHECK(ctx, window >= 1 && epochs >= 0 && negative >= 0, HGX_EINVAL,
            "%s: window %d, epochs %d or negative %d out of range", fn, window, epochs, negative);
  HGX_CHECK(ctx, negative <= kMaxNeg, HGX_EUNSUP, "%s: negative %d above %d", fn, negative,
            kMaxNeg);
  HGX_CHECK(ctx, concurrent == 0 || concurrent == 1, HGX_EINVAL, "%s: concurrent %d is not 0 or 1",
            fn, concurrent);
  if (walks) {
    HGX_CHECK(ctx, n_walks >= 1 && walk_length >= 1, HGX_EINVAL, "%s: %lld walks of length %d",
              fn, (long long)n_walks, walk_length);
    HGX_CHECK(ctx, walk_length <= kMaxL, HGX_EUNSUP, "%s: walk length %d above %d", fn,
              walk_length, kMaxL);
    HGX_CHECK(ctx, n_walks * walk_length < (1ll << 31), HGX_EUNSUP,
              "%s: %lld walks of %d vertices do not fit 31 bits", fn, (long long)n_walks,
              walk_length);
    const size_t n = (size_t)n_walks * walk_length;
    for (size_t i = 0; i < n; i++)
      HGX_CHECK(ctx, walks[i] >= 0 && walks[i] < a->V, HGX_EINVAL,
                "%s: vertex %d at position %zu outside [0, %d)", fn, walks[i], i, a->V);
    a->n_walks = 0;
    HGX_TRY(hgx_ensure(ctx, a->walks, sizeof(int) * n));
    HGX_HIP(ctx, hipMemcpyAsync(a->walks.p, walks, sizeof(int) * n, hipMemcpyHostToDevice,
                                ctx->stream));
    a->n_walks = n_walks;
    a->L = walk_length;
  }
  HGX_CHECK(ctx, a->n_walks > 0, HGX_ESTATE, "%s without walks", fn);
  const int nw = (int)a->n_walks;
  TrainArgs A;
  A.syn0 = a->syn0.as<float>();
  A.syn1 = a->syn1.as<float>();
  A.walks = a->walks.as<int>();
  A.keep = a->keep.as<unsigned>();
  A.cum = a->cum.as<int>();
  A.stats = a->stats.as<unsigned long long>();
  A.ptr = a->ptr.as<int>();
  A.point = a->point.as<int>();
  A.hot_row = a->hot_row.as<int>();
  A.code = a->code.as<uint8_t>();
  A.hot_levels = hs && concurrent ? ctx->tune.dw_hot_levels : 0;
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
  const int npl = a->dp / 64;
  const TrainFn kern = hs ? (concurrent ? train_kernel<true, true>(npl)
                                        : train_kernel<true, false>(npl))
                          : (concurrent ? train_kernel<false, true>(npl)
                                        : train_kernel<false, false>(npl));
  // the hot rows' sums: up to 63 x 512 floats = 126 KiB, one workgroup per CU
  const size_t lds = sizeof(float) * ((1u << A.hot_levels) - 1) * a->dp;
  if (lds)
    HGX_HIP(ctx, hipFuncSetAttribute((const void *)kern,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HGX_HIP(ctx, hipMemsetAsync(a->stats.p, 0, a->stats.bytes, ctx->stream));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  // sequential: one wave, the corpus in order; a launch per kSeqWalks walks
  // keeps every kernel short (the order, and so every bit, is the same).
  // concurrent: a chunk of walks per launch, four to a workgroup
  const int step = concurrent ? chunk_walks(a) : kSeqWalks;
  for (int ep = 0; ep < epochs; ep++)
    for (int w0 = 0; w0 < nw; w0 += step) {
      const int w1 = std::min(nw, w0 + step);
      hipLaunchKernelGGL(kern, dim3(concurrent ? (w1 - w0 + 3) / 4 : 1),
                         dim3(concurrent ? 256 : 64), lds, ctx->stream, A, ep, ep + 1, w0, w1);
      HGX_LAUNCH_CHECK(ctx);
    }
  HGX_TRY(n2v_elapsed(a, &a->train_ms));
  unsigned long long st[3 * kStatSlots];
  HGX_HIP(ctx, hipMemcpy(st, a->stats.p, sizeof(st), hipMemcpyDeviceToHost));
  a->st_words = a->st_pairs = a->st_path_nodes = 0;
  for (int i = 0; i < kStatSlots; i++) {
    a->st_words += (int64_t)st[2 * i];
    a->st_pairs += (int64_t)st[2 * i + 1];
    a->st_path_nodes += (int64_t)st[2 * kStatSlots + i];
  }
  a->st_walks = (int64_t)nw * epochs;
  a->st_line_samples = a->st_line_targets = a->st_line_clamped = 0;
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_n2v_train(hgx_n2v *a, int64_t n_walks, int walk_length,
                             const int32_t *walks, int window, int negative, int epochs,
                             float alpha, float min_alpha, uint64_t seed, int concurrent) {
  if (!a) return HGX_EINVAL;
  return n2v_train_any(a, false, n_walks, walk_length, walks, window, negative, epochs, alpha,
                       min_alpha, seed, concurrent);
}

extern "C" int hgx_n2v_train_hs(hgx_n2v *a, int64_t n_walks, int walk_length,
                                const int32_t *walks, int window, int epochs, float alpha,
                                float min_alpha, uint64_t seed, int concurrent) {
  if (!a) return HGX_EINVAL;
  return n2v_train_any(a, true, n_walks, walk_length, walks, window, 0, epochs, alpha, min_alpha,
                       seed, concurrent);
}

// ---- LINE ----------------------------------------------------------------------
namespace {

// samples per launch of the concurrent LINE trainer: the tuning value, else
// V / 4 rounded down to a multiple of 256 (one workgroup trains 256), in
// [256, 65536]
int64_t line_chunk(const hgx_n2v *a) {
  int64_t ch = a->ctx->tune.line_chunk_samples;
  if (ch <= 0) ch = std::min(65536, std::max(256, a->V / 4 / 256 * 256));
  return ch;
}

int line_args(hgx_n2v *a, const char *fn, int negative, LineArgs *A) {
  hgx_ctx *ctx = a->ctx;
  HGX_CHECK(ctx, a->graph == 0, HGX_ESTATE, "%s: the engine is not on the bipartite graph", fn);
  HGX_CHECK(ctx, negative >= 0, HGX_EINVAL, "%s: negative %d < 0", fn, negative);
  HGX_CHECK(ctx, negative <= kMaxNeg, HGX_EUNSUP, "%s: negative %d above %d", fn, negative,
            kMaxNeg);
  HGX_CHECK(ctx, a->arcs, HGX_ESTATE, "%s before hgx_n2v_set_arcs", fn);
  A->syn0 = a->syn0.as<float>();
  A->tgt = a->syn1.as<float>();
  A->rp_n = ctx->rp_n.as<int>();
  A->col_n = ctx->col_n.as<int>();
  A->thr = a->arc_weighted ? a->arc_thr.as<unsigned>() : nullptr;
  A->alias = a->arc_alias.as<int>();
  A->cum = a->arc_cum.as<int>();
  A->stats = a->stats.as<unsigned long long>();
  A->dp = a->dp;
  A->N = a->N;
  A->V = a->V;
  A->negative = negative;
  A->nnz = (uint32_t)ctx->nnz;
  A->cum_last = a->arc_cum_last;
  A->T = 0;
  A->seed = 0;
  A->rho0 = 0.0;
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_n2v_set_arcs(hgx_n2v *a, const uint32_t *thr, const int32_t *alias,
                                const int32_t *cum) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, a->graph == 0, HGX_ESTATE,
            "hgx_n2v_set_arcs: the engine is not on the bipartite graph");
  const int64_t nnz = ctx->nnz;
  HGX_CHECK(ctx, nnz >= 1, HGX_EINVAL, "hgx_n2v_set_arcs: an incidence without an entry");
  HGX_CHECK(ctx, nnz < (1ll << 31), HGX_EUNSUP, "hgx_n2v_set_arcs: nnz does not fit 31 bits");
  HGX_CHECK(ctx, cum, HGX_EINVAL, "hgx_n2v_set_arcs: null cumulative table");
  HGX_CHECK(ctx, (thr == nullptr) == (alias == nullptr), HGX_EINVAL,
            "hgx_n2v_set_arcs: thr and alias are given together or not at all");
  if (alias)
    for (int64_t p = 0; p < nnz; p++)
      HGX_CHECK(ctx, alias[p] >= 0 && alias[p] < nnz, HGX_EINVAL,
                "hgx_n2v_set_arcs: alias %d at position %lld outside [0, %lld)", alias[p],
                (long long)p, (long long)nnz);
  for (int v = 0; v < a->V; v++)
    HGX_CHECK(ctx, cum[v] >= (v ? cum[v - 1] : 0), HGX_EINVAL,
              "hgx_n2v_set_arcs: the cumulative table decreases at %d", v);
  HGX_CHECK(ctx, cum[a->V - 1] > 0, HGX_EINVAL, "hgx_n2v_set_arcs: an empty cumulative table");
  HGX_TRY(hgx_ensure(ctx, a->arc_thr, sizeof(uint32_t) * (size_t)nnz));
  HGX_TRY(hgx_ensure(ctx, a->arc_alias, sizeof(int32_t) * (size_t)nnz));
  HGX_TRY(hgx_ensure(ctx, a->arc_cum, sizeof(int32_t) * (size_t)a->V));
  a->arcs = false;
  if (thr) {
    HGX_HIP(ctx, hipMemcpyAsync(a->arc_thr.p, thr, sizeof(uint32_t) * (size_t)nnz,
                                hipMemcpyHostToDevice, ctx->stream));
    HGX_HIP(ctx, hipMemcpyAsync(a->arc_alias.p, alias, sizeof(int32_t) * (size_t)nnz,
                                hipMemcpyHostToDevice, ctx->stream));
  }
  HGX_HIP(ctx, hipMemcpyAsync(a->arc_cum.p, cum, sizeof(int32_t) * (size_t)a->V,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  a->arc_weighted = thr != nullptr;
  a->arc_cum_last = (uint32_t)cum[a->V - 1];
  a->arcs = true;
  return HGX_OK;
}

extern "C" int hgx_n2v_line_samples(hgx_n2v *a, int64_t s0, int64_t count, int negative,
                                    uint64_t seed, int32_t *out) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  HGX_TRY(n2v_live(a));
  LineArgs A;
  HGX_TRY(line_args(a, "hgx_n2v_line_samples", negative, &A));
  HGX_CHECK(ctx, s0 >= 0 && count >= 0, HGX_EINVAL,
            "hgx_n2v_line_samples: first sample %lld or count %lld below 0", (long long)s0,
            (long long)count);
  HGX_CHECK(ctx, count == 0 || out, HGX_EINVAL, "hgx_n2v_line_samples: null output");
  HGX_CHECK(ctx, count * (2 + negative) < (1ll << 31), HGX_EUNSUP,
            "hgx_n2v_line_samples: %lld samples of %d vertices do not fit 31 bits",
            (long long)count, 2 + negative);
  if (count == 0) return HGX_OK;
  A.seed = seed;
  const size_t bytes = sizeof(int32_t) * (size_t)count * (2 + negative);
  HGX_TRY(hgx_ensure(ctx, a->arc_out, bytes));
  hipLaunchKernelGGL(n2v_line_samples, dim3((unsigned)((count + 255) / 256)), dim3(256), 0,
                     ctx->stream, A, s0, count, a->arc_out.as<int>());
  HGX_LAUNCH_CHECK(ctx);
  HGX_HIP(ctx, hipMemcpyAsync(out, a->arc_out.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_n2v_train_line(hgx_n2v *a, int order, int negative, int64_t n_samples,
                                  float rho, uint64_t seed, int concurrent) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  const char *fn = "hgx_n2v_train_line";
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, a->graph == 0, HGX_ESTATE, "%s: the engine is not on the bipartite graph", fn);
  HGX_CHECK(ctx, order == 1 || order == 2, HGX_EINVAL, "%s: order %d is not 1 or 2", fn, order);
  HGX_CHECK(ctx, n_samples >= 0, HGX_EINVAL, "%s: %lld samples", fn, (long long)n_samples);
  HGX_CHECK(ctx, concurrent == 0 || concurrent == 1, HGX_EINVAL, "%s: concurrent %d is not 0 or 1",
            fn, concurrent);
  LineArgs A;
  HGX_TRY(line_args(a, fn, negative, &A));
  HGX_CHECK(ctx, a->vectors, HGX_ESTATE, "%s before hgx_n2v_set_vectors", fn);
  if (order == 1) A.tgt = A.syn0;
  A.T = n_samples;
  A.seed = seed;
  A.rho0 = (double)rho;
  const int npl = a->dp / 64;
  const LineFn kern = concurrent ? line_kernel<true>(npl) : line_kernel<false>(npl);
  HGX_HIP(ctx, hipMemsetAsync(a->stats.p, 0, a->stats.bytes, ctx->stream));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  // sequential: one wave, the samples in order, a launch per kSeqSamples so
  // that no kernel runs long (the order, and so every bit, is the same).
  // concurrent: a chunk of samples per launch, 64 to a wave, 4 waves to a
  // workgroup; the launch boundary makes every update visible to the next
  const int64_t step = concurrent ? line_chunk(a) : kSeqSamples;
  for (int64_t s0 = 0; s0 < n_samples; s0 += step) {
    const int64_t s1 = std::min(n_samples, s0 + step);
    const unsigned nb = concurrent ? (unsigned)((s1 - s0 + 255) / 256) : 1u;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(concurrent ? 256 : 64), 0, ctx->stream, A, s0, s1);
    HGX_LAUNCH_CHECK(ctx);
  }
  HGX_TRY(n2v_elapsed(a, &a->train_ms));
  unsigned long long st[3 * kStatSlots];
  HGX_HIP(ctx, hipMemcpy(st, a->stats.p, sizeof(st), hipMemcpyDeviceToHost));
  a->st_line_samples = a->st_line_targets = a->st_line_clamped = 0;
  for (int i = 0; i < kStatSlots; i++) {
    a->st_line_samples += (int64_t)st[3 * i];
    a->st_line_targets += (int64_t)st[3 * i + 1];
    a->st_line_clamped += (int64_t)st[3 * i + 2];
  }
  a->st_words = a->st_pairs = a->st_path_nodes = 0;
  return HGX_OK;
}

extern "C" int hgx_n2v_last_line_stats(const hgx_n2v *a, int64_t *samples, int64_t *targets,
                                       int64_t *clamped) {
  if (!a) return HGX_EINVAL;
  if (samples) *samples = a->st_line_samples;
  if (targets) *targets = a->st_line_targets;
  if (clamped) *clamped = a->st_line_clamped;
  return HGX_OK;
}

extern "C" int hgx_n2v_last_hs_stats(const hgx_n2v *a, int64_t *path_nodes) {
  if (!a) return HGX_EINVAL;
  if (path_nodes) *path_nodes = a->st_path_nodes;
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

// ---- metapath2vec ----------------------------------------------------------------
namespace {

constexpr int kMpEvPairs = 32;  // walk-kernel timings in flight

// walks per chunk: the tuning value, else chunk_walks' rule (the sequential
// trainer: kMpSeqWalks); a multiple of 4
int mp_chunk(const hgx_n2v *a, bool sequential) {
  int ch = a->ctx->tune.mp_chunk_walks;
  if (ch <= 0) ch = sequential ? kMpSeqWalks : chunk_walks(a);
  return (ch + 3) / 4 * 4;
}

// The checks every entry point shares; uploads the source list, sizes the
// chunk buffers for `chunk` walks and returns the corpus size.
int mp_corpus(hgx_n2v *a, const char *fn, int64_t n_src, const int32_t *sources, int num_walks,
              int L, int chunk, int *n_walks) {
  hgx_ctx *ctx = a->ctx;
  HGX_CHECK(ctx, a->graph == 0, HGX_ESTATE, "%s: the engine is not on the bipartite graph", fn);
  HGX_CHECK(ctx, L >= 1 && num_walks >= 1 && n_src >= 1 && sources, HGX_EINVAL,
            "%s: %lld sources, %d walks per source of %d vertices", fn, (long long)n_src,
            num_walks, L);
  HGX_CHECK(ctx, L <= kMpMaxL, HGX_EUNSUP, "%s: %d vertices per walk above %d", fn, L, kMpMaxL);
  HGX_CHECK(ctx, n_src * (int64_t)num_walks < (1ll << 31), HGX_EUNSUP,
            "%s: %lld x %d walks do not fit 31 bits", fn, (long long)n_src, num_walks);
  for (int64_t i = 0; i < n_src; i++) {
    const int s = sources[i];
    HGX_CHECK(ctx, s >= a->N && s < a->V, HGX_EINVAL,
              "%s: source %d at position %lld is not an edge vertex in [%d, %d)", fn, s,
              (long long)i, a->N, a->V);
    HGX_CHECK(ctx, a->h_rp_e[s - a->N + 1] > a->h_rp_e[s - a->N], HGX_EINVAL,
              "%s: source %d at position %lld is an edge without a node", fn, s, (long long)i);
  }
  HGX_TRY(hgx_ensure(ctx, a->mp_sources, sizeof(int) * (size_t)n_src));
  HGX_TRY(hgx_ensure(ctx, a->mp_pass, sizeof(int) * (size_t)chunk));
  HGX_TRY(hgx_ensure(ctx, a->mp_src, sizeof(int) * (size_t)chunk));
  HGX_TRY(hgx_ensure(ctx, a->mp_walks, sizeof(int) * (size_t)chunk * L));
  HGX_HIP(ctx, hipMemcpyAsync(a->mp_sources.p, sources, sizeof(int) * (size_t)n_src,
                              hipMemcpyHostToDevice, ctx->stream));
  *n_walks = (int)(n_src * num_walks);
  return HGX_OK;
}

// The walks g0 .. g0 + n - 1 into the chunk buffer (n at most the chunk the
// buffers were sized for)
int mp_generate(hgx_n2v *a, int g0, int n, int n_src, int L, uint64_t seed) {
  hgx_ctx *ctx = a->ctx;
  const dim3 g((unsigned)((n + 63) / 64)), b(64);
  hipLaunchKernelGGL(n2v_mp_sources, g, b, 0, ctx->stream, n, g0, n_src,
                     a->mp_sources.as<int>(), a->mp_pass.as<int>(), a->mp_src.as<int>());
  HGX_LAUNCH_CHECK(ctx);
  hipLaunchKernelGGL(n2v_walk_bip, g, b, 0, ctx->stream, n, a->mp_pass.as<int>(),
                     a->mp_src.as<int>(), L, 1.0, seed, a->N, ctx->rp_n.as<int>(),
                     ctx->col_n.as<int>(), ctx->rp_e.as<int>(), ctx->col_e.as<int>(),
                     a->mp_walks.as<int>());
  HGX_LAUNCH_CHECK(ctx);
  return HGX_OK;
}

}  // namespace

extern "C" int hgx_n2v_mp_walks(hgx_n2v *a, int64_t n_src, const int32_t *sources, int num_walks,
                                int L, uint64_t walk_seed, int64_t g0, int64_t count,
                                int32_t *out) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  const char *fn = "hgx_n2v_mp_walks";
  HGX_TRY(n2v_live(a));
  const int chunk = mp_chunk(a, false);
  int nw = 0;
  HGX_TRY(mp_corpus(a, fn, n_src, sources, num_walks, L, chunk, &nw));
  HGX_CHECK(ctx, g0 >= 0 && count >= 0 && g0 + count <= nw, HGX_EINVAL,
            "%s: the walks %lld .. %lld + %lld are not all in [0, %d)", fn, (long long)g0,
            (long long)g0, (long long)count, nw);
  HGX_CHECK(ctx, count == 0 || out, HGX_EINVAL, "%s: null output", fn);
  for (int64_t c0 = 0; c0 < count; c0 += chunk) {
    const int n = (int)std::min<int64_t>(chunk, count - c0);
    HGX_TRY(mp_generate(a, (int)(g0 + c0), n, (int)n_src, L, walk_seed));
    HGX_HIP(ctx, hipMemcpyAsync(out + (size_t)c0 * L, a->mp_walks.p, sizeof(int) * (size_t)n * L,
                                hipMemcpyDeviceToHost, ctx->stream));
  }
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return HGX_OK;
}

extern "C" int hgx_n2v_mp_counts(hgx_n2v *a, int64_t n_src, const int32_t *sources, int num_walks,
                                 int L, uint64_t walk_seed, int64_t *counts_out) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  const char *fn = "hgx_n2v_mp_counts";
  HGX_TRY(n2v_live(a));
  const int chunk = mp_chunk(a, false);
  int nw = 0;
  HGX_TRY(mp_corpus(a, fn, n_src, sources, num_walks, L, chunk, &nw));
  HGX_CHECK(ctx, counts_out, HGX_EINVAL, "%s: null output", fn);
  static_assert(sizeof(unsigned long long) == sizeof(int64_t), "64-bit counts");
  HGX_TRY(hgx_ensure(ctx, a->mp_count, sizeof(int64_t) * (size_t)a->V));
  HGX_HIP(ctx, hipMemsetAsync(a->mp_count.p, 0, sizeof(int64_t) * (size_t)a->V, ctx->stream));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  for (int64_t g0 = 0; g0 < nw; g0 += chunk) {
    const int n = (int)std::min<int64_t>(chunk, nw - g0);
    HGX_TRY(mp_generate(a, (int)g0, n, (int)n_src, L, walk_seed));
    const size_t tokens = (size_t)n * L;
    hipLaunchKernelGGL(n2v_hist64, dim3((unsigned)((tokens + 255) / 256)), dim3(256), 0,
                       ctx->stream, a->mp_walks.as<int>(), tokens,
                       a->mp_count.as<unsigned long long>());
    HGX_LAUNCH_CHECK(ctx);
  }
  HGX_TRY(n2v_elapsed(a, &a->walk_ms));
  HGX_HIP(ctx, hipMemcpy(counts_out, a->mp_count.p, sizeof(int64_t) * (size_t)a->V,
                         hipMemcpyDeviceToHost));
  return HGX_OK;
}

extern "C" int hgx_n2v_set_vocab_typed(hgx_n2v *a, const uint32_t *keep, const int32_t *cum,
                                       int typed) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  const char *fn = "hgx_n2v_set_vocab_typed";
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, a->graph == 0, HGX_ESTATE, "%s: the engine is not on the bipartite graph", fn);
  HGX_CHECK(ctx, keep && cum, HGX_EINVAL, "%s: null table", fn);
  HGX_CHECK(ctx, typed == 0 || typed == 1, HGX_EINVAL, "%s: typed %d is not 0 or 1", fn, typed);
  for (int v = 0; v < a->V; v++)
    HGX_CHECK(ctx, cum[v] >= (v && !(typed && v == a->N) ? cum[v - 1] : 0), HGX_EINVAL,
              "%s: the cumulative table decreases at %d", fn, v);
  HGX_CHECK(ctx, cum[a->V - 1] > 0 && (!typed || cum[a->N - 1] > 0), HGX_EINVAL,
            "%s: an empty cumulative table", fn);
  HGX_TRY(hgx_ensure(ctx, a->mp_keep, sizeof(uint32_t) * (size_t)a->V));
  HGX_TRY(hgx_ensure(ctx, a->mp_cum, sizeof(int32_t) * (size_t)a->V));
  a->mp_vocab = false;
  HGX_HIP(ctx, hipMemcpyAsync(a->mp_keep.p, keep, sizeof(uint32_t) * (size_t)a->V,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipMemcpyAsync(a->mp_cum.p, cum, sizeof(int32_t) * (size_t)a->V,
                              hipMemcpyHostToDevice, ctx->stream));
  HGX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  a->mp_typed = typed;
  a->mp_last_node = (uint32_t)cum[a->N - 1];
  a->mp_last_edge = (uint32_t)cum[a->V - 1];
  a->mp_vocab = true;
  return HGX_OK;
}

extern "C" int hgx_n2v_train_mp(hgx_n2v *a, int64_t n_src, const int32_t *sources, int num_walks,
                                int L, int window, int negative, int epochs, float alpha,
                                float min_alpha, uint64_t walk_seed, uint64_t train_seed,
                                int concurrent) {
  if (!a) return HGX_EINVAL;
  hgx_ctx *ctx = a->ctx;
  const char *fn = "hgx_n2v_train_mp";
  HGX_TRY(n2v_live(a));
  HGX_CHECK(ctx, a->graph == 0, HGX_ESTATE, "%s: the engine is not on the bipartite graph", fn);
  HGX_CHECK(ctx, window >= 1 && epochs >= 0 && negative >= 0, HGX_EINVAL,
            "%s: window %d, epochs %d or negative %d out of range", fn, window, epochs, negative);
  HGX_CHECK(ctx, concurrent == 0 || concurrent == 1, HGX_EINVAL, "%s: concurrent %d is not 0 or 1",
            fn, concurrent);
  HGX_CHECK(ctx, negative <= kMaxNeg, HGX_EUNSUP, "%s: negative %d above %d", fn, negative,
            kMaxNeg);
  const int chunk = mp_chunk(a, !concurrent);
  int nw = 0;
  HGX_TRY(mp_corpus(a, fn, n_src, sources, num_walks, L, chunk, &nw));
  HGX_CHECK(ctx, (int64_t)std::min<int64_t>(2 * (int64_t)window + 1, L) * negative <= kMpStage,
            HGX_EUNSUP, "%s: window %d with %d negatives stages more than %d negatives per word",
            fn, window, negative, kMpStage);
  HGX_CHECK(ctx, a->mp_vocab, HGX_ESTATE, "%s before hgx_n2v_set_vocab_typed", fn);
  HGX_CHECK(ctx, a->vectors, HGX_ESTATE, "%s before hgx_n2v_set_vectors", fn);
  HGX_TRY(hgx_ensure(ctx, a->mp_stats, sizeof(unsigned long long) * kMpStat * kStatSlots));
  if (a->mp_ev.empty()) {
    a->mp_ev.assign(2 * kMpEvPairs, nullptr);
    for (hipEvent_t &e : a->mp_ev) HGX_HIP(ctx, hipEventCreate(&e));
  }
  MpArgs A;
  A.syn0 = a->syn0.as<float>();
  A.syn1 = a->syn1.as<float>();
  A.walks = a->mp_walks.as<int>();
  A.keep = a->mp_keep.as<unsigned>();
  A.cum = a->mp_cum.as<int>();
  A.stats = a->mp_stats.as<unsigned long long>();
  A.dp = a->dp;
  A.L = L;
  A.V = a->V;
  A.N = a->N;
  A.window = window;
  A.negative = negative;
  A.epochs = epochs;
  A.typed = a->mp_typed;
  A.n_walks = nw;
  A.last_node = a->mp_last_node;
  A.last_edge = a->mp_last_edge;
  A.seed = train_seed;
  A.alpha = (double)alpha;
  A.min_alpha = (double)min_alpha;
  const int npl = a->dp / 64;
  const MpFn kern = concurrent ? mp_kernel<true>(npl) : mp_kernel<false>(npl);
  HGX_HIP(ctx, hipMemsetAsync(a->mp_stats.p, 0, a->mp_stats.bytes, ctx->stream));
  HGX_HIP(ctx, hipEventRecord(a->e0, ctx->stream));
  // per chunk: the walks into the chunk buffer, then the trainer over them.
  // The stream orders the two, and the next chunk's walks after the trainer.
  // The walk kernels are timed by a ring of event pairs, read kMpEvPairs
  // chunks later so that the host does not wait on the chunk in flight.
  double walk_ms = 0;
  int64_t launched = 0;
  auto collect = [&](int slot) -> int {
    float t = 0.f;
    HGX_HIP(ctx, hipEventSynchronize(a->mp_ev[2 * slot + 1]));
    HGX_HIP(ctx, hipEventElapsedTime(&t, a->mp_ev[2 * slot], a->mp_ev[2 * slot + 1]));
    walk_ms += t;
    return HGX_OK;
  };
  for (int ep = 0; ep < epochs; ep++)
    for (int64_t g0 = 0; g0 < nw; g0 += chunk) {
      const int n = (int)std::min<int64_t>(chunk, nw - g0);
      const int slot = (int)(launched % kMpEvPairs);
      if (launched >= kMpEvPairs) HGX_TRY(collect(slot));
      HGX_HIP(ctx, hipEventRecord(a->mp_ev[2 * slot], ctx->stream));
      HGX_TRY(mp_generate(a, (int)g0, n, (int)n_src, L, walk_seed));
      HGX_HIP(ctx, hipEventRecord(a->mp_ev[2 * slot + 1], ctx->stream));
      hipLaunchKernelGGL(kern, dim3(concurrent ? (n + 3) / 4 : 1), dim3(concurrent ? 256 : 64), 0,
                         ctx->stream, A, ep, (int)g0, (int)g0 + n);
      HGX_LAUNCH_CHECK(ctx);
      launched++;
    }
  double total_ms = 0;
  HGX_TRY(n2v_elapsed(a, &total_ms));
  for (int64_t i = std::max<int64_t>(0, launched - kMpEvPairs); i < launched; i++)
    HGX_TRY(collect((int)(i % kMpEvPairs)));
  a->walk_ms = walk_ms;
  a->train_ms = std::max(0.0, total_ms - walk_ms);
  unsigned long long st[kMpStat * kStatSlots];
  HGX_HIP(ctx, hipMemcpy(st, a->mp_stats.p, sizeof(st), hipMemcpyDeviceToHost));
  a->st_mp_words = a->st_mp_pairs = a->st_mp_targets = a->st_mp_clamped = 0;
  for (int i = 0; i < kStatSlots; i++) {
    a->st_mp_words += (int64_t)st[kMpStat * i];
    a->st_mp_pairs += (int64_t)st[kMpStat * i + 1];
    a->st_mp_targets += (int64_t)st[kMpStat * i + 2];
    a->st_mp_clamped += (int64_t)st[kMpStat * i + 3];
  }
  a->st_mp_walks = (int64_t)nw * epochs;
  a->st_walks = a->st_mp_walks;
  a->st_words = a->st_mp_words;
  a->st_pairs = a->st_mp_pairs;
  a->st_path_nodes = 0;
  a->st_line_samples = a->st_line_targets = a->st_line_clamped = 0;
  return HGX_OK;
}

extern "C" int hgx_n2v_last_mp_stats(const hgx_n2v *a, int64_t *walks, int64_t *words,
                                     int64_t *pairs, int64_t *targets, int64_t *clamped) {
  if (!a) return HGX_EINVAL;
  if (walks) *walks = a->st_mp_walks;
  if (words) *words = a->st_mp_words;
  if (pairs) *pairs = a->st_mp_pairs;
  if (targets) *targets = a->st_mp_targets;
  if (clamped) *clamped = a->st_mp_clamped;
  return HGX_OK;
}
