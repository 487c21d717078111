"""Weighted-Jaccard test cases: planted graphs, labelled rows and pairs,
feature sets, a float64 reference, the float32 error bound of a correct
result, the restated branch selection of hgx_jaccard.hip, exact-property
checkers and named wrong variants of the reference (CPU only; used by
test_jaccard_cases_cpu.py and test_gpu_jaccard_kernels.py).

What is computed (hg2v_sample.py:250-326, :395-510). node2features is N x E
and edge2features E x N, both on the incidence pattern (fn in A's CSR order,
fe in A^T's). The node centroid of v is the mean over e in E(v) of
edge2features[e] (N rows over N columns), the edge centroid of e the mean
over v in N(e) of node2features[v] (E rows over E columns), zeros dropped.
SWJ(x, y) = sum min / sum max over the union of the supports, 0 if the
denominator is 0. nn / ee pairs are SWJ of two feature rows; a node-edge
pair (v, e) is SWJ(node2features[v], edge centroid[e]) *
SWJ(edge2features[e], node centroid[v]).

Cases (``case(name)``), each an Incidence with .rows (label -> (side, row),
side 0 = node centroids, 1 = edge centroids), .pairs (kind -> [(a, b,
label)]) and .plants ((which, row, col, value): planted feature values,
value 0 a stored zero; applied in the two ranges that hold zeros):

  small     300 x 40, random, degree 0 ... 6. The sampler, state and
            numpy-seeded tests and the call of PAIRS_LOOP pairs run on it.
  planted   2400 x 20. Edge 0 empty, edge 1 one member, edges 2 ... 5 of
            255, 256, 257 and 600 members (the feature rows of the z += 256
            loop), node 12 in all four (degree many; a centroid row of up to 1365
            entries); 20 columns on the edge side (one partial bitmap word,
            fewer rows than workgroups), 2400 rows on the node side (1024
            workgroups: some workgroup takes a third row). Edge 6 = nodes
            32 ... 95, 100, 101 with stored zeros at 40, 41 (dropped between
            kept columns of word 1) and 64 ... 95 (word 2 dropped whole);
            edge 7 repeats the zeros at 40 and 64 ... 70 so node 100 (degree
            2) has them as zero means too, and stores a zero at 42 where
            edge 6 has a value. Nodes 1 ... 11 carry the swj
            plants (see _planted).
  c8192     8193 x 8192: one compaction pass on the edge side (256 words),
            two on the node side (the second holds column 8192 alone, which
            node 0's row keeps last); an edge whose four members sit in the
            four waves of pass 1.
  c3pass    16,390 x 1500: three passes. Edge 0 = {10, 5000, 16385, 16389}:
            kept columns in passes 1 and 3 only, the last one the last
            column. Edge 1 = {100, 2148, 4196, 6244}: all four waves.
  rows70k   70,001 x 9000, node degree 0 ... 2: compact_rows strides over
            rows beyond 65,536; nine passes on the node side.
  shrink    N_SHRINK x about 0.7 N, every degree <= 2 (a random path with
            30 % of its links removed): build_centroids halves its 1024
            workgroups. N_SHRINK is the smallest N for which
            1024 * (4 N + 4 ceil(N / 32)) > 2e9 (the expression of
            build_centroids, hgx_jaccard.hip:260-261): 4 N + 4 ceil(N / 32)
            > 1,953,125, N + ceil(N / 32) >= 488,282, and N = 473,485 gives
            473,485 + 14,797 = 488,282 while 473,484 gives 488,281.
  fill_big  1110 x 6: edge 0 holds 1100 nodes, so node quotas of 1000 give
            1.1M node-node records (jac_fill's grid stride; i * R in 64
            bits).

Features (``features``). float32 per incidence, independent for fn and fe:
"ones" (UniformWeight), "small" in [0.01, 1), "big" in [1, 1000); the last
two with 5 % exact zeros and the case's plants. Every non-zero value is at
least 2^-20 (asserted), so that a float32 mean of at most 2^20 terms cannot
underflow to 0 and the support of the float32 centroid is that of the
exact one.

Reference (``ref_centroids``, ``ref_probs``, ``swj64``), float64 scipy /
numpy, does not call oracle/hgref.c: centroid = (pattern @ features) /
degree with zeros eliminated; probability = sum min / sum max over the
union (scipy's elementwise minimum / maximum of the two row blocks), 0 when
the denominator is 0; kind 2 the product of the two. ``swj64`` is the same
for one pair in plain numpy and takes the wrong variants.

Bound (``gamma``; nothing measured). u = 2^-24, gamma(k) = k u / (1 - k u).
Every term is non-negative, so relative errors only add:
  * a centroid entry is a sum of at most len terms (len - 1 additions) and
    one division: within gamma(len) c of c, len the row's degree;
  * an nn / ee probability is two sums of at most n terms (n - 1 additions
    each; n the size of the union of the non-zero supports, adding a zero
    being exact) and one division: a quotient of (1 + theta_{n-1}) factors
    times (1 + delta), within gamma(2 n - 1) p <= gamma(2 n + 1) p;
  * a kind-2 factor has one operand whose entries already carry
    gamma(len): min and max are monotone, so the sums carry len + n - 1 and
    the factor gamma(2 n + 2 len + 1) p, len the degree behind its centroid
    operand; the product's k is the sum of the two factors' k plus 1;
  * where the reference is 0 the bound is 0: the result must be exactly 0.

Branch selection restated (``swj_branches``, ``centroid_branches``,
``workgroups``): swj :41-61, centroid_rows :86-133 (the z += 256 loop, the
bitmap passes of 256 words, four waves of 64 words each), build_centroids
:260-261, compact_rows :161-166. REQUIRED_BRANCHES lists every label the
CPU test must find reached by some case and range.

Wrong variants (VARIANTS): see there.
"""

import numpy as np
import scipy.sparse as sp

from hypergraphembedding_amd.hypergraph_util import Incidence

U = 2.0 ** -24
RANGES = ("ones", "small", "big")
NN, EE, NE = 0, 1, 2
PASS_COLS = 8192        # 256 words of 32 columns, hgx_jaccard.hip:101
WAVE_COLS = 2048        # 64 words
PAIRS_LOOP = 1048576 + 300   # one jac_pairs call beyond 4096 x 256 items
FILL_LOOP = 1048576          # a record block must exceed this
MIN_NONZERO = 2.0 ** -20


def workgroups(ncols):
  """build_centroids, hgx_jaccard.hip:259-261."""
  nwords = (ncols + 31) // 32
  nwg = 1024
  while nwg > 32 and float(nwg) * (float(ncols) * 4 + nwords * 4) > 2e9:
    nwg //= 2
  return nwg


def _n_shrink():
  n = int(2e9 / 1024 / 4.125) - 64
  while workgroups(n) == 1024:
    n += 1
  return n


N_SHRINK = _n_shrink()
assert N_SHRINK == 473485 and workgroups(N_SHRINK - 1) == 1024
assert workgroups(N_SHRINK) == 512


def gamma(k):
  k = np.asarray(k, np.float64)
  return k * U / (1 - k * U)


# ---- cases --------------------------------------------------------------------

def _incidence(N, E, pairs):
  pairs = np.unique(np.asarray(pairs, np.int64).reshape(-1, 2), axis=0)
  assert pairs[:, 0].max() < N and pairs[:, 1].max() < E
  rp = np.zeros(N + 1, np.int64)
  np.add.at(rp, pairs[:, 0] + 1, 1)
  inc = Incidence(N, E, np.cumsum(rp), pairs[:, 1])
  inc.rows, inc.plants = {}, []
  inc.pairs = {NN: [], EE: [], NE: []}
  return inc


def _random_pairs(rng, nodes, lo_edge, hi_edge, degs):
  """(node, edge) pairs: node i in degs[i] random edges of [lo, hi)."""
  out = []
  for d in range(1, int(degs.max()) + 1):
    v = nodes[degs >= d]
    out.append(np.stack([v, rng.integers(lo_edge, hi_edge, v.size)], 1))
  return np.concatenate(out)


def _small():
  rng = np.random.default_rng(31)
  N, E = 300, 40
  degs = rng.integers(0, 7, N)
  degs[:4] = (0, 1, 1, 6)
  inc = _incidence(N, E, _random_pairs(rng, np.arange(N), 1, E, degs))
  # edge 0 is empty, node 0 isolated
  inc.pairs[NE] = [(0, 5, "ne_empty_centroid"), (3, 0, "ne_empty_centroid")]
  return inc


PLANTED_NODES = {
    # node: {edge: value}; value 0 is a stored zero
    0: {1: 1, 8: 2, 9: 0, 10: 3},
    1: {8: 3, 10: 1, 12: 2},      # A
    2: {9: 1, 10: 2, 13: 1},      # B
    3: {10: 1, 11: 2, 12: 3},     # C
    4: {10: 2, 11: 1, 12: 3},     # D
    5: {8: 0, 9: 0},              # Y1: all stored values zero
    6: {9: 0, 11: 0},             # Y2
    7: {8: 1, 9: 2},              # F
    8: {14: 2, 15: 1},            # G: disjoint from F
    9: {8: 1, 10: 0, 12: 2},      # H: a stored zero where A has a value
}
PLANTED_EMPTY = (10, 11)          # Z, Z2: degree 0
PLANTED_HUB = 12                  # in edges 2, 3, 4, 5
EDGE_SIZES = {2: 255, 3: 256, 4: 257, 5: 600}


def _planted():
  rng = np.random.default_rng(32)
  E = 20
  pairs, plants = [], []
  for v, row in PLANTED_NODES.items():
    for e, val in row.items():
      pairs.append((v, e))
      plants.append(("fn", v, e, val))
  e6 = list(range(32, 96)) + [100, 101]
  e7 = [40, 42] + list(range(64, 71)) + [100, 101]
  zero6 = {40, 41} | set(range(64, 96))
  zero7 = {40, 42} | set(range(64, 71))
  for v in e6:
    pairs.append((v, 6))
    plants.append(("fe", 6, v, 0 if v in zero6 else 1 + v % 3))
  for v in e7:
    pairs.append((v, 7))
    plants.append(("fe", 7, v, 0 if v in zero7 else 1 + v % 2))
  plants.append(("fe", 1, 0, 2))
  nxt = 120
  for e, size in EDGE_SIZES.items():
    pairs.append((PLANTED_HUB, e))
    pairs += [(v, e) for v in range(nxt, nxt + size - 1)]
    nxt += size - 1
  pool = np.arange(nxt, 2400)
  degs = rng.choice([1, 2, 3], pool.size, p=[0.7, 0.2, 0.1])
  pairs += _random_pairs(rng, pool, 8, E, degs).tolist()
  inc = _incidence(2400, E, pairs)
  inc.plants = plants
  inc.first_private = {e: 120 + sum(s - 1 for f, s in EDGE_SIZES.items() if f < e)
                       for e in EDGE_SIZES}
  inc.rows = {"cen_deg0_node": (0, 10), "cen_deg1_node": (0, 33),
              "cen_deg_many_node": (0, PLANTED_HUB), "cen_zero_mean_many": (0, 100),
              "cen_deg0_edge": (1, 0), "cen_deg1_edge": (1, 1),
              "cen_deg_many_edge": (1, 5)}
  A, B, C, D, Y1, Y2, F, G, H, Z, Z2 = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
  inc.pairs[NN] = [
      (A, B, "swj_left_only"), (A, B, "swj_right_only"), (A, B, "swj_tail_right"),
      (B, A, "swj_tail_left"), (C, D, "swj_match_lt"), (C, D, "swj_match_gt"),
      (C, D, "swj_match_eq"), (A, H, "swj_stored_zero"),
      (A, Z, "swj_one_empty"), (Z, A, "swj_one_empty"),
      (Z, Z2, "swj_both_empty"), (Z, Z, "swj_both_empty"),
      (Y1, Y2, "swj_all_zero"), (Y1, Y1, "swj_all_zero"),
      (A, A, "swj_same"), (PLANTED_HUB, PLANTED_HUB, "swj_same"),
      (F, G, "swj_disjoint"), (G, F, "swj_disjoint")]
  inc.pairs[EE] = [
      (2, 3, "swj_left_only"), (3, 2, "swj_right_only"), (5, 5, "swj_same"),
      (1, 1, "swj_same"), (0, 5, "swj_one_empty"), (5, 0, "swj_one_empty"),
      (0, 0, "swj_both_empty"), (6, 7, "swj_stored_zero"), (6, 2, "swj_disjoint")]
  inc.pairs[NE] = [
      (Z, 8, "ne_empty_centroid"), (A, 0, "ne_empty_centroid"),
      (Z, 0, "ne_empty_centroid"), (A, 8, "ne_node_in_edge"),
      (A, 9, "ne_node_not_in_edge"), (C, 10, "ne_node_in_edge"),
      (C, 8, "ne_node_not_in_edge"), (PLANTED_HUB, 5, "ne_node_in_edge"),
      (100, 6, "ne_node_in_edge"), (33, 7, "ne_node_not_in_edge")]
  return inc


def _c8192():
  rng = np.random.default_rng(33)
  N, E = 8193, 8192
  four = (100, 2148, 4196, 6244)
  nodes = np.setdiff1d(np.arange(1, N - 1), four)
  degs = rng.choice([0, 1, 2, 3], nodes.size, p=[0.05, 0.5, 0.3, 0.15])
  pairs = _random_pairs(rng, nodes, 6, E - 1, degs).tolist()
  pairs += [(N - 1, E - 1), (N - 1, 0), (0, 0), (0, E - 1)]
  pairs += [(v, 5) for v in four]
  inc = _incidence(N, E, pairs)
  inc.rows = {"cen_last_col_node": (0, 0), "cen_last_col_edge": (1, 0),
              "cen_four_waves": (0, four[0])}
  inc.pairs[NE] = [(0, 0, "ne_node_in_edge"), (four[0], 0, "ne_node_not_in_edge"),
                   (0, 1, "ne_empty_centroid")]
  return inc


def _c3pass():
  rng = np.random.default_rng(34)
  N, E = 16390, 1500
  e0 = (10, 5000, 16385, 16389)
  four = (100, 2148, 4196, 6244)
  nodes = np.setdiff1d(np.arange(N), e0 + four)
  degs = rng.choice([0, 1, 2, 3], nodes.size, p=[0.05, 0.5, 0.3, 0.15])
  pairs = _random_pairs(rng, nodes, 2, E, degs).tolist()
  pairs += [(v, 0) for v in e0] + [(v, 1) for v in four]
  inc = _incidence(N, E, pairs)
  inc.rows = {"cen_pass_1_and_3_only": (0, 10), "cen_last_col_node": (0, 10),
              "cen_four_waves": (0, 100)}
  for which, e, members in (("fe", 0, e0), ("fe", 1, four)):
    inc.plants += [(which, e, v, 1 + v % 3) for v in members]
  inc.pairs[NE] = [(10, 0, "ne_node_in_edge"), (10, 1, "ne_node_not_in_edge")]
  return inc


def _rows70k():
  rng = np.random.default_rng(35)
  N, E = 70001, 9000
  degs = rng.choice([0, 1, 2], N, p=[0.02, 0.58, 0.4])
  degs[N - 1] = 2
  return _incidence(N, E, _random_pairs(rng, np.arange(N), 0, E, degs))


def _shrink():
  rng = np.random.default_rng(36)
  N = N_SHRINK
  perm = rng.permutation(N)
  keep = np.flatnonzero(rng.random(N - 1) < 0.7)
  e = np.arange(keep.size)
  one = rng.random(keep.size) < 0.1       # an edge of one member
  pairs = np.concatenate([np.stack([perm[keep], e], 1),
                          np.stack([perm[keep + 1], e], 1)[~one]])
  inc = _incidence(N, keep.size, pairs)
  assert inc.node_degree().max() <= 2 and inc.edge_size().max() <= 2
  return inc


def _fill_big():
  rng = np.random.default_rng(37)
  N, E = 1110, 6
  pairs = [(v, 0) for v in range(1100)]
  pairs += _random_pairs(rng, np.arange(1090, N), 1, E, np.full(20, 2)).tolist()
  return _incidence(N, E, pairs)


_BUILD = dict(small=_small, planted=_planted, c8192=_c8192, c3pass=_c3pass,
              rows70k=_rows70k, shrink=_shrink, fill_big=_fill_big)
CASES = ("small", "planted", "c8192", "c3pass", "rows70k")   # shared Context
LARGE = "shrink"
_CASE = {}


def case(name):
  if name not in _CASE:
    inc = _BUILD[name]()
    inc.name = name
    _CASE[name] = inc
  return _CASE[name]


def _find(rp, col, r, c):
  i = int(rp[r] + np.searchsorted(col[rp[r]:rp[r + 1]], c))
  assert col[i] == c, (r, c)
  return i


def features(inc, rng_name):
  """(fn, fe) float32 of one range (module docstring)."""
  nnz = inc.nnz
  if rng_name == "ones":
    return np.ones(nnz, np.float32), np.ones(nnz, np.float32)
  lo, hi, scale = (0.01, 1.0, 0.1) if rng_name == "small" else (1.0, 1000.0, 100.0)
  rng = np.random.default_rng([11, RANGES.index(rng_name), nnz])
  out = []
  for which in ("fn", "fe"):
    f = rng.uniform(lo, hi, nnz).astype(np.float32)
    f = np.clip(f, np.float32(lo), np.nextafter(np.float32(hi), np.float32(0)))
    f[rng.random(nnz) < 0.05] = 0
    rp, col = (inc.rp_n, inc.col_n) if which == "fn" else (inc.rp_e, inc.col_e)
    for w, r, c, val in inc.plants:
      if w == which:
        f[_find(rp, col, r, c)] = np.float32(val * scale)
    assert np.isfinite(f).all() and np.all((f == 0) | (f >= MIN_NONZERO))
    assert np.all(f < hi) and np.all((f == 0) | (f >= np.float32(lo)))
    out.append(f)
  return out[0], out[1]


def labelled_pairs(inc, kind):
  p = inc.pairs[kind]
  return (np.array([q[0] for q in p], np.int32),
          np.array([q[1] for q in p], np.int32), [q[2] for q in p])


def pair_arrays(inc, kind, n_random):
  """The labelled pairs followed by n_random random ones (fixed seed)."""
  a, b, lab = labelled_pairs(inc, kind)
  rng = np.random.default_rng([41, kind, inc.N])
  na = inc.E if kind == EE else inc.N
  nb = inc.N if kind == NN else inc.E
  ra = rng.integers(0, na, n_random).astype(np.int32)
  rb = rng.integers(0, nb, n_random).astype(np.int32)
  if kind != NE:  # a fifth of them within two hops, so that they intersect
    rp, col = (inc.rp_n, inc.col_n) if kind == NN else (inc.rp_e, inc.col_e)
    rp2, col2 = (inc.rp_e, inc.col_e) if kind == NN else (inc.rp_n, inc.col_n)
    for q in range(0, n_random, 5):
      r = ra[q]
      if rp[r + 1] > rp[r]:
        t = col[rng.integers(rp[r], rp[r + 1])]
        rb[q] = col2[rng.integers(rp2[t], rp2[t + 1])]
  else:  # a fifth of them incidences
    t = rng.integers(0, inc.nnz, len(range(0, n_random, 5)))
    row_n = np.repeat(np.arange(inc.N), np.diff(inc.rp_n))
    ra[::5], rb[::5] = row_n[t], inc.col_n[t]
  return (np.concatenate([a, ra]), np.concatenate([b, rb]),
          lab + ["random"] * n_random)


# ---- float64 reference --------------------------------------------------------

def _mats(inc, fn, fe, width=None):
  fn, fe = np.asarray(fn, np.float64), np.asarray(fe, np.float64)
  wn, we = (inc.E, inc.N) if width is None else (width, width)
  xn = sp.csr_matrix((fn, inc.col_n, inc.rp_n), shape=(inc.N, wn))
  xe = sp.csr_matrix((fe, inc.col_e, inc.rp_e), shape=(inc.E, we))
  return xn, xe


def _pattern(x):
  return sp.csr_matrix((np.ones(x.data.size), x.indices, x.indptr), shape=x.shape)


def _side(inc, which, fn, fe):
  """(R, rp, col, frp, fcol, fval, ncols) of build_centroids' two calls."""
  if which == 0:
    return inc.N, inc.rp_n, inc.col_n, inc.rp_e, inc.col_e, fe, inc.N
  return inc.E, inc.rp_e, inc.col_e, inc.rp_n, inc.col_n, fn, inc.E


def centroid_args(inc, which, fn, fe):
  """The arguments of oracle.centroids for one side."""
  R, rp, col, frp, fcol, fval, ncols = _side(inc, which, fn, fe)
  return R, rp, col, ncols, frp, fcol, fval


def ref_centroids(inc, which, fn, fe, variant=None):
  """(p int64, j int32, v float64) of the node (0) / edge (1) centroids:
  (pattern @ features) / degree, zeros eliminated. variant: by_contributors
  or zero_kept."""
  R, rp, col, frp, fcol, fval, ncols = _side(inc, which, fn, fe)
  T = frp.size - 1
  pat = sp.csr_matrix((np.ones(col.size), col, rp), shape=(R, T))
  f = sp.csr_matrix((np.asarray(fval, np.float64), fcol, frp), shape=(T, ncols))
  cand = (pat @ _pattern(f)).tocsr()      # contributors per candidate column
  cand.sort_indices()
  s = (pat @ f).tocsr()
  s.sort_indices()
  # the sums on the candidates' pattern (a product may or may not store an
  # exact zero)
  key = lambda m: (np.repeat(np.arange(R, dtype=np.int64), np.diff(m.indptr))
                   * ncols + m.indices)
  val = np.zeros(cand.data.size)
  val[np.searchsorted(key(cand), key(s))] = s.data
  deg = np.repeat(np.diff(rp).astype(np.float64), np.diff(cand.indptr))
  val = val / (cand.data if variant == "by_contributors" else deg)
  c = sp.csr_matrix((val, cand.indices, cand.indptr), shape=(R, ncols))
  if variant != "zero_kept":
    c.eliminate_zeros()
  return c.indptr.astype(np.int64), c.indices.astype(np.int32), c.data.copy()


def candidates(inc, which, fn, fe):
  """(p, j) of every column a centroid row touches (the bitmap's bits)."""
  return ref_centroids(inc, which, fn, fe, "zero_kept")[:2]


def centroid_bound(inc, which, p, v64):
  R, rp = (inc.N, inc.rp_n) if which == 0 else (inc.E, inc.rp_e)
  return gamma(np.repeat(np.diff(rp), np.diff(p))) * v64


def _swj_blocks(x, y):
  """Rowwise sum min / sum max of two CSR blocks, and the union size."""
  num = np.asarray(x.minimum(y).sum(1)).ravel()
  mx = x.maximum(y).tocsr()
  mx.eliminate_zeros()
  den = np.asarray(mx.sum(1)).ravel()
  p = np.divide(num, den, out=np.zeros_like(num), where=den > 0)
  return p, np.diff(mx.indptr)


class Reference:
  """The float64 reference of one case and feature set; built once."""

  def __init__(self, inc, fn, fe, wrong_side=False):
    self.inc = inc
    w = max(inc.N, inc.E) if wrong_side else None
    self.xn, self.xe = _mats(inc, fn, fe, w)
    self.cen = [ref_centroids(inc, 0, fn, fe), ref_centroids(inc, 1, fn, fe)]
    wn, we = (inc.N, inc.E) if w is None else (w, w)
    self.cn = sp.csr_matrix((self.cen[0][2], self.cen[0][1], self.cen[0][0]),
                            shape=(inc.N, wn))
    self.ce = sp.csr_matrix((self.cen[1][2], self.cen[1][1], self.cen[1][0]),
                            shape=(inc.E, we))
    self.wrong_side = wrong_side

  def probs(self, kind, a, b):
    """(float64 probabilities, k of the bound gamma(k) p) of the pairs."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if a.size == 0:
      return np.zeros(0), np.zeros(0)
    if kind == NN:
      p, n = _swj_blocks(self.xn[a], self.xn[b])
      return p, 2 * n + 1
    if kind == EE:
      p, n = _swj_blocks(self.xe[a], self.xe[b])
      return p, 2 * n + 1
    inc = self.inc
    if self.wrong_side:   # each factor against its own side's centroid
      pn, n1 = _swj_blocks(self.xn[a], self.cn[a])
      pe, n2 = _swj_blocks(self.xe[b], self.ce[b])
    else:
      pn, n1 = _swj_blocks(self.xn[a], self.ce[b])
      pe, n2 = _swj_blocks(self.xe[b], self.cn[a])
    k1 = 2 * n1 + 2 * np.diff(inc.rp_e)[b] + 1
    k2 = 2 * n2 + 2 * np.diff(inc.rp_n)[a] + 1
    return pn * pe, k1 + k2 + 1

  def bound(self, kind, a, b):
    p, k = self.probs(kind, a, b)
    return p, gamma(k) * p


def swj64(ac, av, bc, bv, variant=None):
  """One pair in plain numpy: sum min / sum max over the union of the two
  sorted sparse rows. variant: intersection, tail_dropped."""
  ac, bc = np.asarray(ac, np.int64), np.asarray(bc, np.int64)
  cols = np.union1d(ac, bc)
  x, y = np.zeros(cols.size), np.zeros(cols.size)
  x[np.searchsorted(cols, ac)] = av
  y[np.searchsorted(cols, bc)] = bv
  keep = np.ones(cols.size, bool)
  if variant == "intersection":
    keep = np.isin(cols, ac) & np.isin(cols, bc)
  elif variant == "tail_dropped":
    last = min(ac[-1], bc[-1]) if ac.size and bc.size else -1
    keep = cols <= last
  num, den = np.minimum(x, y)[keep].sum(), np.maximum(x, y)[keep].sum()
  return num / den if den > 0 else 0.0


def row_of(inc, kind_side, r, fn, fe):
  """(columns, values) of node2features[r] (0) / edge2features[r] (1)."""
  rp, col, f = (inc.rp_n, inc.col_n, fn) if kind_side == 0 else (inc.rp_e, inc.col_e, fe)
  return col[rp[r]:rp[r + 1]], np.asarray(f[rp[r]:rp[r + 1]], np.float64)


def pair_prob64(inc, ref, kind, a, b, fn, fe, variant=None):
  """One pair through swj64 (the centroids from ref)."""
  if kind in (NN, EE):
    return swj64(*row_of(inc, kind, a, fn, fe), *row_of(inc, kind, b, fn, fe),
                 variant=variant)
  cen = lambda w, r: (ref.cen[w][1][ref.cen[w][0][r]:ref.cen[w][0][r + 1]],
                      ref.cen[w][2][ref.cen[w][0][r]:ref.cen[w][0][r + 1]])
  return (swj64(*row_of(inc, 0, a, fn, fe), *cen(1, b), variant=variant)
          * swj64(*row_of(inc, 1, b, fn, fe), *cen(0, a), variant=variant))


# ---- branch selection, restated -------------------------------------------------

SWJ_BRANCHES = ["swj_left_only", "swj_right_only", "swj_match_lt",
                "swj_match_gt", "swj_match_eq", "swj_tail_left",
                "swj_tail_right", "swj_one_empty", "swj_both_empty",
                "swj_all_zero", "swj_same", "swj_disjoint", "swj_stored_zero"]
CENTROID_BRANCHES = ["cen_deg0", "cen_deg1", "cen_deg_many", "cen_frow_255",
                     "cen_frow_256", "cen_frow_257", "cen_frow_gt512",
                     "cen_cols_le32", "cen_cols_8192", "cen_cols_8193",
                     "cen_cols_3pass", "cen_pass_1_and_3_only",
                     "cen_four_waves", "cen_last_col", "cen_zero_between",
                     "cen_zero_word", "cen_rows_gt2048", "cen_rows_lt_wg",
                     "cen_row_gt64", "cen_rows_gt65536", "cen_wg_shrink"]
NE_BRANCHES = ["ne_empty_centroid", "ne_node_not_in_edge", "ne_node_in_edge"]
REQUIRED_BRANCHES = SWJ_BRANCHES + CENTROID_BRANCHES + NE_BRANCHES
# labels that need feature values other than 1 (asserted per labelled pair
# in the ranges "small" and "big" only)
NEEDS_VALUES = {"swj_match_lt", "swj_match_gt", "swj_all_zero", "swj_stored_zero"}


def swj_branches(ac, av, bc, bv):
  """The branches swj (hgx_jaccard.hip:37-62) takes on two sorted sparse
  rows, and its float32 result computed the same way."""
  f = np.float32
  na, nb = len(ac), len(bc)
  seen = set()
  num = den = f(0)
  i = j = 0
  matched = False
  while i < na or j < nb:
    if j >= nb or (i < na and ac[i] < bc[j]):
      seen.add("swj_tail_left" if j >= nb and nb else "swj_left_only" if nb else "")
      x, y = f(av[i]), f(0)
      i += 1
    elif i >= na or bc[j] < ac[i]:
      seen.add("swj_tail_right" if i >= na and na else "swj_right_only" if na else "")
      x, y = f(0), f(bv[j])
      j += 1
    else:
      x, y = f(av[i]), f(bv[j])
      matched = True
      seen.add("swj_match_lt" if x < y else "swj_match_gt" if x > y else "swj_match_eq")
      if (x == 0) != (y == 0):
        seen.add("swj_stored_zero")
      i += 1
      j += 1
    if x < y:
      num, den = f(num + x), f(den + y)
    else:
      num, den = f(num + y), f(den + x)
  seen.discard("")
  if na == 0 and nb == 0:
    seen.add("swj_both_empty")
  elif na == 0 or nb == 0:
    seen.add("swj_one_empty")
  elif den == 0:
    seen.add("swj_all_zero")
  if na and nb and not matched and den > 0:
    seen.add("swj_disjoint")
  if na and na == nb and np.array_equal(ac, bc) and np.array_equal(av, bv) and den > 0:
    seen.add("swj_same")
  return seen, (f(0) if den == 0 else f(num / den))


def centroid_branches(inc, which, fn, fe, ref_cen):
  """Labels of CENTROID_BRANCHES that build_centroids / centroid_rows /
  compact_rows reach on one side (ref_cen: that side's reference CSR)."""
  R, rp, col, frp, fcol, fval, ncols = _side(inc, which, fn, fe)
  p, j, _ = ref_cen
  seen = set()
  deg = np.diff(rp)
  seen |= {l for l, ok in (("cen_deg0", (deg == 0).any()), ("cen_deg1", (deg == 1).any()),
                           ("cen_deg_many", (deg > 2).any())) if ok}
  flen = np.diff(frp)[col]          # the feature rows the z += 256 loop reads
  for l, ok in (("cen_frow_255", 255 in flen), ("cen_frow_256", 256 in flen),
                ("cen_frow_257", 257 in flen), ("cen_frow_gt512", (flen > 512).any()),
                ("cen_cols_le32", ncols <= 32 and ncols % 32 != 0),
                ("cen_cols_8192", ncols == PASS_COLS),
                ("cen_cols_8193", ncols == PASS_COLS + 1),
                ("cen_cols_3pass", ncols >= 2 * PASS_COLS + 1),
                ("cen_rows_gt2048", R > 2048), ("cen_rows_lt_wg", R < 1024),
                ("cen_rows_gt65536", R > 65536),
                ("cen_wg_shrink", workgroups(ncols) < 1024),
                ("cen_row_gt64", np.diff(p).max() > 64)):
    if ok:
      seen.add(l)
  row = np.repeat(np.arange(R, dtype=np.int64), np.diff(p))
  jj = j.astype(np.int64)
  has = np.diff(p) > 0
  if has.any():
    last = jj[p[1:][has] - 1]
    if (last == ncols - 1).any():
      seen.add("cen_last_col")
    start = p[:-1][has]
    mask = np.bitwise_or.reduceat(1 << np.minimum(jj // PASS_COLS, 40), start)
    if (mask == 0b101).any():
      seen.add("cen_pass_1_and_3_only")
    npass = -(-ncols // PASS_COLS)
    rpw = np.unique((row * npass + jj // PASS_COLS) * 4 + (jj % PASS_COLS) // WAVE_COLS)
    _, cnt = np.unique(rpw // 4, return_counts=True)
    if (cnt == 4).any():
      seen.add("cen_four_waves")
  # candidates that the mean drops
  cp, cj = candidates(inc, which, fn, fe)
  crow = np.repeat(np.arange(R, dtype=np.int64), np.diff(cp))
  nw = (ncols + 31) // 32
  ckey, kkey = crow * ncols + cj, row * ncols + jj
  dropped = ~np.isin(ckey, kkey)
  if dropped.any():
    kw = row * nw + jj // 32          # sorted: rows and columns ascend
    dw, dc = (crow * nw + cj // 32)[dropped], cj[dropped]
    lo, hi = np.searchsorted(kw, dw, "left"), np.searchsorted(kw, dw, "right")
    ok = hi > lo
    if np.any(ok & (jj[np.minimum(lo, jj.size - 1)] < dc)
              & (jj[np.maximum(hi - 1, 0)] > dc)):
      seen.add("cen_zero_between")
    words, cnt = np.unique(crow * nw + cj // 32, return_counts=True)
    full = words[cnt == 32]
    full = full[~np.isin(full, kw)]
    if np.any(has[full // nw]):
      seen.add("cen_zero_word")
  return seen


# ---- exact properties -----------------------------------------------------------

def bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_support(got_p, got_j, ref_p, ref_j, where=""):
  """The centroid's support is the float64 centroid's."""
  assert np.array_equal(got_p, ref_p), (where, "rowptr")
  assert np.array_equal(got_j, ref_j), (where, "columns")


def check_symmetric(fwd, rev, where=""):
  """nn / ee: p(a, b) and p(b, a) are the same float32."""
  assert np.array_equal(bits(fwd), bits(rev)), (where, "not symmetric")


def check_scale_invariant(base, scaled, where=""):
  """All features times a power of two: the same float32."""
  bad = np.flatnonzero(bits(base) != bits(scaled))
  assert bad.size == 0, (where, "rescaling moved", bad[:5], base[bad[:5]], scaled[bad[:5]])


def check_same_is_one(inc, kind, a, b, p, fn, fe, where=""):
  """a == b: exactly 1.0f when the row holds a non-zero value, else 0."""
  rp, f = (inc.rp_n, fn) if kind == NN else (inc.rp_e, fe)
  R = rp.size - 1
  nz = np.bincount(np.repeat(np.arange(R), np.diff(rp)), weights=(f != 0), minlength=R)
  same = np.flatnonzero(np.asarray(a) == np.asarray(b))
  want = np.where(nz[np.asarray(a)[same]] > 0, np.float32(1), np.float32(0))
  assert np.array_equal(bits(p[same]), bits(want)), where
  return same.size


def check_degree_one(inc, which, p, j, v, fn, fe, where=""):
  """A degree-1 row's centroid is that feature row bit for bit, minus its
  zeros. Returns the number of rows checked."""
  R, rp, col, frp, fcol, fval, _ = _side(inc, which, fn, fe)
  rows = np.flatnonzero(np.diff(rp) == 1)
  t = col[rp[rows]]
  src = np.concatenate([np.arange(frp[x], frp[x + 1]) for x in t]) if t.size else np.zeros(0, np.int64)
  src = src[fval[src] != 0]
  dst = np.concatenate([np.arange(p[r], p[r + 1]) for r in rows]) if rows.size else np.zeros(0, np.int64)
  assert src.size == dst.size, where
  assert np.array_equal(j[dst], fcol[src]), where
  assert np.array_equal(bits(v[dst]), bits(fval[src])), where
  return rows.size


# ---- wrong variants of the reference --------------------------------------------

VARIANTS = {
    # name: what it does, the class it is aimed at
    # centroid entry divided by the number of rows that hold the column
    "by_contributors": "centroid entries with fewer contributors than the degree",
    # columns whose mean is zero kept in the centroid
    "zero_kept": "the rows cen_deg1_node, cen_zero_mean_many, cen_deg1_edge",
    # sum min / sum max over the intersection of the supports
    "intersection": "pairs labelled swj_left_only / swj_right_only",
    # the entries after the shorter operand's last column dropped
    "tail_dropped": "pairs labelled swj_tail_left / swj_tail_right",
    # pn against the node centroid of v, pe against the edge centroid of e
    "wrong_side": "pairs labelled ne_node_in_edge / ne_node_not_in_edge",
}
