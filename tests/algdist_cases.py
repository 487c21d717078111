"""Alg-dist test cases: planted graphs, inputs, a float64 reference and the
float32 error bound of a correct implementation (CPU only; used by
test_algdist_cases_cpu.py and test_gpu_algdist_kernels.py).

Graphs. ``planted_graph`` realises two degree sequences exactly (bipartite
Havel-Hakimi: the side with fewer rows, longest row first, takes the columns
of the largest residual degree), so a graph holds rows of exactly the planted
lengths on both sides and its two average degrees select the kernel
instantiation (G lanes per row) the case names. The filler rows vary between
half and one and a half times their mean, so the 1/deg weights differ inside
a row.

Planted lengths, for the side's G. Quad kernel (Q = G/4 quads stride the row,
M = 4 in flight): 1, Q-1, Q, Q+1, 4Q-1, 4Q, 4Q+1, 8Q+1. Narrow kernel (G
lanes stride the row, M = 2 in flight): 1, G-1, G, G+1, GM-1, GM, GM+1,
2GM+1. Zeros and repeats dropped.

Reference. ``reference`` restates algebraic_distance.py:34-123 in float64
with scipy sparse products: node half x' = (x + sum(w y) / sum(w)) / 2 with
w = 1/|edge|, edge half on the NEW x' with w = 1/deg(node), joint per
dimension min-max rescale of both tables. It does not call oracle/hgref.c.

Bound. u = 2^-24 (float32 unit roundoff). hypergraphembedding_amd/build.py
compiles with -O3 and no fast-math flag, so hipcc keeps its default of
correctly rounded float32 division (and 1/x): one division or reciprocal is
one rounding, relative error u. Fused multiply-adds only remove roundings.

The device keeps RAW (unscaled) values z_t of iteration t and the min / max
words; iteration t + 1 applies s_t(z) = (z - m_t) / d_t, d_t = max_t - m_t,
when it reads. With e the elementwise error bound of the raw values:

  min / max:  the device's minimum lies in [min(z - e), min(z + e)], so
    em = max(min z - min(z - e), min(z + e) - min z), eM likewise, and
    ed = em + eM for the span.
  s(z), true value in [0, 1]:  (e + em + ed) / d  for the inputs, plus 4 u:
    the subtraction, the span's own subtraction, the reciprocal and the
    multiply, each relative to a value <= 1.
  weighted mean of a row of n incidences, A = sum(w |src|) / sum(w):
    numerator: n u on the sum in any order, u for the rounded weight
    1/len, u for the multiply, relative to sum |w src|; denominator: n u
    and u for the weight, relative to sum w; then the reciprocal and the
    multiply, 2 u. In all (2 n + 5) u A, since |mean| <= A; plus the
    w-weighted mean of the sources' own e. ``extra`` adds roundings to each
    sum (the sharded exchange adds two partial sums: one more).
  v = (sv + mv) / 2:  (e_sv + e_mv) / 2 + u |v|  (the halving is exact).
  first iteration: no affine on the way in, e_sv = 0 (the inputs are the
    float32 values themselves).
  final affine (z - m) / d:  (e + em + ed) / d + 3 u.

So e_(t+1) = (e_t + delta_t) / span_t plus the rescale's roundings, carried
elementwise through the same sparse products. The result is multiplied by
1.01 for the second-order terms dropped above.
"""

import numpy as np
import scipy.sparse as sps

from hypergraphembedding_amd.hypergraph_util import Incidence

U = 2.0 ** -24
QUAD_M, NARROW_M = 4, 2
DEFAULT_LONG = 512  # kLongRow; the alg_long tuning takes 64 ... 2^20
BLOCK = 256
MAX_WG = 64  # kRep: the sampled intermediate flush is the full one up to here


def quad_g(avg):
  """quad_fn, hgx_algdist.hip:1149-1151: q doubles while q * 8 < avg."""
  q = 1
  while q < 16 and q * 8 < avg:
    q *= 2
  return 4 * q


def narrow_g(avg):
  """pick_g, hgx_algdist.hip:1045-1047: g doubles while g * 4 < avg."""
  g = 1
  while g < 64 and g * 4 < avg:
    g *= 2
  return g


INF = float("inf")
# (lo, hi]: the averages for which the while loops above stop at G
QUAD_CLASS = {4: (0, 8), 8: (8, 16), 16: (16, 32), 32: (32, 64), 64: (64, INF)}
NARROW_CLASS = {1: (0, 4), 2: (4, 8), 4: (8, 16), 8: (16, 32), 16: (32, 64),
                32: (64, 128), 64: (128, INF)}


def planted_lengths(qg, ng):
  """Row lengths around the strides of quad G = qg and narrow G = ng."""
  q, p = qg // 4, ng
  s = {1, q - 1, q, q + 1, 4 * q - 1, 4 * q, 4 * q + 1, 8 * q + 1,
       p - 1, p, p + 1, p * NARROW_M - 1, p * NARROW_M, p * NARROW_M + 1,
       2 * p * NARROW_M + 1}
  return sorted(v for v in s if v > 0)


def _degrees(rows, total, planted, rng, cap):
  f = rows - len(planted)
  t = total - int(sum(planted))
  assert f > 0 and t >= f, "filler rows cannot absorb the planted lengths"
  base = t / f
  lo = max(1, int(base / 2))
  hi = max(lo, min(cap, int(round(1.5 * base))))
  assert lo * f <= t <= hi * f, (lo, hi, f, t)
  d = rng.integers(lo, hi + 1, f)
  while d.sum() != t:
    diff = t - int(d.sum())
    ok = np.flatnonzero(d < hi if diff > 0 else d > lo)
    d[rng.permutation(ok)[:abs(diff)]] += 1 if diff > 0 else -1
  deg = np.concatenate([np.asarray(planted, np.int64), d])
  perm = rng.permutation(rows)  # planted rows at scattered positions
  out = np.empty(rows, np.int64)
  out[perm] = deg
  return out, {int(n): int(perm[i]) for i, n in enumerate(planted)}


def _realize(da, db, rng):
  """Rows of degrees da over columns of degrees db, both exact. Columns are
  kept sorted by residual degree; a row takes every column above the value
  of its d-th and the tail of that value's run, which keeps the order."""
  nb = len(db)
  order = rng.permutation(nb)
  order = order[np.argsort(-db[order], kind="stable")]
  neg = -db[order].astype(np.int64)
  rows, cols = [], []
  for r in np.argsort(-da, kind="stable"):
    d = int(da[r])
    assert d <= nb and neg[d - 1] < 0, "degree sequences are not realisable"
    a = int(np.searchsorted(neg, neg[d - 1], side="left"))
    b = int(np.searchsorted(neg, neg[d - 1], side="right"))
    take = np.concatenate([np.arange(a), np.arange(b - (d - a), b)])
    neg[take] += 1
    rows.append(np.full(d, r, np.int64))
    cols.append(order[take])
  assert not neg.any(), "degree sequences are not realisable"
  return np.concatenate(rows), np.concatenate(cols)


def planted_graph(avg_n, avg_e, rows, planted_n, planted_e, seed,
                  cap_n=DEFAULT_LONG, cap_e=DEFAULT_LONG):
  """Incidence of `rows` node rows at average degree avg_n and
  round(rows * avg_n / avg_e) edge rows, holding one node row of every length
  in planted_n and one edge row of every length in planted_e (inc.planted_n /
  inc.planted_e: length -> row). Filler rows stay within cap_n / cap_e."""
  rng = np.random.default_rng(seed)
  N = int(rows)
  nnz = int(round(N * avg_n))
  E = int(round(nnz / avg_e))
  dn, pn = _degrees(N, nnz, planted_n, rng, cap_n)
  de, pe = _degrees(E, nnz, planted_e, rng, cap_e)
  if N <= E:
    r, c = _realize(dn, de, rng)
  else:
    c, r = _realize(de, dn, rng)
  a = sps.csr_matrix((np.ones(nnz, bool), (r, c)), shape=(N, E))
  inc = Incidence.from_scipy(a)
  assert inc.nnz == nnz  # no incidence twice
  assert np.array_equal(inc.node_degree(), dn)
  assert np.array_equal(inc.edge_size(), de)
  inc.planted_n, inc.planted_e = pn, pe
  return inc


class Case:
  """A graph with the instantiation it selects on each side."""

  def __init__(self, name, avg_n, avg_e, rows, seed, iters=(1, 2, 3),
               planted_n=None, planted_e=None, long_thresh=DEFAULT_LONG,
               cap_n=None, cap_e=None):
    self.name, self.avg_n, self.avg_e = name, avg_n, avg_e
    self.rows, self.seed, self.iters = rows, seed, iters
    self.long_thresh = long_thresh
    self.quad = (quad_g(avg_n), quad_g(avg_e))
    self.narrow = (narrow_g(avg_n), narrow_g(avg_e))
    self.planted_n = (planted_lengths(self.quad[0], self.narrow[0])
                      if planted_n is None else planted_n)
    self.planted_e = (planted_lengths(self.quad[1], self.narrow[1])
                      if planted_e is None else planted_e)
    self.cap_n = cap_n or long_thresh
    self.cap_e = cap_e or long_thresh
    self._inc = None

  @property
  def inc(self):
    if self._inc is None:
      self._inc = planted_graph(self.avg_n, self.avg_e, self.rows,
                                self.planted_n, self.planted_e, self.seed,
                                self.cap_n, self.cap_e)
    return self._inc


# The seven graphs. Per side: quad G (quad_fn, hgx_algdist.hip:1149-1151) and
# narrow G (pick_g, :1045-1047) with the interval of averages that selects it.
# Rows per workgroup are 256 / G; each side has at most 64 * 256 / G rows for
# both of its G, and no row count is a multiple of 256 / G. The graph seeds
# are ones at which the mutant condition of test_algdist_cases_cpu.py holds
# for all three input distributions at k = 3, 7 and 19 (a condition on the
# inputs, found with the reference alone).
#        name       avg_n avg_e  N      node: quad (lo,hi]  narrow (lo,hi]   edge: quad      narrow
SEVEN = [
    Case("d3x200", 3, 200, 3000, 1),   # G 4 (0,8]    1 (0,4]      64 (64,inf)  64 (128,inf)  E 45
    Case("d6x100", 6, 100, 2500, 2),   # G 4 (0,8]    2 (4,8]      64 (64,inf)  32 (64,128]   E 150
    Case("d12x48", 12, 48, 1500, 3),   # G 8 (8,16]   4 (8,16]     32 (32,64]   16 (32,64]    E 375
    Case("d24x24", 24, 24, 700, 24),   # G 16 (16,32] 8 (16,32]    16 (16,32]   8 (16,32]     E 700
    Case("d48x12", 48, 12, 370, 5),    # G 32 (32,64] 16 (32,64]   8 (8,16]     4 (8,16]      E 1480
    Case("d100x6", 100, 6, 150, 6),    # G 64 (64,inf) 32 (64,128] 4 (0,8]      2 (4,8]       E 2500
    Case("d200x3", 200, 3, 45, 34),    # G 64 (64,inf) 64 (128,inf) 4 (0,8]     1 (0,4]       E 3000
]
# fewer rows than 256 / G on both sides (40 and 30 rows, G 4: 64 per
# workgroup); also the graph of the wide kernel's cases
SMALL = Case("small40x30", 6, 8, 40, 8, planted_n=[1, 3, 4, 5, 9],
             planted_e=[1, 3, 4, 5, 9, 17])
# long edge rows under alg_long = 64: 64 is not long, 65 is two pieces, 4097
# is 65 pieces (the lane-strided loop of long_finish)
LONG64 = Case("long64", 3, 48, 4400, 9, iters=(1,), long_thresh=64,
              planted_n=[1, 2, 5], planted_e=[64, 65, 128, 129, 4097],
              cap_n=64, cap_e=64)
# long edge rows under the default threshold
LONG512 = Case("long512", 3, 40, 1200, 10, iters=(1,),
               planted_n=[1, 2, 5], planted_e=[512, 513, 1025], cap_e=256)
# a long NODE row under the default threshold (push falls back to gather)
LONGNODE = Case("longnode", 4, 4, 700, 11, iters=(1,),
                planted_n=[513], planted_e=[1, 2], cap_n=64, cap_e=64)
# grid-stride: more rows than the resident grid times 256 / G on both sides
GRID = Case("gridstride", 6.4, 100, 140000, 12, iters=(1,),
            planted_n=[1], planted_e=[1])

ALL = SEVEN + [SMALL, LONG64, LONG512, LONGNODE, GRID]
DISTS = ("u01", "sym", "off100")


def inputs(inc, k, dist, seed=0):
  """float32 (x0, y0): uniform [0, 1), [-1, 1) or [100, 101)."""
  rng = np.random.default_rng([seed, k, DISTS.index(dist)])
  x = rng.random((inc.N, k))
  y = rng.random((inc.E, k))
  if dist == "sym":
    x, y = 2 * x - 1, 2 * y - 1
  elif dist == "off100":
    x, y = 100 + x, 100 + y
  x, y = x.astype(np.float32), y.astype(np.float32)
  if dist == "off100":  # float32 rounding may reach 101
    x, y = np.minimum(x, np.float32(100.99999)), np.minimum(y, np.float32(100.99999))
  return x, y


LONG_DISTS = ("u01", "sym", "near1")


def long_inputs(inc, k, dist, seed=0):
  """Inputs for the long-row graphs: a long row's mean of n sources has a
  float32 floor of n u A, above what one lost incidence moves it unless A
  (the sources' weighted mean magnitude) is small. Every source of a planted
  edge row is scaled by 2^-10 except the row's first and last, which keep
  magnitude ~1: `u01` and `sym` as drawn, `near1` (no offset of 100 can be
  made small) the u01 draw plus 1 on those two."""
  assert dist in LONG_DISTS
  x, y = inputs(inc, k, "u01" if dist == "near1" else dist, seed)
  keep = np.zeros(inc.N, bool)
  small = np.zeros(inc.N, bool)
  for n, e in inc.planted_e.items():
    c = inc.col_e[inc.rp_e[e]:inc.rp_e[e + 1]]
    small[c] = True
    keep[c[0]] = keep[c[-1]] = True
  x = x.copy()
  x[small & ~keep] *= np.float32(2.0 ** -10)
  if dist == "near1":
    x[keep] += np.float32(1.0)
  return x, y


def case_inputs(case, k, dist):
  """The long-row graphs take LONG_DISTS through long_inputs and `off100`
  as drawn (a real offset; not under the mutant condition: a row of n
  incidences moves by at most 1 / (2 n) when it loses one, its bound is
  about 100 n u, so 2 x needs n^2 < 1 / (400 u), n < 205). Every other
  graph takes DISTS as drawn."""
  if case in (LONG64, LONG512) and dist != "off100":
    return long_inputs(case.inc, k, dist)
  return inputs(case.inc, k, dist)


def _mats(inc):
  a, at = inc.to_scipy()
  return a.astype(np.float64), at.astype(np.float64)


def _minmax_err(z, e):
  lo, hi = z.min(0), z.max(0)
  em = np.maximum(lo - (z - e).min(0), (z + e).min(0) - lo)
  eM = np.maximum((z + e).max(0) - hi, hi - (z - e).max(0))
  return em, eM


def reference(inc, x0, y0, iters, mutant=None):
  """float64 relaxation. Returns (x, y, hist); hist[t] holds the joint span
  and minimum per dimension, the raw (unscaled) values of iteration t and,
  per row, mag = sum(w |src|) / sum(w) over the values the device sums (the
  raw edge rows of iteration t - 1 for the node half, the new raw node rows
  for the edge half). `mutant` names a deliberately wrong variant (CPU tests
  of the bound): drop_last, first_twice, uniform_w, old_x, no_src_affine."""
  a, at = _mats(inc)
  if mutant in ("drop_last", "first_twice"):
    def edit(m):  # sorted CSR: a row's first / last entry, rows of >= 2
      m = m.copy()
      rows = np.flatnonzero(np.diff(m.indptr) >= 2)
      if mutant == "drop_last":
        m.data[m.indptr[rows + 1] - 1] = 0.0
        m.eliminate_zeros()
      else:
        m.data[m.indptr[rows]] = 2.0
      return m
    a, at = edit(a), edit(at)
  wn = 1.0 / inc.node_degree().astype(np.float64)
  we = 1.0 / inc.edge_size().astype(np.float64)
  if mutant == "uniform_w":
    wn[:], we[:] = 1.0, 1.0
  x = np.asarray(x0, np.float64).copy()
  y = np.asarray(y0, np.float64).copy()
  yraw, lo, span = y, None, None
  hist = []
  for t in range(iters):
    den_n = (a @ we)[:, None]
    mean = (a @ (we[:, None] * y)) / den_n
    if mutant == "no_src_affine" and t > 0:
      mean = (a @ (we[:, None] * yraw)) / den_n
    mag_n = (a @ (we[:, None] * np.abs(yraw))) / den_n
    xn = (x + mean) / 2
    den_e = (at @ wn)[:, None]
    src = x if mutant == "old_x" else xn
    yn = (y + (at @ (wn[:, None] * src)) / den_e) / 2
    mag_e = (at @ (wn[:, None] * np.abs(xn))) / den_e
    lo = np.minimum(xn.min(0), yn.min(0))
    span = np.maximum(xn.max(0), yn.max(0)) - lo
    hist.append(dict(span=span, lo=lo, xraw=xn, yraw=yn, mag_n=mag_n,
                     mag_e=mag_e))
    yraw = yn
    x, y = (xn - lo) / span, (yn - lo) / span
  return x, y, hist


def bound(inc, hist, extra=0):
  """Elementwise float32 error bounds (bx, by) of the coordinates after
  len(hist) iterations (module docstring)."""
  a, at = _mats(inc)
  dn = inc.node_degree().astype(np.float64)[:, None]
  de = inc.edge_size().astype(np.float64)[:, None]
  wn, we = 1.0 / dn, 1.0 / de
  den_n, den_e = a @ we, at @ wn
  k = hist[0]["span"].size
  ex, ey = np.zeros((inc.N, k)), np.zeros((inc.E, k))
  prev = None
  for h in hist:
    if prev is not None:
      both = np.vstack([prev["xraw"], prev["yraw"]])
      em, eM = _minmax_err(both, np.vstack([ex, ey]))
      aff = em + (em + eM)
      d = prev["span"]
    def scaled(e):
      return e if prev is None else (e + aff) / d + 4 * U
    dmean = (a @ (we * ey)) / den_n + (2 * dn + 5 + 2 * extra) * U * h["mag_n"]
    exn = (scaled(ex) + scaled(dmean)) / 2 + U * np.abs(h["xraw"])
    dmean = (at @ (wn * exn)) / den_e + (2 * de + 5 + 2 * extra) * U * h["mag_e"]
    eyn = (scaled(ey) + dmean) / 2 + U * np.abs(h["yraw"])
    ex, ey, prev = exn, eyn, h
  both = np.vstack([prev["xraw"], prev["yraw"]])
  em, eM = _minmax_err(both, np.vstack([ex, ey]))
  aff = em + (em + eM)
  d = prev["span"]
  return 1.01 * ((ex + aff) / d + 3 * U), 1.01 * ((ey + aff) / d + 3 * U)
