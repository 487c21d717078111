"""LINE baseline on the device (the ``"LINE"`` key of ``EMBEDDING_OPTIONS``;
the reference writes LINE's input with ``SaveEdgeList``, the bipartite
node-edge list in both directions with weight 1, and imports its output
through ``utilities/convert_from_line.py`` as ``method_name = "LINE"``). The
LINE binary is not a dependency and is not replayed: the edge-sampling
trainer of first and second order is restated from its formulas (DESIGN
§4.12), and nothing beyond the formulas below is claimed.

Graph. Bipartite, V = N + E: node ``v`` is vertex ``v``, edge ``e`` is vertex
``N + e``. Incidence ``p`` is position ``p`` of the node-major CSR (``rp_n``,
``col_n``), ``p`` in [0, nnz), with weight ``w_p >= 0``: 1 by default, or an
optional ``weights`` float array of length nnz. Each incidence is two arcs of
the same weight, node -> edge and edge -> node. ``deg(x)`` is the sum of
``w_p`` over x's incidences.

Tables, built on the host. ``alias_table(w) -> (thr uint32[nnz], alias
int32[nnz])`` is Vose's method computed in float64, the thresholds rounded to
32 bits: draw a position ``p0`` uniformly, then a 32-bit value ``a`` below
``2**32 - 1``; take ``p0`` if ``a < thr[p0]``, else ``alias[p0]``. With all
weights equal ``thr = 2**32 - 1`` everywhere and the device needs no table.
``cum = node2vec.cum_table(deg, 0.75)`` over the V vertices; a vertex of
degree 0 is never drawn.

Draws of sample ``s`` (the global index, 0 <= s < T, held in 64 bits). ``key =
_rand64_key(seed, s)``; counter ``c`` gives ``_draw(key, c)`` (both are
node2vec.py's). ``c = 0``: ``p0 = _bounded(draw, nnz)``. ``c = 1``: ``a =
_bounded(draw, 0xffffffff)``, then ``p = p0`` if ``a < thr[p0]`` else
``alias[p0]``. ``c = 2``: the direction ``_bounded(draw, 2)``; 0 means ``u =
row(p)`` and ``v = N + col_n[p]``, 1 the reverse; ``row(p)`` is found by
binary search in ``rp_n``, no arc array is materialised. ``c = 3 + k``:
negative ``k = bisect_left(cum, _bounded(draw, cum[V - 1]))``. Negatives are
kept as drawn: none is rejected for equalling ``u``, ``v`` or another
negative.

Step of sample ``s`` at ``order`` 1 or 2. ``Tgt`` is ``syn0`` (the vertex
vectors) at order 1 and ``syn1`` (the context vectors) at order 2. ``l1 =
syn0[u]`` is read once and held fixed, ``err = 0``. The targets are ``t_0 =
v`` with label 1, then the K negatives with label 0, in order; for each:
``row = Tgt[t]`` as it stands now, this sample's earlier updates included;
``x = l1 . row``; ``g = float32(label - sigma(x)) rho_s``; ``err += g row``
(the row before its own update); ``Tgt[t] += g l1``. At the end ``syn0[u] +=
err``, added to the row as it then stands: at order 1 a target equal to ``u``
has already moved it. ``sigma`` is LINE's bounded sigmoid: 1 for ``x > 6``, 0
for ``x < -6``, else the exact logistic computed in float64; ``label - sigma``
is rounded to float32 once. A product and the sum it enters are two
roundings. ``rho_s = float32(max(r0 (1 - s / (T + 1)), 1e-4 r0))`` computed in
float64 with ``r0 = float(float32(rho))``.

Deviations from the LINE program. (1) The exact logistic replaces its
1000-entry table. (2) Counter-based draws replace its generators and its
1e8-entry negative table. (3) rho moves per sample, not per 10,000 samples of
a thread. (4) ``l1`` is held fixed within a sample, where LINE's code reads
it live. (5) The concurrent mode (``line_chunk_samples`` samples per launch,
64 consecutive samples to a wave, float atomic adds) stands in for
``-threads > 1``.
"""

import bisect

import numpy as np

from . import _hgx
from . import node2vec as n2v
from .hypergraph_util import Incidence
from .node2vec import BIPARTITE, MAX_DIM, MAX_EXP, MAX_NEGATIVE

_T32 = 2**32 - 1


def alias_table(w):
  """``(thr, alias)`` of the module docstring over the weights ``w``."""
  w = np.asarray(w, np.float64).ravel()
  n = w.size
  assert n > 0 and np.all(w >= 0) and np.all(np.isfinite(w)) and w.sum() > 0
  alias = np.arange(n, dtype=np.int32)
  if np.all(w == w[0]):
    return np.full(n, _T32, np.uint32), alias
  q = w * (n / w.sum())
  prob = np.ones(n)
  order = np.argsort(q, kind="stable")
  # stacks: the smallest of the small ones and the largest of the large ones
  # on top, so a position of weight 0 is paired while large ones remain
  small = [int(i) for i in order[::-1] if q[i] < 1.0]
  large = [int(i) for i in order if q[i] >= 1.0]
  while small and large:
    s, g = small.pop(), large.pop()
    prob[s], alias[s] = q[s], g
    q[g] = (q[g] + q[s]) - 1.0
    (small if q[g] < 1.0 else large).append(g)
  # what is left holds 1 up to rounding: it keeps itself
  assert all(w[i] > 0 for i in small + large)
  thr = np.minimum(np.round(prob * float(_T32)), float(_T32)).astype(np.uint32)
  return thr, alias


def line_degrees(inc, weights=None):
  """float64 ``deg`` over the V = N + E vertices."""
  w = (np.ones(inc.nnz) if weights is None else
       np.asarray(weights, np.float64).ravel())
  assert w.size == inc.nnz and np.all(w >= 0)
  rows = np.repeat(np.arange(inc.N), np.diff(inc.rp_n))
  return np.concatenate([np.bincount(rows, weights=w, minlength=inc.N),
                         np.bincount(inc.col_n, weights=w, minlength=inc.E)])


def line_rho(rho, s, T):
  """rho of sample ``s`` of ``T`` (float32)."""
  r0 = float(np.float32(rho))
  return np.float32(max(r0 * (1.0 - s / (T + 1)), 1e-4 * r0))


def line_plan(inc, thr, alias, cum, negative, n_samples, seed, s0=0):
  """The draws of the samples ``s0 .. s0 + n_samples - 1`` in Python
  integers: an (n_samples, 2 + negative) int64 array of (u, v, negatives).
  ``thr`` and ``alias`` are None for equal weights."""
  N, nnz = inc.N, int(inc.nnz)
  assert nnz > 0 and negative >= 0
  rp = [int(x) for x in inc.rp_n]
  col = inc.col_n
  cl = [int(x) for x in cum]
  out = np.empty((n_samples, 2 + negative), np.int64)
  for i in range(n_samples):
    key = n2v._rand64_key(seed, s0 + i)
    p = n2v._bounded(n2v._draw(key, 0), nnz)
    if thr is not None:
      a = n2v._bounded(n2v._draw(key, 1), 0xffffffff)
      if not a < int(thr[p]):
        p = int(alias[p])
    nd, ed = bisect.bisect_right(rp, p) - 1, N + int(col[p])
    out[i, :2] = (ed, nd) if n2v._bounded(n2v._draw(key, 2), 2) else (nd, ed)
    for k in range(negative):
      out[i, 2 + k] = bisect.bisect_left(
          cl, n2v._bounded(n2v._draw(key, 3 + k), cl[-1]))
  return out


def bounded_sigmoid(x):
  """LINE's sigmoid in float64: 1 above 6, 0 below -6, the logistic
  between."""
  if x > MAX_EXP:
    return 1.0
  if x < -MAX_EXP:
    return 0.0
  return 1.0 / (1.0 + np.exp(-np.float64(x)))


class NumpyBackendLine(n2v.NumpyBackend):
  """``NumpyBackend`` plus the float32 host restatement of the LINE trainer
  (``set_arcs``, ``line_samples``, ``train_line``); sequential whatever
  ``concurrent`` says, ``reverse=True`` sums every dot product in the
  reversed column order."""

  def __init__(self, inc, graph, dim, reverse=False):
    super().__init__(inc, graph, dim, reverse=reverse)
    self._arcs = None
    self._vectors = False
    self._stats.update(samples=0, targets=0, clamped=0)

  def set_vectors(self, syn0, syn1=None):
    super().set_vectors(syn0, syn1)
    self._vectors = True

  def set_arcs(self, thr, alias, cum):
    if self.graph != BIPARTITE:
      raise _hgx.HgxError("LINE: the engine is not on the bipartite graph")
    assert (thr is None) == (alias is None)
    cum = np.asarray(cum, np.int32)
    assert cum.size == self.V and np.all(np.diff(cum) >= 0) and cum[-1] > 0
    if thr is not None:
      thr, alias = np.asarray(thr, np.uint32), np.asarray(alias, np.int32)
      assert thr.size == alias.size == self.inc.nnz
      assert alias.min() >= 0 and alias.max() < self.inc.nnz
    self._arcs = (thr, alias, cum)

  def _line_check(self, negative):
    if self.graph != BIPARTITE:
      raise _hgx.HgxError("LINE: the engine is not on the bipartite graph")
    assert negative >= 0
    if negative > MAX_NEGATIVE:
      raise _hgx.HgxError("LINE: negative %d above %d" %
                          (negative, MAX_NEGATIVE))
    if self._arcs is None:
      raise _hgx.HgxError("LINE: before set_arcs")

  def line_samples(self, s0, count, negative, seed):
    self._line_check(negative)
    assert s0 >= 0 and count >= 0
    return line_plan(self.inc, *self._arcs, negative, count, seed,
                     s0).astype(np.int32)

  def train_line(self, order, negative, n_samples, rho=0.025, seed=0,
                 concurrent=True, plan=None):
    import time
    t0 = time.perf_counter()
    assert order in (1, 2) and n_samples >= 0
    self._line_check(negative)
    if not self._vectors:
      raise _hgx.HgxError("LINE: train_line before set_vectors")
    if plan is None:
      plan = line_plan(self.inc, *self._arcs, negative, n_samples, seed)
    assert len(plan) == n_samples
    syn0 = self.syn0
    tgt = syn0 if order == 1 else self.syn1
    clamped = 0
    for s, smp in enumerate(plan):
      rho_s = line_rho(rho, s, n_samples)
      u = int(smp[0])
      l1 = syn0[u].copy()
      err = np.zeros(self.dim, np.float32)
      for k, t in enumerate(smp[1:]):
        row = tgt[int(t)]
        x = self._dot(l1, row)
        clamped += bool(abs(x) > np.float32(MAX_EXP))
        g = np.float32((1.0 if k == 0 else 0.0) - bounded_sigmoid(x)) * rho_s
        err += g * row
        row += g * l1
      syn0[u] += err
    self._stats.update(train_ms=(time.perf_counter() - t0) * 1e3, words=0,
                       pairs=0, samples=n_samples,
                       targets=n_samples * (1 + negative), clamped=clamped)


def _unit_rows(x):
  """Every row divided by its L2 norm taken in float64, rounded to float32;
  a zero row stays zero."""
  x64 = np.asarray(x, np.float64)
  nrm = np.sqrt((x64 * x64).sum(axis=1))
  out = np.zeros_like(x64)
  np.divide(x64, nrm[:, None], out=out, where=(nrm > 0)[:, None])
  return out.astype(np.float32)


def line_incidence(inc, dimension, *, order=2, negative=5, samples=1_000_000,
                   rho=0.025, weights=None, run_in_parallel=True, vectors=None,
                   ctx=None, backend=None):
  """LINE on the bipartite graph of ``inc``; returns ``(V x dimension
  float32, info)``, V = N + E.

  ``order`` 1 or 2 trains that order over ``samples`` edge samples.
  ``order="both"`` needs an even dimension: order 1 and then order 2 are
  trained at ``d' = dimension / 2`` with the full ``samples`` each, every row
  of each half is divided by its L2 norm (taken in float64, the row rounded to
  float32, a zero row stays zero) and the result is ``[first | second]``,
  LINE's normalize + concatenate pipeline.

  Host draws come from numpy's global RandomState; per trained order the
  sequence is the seed ``np.random.randint(0, 2**31 - 1)``, then the vectors
  ``(np.random.random((V, d')).astype(float32) - 0.5) / d'`` unless
  ``vectors`` is given (V x d', used for every trained order). The context
  table starts at zero. ``run_in_parallel=False`` trains the samples one
  after another (bit for bit reproducible after ``np.random.seed``), ``True``
  concurrently with the same draws.

  A vertex of degree 0 gets a zero vector; ``nnz = 0`` is an
  ``AssertionError``. ``info``: ``degrees``, ``n_samples`` and the backend's
  ``stats`` (of the last trained order; with ``samples``, ``targets`` and
  ``clamped``). ``ctx`` and ``backend`` are ``node2vec_incidence``'s; a host
  backend is ``NumpyBackendLine(inc, BIPARTITE, d')``.
  """
  d = int(dimension)
  assert d > 0
  assert order in (1, 2, "both")
  assert negative >= 0 and samples >= 0
  assert inc.N > 0 and inc.E > 0
  assert inc.nnz > 0, "LINE: an incidence without an entry"
  if order == "both":
    assert d % 2 == 0, "order='both' needs an even dimension"
  dh = d // 2 if order == "both" else d
  if dh > MAX_DIM:
    raise _hgx.HgxError("line_incidence: dimension %d is above the %d the "
                        "device engine takes" % (dh, MAX_DIM))
  if negative > MAX_NEGATIVE:
    raise _hgx.HgxError("line_incidence: negative %d is above the %d the "
                        "device engine takes" % (negative, MAX_NEGATIVE))
  V = inc.N + inc.E
  deg = line_degrees(inc, weights)
  assert deg.sum() > 0, "LINE: every weight is zero"
  thr = alias = None
  if weights is not None:
    thr, alias = alias_table(weights)
    if np.all(thr == _T32):
      thr = alias = None
  cum = n2v.cum_table(deg, 0.75)
  own = backend is None
  if own:
    from .runtime import get_context
    ctx = ctx or get_context()
    ctx.upload(inc)
    backend = _hgx.N2v(ctx, BIPARTITE, dh)
  be = backend
  halves = []
  try:
    be.set_arcs(thr, alias, cum)
    for o in ((1, 2) if order == "both" else (order,)):
      seed = int(np.random.randint(0, 2**31 - 1))
      init = vectors
      if init is None:
        init = (np.random.random((V, dh)).astype(np.float32) -
                np.float32(0.5)) / np.float32(dh)
      be.set_vectors(init, None)
      be.train_line(o, negative, samples, rho=rho, seed=seed,
                    concurrent=bool(run_in_parallel))
      halves.append(be.get_vectors()[0])
    stats = be.stats()
  finally:
    if own:
      be.close()
  if order == "both":
    halves = [_unit_rows(h) for h in halves]
  out = np.concatenate(halves, axis=1)
  out = np.where((deg > 0)[:, None], out, np.float32(0)).astype(np.float32)
  return out, {"degrees": deg, "n_samples": int(samples), "stats": stats}


def EmbedLine(hypergraph, dimension, order=2, negative=5, samples=1_000_000,
              rho=0.025, run_in_parallel=True, disable_pbar=False, *,
              weights=None, ctx=None, backend_factory=None, info=None):
  """LINE as an embedder, ``method_name = "LINE"``: node vector ``syn0[v]``,
  edge vector ``syn0[N + e]``, keyed by the original ids; a vertex of degree 0
  gets zeros. ``order`` is 1, 2 or ``"both"`` (``line_incidence``);
  ``run_in_parallel`` picks the concurrent trainer; ``disable_pbar`` changes
  nothing. ``weights`` are per incidence in node-major order.
  ``backend_factory`` (a callable: (Incidence, graph, dimension) -> backend,
  e.g. ``NumpyBackendLine``) replaces the device and is called with the
  dimension that is trained (half of it at ``order="both"``); a dict passed as
  ``info`` receives ``line_incidence``'s."""
  from .algebraic_distance import coords_to_embedding
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension > 0
  assert inc.N > 0
  assert inc.E > 0
  if order == "both":
    assert dimension % 2 == 0, "order='both' needs an even dimension"
  dh = dimension // 2 if order == "both" else dimension
  syn0, i = line_incidence(
      inc, dimension, order=order, negative=negative, samples=samples, rho=rho,
      weights=weights, run_in_parallel=run_in_parallel, ctx=ctx,
      backend=(backend_factory(inc, BIPARTITE, dh) if backend_factory
               else None))
  if info is not None:
    info.update(i)
  return coords_to_embedding(inc, syn0[:inc.N], syn0[inc.N:], dimension, "LINE")


__all__ = ["line_incidence", "EmbedLine", "NumpyBackendLine", "alias_table",
           "line_degrees", "line_rho", "line_plan", "bounded_sigmoid",
           "BIPARTITE"]
