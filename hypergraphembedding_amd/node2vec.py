"""node2vec baselines on the device (reference: ``EmbedNode2VecBipartide`` and
``EmbedNode2VecClique``, hypergraph_embedding/embedding.py:165-261, which
build a networkx graph and call the ``node2vec`` package and gensim's
``Word2Vec``). Neither library is a dependency here: the walks and the
skip-gram negative-sampling (SGNS) trainer are restated from their formulas
(DESIGN §4.10), and nothing beyond those formulas is claimed.

Vertices. Bipartite graph: node ``v`` is vertex ``v``, edge ``e`` is vertex
``N + e``. Clique graph: the vertices are the nodes, ``u ~ v`` iff ``u != v``
and they share an edge, every distinct neighbour with weight 1; a node
without a distinct neighbour is not in the graph, starts no walk and gets a
zero vector.

Walks. A pass is ``np.random.permutation(sources)``; the corpus is
``num_walks`` passes in order, one walk of ``walk_length`` vertices per source
and pass. Step 1 is uniform over the neighbours, from step 2 the previous
vertex has weight ``1 / p`` and every other neighbour 1 (``q == 1``).

Vocabulary. ``count[w]`` occurrences in the corpus; a word stays with
probability ``min(1, (sqrt(count / thr) + 1) thr / count)``, ``thr = sample *
total``; negatives come from the cumulative table of ``count ** 0.75`` scaled
to ``2 ** 31 - 1``.

Training. Per kept word ``i`` of a walk, ``b = bounded(r, window)``; per kept
word ``j != i`` with ``|i - j| <= window - b``: ``l1 = syn0[w_j]`` held
fixed; for ``t = w_i`` (label 1) and then each negative (label 0, one equal to
``w_i`` skipped) in order: ``x = l1 . syn1[t]``, skipped when ``|x| >= 6``,
``g = (label - sigmoid(x)) alpha``, ``neu += g syn1[t]``, ``syn1[t] += g l1``;
then ``syn0[w_j] += neu``. ``alpha`` falls linearly per walk from ``alpha`` to
``min_alpha`` over ``epochs * n_walks`` walks.

Every draw but the permutations and the initial vectors is counter-based
(``rand64`` / ``mix64`` of csrc/hgx_internal.h) and restated here, so the
device engine (``_hgx.N2v``, csrc/hgx_n2v.hip) and ``NumpyBackend`` read the
same walks (bipartite), keep decisions, windows and negatives.
"""

import bisect

import numpy as np

from . import _hgx
from .hypergraph_util import Incidence

BIPARTITE, CLIQUE = 0, 1
MAX_DIM = 512       # hgx_n2v_create's limit (include/hgx.h)
MAX_WALK = 128      # hgx_n2v_walks' limit
MAX_NEGATIVE = 8    # hgx_n2v_train's limit
MAX_EXP = 6.0       # word2vec's MAX_EXP
_M64 = (1 << 64) - 1


# ---- the library's counter-based generator (csrc/hgx_internal.h) ------------
def _mix64(z):
  z = (z + 0x9e3779b97f4a7c15) & _M64
  z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
  z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
  return z ^ (z >> 31)


def _rand64_key(seed, stream):
  return _mix64((seed & _M64) ^ _mix64((stream + 0x632be59bd9b4e019) & _M64))


def _draw(key, ctr):
  return _mix64((key + ctr) & _M64)


def _bounded(r, n):
  return (r * n) >> 64


def _u01(r):
  return (r >> 11) * 2.0**-53


def _walk_ctr(step, it, slot):
  return (step << 24) | (it << 2) | slot


def _train_ctr(pi, pj, slot):
  return (((pi << 7) | pj) << 4) | slot


# ---- walks -------------------------------------------------------------------
def walk_row(inc, source, pass_, walk_length, p, seed):
  """The walk hgx_n2v_walks gives (pass_, source) on the bipartite graph of
  ``inc``: keyed by (seed, pass_, source) and the step alone."""
  N = inc.N
  invp = 1.0 / p
  key = _rand64_key(seed, ((pass_ & 0xffffffff) << 32) | source)
  cur, prev = int(source), -1
  out = [cur]
  for t in range(1, walk_length):
    if cur < N:
      row = inc.col_n[inc.rp_n[cur]:inc.rp_n[cur + 1]]
      shift = N
    else:
      row = inc.col_e[inc.rp_e[cur - N]:inc.rp_e[cur - N + 1]]
      shift = 0
    deg = len(row)
    r0 = _draw(key, _walk_ctr(t, 0, 0))
    if t == 1 or invp == 1.0:
      nxt = int(row[_bounded(r0, deg)]) + shift
    elif _u01(r0) * (float(deg - 1) + invp) < invp:
      nxt = prev
    else:
      k = _bounded(_draw(key, _walk_ctr(t, 0, 1)), deg - 1)
      if k >= int(np.searchsorted(row, prev - shift)):
        k += 1
      nxt = int(row[k]) + shift
    prev, cur = cur, nxt
    out.append(cur)
  return out


def clique_neighbours(inc):
  """Sorted distinct co-members of every node (host, small inputs only)."""
  out = []
  for u in range(inc.N):
    s = set()
    for e in inc.col_n[inc.rp_n[u]:inc.rp_n[u + 1]]:
      s.update(int(v) for v in inc.col_e[inc.rp_e[e]:inc.rp_e[e + 1]])
    s.discard(u)
    out.append(np.array(sorted(s), np.int64))
  return out


def clique_sources(inc):
  """The nodes of the clique graph: those in some edge of two or more."""
  big = inc.edge_size() > 1
  has = np.zeros(inc.N, bool)
  rows = np.repeat(np.arange(inc.N), np.diff(inc.rp_n))
  has[rows[big[inc.col_n]]] = True
  return np.flatnonzero(has)


def _clique_walk_host(nbrs, source, pass_, walk_length, p, seed):
  """A walk on the materialised clique graph with the same law as the
  device's (its draws differ: the device never lists the neighbours)."""
  invp = 1.0 / p
  key = _rand64_key(seed, ((pass_ & 0xffffffff) << 32) | source)
  cur, prev = int(source), -1
  out = [cur]
  for t in range(1, walk_length):
    row = nbrs[cur]
    deg = len(row)
    r0 = _draw(key, _walk_ctr(t, 0, 0))
    if t == 1 or invp == 1.0:
      nxt = int(row[_bounded(r0, deg)])
    elif _u01(r0) * (float(deg - 1) + invp) < invp:
      nxt = prev
    else:
      k = _bounded(_draw(key, _walk_ctr(t, 0, 1)), deg - 1)
      if k >= int(np.searchsorted(row, prev)):
        k += 1
      nxt = int(row[k])
    prev, cur = cur, nxt
    out.append(cur)
  return out


# ---- vocabulary tables ---------------------------------------------------------
def keep_thresholds(counts, sample=1e-3):
  """32-bit subsampling thresholds: a word stays iff its threshold exceeds a
  uniform draw below 2**32 - 1. ``sample = 0`` keeps every word; a word that
  does not occur has threshold 0."""
  c = np.asarray(counts, np.float64)
  prob = np.ones_like(c)
  if sample > 0:
    thr = sample * c.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
      prob = np.minimum(1.0, (np.sqrt(c / thr) + 1.0) * thr / c)
  prob = np.where(c > 0, prob, 0.0)
  return np.minimum(np.round(prob * 2.0**32), 2.0**32 - 1).astype(np.uint32)


def cum_table(counts, power=0.75):
  """gensim's cumulative negative-sampling table over all vertices:
  round(cumsum(count ** power) / Z * (2**31 - 1))."""
  c = np.asarray(counts, np.float64)**power
  c = np.where(np.asarray(counts) > 0, c, 0.0)
  cs = np.cumsum(c)
  assert cs[-1] > 0, "an empty corpus"
  return np.round(cs / cs[-1] * (2.0**31 - 1)).astype(np.int32)


# ---- the trainer's draws -----------------------------------------------------
def walk_alpha(alpha, min_alpha, g, total):
  """alpha of the walk with global index g (float64 of float32 arguments,
  as hgx_n2v_train computes it)."""
  a0, m0 = float(np.float32(alpha)), float(np.float32(min_alpha))
  return max(m0, a0 - (a0 - m0) * float(g) / float(total))


def walk_pairs(walk, keep, cum, window, negative, seed, epoch, w):
  """(kept words, pairs) of walk ``w`` in ``epoch``: the pairs in training
  order as (input word w_j, output word w_i, [negatives]). ``cum`` is a list
  (bisect)."""
  key = _rand64_key(seed, (epoch << 32) | w)
  kept = []
  for pos, word in enumerate(walk):
    if int(keep[word]) > _bounded(_draw(key, _train_ctr(pos, 0, 0)), 0xffffffff):
      b = _bounded(_draw(key, _train_ctr(pos, 0, 1)), window)
      kept.append((pos, int(word), min(window - b, MAX_WALK)))
  pairs = []
  last = cum[-1]
  for i, (pi, wi, span) in enumerate(kept):
    for j in range(max(0, i - span), min(len(kept) - 1, i + span) + 1):
      if j == i:
        continue
      pj, wj, _ = kept[j]
      negs = [bisect.bisect_left(
          cum, _bounded(_draw(key, _train_ctr(pi, pj, 2 + k)), last))
              for k in range(negative)]
      pairs.append((wj, wi, negs))
  return len(kept), pairs


def corpus_plan(walks, keep, cum, window, negative, epochs, seed):
  """walk_pairs of every (epoch, walk) in training order: a list of
  (kept words, pairs)."""
  cl = [int(v) for v in cum]
  return [walk_pairs(wk, keep, cl, window, negative, seed, ep, w)
          for ep in range(epochs) for w, wk in enumerate(walks)]


def _sigmoid64(x):
  return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


class NumpyBackend:
  """Float32 host restatement of the engine with the same protocol (walks,
  counts, set_vocab, set_vectors, get_vectors, train, stats). Training is
  sequential whatever ``concurrent`` says. ``reverse=True`` sums every dot
  product in the reversed column order: the distance between the two orders
  is the float32 floor the device tests take their bar from. For the clique
  graph it materialises the distinct-neighbour lists (small inputs only) and
  its walks follow the device's law, not the device's draws."""

  def __init__(self, inc, graph, dim, reverse=False):
    self.inc, self.graph, self.dim = inc, int(graph), int(dim)
    assert self.graph in (BIPARTITE, CLIQUE)
    self.reverse = bool(reverse)
    self.V = inc.N if self.graph == CLIQUE else inc.N + inc.E
    self.syn0 = np.zeros((self.V, self.dim), np.float32)
    self.syn1 = np.zeros((self.V, self.dim), np.float32)
    self._walks = None
    self._keep = self._cum = None
    self._nbrs = None
    self._stats = {"walk_ms": 0.0, "train_ms": 0.0, "walks": 0, "words": 0,
                   "pairs": 0, "expand_steps": 0, "reject_steps": 0}

  def close(self):
    pass

  def walks(self, passes, sources, walk_length, p, seed, copy=True):
    if p == 0:
      raise ZeroDivisionError("node2vec: p = 0 (the return weight is 1 / p)")
    assert 0 < p <= 1 and walk_length >= 1
    if walk_length > MAX_WALK:
      raise _hgx.HgxError("node2vec: walk length %d above %d" %
                          (walk_length, MAX_WALK))
    passes = np.asarray(passes, np.int64).ravel()
    sources = np.asarray(sources, np.int64).ravel()
    assert passes.size == sources.size and sources.size > 0
    if self.graph == BIPARTITE:
      assert walk_length == 1 or (np.diff(self.inc.rp_n).min() > 0 and
                                  np.diff(self.inc.rp_e).min() > 0), \
          "node2vec: a zero-degree row"
      out = [walk_row(self.inc, int(s), int(ps), walk_length, p, seed)
             for ps, s in zip(passes, sources)]
    else:
      if self._nbrs is None:
        self._nbrs = clique_neighbours(self.inc)
      for s in sources:
        assert len(self._nbrs[s]) > 0, "node %d is not in the clique graph" % s
      out = [_clique_walk_host(self._nbrs, int(s), int(ps), walk_length, p, seed)
             for ps, s in zip(passes, sources)]
    self._walks = np.array(out, np.int32).reshape(sources.size, walk_length)
    self._stats["walks"] = sources.size
    return self._walks.copy() if copy else None

  def counts(self):
    assert self._walks is not None
    return np.bincount(self._walks.ravel(), minlength=self.V).astype(np.int64)

  def set_vocab(self, keep, cum):
    keep, cum = np.asarray(keep, np.uint32), np.asarray(cum, np.int32)
    assert keep.size == cum.size == self.V
    assert np.all(np.diff(cum) >= 0) and cum[-1] > 0
    self._keep, self._cum = keep, cum

  def set_vectors(self, syn0, syn1=None):
    self.syn0 = np.array(syn0, np.float32).reshape(self.V, self.dim)
    self.syn1 = (np.zeros_like(self.syn0) if syn1 is None else
                 np.array(syn1, np.float32).reshape(self.V, self.dim))

  def get_vectors(self):
    return self.syn0.copy(), self.syn1.copy()

  def _dot(self, a, b):
    if self.reverse:
      a, b = a[::-1], b[::-1]
    # products rounded to float32, summed one by one in column order
    return np.cumsum(a * b, dtype=np.float32)[-1]

  def train(self, walks=None, *, window=3, negative=5, epochs=5, alpha=0.025,
            min_alpha=1e-4, seed=0, concurrent=True, plan=None):
    import time
    t0 = time.perf_counter()
    if walks is not None:
      self._walks = np.array(walks, np.int32)
      assert self._walks.ndim == 2 and self._walks.shape[1] <= MAX_WALK
      assert self._walks.min() >= 0 and self._walks.max() < self.V
    assert self._walks is not None and self._keep is not None
    assert window >= 1 and epochs >= 0 and negative >= 0
    if negative > MAX_NEGATIVE:
      raise _hgx.HgxError("node2vec: negative %d above %d" %
                          (negative, MAX_NEGATIVE))
    wk = self._walks
    if plan is None:
      plan = corpus_plan(wk, self._keep, self._cum, window, negative, epochs,
                         seed)
    syn0, syn1 = self.syn0, self.syn1
    total = epochs * len(wk)
    words = npairs = 0
    for g, (nk, pairs) in enumerate(plan):
      a = np.float32(walk_alpha(alpha, min_alpha, g, total))
      words += nk
      npairs += len(pairs)
      for wj, wi, negs in pairs:
        l1 = syn0[wj].copy()
        ts = [wi] + [t for t in negs if t != wi]
        if len(set(ts)) == len(ts):
          # no row repeats: with l1 fixed the targets do not see each other
          S = syn1[ts]
          P = S * l1
          if self.reverse:
            P = P[:, ::-1]
          x = np.cumsum(P, axis=1, dtype=np.float32)[:, -1]
          lab = np.zeros(len(ts))
          lab[0] = 1.0
          gg = np.where(np.abs(x) < np.float32(MAX_EXP),
                        (lab - _sigmoid64(x)).astype(np.float32) * a,
                        np.float32(0))
          neu = np.cumsum(gg[:, None] * S, axis=0, dtype=np.float32)[-1]
          syn1[ts] = S + gg[:, None] * l1
          syn0[wj] = l1 + neu
          continue
        neu = np.zeros(self.dim, np.float32)
        for k, t in enumerate([wi] + negs):
          if k > 0 and t == wi:
            continue
          x = self._dot(l1, syn1[t])
          if not abs(x) < np.float32(MAX_EXP):
            continue
          lab = 1.0 if k == 0 else 0.0
          gg = np.float32(lab - _sigmoid64(x)) * a
          neu += gg * syn1[t]
          syn1[t] += gg * l1
        syn0[wj] = l1 + neu
    self._stats.update(train_ms=(time.perf_counter() - t0) * 1e3,
                       walks=total, words=words, pairs=npairs)

  def stats(self):
    return dict(self._stats)


def node2vec_incidence(inc, graph, dimension, *, p=1, num_walks=10,
                       walk_length=5, window=3, epochs=5, alpha=0.025,
                       min_alpha=1e-4, negative=5, sample=1e-3,
                       run_in_parallel=True, vectors=None, ctx=None,
                       backend=None):
  """node2vec on the bipartite (``BIPARTITE``) or clique (``CLIQUE``) graph
  of ``inc``; returns ``(syn0 V x dimension float32, info)``, V = N + E or N.

  Host draws come from numpy's global RandomState in this order: one
  ``np.random.permutation(sources)`` per pass, then the two device seeds (the
  walks', the trainer's), then the initial vectors ``(np.random.random((V,
  d)).astype(float32) - 0.5) / d`` unless ``vectors`` is given. With
  ``run_in_parallel=False`` the walks train one after another in corpus
  order and after ``np.random.seed`` a run is reproducible bit for bit;
  ``True`` trains them concurrently with the same draws, and results may
  differ in the last bits between runs (gensim with ``workers > 1`` is
  asynchronous too).

  A vertex that starts no walk (a node outside the clique graph) keeps a
  zero vector. ``info``: ``sources``, ``n_walks``, ``counts``, ``stats`` of
  the backend. ``ctx`` is the device context (the process-wide one by
  default; its resident incidence is replaced by ``inc``); ``backend`` is any
  object with the engine's protocol instead, e.g. ``NumpyBackend(inc, graph,
  dimension)``.
  """
  d = int(dimension)
  assert d > 0
  assert p >= 0 and p <= 1
  assert num_walks > 0 and walk_length > 0
  assert window >= 1 and epochs >= 0 and negative >= 0
  assert graph in (BIPARTITE, CLIQUE)
  invp = 1 / p  # ZeroDivisionError at p = 0, as the library's 1 / p
  del invp
  if d > MAX_DIM:
    raise _hgx.HgxError("node2vec_incidence: dimension %d is above the %d "
                        "the device engine takes" % (d, MAX_DIM))
  if walk_length > MAX_WALK:
    raise _hgx.HgxError("node2vec_incidence: walk length %d is above the %d "
                        "the device engine takes" % (walk_length, MAX_WALK))
  if negative > MAX_NEGATIVE:
    raise _hgx.HgxError("node2vec_incidence: negative %d is above the %d "
                        "the device engine takes" % (negative, MAX_NEGATIVE))
  if graph == BIPARTITE:
    V = inc.N + inc.E
    # the reference's `assert str(idx) in model.wv`
    assert inc.N > 0 and inc.E > 0
    assert np.diff(inc.rp_n).min() > 0, "a node without an edge"
    assert np.diff(inc.rp_e).min() > 0, "an edge without a node"
    sources = np.arange(V, dtype=np.int64)
  else:
    V = inc.N
    sources = clique_sources(inc).astype(np.int64)
  info = {"sources": sources, "n_walks": num_walks * sources.size}
  if sources.size == 0:  # no edge of two nodes: nothing to walk on
    info.update(counts=np.zeros(V, np.int64), stats={})
    return np.zeros((V, d), np.float32), info
  own = backend is None
  if own:
    from .runtime import get_context
    ctx = ctx or get_context()
    ctx.upload(inc)
    backend = _hgx.N2v(ctx, graph, d)
  be = backend
  try:
    perms = [np.random.permutation(sources) for _ in range(num_walks)]
    wseed = int(np.random.randint(0, 2**31 - 1))
    tseed = int(np.random.randint(0, 2**31 - 1))
    if vectors is None:
      vectors = (np.random.random((V, d)).astype(np.float32) -
                 np.float32(0.5)) / np.float32(d)
    passes = np.repeat(np.arange(num_walks, dtype=np.int32), sources.size)
    be.walks(passes, np.concatenate(perms), walk_length, p, wseed, copy=False)
    counts = be.counts()
    be.set_vocab(keep_thresholds(counts, sample), cum_table(counts))
    be.set_vectors(vectors, None)
    be.train(window=window, negative=negative, epochs=epochs, alpha=alpha,
             min_alpha=min_alpha, seed=tseed, concurrent=bool(run_in_parallel))
    syn0, _ = be.get_vectors()
    info.update(counts=counts, stats=be.stats())
  finally:
    if own:
      be.close()
  syn0 = np.where((counts > 0)[:, None], syn0, np.float32(0))
  return syn0.astype(np.float32), info


def _embed(hypergraph, graph, dimension, p, q, num_walks_per_node, walk_length,
           window, run_in_parallel, ctx, backend_factory, info):
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension > 0
  assert p >= 0 and p <= 1
  assert q >= 1 and q <= 1
  assert num_walks_per_node > 0
  assert walk_length > 0
  assert inc.N > 0
  assert inc.E > 0
  syn0, i = node2vec_incidence(
      inc, graph, dimension, p=p, num_walks=num_walks_per_node,
      walk_length=walk_length, window=window, run_in_parallel=run_in_parallel,
      ctx=ctx, backend=(backend_factory(inc, graph, dimension)
                        if backend_factory else None))
  if info is not None:
    info.update(i)
  return inc, syn0


def EmbedNode2VecBipartide(hypergraph, dimension, p=1, q=1,
                           num_walks_per_node=10, walk_length=5, window=3,
                           run_in_parallel=True, disable_pbar=False, *,
                           ctx=None, backend_factory=None, info=None):
  """embedding.py:165-210: node2vec on the bipartite graph; node vector =
  ``syn0[v]``, edge vector = ``syn0[N + e]``, keyed by the original ids,
  ``method_name = "N2V{walk_length}_BIPARTIDE"``. A node without an edge or
  an edge without a node is an ``AssertionError`` (the reference's ``assert
  str(idx) in model.wv``). ``run_in_parallel`` picks the concurrent trainer
  (``node2vec_incidence``); ``disable_pbar`` changes nothing.
  ``backend_factory`` (a callable: (Incidence, graph, dimension) -> backend,
  e.g. ``NumpyBackend``) replaces the device; a dict passed as ``info``
  receives ``node2vec_incidence``'s info."""
  from .algebraic_distance import coords_to_embedding
  inc, syn0 = _embed(hypergraph, BIPARTITE, dimension, p, q,
                     num_walks_per_node, walk_length, window, run_in_parallel,
                     ctx, backend_factory, info)
  return coords_to_embedding(inc, syn0[:inc.N], syn0[inc.N:], dimension,
                             "N2V{}_BIPARTIDE".format(walk_length))


def edge_centroids(inc, node_vectors):
  """Per edge the float64 mean of its members' float32 vectors, rounded to
  float32 (zero rows included; zeros for an edge without a node)."""
  x = np.asarray(node_vectors, np.float32)
  out = np.zeros((inc.E, x.shape[1]), np.float32)
  for e in range(inc.E):
    mem = inc.col_e[inc.rp_e[e]:inc.rp_e[e + 1]]
    if mem.size:
      out[e] = np.mean(x[mem].astype(np.float64), axis=0)
  return out


def EmbedNode2VecClique(hypergraph, dimension, p=1, q=1, num_walks_per_node=10,
                        walk_length=5, window=3, run_in_parallel=True,
                        disable_pbar=False, *, ctx=None, backend_factory=None,
                        info=None):
  """embedding.py:213-261: node2vec on the clique graph; node vector =
  ``syn0[v]``, zeros for a node outside the graph (one that shares no edge
  with another node), edge vector = the mean of its members' node vectors,
  ``method_name = "N2V{walk_length}_CLIQUE"``. The other arguments are
  ``EmbedNode2VecBipartide``'s."""
  from .algebraic_distance import coords_to_embedding
  inc, syn0 = _embed(hypergraph, CLIQUE, dimension, p, q, num_walks_per_node,
                     walk_length, window, run_in_parallel, ctx,
                     backend_factory, info)
  return coords_to_embedding(inc, syn0, edge_centroids(inc, syn0), dimension,
                             "N2V{}_CLIQUE".format(walk_length))


__all__ = ["node2vec_incidence", "EmbedNode2VecBipartide",
           "EmbedNode2VecClique", "NumpyBackend", "walk_row", "walk_pairs",
           "corpus_plan", "walk_alpha", "keep_thresholds", "cum_table",
           "clique_neighbours", "clique_sources", "edge_centroids",
           "BIPARTITE", "CLIQUE"]
