"""DeepWalk baseline on the device (the ``"deepwalk"`` key of
``EMBEDDING_OPTIONS``; the reference only imports its results through
``utilities/convert_from_deepwalk.py``). Neither ``deepwalk`` nor ``gensim``
is a dependency: the corpus, the Huffman tree and the skip-gram trainer with
hierarchical softmax (HS) are restated from their formulas,
and nothing beyond those formulas is claimed.

Corpus. ``num_walks`` passes, each ``np.random.permutation(sources)``, one
walk of ``walk_length`` vertices per source and pass, uniform over the
neighbours at every step: node2vec's walks at ``p = 1`` (node2vec.py), on the
bipartite graph (node ``v`` is vertex ``v``, edge ``e`` is vertex ``N + e``;
the default, the paper's DeepWalk ran on the node-edge edge list) or on the
clique graph. Defaults are DeepWalk's: 10 walks per vertex of length 40,
window 5, 5 epochs, ``alpha`` 0.025 to 1e-4, ``sample`` 1e-3. The walk
engine's limits hold: ``walk_length <= 128``, ``dimension <= 512``.

Huffman tree (``huffman_tree``), built on the host in integers and
deterministic. Items: the vertices with ``count > 0``, keyed ``(count, id)``,
``id`` = the vertex. Repeatedly pop the two smallest keys: the first popped is
the left child (code bit 0), the second the right child (code bit 1); the k-th
merge (k = 0, 1, ...) makes inner node k with key ``(sum, V + k)`` and row
``syn1[k]``. n live vertices give n - 1 inner nodes, the root is the last. A
vertex's path is its inner nodes root first, one code bit per inner node. A
vertex with ``count == 0`` has an empty path and is never a target; one live
vertex alone has an empty path too. Layout: ``ptr int32[V + 1]``, ``point
int32[ptr[V]]``, ``code uint8[ptr[V]]``. A path longer than 64 is not taken
by the device (word2vec's C code stops at 40).

Pair step. Keeps, reduced windows and the pair order are the SGNS trainer's
(node2vec.py; key ``(seed, epoch << 32 | walk)``, counter slots 0 and 1 of
``_train_ctr``). Output word ``w_i``, input word ``w_j``, ``l1 = syn0[w_j]``
held fixed; for each inner node ``t`` of ``w_i``'s path, root first, with code
bit ``c``: ``x = l1 . syn1[t]``, skipped when ``|x| >= 6``, ``g = (1 - c -
sigmoid(x)) alpha``, ``neu += g syn1[t]`` (the row before its own update),
``syn1[t] += g l1``; then ``syn0[w_j] += neu``. The rows of a path are
distinct, so with ``l1`` fixed they do not see each other. The sigmoid is the
exact logistic rounded once; a product and the sum it enters are two
roundings.

Deviations. (1) Those of DESIGN §4.10: the exact logistic instead of
word2vec's table, counter-based draws, and the concurrent trainer standing in
for ``workers > 1``. (2) This is HS only, the DeepWalk paper's algorithm: the
``deepwalk`` command line under gensim >= 1.0 leaves gensim's default
``negative=5`` on and trains both objectives; that mixture is not built.
"""

import heapq

import numpy as np

from . import _hgx
from . import node2vec as n2v
from .hypergraph_util import Incidence
from .node2vec import BIPARTITE, CLIQUE, MAX_DIM, MAX_EXP, MAX_WALK

MAX_CODE = 64  # hgx_n2v_set_tree's limit on a path's length


def huffman_tree(counts):
  """``(ptr, point, code)`` of the module docstring's tree over
  ``counts`` (one integer per vertex)."""
  counts = np.asarray(counts)
  V = counts.size
  live = np.flatnonzero(counts > 0)
  heap = [(int(counts[v]), int(v)) for v in live]
  heapq.heapify(heap)
  n_inner = max(live.size - 1, 0)
  parent = np.full(V + n_inner, -1, np.int64)
  bit = np.zeros(V + n_inner, np.uint8)
  for k in range(n_inner):
    c0, left = heapq.heappop(heap)
    c1, right = heapq.heappop(heap)
    parent[left] = parent[right] = V + k
    bit[right] = 1
    heapq.heappush(heap, (c0 + c1, V + k))
  # depth by inner node, the root (the last one) first
  depth = np.zeros(V + n_inner, np.int64)
  for k in range(n_inner - 2, -1, -1):
    depth[V + k] = depth[parent[V + k]] + 1
  lens = np.zeros(V, np.int64)
  if n_inner:
    lens[live] = depth[parent[live]] + 1
  ptr = np.concatenate([[0], np.cumsum(lens)])
  assert ptr[-1] < 2**31
  point = np.empty(ptr[-1], np.int32)
  code = np.empty(ptr[-1], np.uint8)
  # all the live vertices climb at once; step s fills position len - 1 - s
  cur = live[lens[live] > 0]
  at = ptr[cur] + lens[cur] - 1
  while cur.size:
    up = parent[cur]
    point[at] = up - V
    code[at] = bit[cur]
    go = parent[up] >= 0
    cur, at = up[go], at[go] - 1
  return ptr.astype(np.int32), point, code


class NumpyBackendHS(n2v.NumpyBackend):
  """``NumpyBackend`` plus the float32 host restatement of the HS trainer
  (``set_tree``, ``train_hs``); sequential whatever ``concurrent`` says,
  ``reverse=True`` sums every dot product in the reversed column order."""

  def __init__(self, inc, graph, dim, reverse=False):
    super().__init__(inc, graph, dim, reverse=reverse)
    self._tree = None
    self._stats["path_nodes"] = 0

  def set_tree(self, ptr, point, code):
    ptr = np.asarray(ptr, np.int64)
    point, code = np.asarray(point, np.int64), np.asarray(code, np.int64)
    assert ptr.size == self.V + 1 and ptr[0] == 0
    assert np.all(np.diff(ptr) >= 0)
    if np.diff(ptr).max(initial=0) > MAX_CODE:
      raise _hgx.HgxError("deepwalk: a path of %d inner nodes, above %d" %
                          (np.diff(ptr).max(), MAX_CODE))
    assert point.size >= ptr[-1] and code.size >= ptr[-1]
    assert np.all((point >= 0) & (point < self.V - 1))
    assert np.all((code == 0) | (code == 1))
    self._tree = (ptr, point, code)

  def train_hs(self, walks=None, *, window=5, epochs=5, alpha=0.025,
               min_alpha=1e-4, seed=0, concurrent=True, plan=None):
    import time
    t0 = time.perf_counter()
    if walks is not None:
      self._walks = np.array(walks, np.int32)
      assert self._walks.ndim == 2 and self._walks.shape[1] <= MAX_WALK
      assert self._walks.min() >= 0 and self._walks.max() < self.V
    if self._walks is None or self._keep is None or self._tree is None:
      raise _hgx.HgxError("deepwalk: train_hs before the walks, set_vocab "
                          "and set_tree")
    assert window >= 1 and epochs >= 0
    wk = self._walks
    if plan is None:
      plan = n2v.corpus_plan(wk, self._keep, self._cum, window, 0, epochs,
                             seed)
    ptr, point, code = self._tree
    syn0, syn1 = self.syn0, self.syn1
    total = epochs * len(wk)
    words = npairs = nodes = 0
    for g, (nk, pairs) in enumerate(plan):
      a = np.float32(n2v.walk_alpha(alpha, min_alpha, g, total))
      words += nk
      npairs += len(pairs)
      for wj, wi, _ in pairs:
        ts = point[ptr[wi]:ptr[wi + 1]]
        nodes += ts.size
        l1 = syn0[wj].copy()
        S = syn1[ts]
        P = S * l1
        if self.reverse:
          P = P[:, ::-1]
        # products rounded to float32, summed one by one in column order
        x = np.cumsum(P, axis=1, dtype=np.float32)[:, -1]
        lab = 1.0 - code[ptr[wi]:ptr[wi + 1]]
        gg = np.where(np.abs(x) < np.float32(MAX_EXP),
                      (lab - n2v._sigmoid64(x)).astype(np.float32) * a,
                      np.float32(0))
        neu = np.zeros(self.dim, np.float32)
        if ts.size:
          neu = np.cumsum(gg[:, None] * S, axis=0, dtype=np.float32)[-1]
        syn1[ts] = S + gg[:, None] * l1
        syn0[wj] = l1 + neu
    self._stats.update(train_ms=(time.perf_counter() - t0) * 1e3,
                       walks=total, words=words, pairs=npairs,
                       path_nodes=nodes)


def deepwalk_incidence(inc, graph, dimension, *, num_walks=10, walk_length=40,
                       window=5, epochs=5, alpha=0.025, min_alpha=1e-4,
                       sample=1e-3, run_in_parallel=True, vectors=None,
                       ctx=None, backend=None):
  """DeepWalk on the bipartite (``BIPARTITE``) or clique (``CLIQUE``) graph
  of ``inc``; returns ``(syn0 V x dimension float32, info)``, V = N + E or N.

  Host draws come from numpy's global RandomState in
  ``node2vec_incidence``'s order: one ``np.random.permutation(sources)`` per
  pass, the walks' seed, the trainer's seed, then the initial vectors
  ``(np.random.random((V, d)).astype(float32) - 0.5) / d`` unless
  ``vectors`` is given; ``syn1`` starts at zero. ``run_in_parallel=False``
  trains the walks one after another (bit for bit reproducible after
  ``np.random.seed``), ``True`` concurrently with the same draws.

  A vertex that starts no walk keeps a zero vector. ``info``: ``sources``,
  ``n_walks``, ``counts``, ``max_code`` (the longest Huffman path) and the
  backend's ``stats``. ``ctx`` and ``backend`` are ``node2vec_incidence``'s;
  a host backend is ``NumpyBackendHS(inc, graph, dimension)``.
  """
  d = int(dimension)
  assert d > 0
  assert num_walks > 0 and walk_length > 0
  assert window >= 1 and epochs >= 0
  assert graph in (BIPARTITE, CLIQUE)
  if d > MAX_DIM:
    raise _hgx.HgxError("deepwalk_incidence: dimension %d is above the %d "
                        "the device engine takes" % (d, MAX_DIM))
  if walk_length > MAX_WALK:
    raise _hgx.HgxError("deepwalk_incidence: walk length %d is above the %d "
                        "the device engine takes" % (walk_length, MAX_WALK))
  if graph == BIPARTITE:
    V = inc.N + inc.E
    assert inc.N > 0 and inc.E > 0
    assert np.diff(inc.rp_n).min() > 0, "a node without an edge"
    assert np.diff(inc.rp_e).min() > 0, "an edge without a node"
    sources = np.arange(V, dtype=np.int64)
  else:
    V = inc.N
    sources = n2v.clique_sources(inc).astype(np.int64)
  info = {"sources": sources, "n_walks": num_walks * sources.size}
  if sources.size == 0:  # no edge of two nodes: nothing to walk on
    info.update(counts=np.zeros(V, np.int64), max_code=0, stats={})
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
    be.walks(passes, np.concatenate(perms), walk_length, 1.0, wseed,
             copy=False)
    counts = be.counts()
    be.set_vocab(n2v.keep_thresholds(counts, sample), n2v.cum_table(counts))
    ptr, point, code = huffman_tree(counts)
    be.set_tree(ptr, point, code)
    be.set_vectors(vectors, None)
    be.train_hs(window=window, epochs=epochs, alpha=alpha, min_alpha=min_alpha,
                seed=tseed, concurrent=bool(run_in_parallel))
    syn0, _ = be.get_vectors()
    info.update(counts=counts, max_code=int(np.diff(ptr).max()),
                stats=be.stats())
  finally:
    if own:
      be.close()
  syn0 = np.where((counts > 0)[:, None], syn0, np.float32(0))
  return syn0.astype(np.float32), info


def EmbedDeepWalk(hypergraph, dimension, num_walks_per_node=10, walk_length=40,
                  window=5, run_in_parallel=True, disable_pbar=False, *,
                  graph=BIPARTITE, ctx=None, backend_factory=None, info=None):
  """DeepWalk as an embedder, ``method_name = "deepwalk"``. Bipartite graph
  (the default): node vector ``syn0[v]``, edge vector ``syn0[N + e]``; a node
  without an edge or an edge without a node is an ``AssertionError``, as in
  ``EmbedNode2VecBipartide``. Clique graph: zeros for a node outside the
  graph, edge vector = the mean of its members' node vectors
  (``node2vec.edge_centroids``). ``run_in_parallel`` picks the concurrent
  trainer; ``disable_pbar`` changes nothing. ``backend_factory`` (a callable:
  (Incidence, graph, dimension) -> backend, e.g. ``NumpyBackendHS``) replaces
  the device; a dict passed as ``info`` receives ``deepwalk_incidence``'s."""
  from .algebraic_distance import coords_to_embedding
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension > 0
  assert num_walks_per_node > 0
  assert walk_length > 0
  assert inc.N > 0
  assert inc.E > 0
  assert graph in (BIPARTITE, CLIQUE)
  syn0, i = deepwalk_incidence(
      inc, graph, dimension, num_walks=num_walks_per_node,
      walk_length=walk_length, window=window, run_in_parallel=run_in_parallel,
      ctx=ctx, backend=(backend_factory(inc, graph, dimension)
                        if backend_factory else None))
  if info is not None:
    info.update(i)
  if graph == BIPARTITE:
    return coords_to_embedding(inc, syn0[:inc.N], syn0[inc.N:], dimension,
                               "deepwalk")
  return coords_to_embedding(inc, syn0, n2v.edge_centroids(inc, syn0),
                             dimension, "deepwalk")


__all__ = ["deepwalk_incidence", "EmbedDeepWalk", "NumpyBackendHS",
           "huffman_tree", "BIPARTITE", "CLIQUE", "MAX_CODE"]
