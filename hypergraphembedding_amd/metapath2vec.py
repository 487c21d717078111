"""metapath2vec / metapath2vec++ baseline on the device (the
``"metapath2vec++"`` key of ``EMBEDDING_OPTIONS``; the reference writes the
program's input with ``utilities/convert_to_metapath2vec.py``, which links
every incidence through a one-author, one-venue "paper", and imports its
output through ``convert_from_metapath2vec.py``). The metapath2vec program is
not a dependency and is not replayed: the feature is restated from the
formulas below, and nothing beyond them is claimed.

Graph. Bipartite, V = N + E: node ``v`` is vertex ``v``, edge ``e`` is vertex
``N + e``. A vertex's type is node or edge.

Corpus. With one paper per incidence the venue-author-venue metapath walk is
a uniform walk on the bipartite graph that starts at an edge. ``sources`` are
the edges with at least one node, in increasing order, as vertices ``N + e``
(``mp_sources``); ``n_src`` is their number. Walk ``g``, ``0 <= g < n_walks =
num_walks * n_src``, has ``pass = g // n_src`` and ``source = sources[g %
n_src]`` and ``L = 1 + 2 * walk_length`` vertices, ``L <= 256``: it is
``node2vec.walk_row(inc, source, pass, L, 1.0, walk_seed)``, the existing
keyed walk at p = 1 with its key and counters unchanged. A node of degree 0
and an empty edge are never reached; they are legal here, unlike in
``NumpyBackend.walks``. One walk is one sentence. The corpus is never
resident: it is generated again, chunk by chunk, wherever it is read.

Vocabulary. ``count[w]`` is the number of occurrences of ``w`` over the
corpus (int64). A vertex with ``count < min_count`` is dropped: it is never
kept, it has weight 0 in the tables and its output is a zero vector. ``keep =
node2vec.keep_thresholds(count', sample)`` with ``count'`` = ``count``, the
dropped vertices set to 0. The negative table (``typed_cum_table``) is a
length-V int32 array of segments: with ``plus_plus`` the two segments ``[0,
N)`` and ``[N, V)``, each ``node2vec.cum_table``'s formula over its own
vertices, scaled on its own to ``2**31 - 1``; without it the one segment
``[0, V)``, ``node2vec.cum_table``. A negative for output word ``w_i``: ``x =
_bounded(draw, cum[last of the segment of w_i's type])``, the negative is the
first ``w`` of that segment with ``cum[w] >= x``. A type without any weight
left is an ``AssertionError`` on the host (an output word is a kept word and
has weight, so a type that occurs as an output word always has some).

Training. Keeps, reduced windows, pair order (input word ``w_j``, output word
``w_i``) and the per-walk linear alpha are ``node2vec.walk_pairs``' and
``walk_alpha``'s rules with ``min_alpha = 1e-4 alpha``. The trainer key is
``(train_seed, epoch << 32 | g)``; the position counter is new, because
positions need 8 bits: ``((pi << 8 | pj) << 4) | slot``, slot 0 the keep
draw, 1 the window reduction, ``2 + k`` negative ``k``. Per pair: ``l1 =
syn0[w_j]`` held fixed; the targets are ``t = w_i`` (label 1), then the
negatives (label 0) in order, one equal to ``w_i`` skipped; each reads
``syn1[t]`` as it stands, this pair's earlier updates included; ``x = l1 .
syn1[t]``; ``g = float32(label - s(x)) * alpha`` with ``s =
line.bounded_sigmoid`` (1 above 6, 0 below -6); ``neu += g * syn1[t]`` (the
row before its own update); ``syn1[t] += g * l1``; at the end ``syn0[w_j] +=
neu``. A product and the sum it enters are two roundings.

Deviations from the metapath2vec program. (1) The exact logistic replaces its
table. (2) Counter-based draws replace its generator and its 1e8-entry
tables. (3) alpha moves per walk, not per 10,000 words of a thread. (4) The
corpus is ordered pass-major, not as a file read by threads at different
offsets. (5) ``l1`` is held fixed within a pair. (6) The concurrent mode
(``mp_chunk_walks`` walks per launch, one wave per walk, float atomic adds)
stands in for ``-threads > 1``.
"""

import bisect

import numpy as np

from . import _hgx
from . import node2vec as n2v
from .hypergraph_util import Incidence
from .line import bounded_sigmoid
from .node2vec import BIPARTITE, MAX_DIM, MAX_NEGATIVE

MAX_SENTENCE = 256  # hgx_n2v_train_mp's limit on L
MAX_STAGE = 512     # negatives staged per output word (include/hgx.h)


def _mp_ctr(pi, pj, slot):
  return (((pi << 8) | pj) << 4) | slot


def mp_sources(inc):
  """The edges with at least one node, in increasing order, as vertices."""
  return inc.N + np.flatnonzero(np.diff(inc.rp_e) > 0).astype(np.int64)


def mp_walk(inc, g, sources, L, walk_seed):
  """Walk ``g`` of the corpus: ``L`` vertices."""
  n_src = len(sources)
  return n2v.walk_row(inc, int(sources[g % n_src]), g // n_src, L, 1.0,
                      walk_seed)


def typed_cum_table(counts, N, plus_plus, power=0.75):
  """The negative table of the module docstring (int32, length V)."""
  counts = np.asarray(counts)
  if not plus_plus:
    return n2v.cum_table(counts, power)
  assert 0 < N < counts.size
  return np.concatenate([n2v.cum_table(counts[:N], power),
                         n2v.cum_table(counts[N:], power)])


def mp_pairs(walk, keep, cum, N, typed, window, negative, seed, epoch, g):
  """(kept words, pairs) of walk ``g`` in ``epoch``: the pairs in training
  order as (input word w_j, output word w_i, [negatives]). ``cum`` is a list
  (bisect)."""
  key = n2v._rand64_key(seed, (epoch << 32) | g)
  V = len(cum)
  kept = []
  for pos, word in enumerate(walk):
    if int(keep[word]) > n2v._bounded(
        n2v._draw(key, _mp_ctr(pos, 0, 0)), 0xffffffff):
      b = n2v._bounded(n2v._draw(key, _mp_ctr(pos, 0, 1)), window)
      kept.append((pos, int(word), window - b))
  pairs = []
  for i, (pi, wi, span) in enumerate(kept):
    lo, hi = (0, V) if not typed else ((0, N) if wi < N else (N, V))
    last = cum[hi - 1]
    for j in range(max(0, i - span), min(len(kept) - 1, i + span) + 1):
      if j == i:
        continue
      pj, wj, _ = kept[j]
      negs = [bisect.bisect_left(
          cum, n2v._bounded(n2v._draw(key, _mp_ctr(pi, pj, 2 + k)), last),
          lo, hi) for k in range(negative)]
      pairs.append((wj, wi, negs))
  return len(kept), pairs


def mp_plan(inc, sources, num_walks, L, walk_seed, keep, cum, typed, window,
            negative, epochs, train_seed):
  """mp_pairs of every (epoch, walk) in training order, in Python integers:
  a list of (kept words, pairs)."""
  cl = [int(v) for v in cum]
  n_walks = num_walks * len(sources)
  walks = [mp_walk(inc, g, sources, L, walk_seed) for g in range(n_walks)]
  return [mp_pairs(walks[g], keep, cl, inc.N, bool(typed), window, negative,
                   train_seed, ep, g)
          for ep in range(epochs) for g in range(n_walks)]


class NumpyBackendMp(n2v.NumpyBackend):
  """``NumpyBackend`` plus the float32 host restatement of the metapath2vec
  protocol (``mp_walks``, ``mp_counts``, ``set_vocab_typed``, ``train_mp``,
  ``stats``); sequential whatever ``concurrent`` says, ``reverse=True`` sums
  every dot product in the reversed column order."""

  def __init__(self, inc, graph, dim, reverse=False):
    super().__init__(inc, graph, dim, reverse=reverse)
    self._mp_vocab = None
    self._vectors = False
    self._stats["mp"] = dict(walks=0, words=0, pairs=0, targets=0, clamped=0)

  def set_vectors(self, syn0, syn1=None):
    super().set_vectors(syn0, syn1)
    self._vectors = True

  def _corpus(self, sources, num_walks, L):
    if self.graph != BIPARTITE:
      raise _hgx.HgxError("metapath2vec: the engine is not on the bipartite "
                          "graph")
    sources = np.asarray(sources, np.int64).ravel()
    assert L >= 1 and num_walks >= 1 and sources.size >= 1
    if L > MAX_SENTENCE:
      raise _hgx.HgxError("metapath2vec: %d vertices per walk above %d" %
                          (L, MAX_SENTENCE))
    if sources.size * num_walks >= 2**31:
      raise _hgx.HgxError("metapath2vec: the walks do not fit 31 bits")
    N = self.inc.N
    assert sources.min() >= N and sources.max() < self.V, "a bad source"
    assert np.all(np.diff(self.inc.rp_e)[sources - N] > 0), "an empty source"
    return sources

  def mp_walks(self, sources, num_walks, L, walk_seed, g0, count):
    sources = self._corpus(sources, num_walks, L)
    assert g0 >= 0 and count >= 0
    assert g0 + count <= sources.size * num_walks
    out = [mp_walk(self.inc, g, sources, L, walk_seed)
           for g in range(g0, g0 + count)]
    return np.array(out, np.int32).reshape(count, L)

  def mp_counts(self, sources, num_walks, L, walk_seed):
    sources = self._corpus(sources, num_walks, L)
    out = np.zeros(self.V, np.int64)
    for g in range(sources.size * num_walks):
      out += np.bincount(mp_walk(self.inc, g, sources, L, walk_seed),
                         minlength=self.V)
    return out

  def set_vocab_typed(self, keep, cum, typed):
    if self.graph != BIPARTITE:
      raise _hgx.HgxError("metapath2vec: the engine is not on the bipartite "
                          "graph")
    keep, cum = np.asarray(keep, np.uint32), np.asarray(cum, np.int32)
    assert keep.size == cum.size == self.V
    N = self.inc.N
    for seg in ((cum[:N], cum[N:]) if typed else (cum,)):
      assert seg[0] >= 0 and np.all(np.diff(seg) >= 0) and seg[-1] > 0
    self._mp_vocab = (keep, cum, bool(typed))

  def train_mp(self, sources, num_walks, L, *, window=7, negative=5, epochs=5,
               alpha=0.025, min_alpha=2.5e-6, walk_seed=0, train_seed=0,
               concurrent=True, plan=None):
    import time
    t0 = time.perf_counter()
    if self.graph != BIPARTITE:
      raise _hgx.HgxError("metapath2vec: the engine is not on the bipartite "
                          "graph")
    assert window >= 1 and epochs >= 0 and negative >= 0
    if negative > MAX_NEGATIVE:
      raise _hgx.HgxError("metapath2vec: negative %d above %d" %
                          (negative, MAX_NEGATIVE))
    sources = self._corpus(sources, num_walks, L)
    if min(2 * window + 1, L) * negative > MAX_STAGE:
      raise _hgx.HgxError("metapath2vec: window %d with %d negatives stages "
                          "more than %d negatives per word" %
                          (window, negative, MAX_STAGE))
    if self._mp_vocab is None or not self._vectors:
      raise _hgx.HgxError("metapath2vec: train_mp before set_vocab_typed or "
                          "set_vectors")
    keep, cum, typed = self._mp_vocab
    n_walks = num_walks * sources.size
    if plan is None:
      plan = mp_plan(self.inc, sources, num_walks, L, walk_seed, keep, cum,
                     typed, window, negative, epochs, train_seed)
    total = epochs * n_walks
    assert len(plan) == total
    syn0, syn1 = self.syn0, self.syn1
    words = npairs = targets = clamped = 0
    for g, (nk, pairs) in enumerate(plan):
      a = np.float32(n2v.walk_alpha(alpha, min_alpha, g, total))
      words += nk
      npairs += len(pairs)
      for wj, wi, negs in pairs:
        l1 = syn0[wj].copy()
        neu = np.zeros(self.dim, np.float32)
        for k, t in enumerate([wi] + negs):
          if k > 0 and t == wi:
            continue
          row = syn1[t]
          x = self._dot(l1, row)
          targets += 1
          clamped += bool(abs(x) > np.float32(n2v.MAX_EXP))
          gg = np.float32((1.0 if k == 0 else 0.0) - bounded_sigmoid(x)) * a
          neu += gg * row
          row += gg * l1
        syn0[wj] = l1 + neu
    self._stats.update(
        train_ms=(time.perf_counter() - t0) * 1e3, walks=total, words=words,
        pairs=npairs, mp=dict(walks=total, words=words, pairs=npairs,
                              targets=targets, clamped=clamped))

  def stats(self):
    out = dict(self._stats)
    out["mp"] = dict(out["mp"])
    return out


def metapath2vec_incidence(inc, dimension, *, plus_plus=True, num_walks=1000,
                           walk_length=100, window=7, negative=5, sample=1e-3,
                           min_count=5, epochs=5, alpha=0.025,
                           run_in_parallel=True, vectors=None, ctx=None,
                           backend=None):
  """metapath2vec++ (``plus_plus``) or metapath2vec on the bipartite graph of
  ``inc``; returns ``(syn0 V x dimension float32, info)``, V = N + E.

  ``num_walks`` walks start at every non-empty edge, each of ``walk_length``
  node / edge rounds: sentences of ``1 + 2 * walk_length`` vertices, at most
  256. The defaults are the walk script's usual setting, the program's
  example command line and word2vec.c's; they were not checked against the
  program.

  Host draws come from numpy's global RandomState in this order (as
  ``line_incidence``'s): ``walk_seed``, then ``train_seed`` (each
  ``np.random.randint(0, 2**31 - 1)``), then ``syn0 = (np.random.random((V,
  d)).astype(float32) - 0.5) / d`` unless ``vectors`` is given. ``syn1``
  starts at zero. ``run_in_parallel=False`` trains the walks one after
  another in corpus order (bit for bit reproducible after
  ``np.random.seed``), ``True`` concurrently with the same draws.

  A vertex that is never reached or occurs fewer than ``min_count`` times
  gets a zero vector; a graph without an incidence is an ``AssertionError``.
  ``info``: ``counts`` (int64), ``dropped`` (the number of vertices with
  ``count < min_count``), ``sources``, ``n_walks`` and the backend's
  ``stats`` (``stats["mp"]``: walks, words, pairs, targets, clamped).
  ``ctx`` and ``backend`` are ``node2vec_incidence``'s; a host backend is
  ``NumpyBackendMp(inc, BIPARTITE, dimension)``.
  """
  d = int(dimension)
  assert d > 0
  assert num_walks > 0 and walk_length >= 0
  assert window >= 1 and epochs >= 0 and negative >= 0 and min_count >= 0
  assert inc.N > 0 and inc.E > 0
  L = 1 + 2 * int(walk_length)
  if d > MAX_DIM:
    raise _hgx.HgxError("metapath2vec_incidence: dimension %d is above the "
                        "%d the device engine takes" % (d, MAX_DIM))
  if L > MAX_SENTENCE:
    raise _hgx.HgxError("metapath2vec_incidence: walk length %d gives "
                        "sentences of %d vertices, above the %d the device "
                        "engine takes" % (walk_length, L, MAX_SENTENCE))
  if negative > MAX_NEGATIVE:
    raise _hgx.HgxError("metapath2vec_incidence: negative %d is above the %d "
                        "the device engine takes" % (negative, MAX_NEGATIVE))
  V = inc.N + inc.E
  sources = mp_sources(inc)
  assert sources.size > 0, "metapath2vec: an incidence without an entry"
  n_walks = int(num_walks) * sources.size
  own = backend is None
  if own:
    from .runtime import get_context
    ctx = ctx or get_context()
    ctx.upload(inc)
    backend = _hgx.N2v(ctx, BIPARTITE, d)
  be = backend
  try:
    wseed = int(np.random.randint(0, 2**31 - 1))
    tseed = int(np.random.randint(0, 2**31 - 1))
    if vectors is None:
      vectors = (np.random.random((V, d)).astype(np.float32) -
                 np.float32(0.5)) / np.float32(d)
    counts = np.asarray(be.mp_counts(sources, num_walks, L, wseed), np.int64)
    live = np.where(counts >= min_count, counts, 0)
    keep = n2v.keep_thresholds(live, sample)
    cum = typed_cum_table(live, inc.N, plus_plus)
    be.set_vocab_typed(keep, cum, bool(plus_plus))
    be.set_vectors(vectors, None)
    be.train_mp(sources, num_walks, L, window=window, negative=negative,
                epochs=epochs, alpha=alpha, min_alpha=1e-4 * alpha,
                walk_seed=wseed, train_seed=tseed,
                concurrent=bool(run_in_parallel))
    syn0, _ = be.get_vectors()
    stats = be.stats()
  finally:
    if own:
      be.close()
  syn0 = np.where((live > 0)[:, None], syn0, np.float32(0)).astype(np.float32)
  return syn0, {"counts": counts, "dropped": int((counts < min_count).sum()),
                "sources": sources, "n_walks": n_walks, "stats": stats}


def EmbedMetapath2Vec(hypergraph, dimension, plus_plus=True, num_walks=1000,
                      walk_length=100, window=7, negative=5, sample=1e-3,
                      min_count=5, epochs=5, alpha=0.025, run_in_parallel=True,
                      disable_pbar=False, *, ctx=None, backend_factory=None,
                      info=None):
  """metapath2vec++ as an embedder: node vector ``syn0[v]``, edge vector
  ``syn0[N + e]``, keyed by the original ids; a vertex that is dropped or
  never reached gets zeros. ``method_name`` is ``"metapath2vec++"``, or
  ``"metapath2vec"`` with ``plus_plus=False``. The other arguments are
  ``metapath2vec_incidence``'s; ``disable_pbar`` changes nothing.
  ``backend_factory`` (a callable: (Incidence, graph, dimension) -> backend,
  e.g. ``NumpyBackendMp``) replaces the device; a dict passed as ``info``
  receives ``metapath2vec_incidence``'s."""
  from .algebraic_distance import coords_to_embedding
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension > 0
  assert inc.N > 0
  assert inc.E > 0
  syn0, i = metapath2vec_incidence(
      inc, dimension, plus_plus=plus_plus, num_walks=num_walks,
      walk_length=walk_length, window=window, negative=negative, sample=sample,
      min_count=min_count, epochs=epochs, alpha=alpha,
      run_in_parallel=run_in_parallel, ctx=ctx,
      backend=(backend_factory(inc, BIPARTITE, dimension) if backend_factory
               else None))
  if info is not None:
    info.update(i)
  return coords_to_embedding(
      inc, syn0[:inc.N], syn0[inc.N:], dimension,
      "metapath2vec++" if plus_plus else "metapath2vec")


__all__ = ["metapath2vec_incidence", "EmbedMetapath2Vec", "NumpyBackendMp",
           "mp_sources", "mp_walk", "mp_pairs", "mp_plan", "typed_cum_table",
           "MAX_SENTENCE", "BIPARTITE"]
