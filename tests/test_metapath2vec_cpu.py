"""Host: metapath2vec.py's corpus, vocabulary, plan and NumpyBackendMp (the
float32 restatement of the engine's protocol) against the float64 reference
of mp2v_reference.py, and EmbedMetapath2Vec on the host backend. Inputs,
reference and bar are mp2v_cases.py's.
"""

import numpy as np
import pytest

import mp2v_cases as C
import mp2v_reference as R
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import embedding as emb_api
from hypergraphembedding_amd import metapath2vec as M
from hypergraphembedding_amd import node2vec as n2v
from hypergraphembedding_amd.hypergraph_util import AddNodeToEdge, Incidence
from hypergraphembedding_amd.proto import Hypergraph


# ---- the corpus ----------------------------------------------------------------
@pytest.mark.parametrize("graph", [C.graph_g, C.holes_graph])
def test_walks_start_at_an_edge_and_alternate(graph):
  inc = graph()
  src = M.mp_sources(inc)
  assert list(src) == [inc.N + e for e in range(inc.E) if inc.edge_size()[e]]
  n_src, L = src.size, 11
  for g in (0, 3, n_src - 1, n_src, 2 * n_src + 7):
    w = M.mp_walk(inc, g, src, L, 99)
    assert w == n2v.walk_row(inc, int(src[g % n_src]), g // n_src, L, 1.0, 99)
    assert len(w) == L and w[0] == src[g % n_src]
    assert all((v >= inc.N) == (t % 2 == 0) for t, v in enumerate(w))
    for u, v in zip(w, w[1:]):  # consecutive vertices are incident
      nd, ed = min(u, v), max(u, v) - inc.N
      assert ed in inc.col_n[inc.rp_n[nd]:inc.rp_n[nd + 1]]
  # the same source in another pass draws another walk
  assert M.mp_walk(inc, 0, src, 33, 99) != M.mp_walk(inc, n_src, src, 33, 99)


def test_counts_equal_a_bincount_of_the_walks():
  inc = C.holes_graph()
  src = M.mp_sources(inc)
  be = M.NumpyBackendMp(inc, M.BIPARTITE, 4)
  walks = be.mp_walks(src, 3, 7, 5, 0, 3 * src.size)
  assert walks.shape == (75, 7) and walks.dtype == np.int32
  counts = be.mp_counts(src, 3, 7, 5)
  assert counts.dtype == np.int64 and counts.sum() == 75 * 7
  assert np.array_equal(counts, np.bincount(walks.ravel(), minlength=87))
  assert counts[60] == 0 and counts[61 + 25] == 0  # never reached
  # a window of the corpus across a pass boundary
  part = be.mp_walks(src, 3, 7, 5, 20, 10)
  assert np.array_equal(part, walks[20:30])


# ---- the vocabulary ---------------------------------------------------------------
def test_typed_cum_table():
  rs = np.random.RandomState(0)
  N, V = 7, 12
  counts = rs.randint(1, 50, V)
  counts[[2, 9]] = 0  # dropped
  cum = M.typed_cum_table(counts, N, True)
  assert cum.dtype == np.int32 and cum.size == V
  assert cum[N - 1] == 2**31 - 1 and cum[V - 1] == 2**31 - 1
  assert np.all(np.diff(cum[:N]) >= 0) and np.all(np.diff(cum[N:]) >= 0)
  assert cum[2] == cum[1] and cum[9] == cum[8]  # no weight
  for seg in (slice(0, N), slice(N, V)):
    w = counts[seg].astype(np.float64)**0.75 * (counts[seg] > 0)
    want = np.round(np.cumsum(w) / w.sum() * (2.0**31 - 1))
    assert np.array_equal(cum[seg], want.astype(np.int32))
  assert np.array_equal(M.typed_cum_table(counts, N, False),
                        n2v.cum_table(counts))
  with pytest.raises(AssertionError):  # a type without weight
    M.typed_cum_table(np.array([0, 0, 3, 4]), 2, True)
  # a dropped vertex at the head of a segment
  c2 = np.array([0, 5, 0, 6])
  assert list(M.typed_cum_table(c2, 2, True)) == [0, 2**31 - 1, 0, 2**31 - 1]


def test_plan_negatives_follow_the_type():
  c = C.min_count_case()
  N = c.inc.N
  types = set()
  for _, pairs in c.plan():
    for wj, wi, negs in pairs:
      assert c.live[wj] > 0 and c.live[wi] > 0
      assert len(negs) == 5
      assert all((t < N) == (wi < N) and c.live[t] > 0 for t in negs)
      types.add(wi < N)
  assert types == {True, False}
  u = C.Case("untyped", 16, typed=False, seed=24)
  mixed = [(wi < N, t < N) for _, pairs in u.plan()
           for _, wi, negs in pairs for t in negs]
  assert {(a, b) for a, b in mixed} == {(True, True), (True, False),
                                        (False, True), (False, False)}


def test_plan_counter_and_pair_order():
  """mp_pairs by hand on one walk: keeps, windows and negatives from the
  8-bit counter."""
  c = C.Case("L256", 16, L=256, sources=[60], epochs=1, window=2,
             sample=0.02, seed=43)
  walk = [int(v) for v in c.walks[0]]
  key = n2v._rand64_key(c.train_seed, (0 << 32) | 0)
  kept = []
  for pos, w in enumerate(walk):
    ctr = ((pos << 8) | 0) << 4
    if int(c.keep[w]) > (n2v._draw(key, ctr) * 0xffffffff) >> 64:
      b = (n2v._draw(key, ctr | 1) * 2) >> 64
      kept.append((pos, w, 2 - b))
  nk, pairs = c.plan()[0]
  assert nk == len(kept) and 0 < nk < 256 and kept[-1][0] > 192
  want = []
  for i, (pi, wi, span) in enumerate(kept):
    for j in range(max(0, i - span), min(nk - 1, i + span) + 1):
      if j != i:
        want.append((kept[j][1], wi, pi, kept[j][0]))
  assert [(wj, wi) for wj, wi, _ in pairs] == [(a, b) for a, b, _, _ in want]
  cum = [int(v) for v in c.cum]
  for (wj, wi, negs), (_, _, pi, pj) in zip(pairs[-20:], want[-20:]):
    lo, hi = (0, 60) if wi < 60 else (60, 85)
    for k, t in enumerate(negs):
      x = (n2v._draw(key, ((((pi << 8) | pj) << 4) | (2 + k))) *
           cum[hi - 1]) >> 64
      assert lo <= t < hi and cum[t] >= x and (t == lo or cum[t - 1] < x)


# ---- the trainer -------------------------------------------------------------------
def test_pair_step_is_the_gradient_step():
  """One pair against torch autograd of -log s(x_pos) - sum log s(-x_neg)."""
  import torch
  rs = np.random.RandomState(1)
  s0, s1 = rs.uniform(-1, 1, (6, 5)), rs.uniform(-1, 1, (6, 5))
  a0 = torch.tensor(s0, requires_grad=True)
  a1 = torch.tensor(s1, requires_grad=True)
  wj, wi, negs = 2, 4, [1, 4, 0]  # the negative 4 equals w_i: skipped
  loss = -torch.nn.functional.logsigmoid(a0[wj] @ a1[wi])
  for t in (1, 0):
    loss = loss - torch.nn.functional.logsigmoid(-(a0[wj] @ a1[t]))
  loss.backward()
  r0, r1 = s0.copy(), s1.copy()
  R.pair_step(r0, r1, wj, wi, negs, 0.05)
  assert np.allclose(r0, s0 - 0.05 * a0.grad.numpy(), atol=1e-15)
  assert np.allclose(r1, s1 - 0.05 * a1.grad.numpy(), atol=1e-15)


def test_repeated_negative_reads_the_updated_row():
  rs = np.random.RandomState(2)
  s0, s1 = rs.uniform(-1, 1, (4, 3)), rs.uniform(-1, 1, (4, 3))
  r0, r1 = s0.copy(), s1.copy()
  xs = []
  R.pair_step(r0, r1, 0, 1, [2, 2], 0.5, xs)
  l1 = s0[0]
  x2 = l1 @ s1[2]
  g2 = -R.sigma(x2) * 0.5
  assert np.isclose(xs[2][1], l1 @ (s1[2] + g2 * l1))  # this pair's update
  # clamped: label 1 above 6 moves nothing, label 0 above 6 moves by alpha
  s0 = np.array([[1.0, 0.0]])
  s1 = np.array([[9.0, 0.5]])
  r0, r1 = s0.copy(), s1.copy()
  R.pair_step(r0, r1, 0, 0, [], 0.1)
  assert np.array_equal(r0, s0) and np.array_equal(r1, s1)
  s1 = np.array([[9.0, 0.5], [8.0, 0.0]])
  r0, r1 = np.array([[1.0, 0.0], [0.0, 0.0]]), s1.copy()
  R.pair_step(r0, r1, 0, 0, [1], 0.1)
  assert np.allclose(r1[1], [8.0 - 0.1, 0.0]) and np.allclose(r0[0], [0.2, 0])


CASES = {**C.dims(), **C.d16()}


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_backend_against_float64(name):
  c = CASES[name]()
  ref, E, runs = c.reference()
  for tag, out in zip(("forward", "reversed"), runs):
    C.check(c, out, f"{name} {tag}")
  st = c.numpy_stats
  assert st["mp"] == dict(walks=c.epochs * c.n_walks, words=ref.words,
                          pairs=ref.pairs, targets=ref.targets,
                          clamped=ref.clamped)
  assert st["walks"] == c.epochs * c.n_walks and st["pairs"] == ref.pairs
  assert ref.pairs >= 300 and ref.clamped == 0
  if name != "K0":
    assert not np.array_equal(runs[0][0], runs[1][0])  # two summation orders


def test_clamp_case_on_the_host():
  c = C.clamp_case()
  ref, E, runs = c.reference(margin=1.0)
  assert ref.clamped > 0 and ref.clamped == c.numpy_stats["mp"]["clamped"]
  C.check(c, runs[0], "clamp forward")
  C.check(c, runs[1], "clamp reversed")


# ---- the embedder -------------------------------------------------------------------
def _test_hypergraph():
  hg = Hypergraph()
  for n, e in [(1, 10), (2, 10), (3, 10), (3, 11), (4, 11), (5, 11), (5, 12),
               (6, 12), (1, 12)]:
    AddNodeToEdge(hg, n, e)
  return hg


KW = dict(num_walks=4, walk_length=5, epochs=2, min_count=0,
          backend_factory=M.NumpyBackendMp)


@pytest.mark.parametrize("plus_plus", [True, False])
def test_embedder_repeats_after_seed(plus_plus):
  hg = _test_hypergraph()
  out = []
  for _ in range(2):
    np.random.seed(4)
    info = {}
    e = M.EmbedMetapath2Vec(hg, 6, plus_plus=plus_plus, run_in_parallel=False,
                            info=info, **KW)
    out.append(e.SerializeToString())
  assert out[0] == out[1]
  assert e.dim == 6
  assert e.method_name == ("metapath2vec++" if plus_plus else "metapath2vec")
  assert set(e.node) == set(hg.node) and set(e.edge) == set(hg.edge)
  assert all(len(v.values) == 6 and np.all(np.isfinite(v.values))
             for tab in (e.node, e.edge) for v in tab.values())
  assert info["n_walks"] == 12 and info["counts"].sum() == 12 * 11
  assert info["counts"].dtype == np.int64 and info["dropped"] == 0
  assert info["stats"]["mp"]["walks"] == 24
  assert info["stats"]["mp"]["pairs"] > 0
  np.random.seed(5)
  assert M.EmbedMetapath2Vec(hg, 6, plus_plus=plus_plus,
                             run_in_parallel=False,
                             **KW).SerializeToString() != out[0]


def test_incidence_host_draws_and_zero_vectors():
  # node 1 has no edge, edge 2 no node; node 3 occurs only through edge 1
  inc = Incidence(4, 3, [0, 2, 2, 3, 4], [0, 1, 0, 1])
  np.random.seed(6)
  be = M.NumpyBackendMp(inc, M.BIPARTITE, 5)
  kw = dict(num_walks=6, walk_length=4, sample=0.0, epochs=2)
  out, info = M.metapath2vec_incidence(inc, 5, min_count=0, backend=be, **kw)
  assert out.shape == (7, 5) and out.dtype == np.float32
  dead = np.array([1, 4 + 2])
  assert list(info["sources"]) == [4, 5] and info["n_walks"] == 12
  assert np.all(info["counts"][dead] == 0) and info["dropped"] == 0
  assert np.all(out[dead] == 0)
  live = np.delete(np.arange(7), dead)
  assert np.all(np.any(out[live], axis=1))
  # numpy's global stream: walk seed, train seed, then the vectors
  np.random.seed(6)
  wseed = np.random.randint(0, 2**31 - 1)
  tseed = np.random.randint(0, 2**31 - 1)
  init = (np.random.random((7, 5)).astype(np.float32) - np.float32(0.5)) / 5
  be = M.NumpyBackendMp(inc, M.BIPARTITE, 5)
  counts = be.mp_counts([4, 5], 6, 9, wseed)
  assert np.array_equal(counts, info["counts"])
  be.set_vocab_typed(n2v.keep_thresholds(counts, 0.0),
                     M.typed_cum_table(counts, 4, True), True)
  be.set_vectors(init, None)
  be.train_mp([4, 5], 6, 9, window=7, negative=5, epochs=2, alpha=0.025,
              min_alpha=1e-4 * 0.025, walk_seed=wseed, train_seed=tseed)
  assert np.array_equal(be.get_vectors()[0][live], out[live])
  # epochs = 0 returns the initial vectors
  np.random.seed(6)
  be = M.NumpyBackendMp(inc, M.BIPARTITE, 5)
  same, _ = M.metapath2vec_incidence(inc, 5, min_count=0, backend=be,
                                     **dict(kw, epochs=0))
  assert np.array_equal(same[live], init[live])
  # min_count: the least frequent live vertex is dropped and gets zeros
  least = int(live[np.argmin(counts[live])])
  mc = int(counts[least]) + 1
  assert (counts[live] >= mc).sum() >= 3
  np.random.seed(6)
  be = M.NumpyBackendMp(inc, M.BIPARTITE, 5)
  out2, info2 = M.metapath2vec_incidence(inc, 5, min_count=mc, backend=be,
                                         **kw)
  gone = counts < mc
  assert info2["dropped"] == gone.sum() > 2
  assert np.all(out2[gone] == 0) and np.all(np.any(out2[~gone], axis=1))
  with pytest.raises(AssertionError):  # nnz = 0
    M.metapath2vec_incidence(Incidence(2, 1, [0, 0, 0], []), 4, backend=be)


def test_errors_exports_and_registry():
  import hypergraphembedding_amd as pkg
  hg = _test_hypergraph()
  with pytest.raises(AssertionError):
    M.EmbedMetapath2Vec(hg, 0, **KW)
  with pytest.raises(_hgx.HgxError):
    M.EmbedMetapath2Vec(hg, 513, **KW)
  with pytest.raises(_hgx.HgxError):
    M.EmbedMetapath2Vec(hg, 4, **dict(KW, negative=9))
  with pytest.raises(_hgx.HgxError):  # 257 vertices
    M.EmbedMetapath2Vec(hg, 4, **dict(KW, walk_length=128))
  with pytest.raises(AssertionError):
    M.EmbedMetapath2Vec(hg, 4, **dict(KW, window=0))
  inc = Incidence.from_hypergraph(hg)
  src = M.mp_sources(inc)
  be = M.NumpyBackendMp(inc, M.BIPARTITE, 4)
  with pytest.raises(_hgx.HgxError):  # call order
    be.train_mp(src, 1, 5)
  with pytest.raises(AssertionError):  # a node as a source
    be.mp_walks([0], 1, 5, 0, 0, 1)
  with pytest.raises(_hgx.HgxError):
    be.mp_counts(src, 1, 257, 0)
  with pytest.raises(_hgx.HgxError):  # not the bipartite graph
    M.NumpyBackendMp(inc, n2v.CLIQUE, 4).mp_counts(src, 1, 5, 0)
  for name in ("EmbedMetapath2Vec", "metapath2vec_incidence"):
    assert getattr(emb_api, name) is getattr(M, name) is getattr(pkg, name)
    assert name in emb_api.__all__ and name in pkg.__all__
  with pytest.raises(RuntimeError):  # the registry is unchanged
    emb_api.EMBEDDING_OPTIONS["metapath2vec++"](hg, 4)


def test_new_symbols_are_declared_and_bound():
  names = {"hgx_n2v_mp_walks", "hgx_n2v_mp_counts", "hgx_n2v_set_vocab_typed",
           "hgx_n2v_train_mp", "hgx_n2v_last_mp_stats"}
  assert names <= set(_hgx.header_symbols())
  assert names <= set(_hgx.SIGNATURES)
  for m in ("mp_walks", "mp_counts", "set_vocab_typed", "train_mp",
            "mp_stats"):
    assert callable(getattr(_hgx.N2v, m))
  with open(_hgx.HEADER) as f:
    assert '"mp_chunk_walks"' in f.read()
  assert "mp_chunk_walks" in _hgx.Context.set_tuning.__doc__
  for word in ("exact logistic", "Counter-based draws", "per walk",
               "pass-major", "held fixed within a pair", "-threads > 1"):
    assert word in M.__doc__, word
