"""CPU: the DeepWalk restatement (hypergraphembedding_amd/deepwalk.py) without
a device: the Huffman tree, the float64 hierarchical-softmax reference
against torch autograd and by hand, NumpyBackendHS against it, and the
embedder through ``backend_factory=NumpyBackendHS``."""

import heapq

import numpy as np
import pytest

import dw_cases as C
import dw_reference as R
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import deepwalk as dw
from hypergraphembedding_amd import embedding as emb_api
from hypergraphembedding_amd import node2vec as n2v
from hypergraphembedding_amd.hypergraph_util import AddNodeToEdge
from hypergraphembedding_amd.proto import Hypergraph


# ---- the Huffman tree ---------------------------------------------------------
def _codes(tree):
  ptr, point, code = tree
  return [tuple(code[ptr[v]:ptr[v + 1]]) for v in range(ptr.size - 1)]


COUNTS = {
    "random": np.random.RandomState(0).randint(0, 50, 200),
    "zipf": (1000 / np.arange(1, 300)).astype(int),
    "equal": np.full(37, 5),
    "some_zero": np.array([4, 0, 0, 9, 1, 0, 2, 2]),
}


@pytest.mark.parametrize("name", list(COUNTS))
def test_huffman_tree_is_a_prefix_code_of_least_cost(name):
  counts = COUNTS[name]
  V = counts.size
  ptr, point, code = tree = dw.huffman_tree(counts)
  assert ptr.dtype == np.int32 and point.dtype == np.int32
  assert code.dtype == np.uint8
  assert ptr.size == V + 1 and ptr[0] == 0 and point.size == code.size == ptr[-1]
  live = np.flatnonzero(counts > 0)
  lens = np.diff(ptr)
  assert np.all(lens[counts == 0] == 0) and np.all(lens[live] > 0)
  assert point.min() >= 0 and point.max() == live.size - 2
  assert set(code) <= {0, 1}
  cs = _codes(tree)
  words = sorted(cs[v] for v in live)
  for a, b in zip(words[:-1], words[1:]):  # sorted: a prefix sits next to it
    assert a != b[:len(a)], (a, b)
  assert sum(2.0**-len(cs[v]) for v in live) == 1.0
  # the cost against an independent Huffman run: the sum of the inner keys
  heap = [int(c) for c in counts[live]]
  heapq.heapify(heap)
  cost = 0
  while len(heap) > 1:
    s = heapq.heappop(heap) + heapq.heappop(heap)
    cost += s
    heapq.heappush(heap, s)
  assert int((counts * lens).sum()) == cost
  # every path starts at the root, and a code prefix names one inner node
  assert np.all(point[ptr[live]] == live.size - 2)
  at = {}
  for v in live:
    for j in range(lens[v]):
      assert at.setdefault(cs[v][:j], point[ptr[v] + j]) == point[ptr[v] + j]
  assert len(set(at.values())) == len(at) == live.size - 1
  again = dw.huffman_tree(counts.copy())
  assert all(np.array_equal(a, b) for a, b in zip(tree, again))


def test_huffman_tree_small_and_tie_rules():
  ptr, point, code = dw.huffman_tree([0, 7, 0])
  assert list(ptr) == [0, 0, 0, 0] and point.size == 0  # one live vertex
  ptr, point, code = dw.huffman_tree([3, 0, 3])          # a tie: the smaller id
  assert list(ptr) == [0, 1, 1, 2] and list(point) == [0, 0]
  assert list(code) == [0, 1]                            # first popped: left, 0
  ptr, point, code = dw.huffman_tree([5, 2])
  assert list(code) == [1, 0]                            # the smaller count: left
  # counts (1, 1, 2): pops (1, 0) and (1, 1) into inner 0 = (2, 3); then pops
  # (2, 2) before (2, 3): vertex 2 is the left child of the root, inner 0 the
  # right one
  ptr, point, code = dw.huffman_tree([1, 1, 2])
  assert list(ptr) == [0, 2, 4, 5]
  assert list(point) == [1, 0, 1, 0, 1] and list(code) == [1, 0, 1, 1, 0]
  # all equal: fixed by the ids alone
  ptr, point, code = dw.huffman_tree([1, 1, 1, 1])
  assert list(point) == [2, 0, 2, 0, 2, 1, 2, 1]
  assert list(code) == [0, 0, 0, 1, 1, 0, 1, 1]


# ---- the float64 reference -------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 64])
def test_pair_update_is_alpha_times_the_autograd_gradient(n):
  """The update of l1 and of every row of the path is -alpha times the
  gradient of the loss -sum_path log s((1 - 2 c) x)."""
  import torch
  rs = np.random.RandomState(n)
  V, d, alpha = 70, 12, 0.05
  syn0, syn1 = rs.uniform(-1, 1, (V, d)), rs.uniform(-0.5, 0.5, (V, d))
  wj = 4
  ts = rs.permutation(V - 1)[:n]
  cs = rs.randint(0, 2, n).astype(np.float64)
  a, b = syn0.copy(), syn1.copy()
  xs = []
  R.pair_step(a, b, wj, ts, cs, alpha, xs)
  assert len(xs) == n and max(abs(x) for x in xs) < 6
  l1 = torch.tensor(syn0[wj], requires_grad=True)
  S = torch.tensor(syn1, requires_grad=True)
  sign = torch.tensor(1.0 - 2.0 * cs)
  loss = -torch.nn.functional.logsigmoid(sign * (S[ts] @ l1)).sum()
  loss.backward()
  assert np.allclose(a[wj] - syn0[wj], -alpha * l1.grad.numpy(), rtol=1e-12,
                     atol=1e-15)
  assert np.allclose(b - syn1, -alpha * S.grad.numpy(), rtol=1e-12, atol=1e-15)
  untouched = [v for v in range(V) if v != wj]
  assert np.array_equal(a[untouched], syn0[untouched])
  # the plan-level trainer's all-rows-at-once form agrees
  tree = (np.array([0, n] + [n] * (V - 1)), ts, cs.astype(np.uint8))
  ref = R.train(syn0, syn1, [(2, [(wj, 0, [])])], tree, alpha, alpha)
  assert np.allclose(ref.syn0, a, rtol=0, atol=1e-15)
  assert np.allclose(ref.syn1, b, rtol=0, atol=1e-15)
  assert ref.path_nodes == n


def test_pair_update_skip_rule_by_hand():
  """A node with |x| >= 6 is skipped while the others of its path are not;
  neu takes a row as it was before its own update."""
  alpha = 0.5
  s = R.sigmoid
  syn0 = np.array([[1.0, 0, 0, 0], [0.5, 0.5, 0, 0]])
  syn1 = np.array([[2.0, 0, 0, 0], [6.5, 1.0, 0, 0], [0, 1.0, 0, 0],
                   [-6.0, 0, 0, 0]])
  a, b = syn0.copy(), syn1.copy()
  # input word 0 (l1 = e_0); the path 0 (c = 0), 1 (x = 6.5), 2 (c = 1, x = 0),
  # 3 (x = -6: at the bound, skipped)
  xs = []
  R.pair_step(a, b, 0, [0, 1, 2, 3], [0, 0, 1, 1], alpha, xs)
  assert xs == [2.0, 6.5, 0.0, -6.0]
  l1 = syn0[0]
  g0 = (1 - 0 - s(2.0)) * alpha
  g2 = (1 - 1 - s(0.0)) * alpha
  assert np.allclose(b[0], syn1[0] + g0 * l1, rtol=0, atol=1e-15)
  assert np.array_equal(b[1], syn1[1]) and np.array_equal(b[3], syn1[3])
  assert np.allclose(b[2], syn1[2] + g2 * l1, rtol=0, atol=1e-15)
  assert np.allclose(a[0], l1 + g0 * syn1[0] + g2 * syn1[2], rtol=0, atol=1e-15)
  assert np.array_equal(a[1], syn0[1])
  tree = (np.array([0, 4, 4]), np.array([0, 1, 2, 3]), np.array([0, 0, 1, 1]))
  ref = R.train(syn0, syn1, [(2, [(0, 0, [])])], tree, alpha, alpha)
  assert np.allclose(ref.syn0, a, rtol=0, atol=1e-15)
  assert np.allclose(ref.syn1, b, rtol=0, atol=1e-15)
  assert ref.margin == 0.0
  # the float32 backend skips the same nodes
  be = dw.NumpyBackendHS(C.K.one_edge_inc(5), n2v.CLIQUE, 4)
  be.set_vocab(np.full(5, 2**32 - 1, np.uint32), np.arange(1, 6))
  be.set_tree(np.array([0, 4, 4, 4, 4, 4]), tree[1], tree[2])
  s0, s1 = np.zeros((5, 4)), np.zeros((5, 4))
  s0[:2], s1[:4] = syn0, syn1
  be.set_vectors(s0, s1)
  be.train_hs(np.array([[1, 0]]), epochs=1, alpha=alpha, min_alpha=alpha,
              plan=[(2, [(0, 0, [])])])
  o0, o1 = be.get_vectors()
  assert np.array_equal(o1[[1, 3]], syn1[[1, 3]].astype(np.float32))
  assert np.allclose(o1[:4], b, rtol=0, atol=1e-6)
  assert np.allclose(o0[:2], a, rtol=0, atol=1e-6)
  assert be.stats()["path_nodes"] == 4


CPU_CASES = {**{k: v for k, v in C.dims().items() if k in ("d8", "d65")},
             **{k: v for k, v in C.windows().items()
                if k in ("L3w9", "L7w3", "L7w1")},
             "chain64_d16": lambda: C.chain64(16), "tiny3": C.tiny3,
             "two": C.two, "hub": C.hub, "zero_count": C.zero_count,
             "skip": C.skip_case}


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_numpy_backend_against_float64(name):
  """Both summation orders sit at float32 distance from the reference."""
  c = CPU_CASES[name]()
  ref, E, runs = c.reference(margin=1.0 if name == "skip" else C.MARGIN)
  print(f"MARGIN {name}: {ref.margin:.3f} E {E[0]:.3g} {E[1]:.3g}")
  for t, rw in enumerate((ref.syn0, ref.syn1)):
    scale = np.abs(rw).max()
    assert E[t] <= 64 * c.d * R.ulp32(scale), (name, C.K.NAMES[t], E[t])
    for w in runs:
      assert w[t].dtype == np.float32
      C.check(c, w, name)
  assert ref.path_nodes == sum(c.path_lengths())
  if name == "skip":
    for w in runs:
      assert np.array_equal(w[1][c.skipped], c.syn1[c.skipped])
      assert not np.any(np.all(w[1][c.moved] == c.syn1[c.moved], axis=1))
    assert np.array_equal(ref.syn1[c.skipped], c.syn1[c.skipped].astype(float))
  if name == "zero_count":
    for w in runs:
      assert np.array_equal(w[0][c.absent], c.syn0[c.absent])


# ---- the drivers on the host backend ---------------------------------------------
def _test_hypergraph():
  hg = Hypergraph()
  for n, e in [(1, 10), (2, 10), (3, 10), (3, 11), (4, 11), (5, 11), (5, 12),
               (6, 12), (1, 12)]:
    AddNodeToEdge(hg, n, e)
  return hg


KW = dict(num_walks_per_node=2, walk_length=6,
          backend_factory=dw.NumpyBackendHS)


def test_embedder_repeats_after_seed():
  hg = _test_hypergraph()
  for graph in (dw.BIPARTITE, dw.CLIQUE):
    out = []
    for _ in range(2):
      np.random.seed(4)
      info = {}
      e = dw.EmbedDeepWalk(hg, 6, run_in_parallel=False, graph=graph,
                           info=info, **KW)
      out.append(e.SerializeToString())
    assert out[0] == out[1]
    assert e.dim == 6 and e.method_name == "deepwalk"
    assert set(e.node) == set(hg.node) and set(e.edge) == set(hg.edge)
    assert all(len(v.values) == 6 and np.all(np.isfinite(v.values))
               for tab in (e.node, e.edge) for v in tab.values())
    assert info["max_code"] >= 3 and info["stats"]["path_nodes"] > 0
    np.random.seed(5)
    assert dw.EmbedDeepWalk(hg, 6, run_in_parallel=False, graph=graph,
                            **KW).SerializeToString() != out[0]


def test_deepwalk_incidence_repeats_after_seed():
  from hypergraphembedding_amd.hypergraph_util import Incidence
  inc = Incidence.from_hypergraph(_test_hypergraph())
  out = []
  for _ in range(2):
    np.random.seed(6)
    be = dw.NumpyBackendHS(inc, dw.BIPARTITE, 5)
    syn0, info = dw.deepwalk_incidence(inc, dw.BIPARTITE, 5, num_walks=2,
                                       walk_length=6, epochs=2, backend=be)
    out.append(syn0)
  assert np.array_equal(out[0], out[1]) and out[0].shape == (9, 5)
  assert out[0].dtype == np.float32 and np.all(np.any(out[0], axis=1))
  assert info["n_walks"] == 18 and info["counts"].sum() == 18 * 6
  # numpy's global stream is drawn in node2vec_incidence's order
  np.random.seed(6)
  [np.random.permutation(9) for _ in range(2)]
  [np.random.randint(0, 2**31 - 1) for _ in range(2)]
  init = (np.random.random((9, 5)).astype(np.float32) - np.float32(0.5)) / 5
  np.random.seed(6)
  be = dw.NumpyBackendHS(inc, dw.BIPARTITE, 5)
  same, _ = dw.deepwalk_incidence(inc, dw.BIPARTITE, 5, num_walks=2,
                                  walk_length=6, epochs=0, backend=be)
  assert np.array_equal(same, init)


def test_errors_exports_and_registry():
  import hypergraphembedding_amd as pkg
  hg = _test_hypergraph()
  with pytest.raises(AssertionError):
    dw.EmbedDeepWalk(hg, 0, **KW)
  with pytest.raises(_hgx.HgxError):
    dw.EmbedDeepWalk(hg, 513, **KW)
  with pytest.raises(_hgx.HgxError):
    dw.EmbedDeepWalk(hg, 4, num_walks_per_node=1, walk_length=129,
                     backend_factory=dw.NumpyBackendHS)
  bad = _test_hypergraph()
  bad.edge[99].weight = 1.0  # an edge no node lists
  with pytest.raises(AssertionError):
    dw.EmbedDeepWalk(bad, 4, **KW)
  be = dw.NumpyBackendHS(C.K.one_edge_inc(70), n2v.CLIQUE, 4)
  with pytest.raises(_hgx.HgxError):  # a path of 65
    be.set_tree(np.array([0, 65] + [65] * 69), np.arange(65) % 60,
                np.zeros(65))
  with pytest.raises(_hgx.HgxError):  # call order
    be.train_hs(np.array([[0, 1]]))
  assert emb_api.EmbedDeepWalk is dw.EmbedDeepWalk is pkg.EmbedDeepWalk
  assert emb_api.deepwalk_incidence is dw.deepwalk_incidence
  assert pkg.deepwalk_incidence is dw.deepwalk_incidence
  assert "EmbedDeepWalk" in emb_api.__all__ and "EmbedDeepWalk" in pkg.__all__
  with pytest.raises(RuntimeError):  # the registry is unchanged
    emb_api.EMBEDDING_OPTIONS["deepwalk"](hg, 4)
