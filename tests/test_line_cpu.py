"""CPU: the LINE restatement (hypergraphembedding_amd/line.py) without a
device: the alias table's law, the draws (line_plan), the float64 reference
(line_reference.py) against torch autograd and by hand, NumpyBackendLine
against it on every case of the GPU tests, and the embedder through
``backend_factory=NumpyBackendLine``."""

import numpy as np
import pytest
from scipy.stats import chi2

import line_cases as C
import line_reference as R
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import embedding as emb_api
from hypergraphembedding_amd import line as L
from hypergraphembedding_amd import node2vec as n2v
from hypergraphembedding_amd.hypergraph_util import AddNodeToEdge, Incidence
from hypergraphembedding_amd.proto import Hypergraph

T32 = 2**32 - 1


# ---- the alias table -----------------------------------------------------------
def table_law(thr, alias):
  """The law of the two draws read off the table, in float64: a is uniform
  over the 2^32 - 1 values below 2^32 - 1."""
  n = thr.size
  keep = thr.astype(np.float64) / T32
  law = keep.copy()
  np.add.at(law, alias, 1.0 - keep)
  return law / n


WEIGHTS = {
    "random": np.random.RandomState(0).uniform(0.1, 5.0, 166),
    "zeros": C.weights_g(),
    "heavy": np.r_[np.ones(99), 1e6],
    "equal": np.full(50, 2.5),
    "two": np.array([1.0, 3.0]),
}


@pytest.mark.parametrize("name", list(WEIGHTS))
def test_alias_table_law(name):
  w = WEIGHTS[name]
  thr, alias = L.alias_table(w)
  assert thr.dtype == np.uint32 and alias.dtype == np.int32
  assert thr.size == alias.size == w.size
  assert alias.min() >= 0 and alias.max() < w.size
  law = table_law(thr, alias)
  assert np.abs(law - w / w.sum()).max() <= 2.0**-31
  assert np.all(law[w == 0] == 0.0)
  if name == "equal":
    assert np.all(thr == T32)
  if name == "zeros":
    assert (w == 0).sum() == 10


# ---- the draws -----------------------------------------------------------------
def _arcs(inc):
  rows = np.repeat(np.arange(inc.N), np.diff(inc.rp_n))
  return rows, inc.N + np.asarray(inc.col_n, np.int64)


def _chi2_p(obs, law, n):
  """p-value of the counts ``obs`` of ``n`` draws against ``law``; cells of
  probability 0 must be empty, every other expects at least 20."""
  live = law > 0
  assert np.all(obs[~live] == 0)
  exp = n * law[live]
  assert exp.min() >= 20, exp.min()
  stat = ((obs[live] - exp)**2 / exp).sum()
  return chi2.sf(stat, live.sum() - 1)


@pytest.mark.parametrize("weighted", [False, True])
def test_line_plan_arcs_and_laws(weighted):
  inc = C.graph_g()
  w = C.weights_g() if weighted else None
  thr, alias, cum = C.tables(inc, w)
  law_p = (np.full(166, 1 / 166) if w is None else w / w.sum())
  rows, cols = _arcs(inc)
  # positions and direction: K = 0, sized by the rarest position
  n = int(np.ceil(20.5 / law_p[law_p > 0].min()))
  plan = L.line_plan(inc, thr, alias, cum, 0, n, seed=5)
  assert plan.shape == (n, 2)
  node_first = plan[:, 0] < inc.N
  nd = np.where(node_first, plan[:, 0], plan[:, 1])
  ed = np.where(node_first, plan[:, 1], plan[:, 0])
  assert np.all((nd < inc.N) & (ed >= inc.N) & (ed < inc.N + inc.E))
  # every (u, v) is an incidence: its position in the node-major CSR
  pos = np.array([inc.rp_n[a] + np.searchsorted(
      inc.col_n[inc.rp_n[a]:inc.rp_n[a + 1]], b - inc.N)
                  for a, b in zip(nd, ed)])
  assert np.all(rows[pos] == nd) and np.all(cols[pos] == ed)
  # the stated direction: counter 2 of the sample's key
  for s in range(200):
    back = n2v._bounded(n2v._draw(n2v._rand64_key(5, s), 2), 2)
    assert bool(back) == (not node_first[s])
  p_pos = _chi2_p(np.bincount(pos, minlength=166), law_p, n)
  p_dir = _chi2_p(np.bincount(node_first.astype(int), minlength=2),
                  np.array([0.5, 0.5]), n)
  # negatives against deg ** 0.75: K = 8, sized by the rarest vertex
  deg = L.line_degrees(inc, w)
  law_v = np.where(deg > 0, deg**0.75, 0.0)
  law_v /= law_v.sum()
  m = int(np.ceil(20.5 / law_v[law_v > 0].min() / 8))
  negs = L.line_plan(inc, thr, alias, cum, 8, m, seed=6)[:, 2:]
  p_neg = _chi2_p(np.bincount(negs.ravel(), minlength=85), law_v, 8 * m)
  print(f"CHI2 weighted={weighted} n {n} m {m}: positions {p_pos:.3g} "
        f"direction {p_dir:.3g} negatives {p_neg:.3g}")
  assert min(p_pos, p_dir, p_neg) > 1e-4, (p_pos, p_dir, p_neg)


def test_line_plan_from_s0_is_a_slice():
  inc = C.graph_g()
  arcs = C.tables(inc, C.weights_g())
  full = L.line_plan(inc, *arcs, 5, 300, seed=9)
  assert np.array_equal(L.line_plan(inc, *arcs, 5, 100, seed=9, s0=150),
                        full[150:250])
  big = L.line_plan(inc, *arcs, 3, 4, seed=9, s0=2**33 + 5)
  assert big.shape == (4, 5) and big.min() >= 0 and big.max() < 85
  assert not np.array_equal(big, L.line_plan(inc, *arcs, 3, 4, seed=9, s0=5))


def test_line_rho_schedule():
  r0 = float(np.float32(0.025))
  assert L.line_rho(0.025, 0, 100) == np.float32(r0)
  assert L.line_rho(0.025, 50, 100) == np.float32(r0 * (1 - 50 / 101))
  assert L.line_rho(0.025, 10**9, 10**9) == np.float32(1e-4 * r0)
  assert L.line_rho(0.025, 3, 7).dtype == np.float32


# ---- the float64 reference ------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_step_is_rho_times_the_autograd_gradient(order):
  """Distinct targets, none equal to u: the update of l1 and of every target
  row is -rho times the gradient of -log s(x_v) - sum log s(-x_neg)."""
  import torch
  rs = np.random.RandomState(order)
  V, d, rho = 30, 12, 0.05
  syn0, syn1 = rs.uniform(-1, 1, (V, d)), rs.uniform(-0.5, 0.5, (V, d))
  smp = [4, 9, 1, 17, 22, 8, 29]
  a, b = syn0.copy(), syn1.copy()
  xs = []
  R.step(a, a if order == 1 else b, smp, rho, xs)
  assert len(xs) == 6 and max(abs(x) for _, x in xs) < 6
  S0 = torch.tensor(syn0, requires_grad=True)
  S1 = torch.tensor(syn1, requires_grad=True)
  tg = S0 if order == 1 else S1
  # l1 is held fixed while the targets move: the targets' gradient is taken
  # at the initial l1, and l1's at the initial targets
  x = tg[smp[1:]] @ S0[smp[0]]
  sign = torch.tensor([1.0] + [-1.0] * 5)
  loss = -torch.nn.functional.logsigmoid(sign * x).sum()
  loss.backward()
  assert np.allclose(a - syn0, -rho * S0.grad.numpy(), rtol=1e-12, atol=1e-15)
  if order == 2:
    assert np.allclose(b - syn1, -rho * S1.grad.numpy(), rtol=1e-12,
                       atol=1e-15)
  else:
    assert np.array_equal(b, syn1)
  ref = R.train(syn0, syn1, np.array([smp]), order, rho)
  rho0 = R.rho_of(rho, 0, 1)
  c, e = syn0.copy(), syn1.copy()
  R.step(c, c if order == 1 else e, smp, rho0)
  assert np.array_equal(ref.syn0, c) and np.array_equal(ref.syn1, e)
  assert ref.clamped == 0 and ref.targets == 6


def test_step_by_hand_repeats_and_collisions():
  s, rho = R.sigma, 0.5
  l1 = np.array([1.0, 2.0])
  # order 2, a repeated negative: the second visit reads the moved row
  syn0 = np.array([l1, [0.0, 0.0], [0.0, 0.0]])
  syn1 = np.array([[0.0, 0.0], [0.5, -0.25], [0.25, 0.5]])
  a, b = syn0.copy(), syn1.copy()
  R.step(a, b, [0, 1, 2, 2], rho)
  g0 = (1 - s(l1 @ syn1[1])) * rho
  g1 = (0 - s(l1 @ syn1[2])) * rho
  row = syn1[2] + g1 * l1
  g2 = (0 - s(l1 @ row)) * rho
  assert np.allclose(b[1], syn1[1] + g0 * l1, rtol=0, atol=1e-15)
  assert np.allclose(b[2], row + g2 * l1, rtol=0, atol=1e-15)
  assert np.allclose(a[0], l1 + g0 * syn1[1] + g1 * syn1[2] + g2 * row, rtol=0,
                     atol=1e-15)
  # order 2, a negative equal to v: it is kept, and reads v's moved row
  a, b = syn0.copy(), syn1.copy()
  R.step(a, b, [0, 1, 1], rho)
  row = syn1[1] + g0 * l1
  g1 = (0 - s(l1 @ row)) * rho
  assert np.allclose(b[1], row + g1 * l1, rtol=0, atol=1e-15)
  assert np.allclose(a[0], l1 + g0 * syn1[1] + g1 * row, rtol=0, atol=1e-15)
  # order 1, a negative equal to u: final row = l1 + g l1 + err
  t0 = np.array([l1, [0.5, -0.25], [0.0, 0.0]])
  a = t0.copy()
  R.step(a, a, [0, 1, 0], rho)
  g0 = (1 - s(l1 @ t0[1])) * rho
  g1 = (0 - s(l1 @ l1)) * rho
  err = g0 * t0[1] + g1 * l1
  assert np.allclose(a[1], t0[1] + g0 * l1, rtol=0, atol=1e-15)
  assert np.allclose(a[0], l1 + g1 * l1 + err, rtol=0, atol=1e-15)


def test_step_by_hand_clamped_targets():
  """One clamped target of each sign and label: sigma is 1 or 0 exactly, so
  g is 0, -rho (label 0, x > 6) or +rho (label 1, x < -6)."""
  rho = 0.5
  l1 = np.array([1.0, 0.0])
  syn0 = np.array([l1] + [[0.0, 0.0]] * 4)
  syn1 = np.array([[0.0, 0.0], [7.0, 1.0], [-8.0, 1.0], [9.0, 2.0],
                   [-6.5, 3.0]])
  for v, negs, moved in ((1, [3, 4], {3: -rho}), (2, [4, 3], {2: rho, 3: -rho})):
    a, b = syn0.copy(), syn1.copy()
    xs = []
    R.step(a, b, [0, v] + negs, rho, xs)
    assert [x for _, x in xs] == [syn1[t][0] for t in [v] + negs]
    err = np.zeros(2)
    for t in range(5):
      g = moved.get(t, 0.0)
      assert np.array_equal(b[t], syn1[t] + g * l1), t
      err += g * syn1[t]
    assert np.array_equal(a[0], l1 + err)
  kinds = set()
  for smp in ([0, 1, 3, 4], [0, 2, 4, 3]):
    ref = R.train(syn0, syn1, np.array([smp]), 2, rho)
    assert ref.clamped == 3 and ref.margin == 0.5 and ref.targets == 3
    kinds |= ref.kinds
  assert kinds == {(1, 1), (1, -1), (0, 1), (0, -1)}
  assert R.sigma(6.0) == 1 / (1 + np.exp(-6.0)) and R.sigma(-6.0) > 0


# ---- NumpyBackendLine against float64 --------------------------------------------
CPU_CASES = {**C.dims(), **C.d16(),
             "clamp_o1": lambda: C.clamp_case(1),
             "clamp_o2": lambda: C.clamp_case(2),
             "wave_d16o1": lambda: C.one_wave(16, 1),
             "wave_d200o2": lambda: C.one_wave(200, 2)}


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_numpy_backend_against_float64(name):
  """Both summation orders sit at float32 distance from the reference."""
  c = CPU_CASES[name]()
  clamp = name.startswith("clamp")
  ref, E, runs = c.reference(margin=1.0 if clamp else C.MARGIN)
  print(f"MARGIN {name}: {ref.margin:.3f} max |x| {ref.max_x:.3f} "
        f"E {E[0]:.3g} {E[1]:.3g}")
  for t, rw in enumerate((ref.syn0, ref.syn1)):
    scale = np.abs(rw).max()
    assert E[t] <= 64 * c.d * R.ulp32(scale), (name, C.NAMES[t], E[t])
  for w in runs:
    assert w[0].dtype == np.float32
    C.check(c, w, name)
  st = c.numpy_stats
  assert st["samples"] == c.T and st["targets"] == c.T * (1 + c.negative)
  assert st["clamped"] == ref.clamped and ref.targets == st["targets"]
  assert (ref.clamped > 0) == clamp
  if c.order == 1:
    assert all(np.array_equal(w[1], c.syn1) for w in runs)


# ---- the drivers on the host backend -----------------------------------------------
def _test_hypergraph():
  hg = Hypergraph()
  for n, e in [(1, 10), (2, 10), (3, 10), (3, 11), (4, 11), (5, 11), (5, 12),
               (6, 12), (1, 12)]:
    AddNodeToEdge(hg, n, e)
  return hg


KW = dict(samples=400, backend_factory=L.NumpyBackendLine)


@pytest.mark.parametrize("order", [1, 2, "both"])
def test_embedder_repeats_after_seed(order):
  hg = _test_hypergraph()
  out = []
  for _ in range(2):
    np.random.seed(4)
    info = {}
    e = L.EmbedLine(hg, 6, order=order, run_in_parallel=False, info=info, **KW)
    out.append(e.SerializeToString())
  assert out[0] == out[1]
  assert e.dim == 6 and e.method_name == "LINE"
  assert set(e.node) == set(hg.node) and set(e.edge) == set(hg.edge)
  assert all(len(v.values) == 6 and np.all(np.isfinite(v.values))
             for tab in (e.node, e.edge) for v in tab.values())
  assert info["n_samples"] == 400 and info["degrees"].size == 9
  assert info["stats"]["samples"] == 400
  assert info["stats"]["targets"] == 2400 and info["stats"]["clamped"] == 0
  np.random.seed(5)
  assert L.EmbedLine(hg, 6, order=order, run_in_parallel=False,
                     **KW).SerializeToString() != out[0]
  if order == "both":
    x = np.array([v.values for tab in (e.node, e.edge) for v in tab.values()])
    for half in (x[:, :3], x[:, 3:]):
      assert np.allclose(np.linalg.norm(half, axis=1), 1.0, atol=1e-6)
    with pytest.raises(AssertionError):
      L.EmbedLine(hg, 5, order="both", **KW)


def test_line_incidence_host_draws_and_zero_degree():
  # node 1 has no edge, edge 2 no node: degree 0, zero vectors
  inc = Incidence(4, 3, [0, 2, 2, 3, 4], [0, 1, 0, 1])
  np.random.seed(6)
  be = L.NumpyBackendLine(inc, L.BIPARTITE, 5)
  out, info = L.line_incidence(inc, 5, samples=200, backend=be)
  assert out.shape == (7, 5) and out.dtype == np.float32
  dead = np.array([1, 4 + 2])
  assert np.all(info["degrees"][dead] == 0)
  assert (info["degrees"] > 0).sum() == 5
  assert np.all(out[dead] == 0)
  assert np.all(np.any(np.delete(out, dead, axis=0), axis=1))
  # numpy's global stream: the seed, then the vectors
  np.random.seed(6)
  seed = np.random.randint(0, 2**31 - 1)
  init = (np.random.random((7, 5)).astype(np.float32) - np.float32(0.5)) / 5
  np.random.seed(6)
  be = L.NumpyBackendLine(inc, L.BIPARTITE, 5)
  same, _ = L.line_incidence(inc, 5, samples=0, backend=be)
  live = np.delete(np.arange(7), dead)
  assert np.array_equal(same[live], init[live])
  # ... and the run above is that seed's
  be = L.NumpyBackendLine(inc, L.BIPARTITE, 5)
  be.set_arcs(None, None, n2v.cum_table(info["degrees"], 0.75))
  be.set_vectors(init, None)
  be.train_line(2, 5, 200, rho=0.025, seed=seed)
  assert np.array_equal(be.get_vectors()[0][live], out[live])
  # weights: an incidence of weight 0 is never drawn
  w = np.array([1.0, 0.0, 2.0, 3.0])
  be = L.NumpyBackendLine(inc, L.BIPARTITE, 5)
  _, info = L.line_incidence(inc, 5, samples=50, weights=w, backend=be)
  assert list(info["degrees"]) == [1.0, 0.0, 2.0, 3.0, 3.0, 3.0, 0.0]
  plan = L.line_plan(inc, *L.alias_table(w), n2v.cum_table(info["degrees"]),
                     0, 300, seed=1)
  assert not np.any(np.all(np.sort(plan, axis=1) == [0, 5], axis=1))
  with pytest.raises(AssertionError):  # nnz = 0
    L.line_incidence(Incidence(2, 1, [0, 0, 0], []), 4, samples=10,
                     backend=None)


def test_errors_exports_and_registry():
  import hypergraphembedding_amd as pkg
  hg = _test_hypergraph()
  with pytest.raises(AssertionError):
    L.EmbedLine(hg, 0, **KW)
  with pytest.raises(_hgx.HgxError):
    L.EmbedLine(hg, 513, **KW)
  with pytest.raises(_hgx.HgxError):
    L.EmbedLine(hg, 4, negative=9, **KW)
  with pytest.raises(AssertionError):
    L.EmbedLine(hg, 4, order=3, **KW)
  inc = Incidence.from_hypergraph(hg)
  be = L.NumpyBackendLine(inc, L.BIPARTITE, 4)
  with pytest.raises(_hgx.HgxError):  # call order
    be.train_line(2, 5, 10)
  with pytest.raises(_hgx.HgxError):  # not the bipartite graph
    L.NumpyBackendLine(inc, n2v.CLIQUE, 4).set_arcs(None, None, np.arange(1, 7))
  assert emb_api.EmbedLine is L.EmbedLine is pkg.EmbedLine
  assert emb_api.line_incidence is L.line_incidence is pkg.line_incidence
  assert "EmbedLine" in emb_api.__all__ and "EmbedLine" in pkg.__all__
  assert "line_incidence" in emb_api.__all__ and "line_incidence" in pkg.__all__
  with pytest.raises(RuntimeError):  # the registry is unchanged
    emb_api.EMBEDDING_OPTIONS["LINE"](hg, 4)


def test_new_symbols_are_declared_and_bound():
  names = {"hgx_n2v_set_arcs", "hgx_n2v_line_samples", "hgx_n2v_train_line",
           "hgx_n2v_last_line_stats"}
  assert names <= set(_hgx.header_symbols())
  assert names <= set(_hgx.SIGNATURES)
  for m in ("set_arcs", "line_samples", "train_line"):
    assert callable(getattr(_hgx.N2v, m))
  with open(_hgx.HEADER) as f:
    assert '"line_chunk_samples"' in f.read()
  assert "line_chunk_samples" in _hgx.Context.set_tuning.__doc__
