"""Batched RBF C-SVC on the device (csrc/hgx_svc.hip) against the reference's
own solver, sklearn.svm.SVC(C=1, gamma=0.1), through the committed fixture
tests/golden/svc_small.npz (make_golden_svc.py), and the per-edge / per-node
link-prediction experiments built on it (evaluation_util.py:286-449).

The bar on a decision value is 3 A, A the reference's own slack stored in the
fixture: the largest distance of a default-tolerance solve (in either sample
order) from the tight solve. A float32 SMO with libsvm's stopping rule was
rehearsed on the CPU at about 2.1 A; beyond 3 A is an error, not rounding."""

import random

import numpy as np
import pytest

from conftest import golden
from hypergraphembedding_amd import EmbedAlgebraicDistance, _hgx
from hypergraphembedding_amd import evaluation_util as E
from hypergraphembedding_amd.hypergraph_util import FromSparseMatrix
from hypergraphembedding_amd.runtime import get_context
from hypergraphembedding_amd.synthetic import random_hypergraph

pytestmark = pytest.mark.gpu

C, GAMMA, EPS = 1.0, 0.1, 1e-3


@pytest.fixture(scope="module")
def fx():
  return golden("svc_small.npz")


@pytest.fixture(scope="module")
def bar(fx):
  return 3.0 * float(fx["A"])


@pytest.fixture(scope="module")
def solved(fx):
  """Every table of the fixture fitted and queried once."""
  out = {}
  for d in fx["dims"]:
    svc = _hgx.Svc(get_context(), fx[f"tab{d}"])
    iters, status = svc.fit(fx[f"off{d}"], fx[f"row{d}"], fx[f"lab{d}"], C=C,
                            gamma=GAMMA, eps=EPS)
    f = svc.decision(fx[f"qprob{d}"], fx[f"qrow{d}"])
    coef, rho = svc.get()
    out[int(d)] = dict(svc=svc, iters=iters, status=status, f=f, coef=coef,
                       rho=rho)
  yield out
  for v in out.values():
    v["svc"].close()


def compared(fx, d, bar):
  """Queries of table d that are compared: all, but of the identical-rows
  problem only those with |f_tight| above the bar."""
  keep = np.ones(len(fx[f"f_tight{d}"]), bool)
  if int(fx["identical"][0]) == d:
    mine = fx[f"qprob{d}"] == int(fx["identical"][1])
    keep &= ~mine | (np.abs(fx[f"f_tight{d}"]) > bar)
  return keep


def test_decision_values(fx, solved, bar):
  worst = 0.0
  for d in fx["dims"]:
    keep = compared(fx, d, bar)
    err = np.abs(solved[int(d)]["f"].astype(np.float64) - fx[f"f_tight{d}"])
    print(f"d={d}: max |f_device - f_tight| = {err[keep].max():.3e} "
          f"(A = {float(fx['A']):.3e}, bar = {bar:.3e}), iterations up to "
          f"{solved[int(d)]['iters'].max()}")
    worst = max(worst, err[keep].max())
  assert worst < bar, (worst, bar)


def test_predictions(fx, solved, bar):
  excluded = total = 0
  for d in fx["dims"]:
    ft = fx[f"f_tight{d}"]
    clear = np.abs(ft) > bar
    excluded += np.count_nonzero(~clear)
    total += len(ft)
    got = solved[int(d)]["f"] > 0
    assert np.array_equal(got[clear], ft[clear] > 0), d
  print(f"{excluded} of {total} queries within {bar:.3e} of zero")
  assert excluded <= 0.02 * total


def test_dual_feasibility(fx, solved):
  worst = 0.0
  for d in fx["dims"]:
    tab = fx[f"tab{d}"].astype(np.float64)
    off, row, lab = fx[f"off{d}"], fx[f"row{d}"], fx[f"lab{d}"]
    s = solved[int(d)]
    assert np.all(s["status"] == 0), np.flatnonzero(s["status"])
    assert np.all(np.isfinite(s["rho"]))
    for p in range(len(off) - 1):
      sl = slice(off[p], off[p + 1])
      x, sg = tab[row[sl]], np.where(lab[sl] > 0, 1.0, -1.0)
      coef = s["coef"][sl].astype(np.float64)
      alpha, m = coef * sg, off[p + 1] - off[p]
      assert alpha.min() >= 0.0 and alpha.max() <= C, (d, p)
      assert abs(coef.sum()) <= 1e-5 * m, (d, p, coef.sum())
      sq = (x * x).sum(1)
      k = np.exp(-GAMMA * np.maximum(sq[:, None] + sq[None, :] - 2 * x @ x.T, 0))
      u = -sg * (sg * (k @ coef) - 1.0)  # -s G, G = Q alpha - 1
      up = np.where(sg > 0, alpha < C, alpha > 0)
      low = np.where(sg > 0, alpha > 0, alpha < C)
      viol = u[up].max() - u[low].min()
      worst = max(worst, viol)
      assert viol < EPS + 1e-4, (d, p, viol)
  print(f"largest KKT violation {worst:.3e}")


def subset_problems(fx, d, order):
  off, row, lab = fx[f"off{d}"], fx[f"row{d}"], fx[f"lab{d}"]
  parts = [slice(off[p], off[p + 1]) for p in order]
  new_off = np.concatenate([[0], np.cumsum([off[p + 1] - off[p]
                                            for p in order])])
  return (new_off, np.concatenate([row[s] for s in parts]),
          np.concatenate([lab[s] for s in parts]))


def test_independent_of_the_rest_of_the_launch(fx, solved):
  """Reverse order and two halves: bitwise the same coefficients and rho
  per problem (d = 16 holds every tier of the solver)."""
  d = 16
  off = fx[f"off{d}"]
  n = len(off) - 1
  base = solved[d]
  svc = _hgx.Svc(get_context(), fx[f"tab{d}"])
  for order in (list(range(n))[::-1], list(range(n // 2)),
                list(range(n // 2, n))):
    o, r, l = subset_problems(fx, d, order)
    svc.fit(o, r, l, C=C, gamma=GAMMA, eps=EPS)
    coef, rho = svc.get()
    for k, p in enumerate(order):
      assert np.array_equal(coef[o[k]:o[k + 1]],
                            base["coef"][off[p]:off[p + 1]]), p
      assert rho[k] == base["rho"][p], p
  svc.close()


def test_lds_cut_is_an_exact_choice(fx, solved):
  """Tuning svc_lds_m = 192 solves the 129-sample problem from an LDS
  kernel matrix instead of recomputed columns: bitwise the same result."""
  d = 16
  ctx = get_context()
  svc = _hgx.Svc(ctx, fx[f"tab{d}"])
  try:
    ctx.set_tuning("svc_lds_m", 192)
    iters, status = svc.fit(fx[f"off{d}"], fx[f"row{d}"], fx[f"lab{d}"], C=C,
                            gamma=GAMMA, eps=EPS)
  finally:
    ctx.set_tuning("svc_lds_m", 128)
  coef, rho = svc.get()
  assert np.array_equal(coef, solved[d]["coef"])
  assert np.array_equal(rho, solved[d]["rho"])
  assert np.array_equal(iters, solved[d]["iters"])
  with pytest.raises(AssertionError):
    ctx.set_tuning("svc_lds_m", 96)
  svc.close()


def test_validation_leaves_the_engine_usable(fx, solved):
  d = 2
  tab = fx[f"tab{d}"]
  with pytest.raises(ValueError):
    bad = tab.copy()
    bad[3, 1] = np.nan
    _hgx.Svc(get_context(), bad)
  svc = _hgx.Svc(get_context(), tab)
  off = np.array([0, 3, 7], np.int64)
  row = np.array([0, 1, 2, 3, 4, 5, 6], np.int32)
  lab = np.array([1, 0, 0, 1, 1, 0, 0], np.uint8)
  cases = [
      dict(row=np.array([0, 1, len(tab), 3, 4, 5, 6], np.int32)),
      dict(row=np.array([0, -1, 2, 3, 4, 5, 6], np.int32)),
      dict(lab=np.array([1, 1, 1, 1, 1, 0, 0], np.uint8)),  # one class
      dict(lab=np.array([1, 0, 0, 0, 0, 0, 0], np.uint8)),
      dict(off=np.array([0, 0, 7], np.int64)),  # m = 0
      dict(gamma=0.0), dict(gamma=-1.0), dict(C=0.0), dict(eps=0.0),
      dict(eps=-1e-3),
  ]
  for case in cases:
    kw = dict(off=off, row=row, label=lab, C=C, gamma=GAMMA, eps=EPS)
    kw.update({("label" if k == "lab" else k): v for k, v in case.items()})
    with pytest.raises(ValueError):
      svc.fit(**kw)
  # the failed calls left nothing behind: a valid fit gives what a fresh
  # engine gives
  o, r, l = fx[f"off{d}"], fx[f"row{d}"], fx[f"lab{d}"]
  svc.fit(o, r, l, C=C, gamma=GAMMA, eps=EPS)
  with pytest.raises(ValueError):
    svc.decision([len(o) - 1], [0])
  with pytest.raises(ValueError):
    svc.decision([0], [len(tab)])
  coef, rho = svc.get()
  assert np.array_equal(coef, solved[d]["coef"])
  assert np.array_equal(rho, solved[d]["rho"])
  assert np.array_equal(svc.decision(fx[f"qprob{d}"], fx[f"qrow{d}"]),
                        solved[d]["f"])
  svc.close()


def test_iteration_cap_is_flagged(fx, solved):
  d = 100
  svc = _hgx.Svc(get_context(), fx[f"tab{d}"])
  iters, status = svc.fit(fx[f"off{d}"], fx[f"row{d}"], fx[f"lab{d}"], C=C,
                          gamma=GAMMA, eps=EPS, max_iter=3)
  need = solved[d]["iters"]
  assert np.array_equal(status, (need > 3).astype(np.int32))
  assert np.all(iters == np.minimum(need, 3))
  coef, rho = svc.get()
  assert np.all(np.isfinite(coef)) and np.all(np.isfinite(rho))
  assert np.abs(coef).max() <= C
  svc.close()


# ---- end to end -------------------------------------------------------------
@pytest.fixture(scope="module")
def lp_case():
  """random_hypergraph(400, 200, 6) with 200 removed and 200 missing links,
  an algebraic-distance embedding at d = 16 of what is left, plus one node
  without edges and one edge that holds every node."""
  inc = random_hypergraph(N=400, E=200, mean_degree=6, seed=1)
  full = FromSparseMatrix(inc.to_scipy()[0])
  random.seed(1)
  np.random.seed(1)
  hg, removed = E.RemoveRandomConnections(full, 0.12)
  assert len(removed) >= 200
  missing = E.SampleMissingConnections(full, 200)
  emb = EmbedAlgebraicDistance(hg, 16)
  lone, everyone = max(hg.node) + 1, max(hg.edge) + 1
  rs = np.random.RandomState(4)
  hg.node[lone].name = "lone"
  emb.node[lone].values.extend(rs.uniform(0, 1, 16).tolist())
  hg.edge[everyone].nodes.extend(list(emb.node))
  emb.edge[everyone].values.extend(rs.uniform(0, 1, 16).tolist())
  links = removed[:200] + missing + [(lone, 0), (lone, everyone),
                                     (5, everyone), (7, 3)]
  return hg, emb, links, lone, everyone


def reference_links(hg, emb, links, per_edge, seed, bar):
  """The reference's loop (evaluation_util.py:318-352, 414-447) on the
  problems the rng="python" sampler draws: (predicted links, links whose
  decision value is within the bar of zero)."""
  from sklearn.svm import SVC
  pairs = [(n, e) if per_edge else (e, n) for n, e in links
           if n in emb.node and e in emb.edge]
  row, tab = E._neighbor_table(emb, per_edge)
  if per_edge:
    idx2neighbors = {i: e.nodes for i, e in hg.edge.items()}
  else:
    idx2neighbors = {i: n.edges for i, n in hg.node.items()}
  random.seed(seed)
  pr = E.PersonalizedClassifierProblems(idx2neighbors, row,
                                        set(c for _, c in pairs), rng="python")
  tab = tab.astype(np.float64)
  clf = {}
  for p, idx in enumerate(pr.trained):
    sl = slice(pr.off[p], pr.off[p + 1])
    clf[idx] = SVC(C=1, gamma=0.1).fit(tab[pr.row[sl]], pr.label[sl])
  predicted, unsure = [], set()
  for ent, c in pairs:
    link = (ent, c) if per_edge else (c, ent)
    if c in clf:
      f = clf[c].decision_function(tab[row[ent]][None])[0]
      assert (f > 0) == (clf[c].predict(tab[row[ent]][None])[0] == 1)
      if abs(f) <= bar:
        unsure.add(link)
      if f > 0:
        predicted.append(link)
    elif c in pr.everything:
      predicted.append(link)
  return predicted, unsure


@pytest.mark.parametrize("per_edge", [True, False])
def test_end_to_end(lp_case, per_edge):
  hg, emb, links, lone, everyone = lp_case
  fn = (E.PersonalizedEdgeClassifierPrediction if per_edge else
        E.PersonalizedNodeClassifierPrediction)
  random.seed(9)
  got = fn(hg, emb, links, rng="python")
  assert len(set(got)) == len(got) and set(got) <= set(links)
  assert len(got) < len(links)
  if per_edge:  # the edge that holds every node lets everything in
    assert (lone, everyone) in got and (5, everyone) in got
  else:  # the node without edges lets nothing in; (a node's 6 edges against
    # 12 others of a 200-row table may well let nothing in either)
    assert (lone, 0) not in got and (lone, everyone) not in got
  random.seed(9)
  assert fn(hg, emb, links, rng="python") == got
  # through the experiment runner (default sampler)
  good, bad = links[:200], links[200:400]
  name = "LP_EDGE_CLASSIFIERS" if per_edge else "LP_NODE_CLASSIFIERS"
  m = E.RunLinkPredictionExperiment(
      E.LinkPredictionData(hg, emb, good, bad, 0.12), name)
  assert m.experiment_name == name and len(m.records) == 400
  assert 0.0 <= m.accuracy <= 1.0


@pytest.mark.parametrize("per_edge", [True, False])
def test_end_to_end_matches_the_reference_loop(lp_case, per_edge, bar):
  pytest.importorskip("sklearn")
  hg, emb, links, _, _ = lp_case
  random.seed(9)
  got = E.PersonalizedClassifierPrediction(hg, emb, links, per_edge=per_edge,
                                           rng="python")
  want, unsure = reference_links(hg, emb, links, per_edge, 9, bar)
  print(f"{len(want)} links predicted, {len(unsure)} within the bar")
  assert [l for l in got if l not in unsure] == \
      [l for l in want if l not in unsure]


def test_free_vectors_match_table_rows(lp_case):
  hg, emb, _, _, everyone = lp_case
  subset = [e for e in list(hg.edge)[:12]] + [everyone]
  random.seed(3)
  clf = E.GetPersonalizedClassifiers(hg, emb, per_edge=True,
                                     idx_subset=subset)
  assert set(clf) == set(subset)
  assert isinstance(clf[everyone], E.LetEverythingIn)
  row, tab = E._neighbor_table(emb, True)
  rows = np.arange(0, len(tab), 7, dtype=np.int32)
  for idx in subset[:12]:
    c = clf[idx]
    in_table = c.engine.decision(np.full(len(rows), c.prob, np.int32), rows)
    free = c.decision_function(tab[rows])
    assert np.abs(free - in_table).max() <= 1e-6
    assert np.array_equal(c.predict(tab[rows]), (in_table > 0).astype(int))
