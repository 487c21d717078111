"""Host side of the per-edge / per-node SVC link prediction
(evaluation_util.py:286-449): the negative sampler, the link filtering, the
experiment registry, the committed fixture against sklearn and the new ABI
symbols. No GPU."""

import ctypes
import importlib.util
import os
import random
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, golden
from hypergraphembedding_amd import Hypergraph, HypergraphEmbedding, _hgx, build
from hypergraphembedding_amd import evaluation_util as E
from hypergraphembedding_amd.hypergraph_util import AddNodeToEdge

SVC_SYMBOLS = ("hgx_svc_create", "hgx_svc_destroy", "hgx_svc_fit",
               "hgx_svc_decision", "hgx_svc_decision_vec", "hgx_svc_get",
               "hgx_svc_last_stats")


def neighbourhoods(seed, n_rows=90, n_idx=40):
  """idx -> neighbours over a table whose ids are not its row numbers, with
  an empty, a full and a nearly full neighbourhood among them."""
  rs = np.random.RandomState(seed)
  ids = [int(v) for v in rs.permutation(1000)[:n_rows]]
  neighbor_row = {v: i for i, v in enumerate(ids)}
  idx2neighbors = {}
  for idx in range(n_idx):
    k = int(rs.randint(1, 30))
    idx2neighbors[idx] = [ids[i] for i in rs.choice(n_rows, k, replace=False)]
  idx2neighbors[n_idx] = []
  idx2neighbors[n_idx + 1] = list(ids)
  idx2neighbors[n_idx + 2] = ids[:n_rows - 3]  # non-neighbours run out
  idx2neighbors[n_idx + 3] = ids[:n_rows // 2]  # more neighbours than 2x fits
  return idx2neighbors, neighbor_row


@pytest.mark.parametrize("rng", [None, "python"])
@pytest.mark.parametrize("seed", [0, 1])
def test_sampler_counts_and_membership(seed, rng):
  idx2neighbors, neighbor_row = neighbourhoods(seed)
  random.seed(seed)
  pr = E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row,
                                        list(idx2neighbors), rng=rng)
  n_rows = len(neighbor_row)
  assert pr.nothing == [40] and pr.everything == [41]
  assert 40 not in pr.trained and 41 not in pr.trained
  assert len(pr.trained) == len(idx2neighbors) - 2 == len(pr.off) - 1
  assert pr.off.dtype == np.int64 and pr.row.dtype == np.int32
  assert pr.label.dtype == np.uint8 and pr.off[0] == 0
  for p, idx in enumerate(pr.trained):
    rows = pr.row[pr.off[p]:pr.off[p + 1]]
    lab = pr.label[pr.off[p]:pr.off[p + 1]]
    want = {neighbor_row[n] for n in idx2neighbors[idx]}
    pos, neg = rows[lab == 1], rows[lab == 0]
    assert set(pos.tolist()) == want and len(pos) == len(want)
    assert len(neg) == min(n_rows - len(want), 2 * len(want))
    assert not set(neg.tolist()) & want          # no neighbour among them
    assert len(set(neg.tolist())) == len(neg)     # no duplicates
    assert neg.min() >= 0 and neg.max() < n_rows


def test_sampler_default_mode_follows_random_seed():
  idx2neighbors, neighbor_row = neighbourhoods(5)
  subset = list(idx2neighbors)
  random.seed(11)
  a = E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row, subset)
  random.seed(11)
  b = E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row, subset)
  random.seed(12)
  c = E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row, subset)
  assert np.array_equal(a.row, b.row) and np.array_equal(a.off, b.off)
  assert np.array_equal(a.label, b.label)
  assert not np.array_equal(a.row, c.row)


def test_sampler_default_mode_is_uniform():
  """Every non-neighbour is equally likely (both the rejection and the
  dense branch): counts over many draws stay within 5 sigma of the mean."""
  n_rows = 40
  neighbor_row = {i: i for i in range(n_rows)}
  for n_pos in (3, 12):  # 2 * 3 of 37: rejection; 2 * 12 of 28: dense
    idx2neighbors = {k: list(range(n_pos)) for k in range(3000)}
    random.seed(n_pos)
    pr = E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row,
                                          list(idx2neighbors))
    neg = pr.row[pr.label == 0]
    counts = np.bincount(neg, minlength=n_rows)[n_pos:]
    prob = 2 * n_pos / (n_rows - n_pos)
    sigma = np.sqrt(3000 * prob * (1 - prob))
    assert np.abs(counts - 3000 * prob).max() < 5 * sigma, counts


def test_sampler_python_mode_is_the_reference_expression():
  idx2neighbors, neighbor_row = neighbourhoods(7)
  subset = [k for k in idx2neighbors if k % 3 != 1]
  random.seed(21)
  pr = E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row, subset,
                                        rng="python")
  state = random.getstate()
  # the reference's lines (evaluation_util.py:327-338) on a tuple of the set
  neighbor_idx2embedding = neighbor_row
  random.seed(21)
  want = {}
  for idx in subset:
    pos_indices = set(idx2neighbors[idx])
    if len(pos_indices) == 0:
      continue
    neg_indices = neighbor_idx2embedding.keys() - pos_indices
    if len(neg_indices) == 0:
      continue
    want[idx] = (list(pos_indices), random.sample(
        tuple(neighbor_idx2embedding.keys() - pos_indices),
        min(len(neg_indices), len(pos_indices) * 2)))
  assert random.getstate() == state
  assert pr.trained == list(want)
  for p, idx in enumerate(pr.trained):
    rows = pr.row[pr.off[p]:pr.off[p + 1]].tolist()
    pos, neg = want[idx]
    assert rows == [neighbor_row[n] for n in pos + neg]


def test_sampler_rejects_unknown_mode_and_missing_idx():
  idx2neighbors, neighbor_row = neighbourhoods(2)
  with pytest.raises(ValueError):
    E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row, [0],
                                     rng="mt19937")
  with pytest.raises(KeyError):
    E.PersonalizedClassifierProblems(idx2neighbors, neighbor_row, [0, 999])


class RecordingSvc:
  """Stands in for _hgx.Svc: records the calls, scores by a fixed rule."""

  def __init__(self, ctx, table):
    self.table = np.array(table)
    self.dim = self.table.shape[1]
    RecordingSvc.last = self

  def fit(self, off, row, label, **kw):
    self.off, self.row, self.label, self.kw = off, row, label, kw
    return np.zeros(len(off) - 1, np.int32), np.zeros(len(off) - 1, np.int32)

  def decision(self, prob, row):
    self.q = (np.array(prob), np.array(row))
    return np.where(np.asarray(row) % 2 == 0, 0.5, -0.5).astype(np.float32)

  def close(self):
    self.closed = True


@pytest.fixture
def recording(monkeypatch):
  monkeypatch.setattr(E._hgx, "Svc", RecordingSvc)
  monkeypatch.setattr(E, "get_context", lambda: None)
  return RecordingSvc


def small_case():
  hg = Hypergraph()
  for n, e in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 1), (5, 2), (0, 2)):
    AddNodeToEdge(hg, n, e)
  emb = HypergraphEmbedding()
  emb.dim = 2
  for n in range(6):
    emb.node[n].values.extend([float(n), 1.0])
  for e in range(3):
    emb.edge[e].values.extend([float(e), -1.0])
  return hg, emb


def test_link_filtering_and_needed_classifiers_only(recording):
  hg, emb = small_case()
  links = [(0, 1), (9, 1), (1, 7), (2, 0), (3, 0), (4, 2)]
  random.seed(0)
  got = E.PersonalizedClassifierPrediction(hg, emb, links, per_edge=True)
  svc = recording.last
  # (9, 1) and (1, 7) have no embedding; edges 0, 1, 2 are needed, not more
  assert len(svc.off) - 1 == 3
  assert svc.kw == {"C": 1.0, "gamma": 0.1, "eps": 1e-3}
  assert sorted(svc.q[1].tolist()) == [0, 2, 3, 4]  # node rows, in place
  assert got == [(0, 1), (2, 0), (4, 2)]  # even rows are let in, in order
  assert svc.closed
  random.seed(0)
  got = E.PersonalizedClassifierPrediction(hg, emb, links, per_edge=False)
  assert len(recording.last.off) - 1 == 4  # nodes 0, 2, 3, 4
  assert set(got) <= set(links)


def test_missing_classifier_id_raises_key_error(recording):
  hg, emb = small_case()
  emb.edge[5].values.extend([0.0, 0.0])  # embedded, but not in the hypergraph
  with pytest.raises(KeyError):
    E.PersonalizedClassifierPrediction(hg, emb, [(0, 5)], per_edge=True)


def test_degenerate_classifiers_never_reach_the_device(recording):
  hg, emb = small_case()
  hg.node[6]  # a node without edges
  emb.node[6].values.extend([6.0, 1.0])
  hg.edge[3].nodes.extend(range(7))  # an edge that holds every node
  emb.edge[3].values.extend([3.0, -1.0])
  recording.last = None
  assert E.PersonalizedClassifierPrediction(
      hg, emb, [(1, 3), (6, 3)], per_edge=True) == [(1, 3), (6, 3)]
  assert E.PersonalizedClassifierPrediction(
      hg, emb, [(6, 0), (6, 3)], per_edge=False) == []
  assert recording.last is None
  clf = E.GetPersonalizedClassifiers(hg, emb, per_edge=True, idx_subset=[3])
  assert isinstance(clf[3], E.LetEverythingIn)
  assert clf[3].predict(np.zeros((4, 2))).tolist() == [1, 1, 1, 1]
  clf = E.GetPersonalizedClassifiers(hg, emb, per_edge=False, idx_subset=[6])
  assert isinstance(clf[6], E.LetNothingIn)
  assert clf[6].predict(np.zeros((2, 2))).tolist() == [0, 0]


def test_registry_runs_the_new_functions():
  assert E.EXPERIMENT_OPTIONS["LP_EDGE_CLASSIFIERS"] is \
      E.PersonalizedEdgeClassifierPrediction
  assert E.EXPERIMENT_OPTIONS["LP_NODE_CLASSIFIERS"] is \
      E.PersonalizedNodeClassifierPrediction
  assert E.PersonalizedEdgeClassifierPrediction is not \
      E.PersonalizedNodeClassifierPrediction
  assert not hasattr(E, "_personalized_not_supported")


def test_registry_entries_pick_the_side(recording):
  hg, emb = small_case()
  random.seed(0)
  E.PersonalizedEdgeClassifierPrediction(hg, emb, [(0, 1), (2, 0)])
  assert recording.last.table.shape[0] == 6  # node table
  E.PersonalizedNodeClassifierPrediction(hg, emb, [(0, 1), (2, 0)])
  assert recording.last.table.shape[0] == 3  # edge table


def load_generator():
  spec = importlib.util.spec_from_file_location(
      "make_golden_svc", os.path.join(GOLDEN, "make_golden_svc.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_fixture_is_small_and_covers_the_tiers():
  z = golden("svc_small.npz")
  size = os.path.getsize(os.path.join(GOLDEN, "svc_small.npz"))
  others = [os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
            if f != "svc_small.npz"]
  assert size <= max(others)
  sizes, ratios = set(), set()
  for d in z["dims"]:
    off, lab = z[f"off{d}"], z[f"lab{d}"]
    for p in range(len(off) - 1):
      l = lab[off[p]:off[p + 1]]
      sizes.add(len(l))
      ratios.add(int(np.sign(2 * int(l.sum()) - len(l))))
  assert {3, 4, 32, 33, 63, 64, 65, 127, 128, 129} <= sizes
  assert max(sizes) >= 700 and ratios == {-1, 0, 1}
  # the share of queries too close to zero to carry a sign: at most 2%
  ft = np.concatenate([z[f"f_tight{d}"] for d in z["dims"]])
  assert np.mean(np.abs(ft) < 3 * float(z["A"])) <= 0.02


def test_fixture_regenerates_with_this_sklearn():
  pytest.importorskip("sklearn")
  z = golden("svc_small.npz")
  out = load_generator().generate()
  assert set(out) == set(z.files)
  for d in z["dims"]:
    for k in ("tab", "off", "row", "lab", "qprob", "qrow"):
      assert np.array_equal(out[f"{k}{d}"], z[f"{k}{d}"]), (k, d)
    # a drifting sklearn is noticed, not hidden
    assert np.abs(out[f"f_tight{d}"] - z[f"f_tight{d}"]).max() <= 1e-9, d
  # the default solves stop anywhere inside their tolerance
  assert abs(float(out["A"]) - float(z["A"])) <= 0.5 * float(z["A"])


def test_new_symbols_are_declared_exported_and_bound():
  declared = set(_hgx.header_symbols())
  for name in SVC_SYMBOLS:
    assert name in declared, f"{name} missing from include/hgx.h"
    assert name in _hgx.SIGNATURES, f"{name} missing from SIGNATURES"
  assert hasattr(_hgx, "Svc")
  if not os.path.exists(build.LIB) and shutil.which("hipcc") is None \
      and not os.path.exists("/opt/rocm/bin/hipcc"):
    pytest.skip("no hipcc and no prebuilt libhgx.so")
  lib = ctypes.CDLL(build.build())
  for name in SVC_SYMBOLS:
    assert hasattr(lib, name), f"{name} not exported by libhgx.so"
