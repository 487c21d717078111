"""Link-prediction evaluation (reference: hypergraph_embedding/evaluation_util.py).

SURVEY §8f rank 3: the end-to-end quality signal for embeddings whose RNG
streams differ from the reference's. Kept surface:
  RemoveRandomConnections (84-122), SampleMissingConnections (125-158),
  CalculateCommunityPredictionMetrics (160-211), AddPredictionRecords
  (37-52), RunLinkPredictionExperiment (55-72),
  LinkPredictionDataToResultProto (75-81), NodeEdgeEmbeddingPrediction
  (508-552) with its classifier (_TrainNodeEdgeEmbeddingClassifier,
  471-505) and EXPERIMENT_OPTIONS (580-590).

The two sampling loops run natively (libhgx, csrc/hgx_lp.hip) but draw from
Python's global ``random`` exactly as the reference's loops do: the state goes
in, the same picks come out and the advanced state is put back, so
``random.seed(s)`` reproduces the reference's removals and negatives. The
classifier trains on the MI355X dense-MLP engine (dense_mlp.py) reading the
embedding rows in place.

The per-edge / per-node SVC experiments (LP_EDGE_CLASSIFIERS /
LP_NODE_CLASSIFIERS, 286-449 and 560-581) run on the device as well: one
``SVC(C=1, gamma=0.1)`` per edge (node) that occurs in the candidate links,
all of them solved in one batched launch (libhgx, csrc/hgx_svc.hip: libsvm's
SMO in float32) and every candidate link scored in a second one. Kept
surface: GetPersonalizedClassifiers, PersonalizedClassifierPrediction,
PersonalizedEdgeClassifierPrediction, PersonalizedNodeClassifierPrediction,
LetNothingIn, LetEverythingIn. The negatives of a classifier are drawn on the
host (PersonalizedClassifierProblems): by default from a numpy generator
seeded from Python's global ``random`` (the reference's distribution, not its
picks), with ``rng="python"`` by the reference's own ``random.sample``
expression.
"""

import logging
import random
from collections import namedtuple

import numpy as np

from . import _hgx
from .dense_mlp import LP_CLASSIFIER, DenseModel
from .hypergraph_util import RemoveNodeFromEdge
from .proto import EvaluationMetrics, ExperimentalResult, Hypergraph
from .runtime import get_context

log = logging.getLogger()

LinkPredictionData = namedtuple(
    "LinkPredictionData",
    ("hypergraph", "embedding", "good_links", "bad_links", "removal_prob"))


def AddPredictionRecords(eval_metric, good_links, bad_links, predictions):
  """evaluation_util.py:37-52: one record per candidate link, positives
  first, with whether it was predicted."""
  predicted = {(n, e) for n, e in predictions}
  for links, label in ((good_links, True), (bad_links, False)):
    for node_idx, edge_idx in links:
      rec = eval_metric.records.add()
      rec.node_idx = node_idx
      rec.edge_idx = edge_idx
      rec.label = label
      rec.prediction = (node_idx, edge_idx) in predicted
  return eval_metric


def RunLinkPredictionExperiment(link_prediction_data, experiment_name):
  """evaluation_util.py:55-72."""
  assert experiment_name in EXPERIMENT_OPTIONS
  hypergraph, embedding, good_links, bad_links, _ = link_prediction_data
  predictor = EXPERIMENT_OPTIONS[experiment_name]
  predicted = predictor(hypergraph, embedding, bad_links + good_links)
  metrics = CalculateCommunityPredictionMetrics(predicted, good_links,
                                                bad_links)
  metrics.experiment_name = experiment_name
  log.info("Result:\n%s", metrics)
  AddPredictionRecords(metrics, good_links, bad_links, predicted)
  return metrics


def LinkPredictionDataToResultProto(lp_data):
  """evaluation_util.py:75-81."""
  hypergraph, embedding, _, _, removal_prob = lp_data
  res = ExperimentalResult()
  res.removal_probability = removal_prob
  res.hypergraph.ParseFromString(hypergraph.SerializeToString())
  res.embedding.ParseFromString(embedding.SerializeToString())
  return res


def RemoveRandomConnections(original_hypergraph, probability):
  """evaluation_util.py:84-122: a copy with random node-edge connections
  removed (never a node's or an edge's last one) and the removed pairs.
  Candidate order = node map order x each node's edge list, shuffled with
  ``random.shuffle``; one ``random.random()`` per candidate that may go."""
  assert probability >= 0
  assert probability <= 1
  new_hg = Hypergraph()
  new_hg.CopyFrom(original_hypergraph)
  pairs = [(n, e) for n, node in original_hypergraph.node.items()
           for e in node.edges]
  if not pairs:
    random.shuffle(pairs)
    return new_hg, []
  node_pos = {n: i for i, n in enumerate(original_hypergraph.node)}
  edge_pos, edge_size = {}, []
  for e, edge in original_hypergraph.edge.items():
    edge_pos[e] = len(edge_size)
    edge_size.append(len(edge.nodes))
  for _, e in pairs:  # edges a node lists but the edge map lacks
    if e not in edge_pos:
      edge_pos[e] = len(edge_size)
      edge_size.append(0)
  node_deg = [len(original_hypergraph.node[n].edges)
              for n in original_hypergraph.node]
  pn = np.fromiter((node_pos[n] for n, _ in pairs), np.int32, len(pairs))
  pe = np.fromiter((edge_pos[e] for _, e in pairs), np.int32, len(pairs))
  removed_idx = _hgx.pyrandom_remove_connections(random._inst, pn, pe,
                                                 node_deg, edge_size,
                                                 probability)
  removed = []
  for i in removed_idx:
    node_idx, edge_idx = pairs[i]
    RemoveNodeFromEdge(new_hg, node_idx, edge_idx)
    removed.append((node_idx, edge_idx))
  return new_hg, removed


def _missing_positions(hypergraph, num_samples):
  """(nodes, edges, node positions, edge positions) of the draws
  SampleMissingConnections makes."""
  assert num_samples < len(hypergraph.node) * len(hypergraph.edge)
  assert len(hypergraph.edge) > 0
  assert len(hypergraph.node) > 0
  nodes = [n for n in hypergraph.node]
  edges = [e for e in hypergraph.edge]
  epos = {e: i for i, e in enumerate(edges)}
  rowptr = np.zeros(len(nodes) + 1, np.int64)
  cols = []
  for i, n in enumerate(nodes):
    c = sorted({epos[e] for e in hypergraph.node[n].edges if e in epos})
    cols.extend(c)
    rowptr[i + 1] = rowptr[i] + len(c)
  npos, ep = _hgx.pyrandom_sample_missing(random._inst, len(nodes), len(edges),
                                          rowptr, np.asarray(cols, np.int32),
                                          int(num_samples))
  return nodes, edges, npos, ep


def SampleMissingConnections(hypergraph, num_samples):
  """evaluation_util.py:125-158: up to num_samples distinct (node, edge)
  pairs with the node not in the edge (10 x num_samples tries), as the list
  of the reference's set -- same members, same iteration order."""
  nodes, edges, npos, epos = _missing_positions(hypergraph, num_samples)
  samples = set()
  for p, q in zip(npos.tolist(), epos.tolist()):
    samples.add((nodes[p], edges[q]))
  if len(samples) < num_samples:
    log.critical("SampleMissingConnections failed to find %i samples",
                 num_samples)
  return list(samples)


def CalculateCommunityPredictionMetrics(predicted_connections, good_links,
                                        bad_links):
  """evaluation_util.py:160-211: precision / recall / f1 only when defined,
  accuracy over positives and negatives."""
  predictions = set(predicted_connections)
  positives = set(good_links)
  negatives = set(bad_links)
  assert len(positives & negatives) == 0
  assert len(predictions & (positives | negatives)) == len(predictions)
  assert len(positives) + len(negatives) > 0
  tp = len(predictions & positives)
  m = EvaluationMetrics()
  if predictions:
    m.precision = tp / len(predictions)
  if positives:
    m.recall = tp / len(positives)
  if m.precision + m.recall:
    m.f1 = 2 * m.precision * m.recall / (m.precision + m.recall)
  m.num_true_pos = tp
  m.num_false_pos = len(predictions) - tp
  m.num_false_neg = len(positives) - tp
  m.num_true_neg = len(negatives - predictions)
  m.accuracy = (m.num_true_pos + m.num_true_neg) / (len(positives) +
                                                    len(negatives))
  return m


def _GetVectorFromIdx(node_idx, edge_idx, embedding):
  """evaluation_util.py:452-457."""
  assert node_idx in embedding.node
  assert edge_idx in embedding.edge
  return np.concatenate((embedding.node[node_idx].values,
                         embedding.edge[edge_idx].values), axis=0)


class NodeEdgeClassifier:
  """The trained node/edge classifier. ``predict(x)`` takes rows of
  [node_emb | edge_emb] like the Keras model; ``predict_pairs`` scores
  (node row, edge row) pairs of the embedding tables in place."""

  def __init__(self, model, node_row, edge_row, dim):
    self.model, self.node_row, self.edge_row, self.dim = (model, node_row,
                                                          edge_row, dim)

  def predict_pairs(self, node_rows, edge_rows):
    return self.model.predict_label(node_rows, edge_rows)

  def predict(self, x):
    x = np.asarray(x, np.float32).reshape(-1, 2 * self.dim)
    if len(x) == 0:
      return np.zeros((0, 1), np.float32)
    # score arbitrary vectors: they become the tables of a scratch engine
    scratch = _hgx.Mlp(self.model.ctx, LP_CLASSIFIER, self.dim)
    scratch.set_weights(self.model.engine.get_weights())
    scratch.set_tables(x[:, :self.dim], x[:, self.dim:])
    rows = np.arange(len(x), dtype=np.int32)
    y = scratch.predict(0, rows, rows)
    scratch.close()
    return y.reshape(-1, 1)


def _embedding_tables(embedding):
  node_ids = list(embedding.node)
  edge_ids = list(embedding.edge)
  d = embedding.dim
  nt = np.zeros((max(len(node_ids), 1), d), np.float32)
  et = np.zeros((max(len(edge_ids), 1), d), np.float32)
  for i, n in enumerate(node_ids):
    nt[i] = embedding.node[n].values
  for i, e in enumerate(edge_ids):
    et[i] = embedding.edge[e].values
  return ({n: i for i, n in enumerate(node_ids)},
          {e: i for i, e in enumerate(edge_ids)}, nt, et)


def _TrainNodeEdgeEmbeddingClassifier(hypergraph, embedding, disable_pbar):
  """evaluation_util.py:471-505: positives = every (node, edge) of the
  hypergraph, as many SampleMissingConnections negatives; Dense(dim, relu)
  -> Dense(1, sigmoid), MSE, Adagrad, batch 256, 30 epochs,
  EarlyStopping(loss, min_delta=1e-3)."""
  del disable_pbar
  nrow, erow, nt, et = _embedding_tables(embedding)
  pos_n, pos_e = [], []
  for node_idx, node in hypergraph.node.items():
    for edge_idx in node.edges:
      assert node_idx in nrow and edge_idx in erow
      pos_n.append(nrow[node_idx])
      pos_e.append(erow[edge_idx])
  neg = SampleMissingConnections(hypergraph, len(pos_n))
  for node_idx, edge_idx in neg:
    assert node_idx in nrow and edge_idx in erow
  nr = np.array(pos_n + [nrow[n] for n, _ in neg], np.int32)
  er = np.array(pos_e + [erow[e] for _, e in neg], np.int32)
  lab = np.concatenate([np.ones(len(pos_n), np.float32),
                        np.zeros(len(neg), np.float32)])
  model = DenseModel(LP_CLASSIFIER, embedding.dim)
  model.set_tables(nt, et)
  model.fit(nr, er, lab, epochs=30, min_delta=1e-3)
  clf = NodeEdgeClassifier(model, nrow, erow, embedding.dim)
  return clf


def NodeEdgeEmbeddingPrediction(hypergraph, embedding, potential_links,
                                classifier=None, disable_pbar=False):
  """evaluation_util.py:508-552: the candidate links whose
  [node | edge] vector the classifier scores above 0.5 (links outside the
  hypergraph are dropped first)."""
  if classifier is None:
    classifier = _TrainNodeEdgeEmbeddingClassifier(hypergraph, embedding,
                                                   disable_pbar)
  potential_links = [(n, e) for n, e in potential_links
                     if n in hypergraph.node and e in hypergraph.edge]
  if isinstance(classifier, NodeEdgeClassifier):
    for n, e in potential_links:
      assert n in classifier.node_row and e in classifier.edge_row
    scores = classifier.predict_pairs(
        np.array([classifier.node_row[n] for n, _ in potential_links], np.int32),
        np.array([classifier.edge_row[e] for _, e in potential_links], np.int32))
  else:
    x = np.array([_GetVectorFromIdx(n, e, embedding)
                  for n, e in potential_links])
    scores = classifier.predict(x)
  return [link for link, s in zip(potential_links, scores)
          if np.asarray(s).reshape(-1)[0] > 0.5]


################################################################################
# Personalized classifiers: one RBF C-SVC per edge / per node (286-449)        #
################################################################################

SVC_C, SVC_GAMMA, SVC_EPS = 1.0, 0.1, 1e-3  # SVC(C=1, gamma=0.1), default tol
PERSONALIZED_RNG_MODES = (None, "python")

PersonalizedProblems = namedtuple(
    "PersonalizedProblems",
    ("off", "row", "label", "trained", "nothing", "everything"))


class LetEverythingIn:
  """evaluation_util.py:286-289: the classifier of an index whose neighbours
  are the whole table (one prediction per vector, like a fitted SVC)."""

  def predict(self, vectors=(), *args, **kargs):
    return np.ones(len(vectors), np.int64)

  def decision_function(self, vectors=()):
    return np.full(len(vectors), np.inf, np.float32)


class LetNothingIn:
  """evaluation_util.py:292-295: the classifier of an index with no
  neighbours."""

  def predict(self, vectors=(), *args, **kargs):
    return np.zeros(len(vectors), np.int64)

  def decision_function(self, vectors=()):
    return np.full(len(vectors), -np.inf, np.float32)


class PersonalizedClassifier:
  """One trained classifier of a batch (problem ``prob`` of ``engine``).
  ``decision_function`` scores free vectors on the device with the kernel
  that scores table rows; ``predict`` is 1 where it is positive."""

  def __init__(self, engine, prob):
    self.engine, self.prob = engine, prob

  def decision_function(self, vectors):
    x = np.asarray(vectors, np.float32).reshape(-1, self.engine.dim)
    if len(x) == 0:
      return np.zeros(0, np.float32)
    return self.engine.decision_vec(np.full(len(x), self.prob, np.int32), x)

  def predict(self, vectors):
    return (self.decision_function(vectors) > 0).astype(np.int64)


def _draw_rows_without(gen, n_rows, taken, mark, k):
  """k distinct rows of range(n_rows) outside `taken`, uniformly without
  replacement, from the numpy generator `gen`. `mark` is a caller-owned
  all-False scratch of n_rows bools (left all False)."""
  free = n_rows - len(taken)
  mark[taken] = True
  if 2 * k > free:  # dense: permute the complement
    rest = np.flatnonzero(~mark)
    out = rest if k >= free else gen.choice(rest, k, replace=False)
  else:  # sparse: rejection, first occurrences in draw order
    out = np.empty(k, np.int64)
    got = 0
    while got < k:
      cand = gen.integers(0, n_rows, 2 * (k - got) + 8)
      cand = cand[~mark[cand]]
      _, first = np.unique(cand, return_index=True)
      cand = cand[np.sort(first)][:k - got]
      mark[cand] = True
      out[got:got + len(cand)] = cand
      got += len(cand)
    mark[out] = False
  mark[taken] = False
  return out


def PersonalizedClassifierProblems(idx2neighbors, neighbor_row, idx_subset,
                                   rng=None):
  """The training problems of _train_personalized_classifier
  (evaluation_util.py:318-352) for every idx of `idx_subset`, as rows of the
  neighbour table: ``neighbor_row`` maps a neighbour's idx to its row (in the
  order of the embedding map). Host only. Returns PersonalizedProblems:
  problem p is samples [off[p], off[p + 1]) of (row, label) and belongs to
  ``trained[p]``; positives (label 1) are the idx's neighbours, negatives
  min(#non-neighbours, 2 * #neighbours) non-neighbours. ``nothing`` /
  ``everything`` list the indices without neighbours / without
  non-neighbours, which get no problem. An idx missing from `idx2neighbors`
  and a neighbour missing from `neighbor_row` raise KeyError.

  rng=None: one 62-bit seed is taken from Python's global ``random``
  (``random.getrandbits(62)``, so ``random.seed(s)`` fixes the run) and the
  negatives come from a numpy generator seeded with it, uniformly without
  replacement per classifier: the reference's distribution, not its picks
  (it calls ``random.sample`` on a set, whose order is the interpreter's hash
  layout and which Python >= 3.11 rejects).
  rng="python": the reference's expression itself on a tuple of that set,
  ``random.sample(tuple(neighbor_row.keys() - pos_indices), k)``, per idx in
  `idx_subset` order: the same picks and the same final ``random`` state as
  the reference on the same interpreter.

  The reference then permutes each problem's samples with
  ``sklearn.utils.shuffle`` (:351). That only changes the order libsvm sees
  them in, which moves the solution by less than its tolerance; it is not
  reproduced and numpy's global state is not advanced."""
  if rng not in PERSONALIZED_RNG_MODES:
    raise ValueError("rng must be None or 'python', not %r" % (rng,))
  n_rows = len(neighbor_row)
  gen = mark = None
  if rng is None:
    gen = np.random.default_rng(random.getrandbits(62))
    mark = np.zeros(n_rows, bool)
  off, rows, labels = [0], [], []
  trained, nothing, everything = [], [], []
  for idx in idx_subset:
    pos_indices = set(idx2neighbors[idx])
    if len(pos_indices) == 0:
      nothing.append(idx)
      continue
    if rng == "python":
      neg_set = neighbor_row.keys() - pos_indices
      num_neg = len(neg_set)
    else:
      num_neg = n_rows - sum(n in neighbor_row for n in pos_indices)
    if num_neg == 0:
      everything.append(idx)
      continue
    k = min(num_neg, len(pos_indices) * 2)
    pos = np.fromiter((neighbor_row[n] for n in pos_indices), np.int64,
                      len(pos_indices))
    if rng == "python":
      neg_indices = random.sample(tuple(neg_set), k)
      neg = np.fromiter((neighbor_row[n] for n in neg_indices), np.int64, k)
    else:
      neg = _draw_rows_without(gen, n_rows, pos, mark, k)
    rows += [pos, neg]
    labels += [np.ones(len(pos), np.uint8), np.zeros(k, np.uint8)]
    off.append(off[-1] + len(pos) + k)
    trained.append(idx)
  cat = lambda parts, dt: (np.concatenate(parts).astype(dt) if parts else
                           np.zeros(0, dt))
  return PersonalizedProblems(np.array(off, np.int64), cat(rows, np.int32),
                              cat(labels, np.uint8), trained, nothing,
                              everything)


def _neighbor_table(embedding, per_edge):
  """(idx -> row, rows x dim float32) of the table the classifiers read:
  node embeddings for per-edge classifiers, edge embeddings per node."""
  emb = embedding.node if per_edge else embedding.edge
  row = {idx: i for i, idx in enumerate(emb)}
  tab = np.zeros((len(row), embedding.dim), np.float32)
  for idx, i in row.items():
    tab[i] = emb[idx].values
  return row, tab


def _TrainPersonalizedClassifiers(hypergraph, embedding, per_edge, idx_subset,
                                  rng):
  """(engine or None, problems, idx -> problem, idx -> table row)."""
  if per_edge:
    idx2neighbors = {idx: edge.nodes for idx, edge in hypergraph.edge.items()}
  else:
    idx2neighbors = {idx: node.edges for idx, node in hypergraph.node.items()}
  log.info("Training classifier per %s", "edge" if per_edge else "node")
  if idx_subset is None:
    idx_subset = idx2neighbors.keys()
  else:
    log.info("Subset provided with %i entires", len(idx_subset))
  row, tab = _neighbor_table(embedding, per_edge)
  problems = PersonalizedClassifierProblems(idx2neighbors, row, idx_subset,
                                            rng=rng)
  engine = None
  if problems.trained:
    engine = _hgx.Svc(get_context(), tab)
    _, status = engine.fit(problems.off, problems.row, problems.label,
                           C=SVC_C, gamma=SVC_GAMMA, eps=SVC_EPS)
    capped = int(np.count_nonzero(status))
    if capped:
      log.warning("%i of %i personalized classifiers stopped at the "
                  "iteration cap before converging", capped, len(status))
  return engine, problems, {idx: p for p, idx in enumerate(problems.trained)}, row


def GetPersonalizedClassifiers(hypergraph, embedding, per_edge=True,
                               idx_subset=None, disable_pbar=False, rng=None):
  """evaluation_util.py:355-386: a dict from idx to classifier, one per edge
  (node embedding -> 0 / 1) or one per node (edge embedding -> 0 / 1), all
  trained in one device launch. A classifier has ``predict(vectors)`` and
  ``decision_function(vectors)``. `rng`: PersonalizedClassifierProblems."""
  del disable_pbar
  engine, problems, prob_of, _ = _TrainPersonalizedClassifiers(
      hypergraph, embedding, per_edge, idx_subset, rng)
  result = {idx: PersonalizedClassifier(engine, p)
            for idx, p in prob_of.items()}
  result.update((idx, LetNothingIn()) for idx in problems.nothing)
  result.update((idx, LetEverythingIn()) for idx in problems.everything)
  return result


def PersonalizedClassifierPrediction(hypergraph, embedding, links,
                                     per_edge=True, run_in_parallel=True,
                                     disable_pbar=False, rng=None):
  """evaluation_util.py:389-449: the candidate (node, edge) links that the
  edge's (per_edge) or the node's classifier lets in. Links whose node or
  edge has no embedding are dropped, only the classifiers the rest needs are
  trained, and every remaining link is scored in place (rows of the
  embedding table) in one device call; a link is predicted when its decision
  value is positive. run_in_parallel and disable_pbar are accepted for
  signature compatibility. `rng`: PersonalizedClassifierProblems."""
  del run_in_parallel, disable_pbar
  assert embedding.dim > 0
  log.info("Removing potential links that do not have embeddings")
  entity_idx_classifier_idx = [(n, e) if per_edge else (e, n)
                               for n, e in links
                               if n in embedding.node and e in embedding.edge]
  necessary_classifiers = set(c for _, c in entity_idx_classifier_idx)
  engine, problems, prob_of, row = _TrainPersonalizedClassifiers(
      hypergraph, embedding, per_edge, necessary_classifiers, rng)
  everything = set(problems.everything)
  log.info("Running each classifier")
  scored = [(k, prob_of[c], row[ent])
            for k, (ent, c) in enumerate(entity_idx_classifier_idx)
            if c in prob_of]
  let_in = [c in everything for _, c in entity_idx_classifier_idx]
  if scored:
    f = engine.decision(np.array([p for _, p, _ in scored], np.int32),
                        np.array([r for _, _, r in scored], np.int32))
    for (k, _, _), v in zip(scored, f):
      let_in[k] = bool(v > 0)
  if engine is not None:
    engine.close()
  return [((ent, c) if per_edge else (c, ent))
          for (ent, c), ok in zip(entity_idx_classifier_idx, let_in) if ok]


def PersonalizedEdgeClassifierPrediction(hypergraph, embedding, links,
                                         run_in_parallel=False, rng=None):
  """evaluation_util.py:560-569."""
  return PersonalizedClassifierPrediction(hypergraph, embedding, links,
                                          per_edge=True,
                                          run_in_parallel=run_in_parallel,
                                          rng=rng)


def PersonalizedNodeClassifierPrediction(hypergraph, embedding, links,
                                         run_in_parallel=False, rng=None):
  """evaluation_util.py:572-581."""
  return PersonalizedClassifierPrediction(hypergraph, embedding, links,
                                          per_edge=False,
                                          run_in_parallel=run_in_parallel,
                                          rng=rng)


EXPERIMENT_OPTIONS = {
    "LP_EDGE_CLASSIFIERS": PersonalizedEdgeClassifierPrediction,
    "LP_NODE_CLASSIFIERS": PersonalizedNodeClassifierPrediction,
    "LP_NODE_EDGE_CLASSIFIER": NodeEdgeEmbeddingPrediction,
}
