"""Float64 restatement of the DeepWalk trainer (skip-gram with hierarchical
softmax, hypergraphembedding_amd/deepwalk.py's contract), for the DeepWalk
tests. A helper module, not a conftest.

It trains a plan (node2vec.corpus_plan with no negatives: per walk the pairs
in order, each (input word w_j, output word w_i, [])) over a tree (ptr,
point, code): the draws are the library's, the arithmetic is written here
from the formulas and checked against torch autograd in
test_deepwalk_cpu.py.
"""

import numpy as np

from n2v_reference import MAX_EXP, Ref, sigmoid, ulp32, walk_alpha  # noqa: F401


def path(tree, w):
  ptr, point, code = tree
  return (np.asarray(point[ptr[w]:ptr[w + 1]], np.int64),
          np.asarray(code[ptr[w]:ptr[w + 1]], np.float64))


def pair_step(syn0, syn1, wj, ts, cs, alpha, xs=None):
  """One pair in place, inner node by inner node (``ts`` root first, code
  bits ``cs``): the definition. Evaluated x are appended to ``xs``."""
  l1 = syn0[wj].copy()
  neu = np.zeros_like(l1)
  for t, c in zip(ts, cs):
    x = float(l1 @ syn1[t])
    if xs is not None:
      xs.append(x)
    if abs(x) >= MAX_EXP:
      continue
    g = (1.0 - c - sigmoid(x)) * alpha
    neu += g * syn1[t]
    syn1[t] += g * l1
  syn0[wj] = l1 + neu


def _pair_step_rows(syn0, syn1, wj, ts, cs, alpha, margin):
  """pair_step with the path's rows all at once: they are distinct and l1
  is fixed, so they do not see each other."""
  l1 = syn0[wj].copy()
  S = syn1[ts]
  x = S @ l1
  if x.size:
    margin[0] = min(margin[0], float(np.abs(np.abs(x) - MAX_EXP).min()))
  g = np.where(np.abs(x) < MAX_EXP, (1.0 - cs - sigmoid(x)) * alpha, 0.0)
  syn0[wj] = l1 + g @ S
  syn1[ts] = S + g[:, None] * l1


def train(syn0, syn1, plan, tree, alpha, min_alpha):
  """Train the whole plan (epochs x walks entries) in order; returns the
  tables, ``margin`` (the least | |x| - 6 | over every evaluated x) and
  ``path_nodes`` (the sum of the path lengths over the pairs)."""
  r = Ref()
  r.syn0 = np.array(syn0, np.float64)
  r.syn1 = np.array(syn1, np.float64)
  margin = [np.inf]
  r.path_nodes = 0
  total = len(plan)
  for g, (_, pairs) in enumerate(plan):
    a = walk_alpha(alpha, min_alpha, g, total)
    for wj, wi, _ in pairs:
      ts, cs = path(tree, wi)
      assert len(set(ts)) == len(ts)
      r.path_nodes += len(ts)
      _pair_step_rows(r.syn0, r.syn1, wj, ts, cs, a, margin)
  r.margin = margin[0]
  return r


def objective(syn0, syn1, plan, tree):
  """Mean over the plan's pairs of -sum_path log s((1 - 2 c) x), float64."""
  s0, s1 = np.asarray(syn0, np.float64), np.asarray(syn1, np.float64)
  tot, n = 0.0, 0
  for _, pairs in plan:
    for wj, wi, _ in pairs:
      ts, cs = path(tree, wi)
      tot += np.logaddexp(0.0, -(1.0 - 2.0 * cs) * (s1[ts] @ s0[wj])).sum()
      n += 1
  return tot / n


def launch_emulation(syn0, syn1, plan, tree, alpha, min_alpha, n_walks, chunk,
                     drop=None):
  """The concurrent trainer's staleness bound on the host, float64: the plan
  is cut into launches of ``chunk`` walks per epoch; every walk of a launch
  reads the launch's start tables plus its own updates, and the walks'
  updates add up. ``drop = (walks, row)``: in every launch the updates of
  those walks (indices within the launch) to that row of syn1 are lost."""
  s0, s1 = np.array(syn0, np.float64), np.array(syn1, np.float64)
  total = len(plan)
  for e0 in range(0, total, n_walks):
    for c0 in range(0, n_walks, chunk):
      d0, d1 = np.zeros_like(s0), np.zeros_like(s1)
      for k in range(c0, min(n_walks, c0 + chunk)):
        a = walk_alpha(alpha, min_alpha, e0 + k, total)
        p0, p1 = s0.copy(), s1.copy()
        m = [np.inf]
        for wj, wi, _ in plan[e0 + k][1]:
          ts, cs = path(tree, wi)
          _pair_step_rows(p0, p1, wj, ts, cs, a, m)
        u1 = p1 - s1
        if drop is not None and k - c0 in drop[0]:
          u1[drop[1]] = 0.0
        d0 += p0 - s0
        d1 += u1
      s0 += d0
      s1 += d1
  return s0, s1
