"""Float64 restatement of the node2vec trainer (skip-gram with negative
sampling, hypergraphembedding_amd/node2vec.py's contract), for the node2vec
tests. A helper module, not a conftest.

It trains a plan (node2vec.corpus_plan: per walk the pairs in order, each
(input word w_j, output word w_i, negatives)): the draws are the library's,
the arithmetic is written here from the formulas and checked against torch
autograd in test_node2vec_cpu.py.
"""

import numpy as np

MAX_EXP = 6.0


def ulp32(x):
  return float(np.spacing(np.float32(abs(x))))


def sigmoid(x):
  return 1.0 / (1.0 + np.exp(-x))


def pair_step(syn0, syn1, wj, wi, negs, alpha, xs=None):
  """One pair in place, target by target: the definition. Evaluated x are
  appended to ``xs``."""
  l1 = syn0[wj].copy()
  neu = np.zeros_like(l1)
  for k, t in enumerate([wi] + list(negs)):
    if k > 0 and t == wi:
      continue
    x = float(l1 @ syn1[t])
    if xs is not None:
      xs.append(x)
    if abs(x) >= MAX_EXP:
      continue
    g = ((1.0 if k == 0 else 0.0) - sigmoid(x)) * alpha
    neu += g * syn1[t]
    syn1[t] += g * l1
  syn0[wj] = l1 + neu


def _pair_step_distinct(syn0, syn1, wj, ts, alpha, margin):
  """pair_step for distinct targets ``ts`` (positive first), all at once:
  with l1 fixed and no row repeated the targets do not see each other."""
  l1 = syn0[wj].copy()
  S = syn1[ts]
  x = S @ l1
  margin[0] = min(margin[0], float(np.abs(np.abs(x) - MAX_EXP).min()))
  lab = np.zeros(len(ts))
  lab[0] = 1.0
  g = np.where(np.abs(x) < MAX_EXP, (lab - sigmoid(x)) * alpha, 0.0)
  syn0[wj] = l1 + g @ S
  syn1[ts] = S + g[:, None] * l1


class Ref:
  pass


def walk_alpha(alpha, min_alpha, g, total):
  return max(min_alpha, alpha - (alpha - min_alpha) * g / total)


def train(syn0, syn1, plan, alpha, min_alpha):
  """Train the whole plan (epochs x walks entries) in order; returns the
  tables and ``margin``, the least | |x| - 6 | over every evaluated x."""
  r = Ref()
  r.syn0 = np.array(syn0, np.float64)
  r.syn1 = np.array(syn1, np.float64)
  margin = [np.inf]
  total = len(plan)
  for g, (_, pairs) in enumerate(plan):
    a = walk_alpha(alpha, min_alpha, g, total)
    for wj, wi, negs in pairs:
      ts = [wi] + [t for t in negs if t != wi]
      if len(set(ts)) == len(ts):
        _pair_step_distinct(r.syn0, r.syn1, wj, ts, a, margin)
      else:
        xs = []
        pair_step(r.syn0, r.syn1, wj, wi, negs, a, xs)
        margin[0] = min(margin[0], min(abs(abs(x) - MAX_EXP) for x in xs))
  r.margin = margin[0]
  return r


def objective(syn0, syn1, plan):
  """Mean over the plan's pairs of -log s(x_pos) - sum log s(-x_neg) (a
  negative equal to the positive is no term), float64."""
  s0, s1 = np.asarray(syn0, np.float64), np.asarray(syn1, np.float64)
  tot, n = 0.0, 0
  for _, pairs in plan:
    for wj, wi, negs in pairs:
      l1 = s0[wj]
      ng = [t for t in negs if t != wi]
      tot += np.logaddexp(0.0, -(l1 @ s1[wi]))
      if ng:
        tot += np.logaddexp(0.0, s1[ng] @ l1).sum()
      n += 1
  return tot / n
