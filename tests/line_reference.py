"""Float64 restatement of the LINE trainer (hypergraphembedding_amd/line.py's
contract), for the LINE tests. A helper module, not a conftest.

It trains a plan (line.line_plan: one row (u, v, negatives) per sample): the
draws are the library's, the arithmetic is written here from the formulas and
checked against torch autograd and by hand in test_line_cpu.py.
"""

import numpy as np

from n2v_reference import MAX_EXP, Ref, ulp32  # noqa: F401
from hypergraphembedding_amd import line as L


def sigma(x):
  """LINE's bounded sigmoid."""
  if x > MAX_EXP:
    return 1.0
  if x < -MAX_EXP:
    return 0.0
  return 1.0 / (1.0 + np.exp(-x))


def step(syn0, tgt, smp, rho, xs=None):
  """One sample in place, target by target: the definition. ``tgt`` is
  ``syn0`` itself at order 1. Every evaluated (label, x) is appended to
  ``xs``."""
  u = int(smp[0])
  l1 = syn0[u].copy()
  err = np.zeros_like(l1)
  for k, t in enumerate(smp[1:]):
    row = tgt[int(t)]
    x = float(l1 @ row)
    if xs is not None:
      xs.append((1 if k == 0 else 0, x))
    g = ((1.0 if k == 0 else 0.0) - sigma(x)) * rho
    err += g * row
    row += g * l1
  syn0[u] += err


def rho_of(rho, s, T):
  return float(L.line_rho(rho, s, T))


def train(syn0, syn1, plan, order, rho, s_range=None):
  """Train the plan's samples in order (sample i of the plan is sample i of
  T = len(plan)); returns the tables, ``margin`` (the least | |x| - 6 | over
  every evaluated x), ``clamped`` (the number with |x| > 6), ``kinds`` (the
  (label, sign) pairs of the clamped ones) and ``max_x``."""
  r = Ref()
  r.syn0 = np.array(syn0, np.float64)
  r.syn1 = np.array(syn1, np.float64)
  tgt = r.syn0 if order == 1 else r.syn1
  T = len(plan)
  xs = []
  for s in (range(T) if s_range is None else s_range):
    step(r.syn0, tgt, plan[s], rho_of(rho, s, T), xs)
  ax = np.abs(np.array([x for _, x in xs])) if xs else np.zeros(0)
  r.margin = float(np.abs(ax - MAX_EXP).min()) if ax.size else np.inf
  r.max_x = float(ax.max()) if ax.size else 0.0
  r.clamped = int((ax > MAX_EXP).sum())
  r.kinds = {(lab, 1 if x > 0 else -1) for lab, x in xs if abs(x) > MAX_EXP}
  r.targets = len(xs)
  return r


def objective(syn0, syn1, samples, order):
  """Mean over the samples of -log s(x_v) - sum_k log s(-x_neg k), float64
  (every negative is a term, as drawn)."""
  s0 = np.asarray(syn0, np.float64)
  tg = s0 if order == 1 else np.asarray(syn1, np.float64)
  tot = 0.0
  for smp in samples:
    l1 = s0[int(smp[0])]
    tot += np.logaddexp(0.0, -(l1 @ tg[int(smp[1])]))
    if len(smp) > 2:
      tot += np.logaddexp(0.0, tg[np.asarray(smp[2:], np.int64)] @ l1).sum()
  return tot / len(samples)


def launch_emulation(syn0, syn1, plan, order, rho, per_launch, run=64,
                     drop=None):
  """The concurrent trainer's staleness bound on the host, float64: the
  samples are cut into launches of ``per_launch``, a launch into waves of
  ``run`` consecutive samples; every wave reads the launch's start tables
  plus its own updates, and the waves' deltas are summed at the launch end.
  ``drop = (waves, row)``: in every launch the updates of those waves
  (indices within the launch) to that row of the target table are lost."""
  s0, s1 = np.array(syn0, np.float64), np.array(syn1, np.float64)
  T = len(plan)
  for a in range(0, T, per_launch):
    d0, d1 = np.zeros_like(s0), np.zeros_like(s1)
    for w, b in enumerate(range(a, min(T, a + per_launch), run)):
      p0, p1 = s0.copy(), s1.copy()
      pt = p0 if order == 1 else p1
      for s in range(b, min(T, a + per_launch, b + run)):
        step(p0, pt, plan[s], rho_of(rho, s, T))
      u0, u1 = p0 - s0, p1 - s1
      if drop is not None and w in drop[0]:
        (u0 if order == 1 else u1)[drop[1]] = 0.0
      d0 += u0
      d1 += u1
    s0 += d0
    s1 += d1
  return s0, s1
