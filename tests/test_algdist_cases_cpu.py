"""CPU: the alg-dist cases are what they claim, the float64 reference agrees
with the oracle and the reference's golden vectors, and the derived bound is
tight enough to see a subtly wrong kernel (algdist_cases.py).

The mutant condition is a condition on the INPUTS, checked with the
reference alone: a wrong variant of the relaxation must move some element of
every planted row class by at least twice that element's bound. It is
checked at k = 3, 7 and 19 for every input distribution a graph is run with:
[0, 1), [-1, 1) and [100, 101) on the seven graphs and the small one; the
scaled-source inputs (algdist_cases.long_inputs: u01, sym, near1) on the
long-row graphs; [0, 1) and [-1, 1) on the long-node-row graph, the two it
is run with. At an offset of 100 the margin is thin (the bound is about
100 n u, one incidence moves a row by at most 1 / (2 n)): the smallest ratio
is just above 2, on rows of 129 and 257, and the graph seeds of d24x24 and
d200x3 are ones at which it holds at k = 3. Rows longer than about 200
cannot meet it at that offset, which is why the long-row graphs' plain
[100, 101) runs and the 513-long node row are outside it.
A row of one incidence has the same mean under the first three mutants, so
they are asked of rows of two or more.
"""

import numpy as np
import pytest

import algdist_cases as C
import oracle as O
from conftest import golden, golden_incidence

MULTI = C.SEVEN + [C.SMALL]
LONGS = [C.LONG64, C.LONG512]


@pytest.mark.parametrize("case", C.ALL, ids=lambda c: c.name)
def test_graph_is_as_stated(case):
  inc = case.inc
  assert inc.node_degree().min() >= 1 and inc.edge_size().min() >= 1
  for rp, col in ((inc.rp_n, inc.col_n), (inc.rp_e, inc.col_e)):
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    same = row[1:] == row[:-1]
    assert np.all(np.diff(col.astype(np.int64))[same] > 0)  # sorted, distinct
  for avg, qg, ng in ((inc.nnz / inc.N, case.quad[0], case.narrow[0]),
                      (inc.nnz / inc.E, case.quad[1], case.narrow[1])):
    lo, hi = C.QUAD_CLASS[qg]
    assert lo < avg <= hi
    lo, hi = C.NARROW_CLASS[ng]
    assert lo < avg <= hi
  for n, r in inc.planted_n.items():
    assert inc.node_degree()[r] == n
  for n, r in inc.planted_e.items():
    assert inc.edge_size()[r] == n
  assert sorted(inc.planted_n) == sorted(case.planted_n)
  assert sorted(inc.planted_e) == sorted(case.planted_e)


def test_seven_graphs_cover_every_group_size_on_both_sides():
  want = {"d3x200": ((4, 64), (1, 64)), "d6x100": ((4, 64), (2, 32)),
          "d12x48": ((8, 32), (4, 16)), "d24x24": ((16, 16), (8, 8)),
          "d48x12": ((32, 8), (16, 4)), "d100x6": ((64, 4), (32, 2)),
          "d200x3": ((64, 4), (64, 1))}
  for c in C.SEVEN:
    assert (c.quad, c.narrow) == want[c.name]
    q, n = c.quad, c.narrow
    # the planted lengths are those of the side's own G
    assert c.planted_n == C.planted_lengths(q[0], n[0])
    assert c.planted_e == C.planted_lengths(q[1], n[1])
  for side in (0, 1):
    assert {c.quad[side] for c in C.SEVEN} == {4, 8, 16, 32, 64}
    assert {c.narrow[side] for c in C.SEVEN} == {1, 2, 4, 8, 16, 32, 64}
  assert C.planted_lengths(64, 64) == [1, 15, 16, 17, 63, 64, 65, 127, 128,
                                       129, 257]


@pytest.mark.parametrize("case", MULTI, ids=lambda c: c.name)
def test_multi_iteration_cases_fit_64_workgroups(case):
  inc = case.inc
  assert len(case.iters) > 1
  for rows, qg, ng in ((inc.N, case.quad[0], case.narrow[0]),
                       (inc.E, case.quad[1], case.narrow[1])):
    for g in (qg, ng):
      per_wg = C.BLOCK // g
      assert rows <= C.MAX_WG * per_wg
      assert rows % per_wg != 0
  if case is C.SMALL:  # also the wide kernel's graph: one row per wave
    assert max(inc.N, inc.E) <= C.MAX_WG * (C.BLOCK // 64)
    assert inc.N < C.BLOCK // case.quad[0] and inc.E < C.BLOCK // case.quad[1]
  else:
    assert 300 <= max(inc.N, inc.E) <= 4000
  assert max(inc.node_degree().max(), inc.edge_size().max()) <= C.DEFAULT_LONG


def test_long_and_grid_stride_graphs():
  for case in LONGS + [C.LONGNODE, C.GRID]:
    assert case.iters == (1,)
  for case in LONGS:
    inc, t = case.inc, case.long_thresh
    assert inc.N >= max(case.planted_e)
    assert inc.node_degree().max() <= t
    long_e = inc.edge_size()[inc.edge_size() > t]
    assert sorted(long_e) == [n for n in case.planted_e if n > t]
  assert -(-4097 // C.LONG64.long_thresh) > 64  # long_finish's strided loop
  assert set(C.LONG64.planted_e) == {64, 65, 128, 129, 4097}
  assert set(C.LONG512.planted_e) == {512, 513, 1025}
  inc = C.LONGNODE.inc
  assert inc.node_degree().max() == 513 and inc.edge_size().max() <= 64
  inc = C.GRID.inc
  assert 8500 <= inc.E <= 9500 and 130_000 <= inc.N <= 150_000
  assert C.GRID.quad == (4, 64)
  # more rows than 2048 resident workgroups (256 CUs x 8 of 256 threads, the
  # most a CU holds) times 256 / G
  assert inc.N > 2048 * 64 and inc.E > 2048 * 4


@pytest.mark.parametrize("case,k,iters", [(C.SMALL, 3, 3), (C.SEVEN[2], 10, 2),
                                          (C.LONG512, 19, 1)],
                         ids=lambda v: getattr(v, "name", str(v)))
def test_reference_matches_oracle(case, k, iters):
  inc = case.inc
  x0, y0 = C.inputs(inc, k, "sym")
  x, y, _ = C.reference(inc, x0, y0, iters)
  xo, yo = O.algdist(inc, x0, y0, iters)
  assert np.abs(x - xo).max() <= 1e-12 and np.abs(y - yo).max() <= 1e-12


def test_reference_matches_golden_vectors():
  z = golden("algdist_tiny.npz")
  inc = golden_incidence("csr_tiny.npz")
  for it in (1, 3, 20):
    r = O.Rng(int(z["seed"]))
    x0, y0 = r.random((inc.N, 10)), r.random((inc.E, 10))
    x, y, _ = C.reference(inc, x0, y0, it)
    assert np.abs(x - z[f"x_{it}"]).max() <= 1e-4
    assert np.abs(y - z[f"y_{it}"]).max() <= 1e-4


def _dists(case, mutants=False):
  """The distributions the GPU module runs the case with; under the mutant
  condition, those of them that can meet it (module docstring)."""
  if case in LONGS:
    return C.LONG_DISTS + (() if mutants else ("off100",))
  return ("u01", "sym") if case is C.LONGNODE else C.DISTS


def _float32_model(inc, x0, y0, iters):
  """The device's formulation in numpy float32: raw values, the previous
  affine applied on read (reciprocal of the span), sequential sums."""
  f = np.float32
  a, at = inc.to_scipy()
  a, at = a.astype(f), at.astype(f)
  wn = (f(1) / inc.node_degree().astype(f))[:, None]
  we = (f(1) / inc.edge_size().astype(f))[:, None]
  x, y = x0.astype(f), y0.astype(f)
  m = inv = None

  def s(z):
    return z if m is None else (z - m) * inv

  for _ in range(iters):
    mean = (a @ (we * y)) * (f(1) / (a @ we))
    xn = (s(x) + s(mean)) * f(0.5)
    mean = (at @ (wn * xn)) * (f(1) / (at @ wn))
    yn = (s(y) + mean) * f(0.5)
    m = np.minimum(xn.min(0), yn.min(0))
    inv = f(1) / (np.maximum(xn.max(0), yn.max(0)) - m)
    x, y = xn, yn
  d = f(1) / inv
  return (x - m) / d, (y - m) / d


@pytest.mark.parametrize("case", MULTI + LONGS + [C.LONGNODE],
                         ids=lambda c: c.name)
def test_float32_model_is_within_the_bound(case):
  """The bound is an upper bound: a plain float32 evaluation stays inside."""
  inc = case.inc
  for dist in _dists(case):
    for k in (3, 10):
      x0, y0 = C.case_inputs(case, k, dist)
      for it in case.iters:
        x, y, h = C.reference(inc, x0, y0, it)
        bx, by = C.bound(inc, h)
        gx, gy = _float32_model(inc, x0, y0, it)
        assert np.all(np.abs(gx - x) <= bx) and np.all(np.abs(gy - y) <= by)


MUTANTS = [("drop_last", 1), ("first_twice", 1), ("uniform_w", 1),
           ("old_x", 1), ("no_src_affine", 2)]


@pytest.mark.parametrize("k", [3, 7, 19])
@pytest.mark.parametrize("case", MULTI + LONGS + [C.LONGNODE],
                         ids=lambda c: c.name)
def test_bound_sees_every_mutant_on_every_planted_class(case, k):
  inc = case.inc
  for dist in _dists(case, mutants=True):
    x0, y0 = C.case_inputs(case, k, dist)
    ref = {}
    for mutant, it in MUTANTS:
      if it not in ref:
        x, y, h = C.reference(inc, x0, y0, it)
        ref[it] = (x, y) + C.bound(inc, h)
      x, y, bx, by = ref[it]
      xm, ym, _ = C.reference(inc, x0, y0, it, mutant=mutant)
      sides = [("edge", inc.planted_e, ym, y, by)]
      if mutant != "old_x":  # the node half does not read x through the edges
        sides.append(("node", inc.planted_n, xm, x, bx))
      for side, planted, got, want, b in sides:
        for n, r in planted.items():
          if n < 2 and mutant in ("drop_last", "first_twice", "uniform_w"):
            continue
          ratio = (np.abs(got[r] - want[r]) / b[r]).max()
          assert ratio >= 2, (case.name, dist, k, mutant, side, n, ratio)
