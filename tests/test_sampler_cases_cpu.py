"""CPU: the host definition of the keyed samplers (tests/sampler_cases.py).

The GPU tests (tests/test_gpu_sampler_kernels.py) require the device's
record stream to equal this restatement record for record, so what the
sampler has to guarantee is tested here, on the restatement, without a
device:

  * its pieces agree with the definitions (pattern rows, smallest keys,
    Python-int and uint64 forms of the hash);
  * every chosen column is in the row, distinct, min(q, |row|) of them, the
    same for the same seed;
  * the case graphs reach every label of REQUIRED_BRANCHES (the GPU tests
    compare every row with a quota of every case, so this is what keeps a
    kernel branch from going unreached);
  * the chosen q-subset is uniform. A q-subset without replacement of n
    columns gives per-column counts of variance T p (1 - p), p = q / n, and
    correlation -1 / (n - 1), so the statistic is
    sum (obs - T p)^2 / (T p (1 - p)) (n - 1) / n on n - 1 degrees of
    freedom (the plain chi-square against T p reads about (1 - p) of it).
    Both tails are faults: 1e-4 < p-value < 1 - 1e-4. The seeds are
    base .. base + T - 1 with the bases below, fixed before the first run;
  * the same test rejects the restatement with the first-path rule removed
    (power control);
  * negatives and neighbour draws (with replacement: plain chi-square)."""

import os

import numpy as np
import pytest
import scipy.stats

import sampler_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
  return S.small_graph()


@pytest.fixture(scope="module")
def hub():
  return S.hub_graph()


# ---- pieces -----------------------------------------------------------------
def test_hash_forms_agree():
  rs = np.random.RandomState(0)
  h = (rs.randint(0, 2**62, 2000).astype(np.uint64) << np.uint64(2)) | \
      rs.randint(0, 4, 2000).astype(np.uint64)
  h[:4] = [0, 1, 2**64 - 1, 2**63]
  assert all(int(a) == S.mix64(int(x)) for a, x in zip(S.mix64_np(h), h))
  for n in (1, 2, 7, 256, 2**31 - 1, 2**32 - 1, 2**40 + 3, 2**62):
    assert all(int(a) == S.bounded(int(x), n) for a, x in zip(S.mulhi_np(h, n), h)), n
  got = S.rand64_np(12345, 0x305, h)
  assert all(int(a) == S.rand64(12345, 0x305, int(x)) for a, x in zip(got, h))
  # splitmix64's published first output for state 0 is mix64(0)
  assert S.mix64(0) == 0xe220a8397b1dcdaf


def test_pattern_rows_by_definition(small, hub):
  for inc in (small, hub):
    rs = np.random.RandomState(1)
    for pattern in range(6):
      n = S.nrows_of(inc, pattern)
      rows = np.unique(np.concatenate([rs.choice(n, 12, replace=False), [0, n - 1, n - 2]]))
      indptr, indices = S.pattern_rows(inc, pattern, rows)
      for i, r in enumerate(rows):
        want = S.pattern_row(inc, pattern, int(r))
        assert np.array_equal(indices[indptr[i]:indptr[i + 1]], want), (pattern, r)
        if pattern >= S.PAT_NN:
          assert np.array_equal(np.unique(S.row_paths(inc, pattern, int(r))[:, -1]), want)


def test_expand_choice_keeps_smallest_keys(small):
  inc = small
  rows = np.arange(0, inc.N, 5)
  indptr, indices = S.pattern_rows(inc, S.PAT_NN, rows)
  quota = (np.arange(rows.size) % 7).astype(np.int64)
  cnt, cols = S.expand_choice_rows(77, S.PAT_NN, rows, indptr, indices, quota)
  ends = np.cumsum(cnt)
  for i, r in enumerate(rows):
    row = indices[indptr[i]:indptr[i + 1]]
    want = S.expand_choice(77, S.PAT_NN, int(r), row, int(quota[i]))
    got = cols[ends[i] - cnt[i]:ends[i]]
    assert np.array_equal(got, want), r
    assert got.size == min(quota[i], row.size) and np.all(np.diff(got) > 0)
    assert np.isin(got, row).all()
    # no unchosen column has a smaller key than a chosen one
    if 0 < got.size < row.size:
      kmax = max(S.expand_key(77, S.PAT_NN, int(r), int(c)) for c in got)
      rest = np.setdiff1d(row, got)
      assert min(S.expand_key(77, S.PAT_NN, int(r), int(c)) for c in rest) > kmax


@pytest.mark.parametrize("pattern", [S.PAT_NN, S.PAT_EE, S.PAT_NNE, S.PAT_EEN])
@pytest.mark.parametrize("mode3", [1, 2])
def test_reject_choice_is_a_subset_of_the_row(small, pattern, mode3):
  inc = small
  stalled = done = 0
  for r in range(0, S.nrows_of(inc, pattern), 3):
    row = S.pattern_row(inc, pattern, r)
    for q in (1, 4, row.size, row.size + 3):
      if q <= 0:
        continue
      res, tr = S.reject_choice(inc, 5, pattern, r, q, 1, mode3)
      again, _ = S.reject_choice(inc, 5, pattern, r, q, 1, mode3)
      if isinstance(res, tuple):
        assert again == res
        assert res[1] == "small" and tr["W"] <= 1 or res[1] == "stall" and q > row.size, \
            (r, q, res, tr)
        stalled += res[1] == "stall"
        continue
      done += 1
      assert np.array_equal(res, again)
      assert res.size == q <= row.size and np.all(np.diff(res) > 0) and np.isin(res, row).all()
  assert done > 20 and stalled > 0


def test_stream_is_deterministic_and_counts_rows(small):
  case = S.cases()["small"]
  run = next(r for r in case["runs"] if r[0] == "hobe-w1-auto")
  a, sa, ba = S.run_stream(case, run)
  b, sb, bb = S.run_stream(case, run)
  assert np.array_equal(a, b) and sa == sb and ba == bb
  other = S.stream(small, "hobe", run[2] + 1, run[3], run[4], None, run[6])[0]
  assert other.shape == a.shape and not np.array_equal(a, other)
  # per-row counts min(q, |row|) in every block
  nq, eq = run[4]
  for blk, (pattern, q, rc) in enumerate(((S.PAT_NN, nq, 0), (S.PAT_EE, eq, 1),
                                          (S.PAT_NNE, nq, 0), (S.PAT_EEN, eq, 3))):
    rows = a[ba[blk]:ba[blk + 1], rc] - 1
    want = [min(int(q[r]), S.pattern_row(small, pattern, r).size) for r in range(q.size)]
    assert np.array_equal(np.bincount(rows, minlength=q.size), want), pattern


# ---- branch coverage --------------------------------------------------------
def test_cases_reach_every_required_branch():
  lines, reached = S.census()
  assert len(set(S.REQUIRED_BRANCHES)) == len(S.REQUIRED_BRANCHES)
  missing = set(S.REQUIRED_BRANCHES) - reached
  assert not missing, sorted(missing)
  assert reached <= set(S.REQUIRED_BRANCHES), sorted(reached - set(S.REQUIRED_BRANCHES))
  stall = next(l for l in lines if l.startswith("stall / fobe-q10"))
  assert "stats [2, 1, 0]" in stall  # exactly one stall fallback
  # the committed census is this one
  with open(os.path.join(ROOT, "profiles", "samplers", "branch_census.txt")) as fh:
    text = fh.read()
  assert "\n".join(lines) in text


# ---- uniformity -------------------------------------------------------------
def subset_pvalue(obs, T, q):
  """p-value of per-column inclusion counts of T uniform q-subsets."""
  n = obs.size
  p = q / n
  stat = float(((obs - T * p) ** 2).sum() / (T * p * (1 - p)) * (n - 1) / n)
  return scipy.stats.chi2.sf(stat, n - 1)


def _largest_row(inc, pattern):
  sizes = [S.pattern_row(inc, pattern, r).size for r in range(S.nrows_of(inc, pattern))]
  return int(np.argmax(sizes))


def _counts(inc, pattern, r, T, base, choose):
  row = S.pattern_row(inc, pattern, r)
  q = max(2, row.size // 3)
  f = S._row_facts(inc, pattern, r)
  # the first-path rule is exercised only where columns differ in path count
  assert f["npaths"].max() >= 3 * f["npaths"].min(), (pattern, r)
  obs = np.zeros(row.size, np.int64)
  for seed in range(base, base + T):
    got = choose(seed, row, q)
    assert got.size == q
    pos = np.searchsorted(row, got)
    assert np.array_equal(row[pos], got)
    obs[pos] += 1
  return obs, q


def _reject(inc, pattern, r, mode3, want_small, canonical=True, staged=None):
  def choose(seed, row, q):
    res, tr = S.reject_choice(inc, seed, pattern, r, q, 1, mode3, canonical=canonical)
    assert not isinstance(res, tuple), res
    assert tr["small"] == want_small and tr["mode"] == (0 if pattern < S.PAT_NNE else mode3)
    if staged is not None:
      assert tr["staged"] == staged
    return res
  return choose


# (graph, pattern, row: None = the largest, forced mode, small, T, seed base)
UNIFORM = {
    "expand-NN": ("small", S.PAT_NN, None, None, None, 300, 1000),
    "paths-NN-small": ("small", S.PAT_NN, None, 0, True, 300, 2000),
    "paths-NN-large": ("hub", S.PAT_NN, 0, 0, False, 150, 3000),
    "paths-EE-large": ("hub", S.PAT_EE, 399, 0, False, 150, 4000),
    "paths-NNE-small": ("small", S.PAT_NNE, None, 1, True, 300, 5000),
    "paths-EEN-small": ("small", S.PAT_EEN, None, 1, True, 300, 6000),
    "paths-NNE-large": ("hub", S.PAT_NNE, 0, 1, False, 150, 7000),
    "paths-EEN-large": ("hub", S.PAT_EEN, 399, 1, False, 150, 8000),
    "uniform-NNE-staged": ("small", S.PAT_NNE, None, 2, True, 300, 9000),
    "uniform-EEN-small": ("small", S.PAT_EEN, None, 2, True, 300, 10000),
    "uniform-NNE-unstaged": ("hub", S.PAT_NNE, 0, 2, False, 150, 11000),
    "uniform-EEN-large": ("hub", S.PAT_EEN, 399, 2, False, 150, 12000),
}


def _uniform_counts(name, small, hub, canonical=True):
  graph, pattern, r, mode3, want_small, T, base = UNIFORM[name]
  inc = small if graph == "small" else hub
  if r is None:
    r = _largest_row(inc, pattern)
  if mode3 is None:
    choose = lambda seed, row, q: S.expand_choice(seed, pattern, r, row, q)
  else:
    staged = None if pattern != S.PAT_NNE or mode3 != 2 else want_small
    choose = _reject(inc, pattern, r, mode3, want_small, canonical, staged)
  obs, q = _counts(inc, pattern, r, T, base, choose)
  return obs, T, q


@pytest.mark.parametrize("name", list(UNIFORM))
def test_restatement_draws_uniform_subsets(name, small, hub):
  obs, T, q = _uniform_counts(name, small, hub)
  p = subset_pvalue(obs, T, q)
  print("%s: n = %d, q = %d, T = %d, p-value %.4g" % (name, obs.size, q, T, p))
  assert 1e-4 < p < 1 - 1e-4, (name, p, obs)


@pytest.mark.parametrize("name", ["paths-NN-small", "paths-NNE-small"])
def test_without_the_first_path_rule_the_test_fails(name, small, hub):
  """Power control: every path accepted instead of the first one to its
  column favours columns with many paths; the same statistic on the same
  row and seeds must reject it."""
  obs, T, q = _uniform_counts(name, small, hub, canonical=False)
  p = subset_pvalue(obs, T, q)
  print("%s without the rule: p-value %.4g" % (name, p))
  assert p < 1e-4, (name, p)


# ---- draws with replacement -------------------------------------------------
def _plain_pvalue(obs):
  return scipy.stats.chisquare(obs, np.full(obs.size, obs.sum() / obs.size)).pvalue


def test_negatives_and_their_neighbours_are_uniform(small):
  inc = small
  assert inc.node_degree().min() > 0 and inc.edge_size().min() > 0
  v = int(np.argmax(inc.node_degree()))
  e = int(np.argmax(inc.edge_size()))
  K, Q = 5, 4000
  nnq, neq = S._q(inc.N, [(v, Q)]), S._q(inc.E, [(e, Q)])
  zero = (np.zeros(inc.N, np.int32), np.zeros(inc.E, np.int32))
  idx, _, b = S.stream(inc, "fobe", 13000, K, zero, (nnq, neq))
  assert b[:5] == [0] * 5 and b[-1] == 5 * Q
  ps = {}
  for blk, (col, n) in enumerate(((2, inc.N), (3, inc.E), (3, inc.E), (3, inc.E), (0, inc.N))):
    c = idx[b[4 + blk]:b[5 + blk], col] - 1
    ps["block %d" % blk] = _plain_pvalue(np.bincount(c, minlength=n))
  # the repeated edge-edge block has a stream of its own
  assert not np.array_equal(idx[b[5]:b[6], 3], idx[b[6]:b[7], 3])
  # node rows' negatives: ne_k from E(v); edge rows' negatives: nn_k from N(e)
  ev = inc.col_n[inc.rp_n[v]:inc.rp_n[v + 1]]
  ne_k = idx[b[7]:b[8], 4 + K:].ravel() - 1
  assert np.isin(ne_k, ev).all()
  ps["ne_k"] = _plain_pvalue(np.bincount(np.searchsorted(ev, ne_k), minlength=ev.size))
  members = inc.col_e[inc.rp_e[e]:inc.rp_e[e + 1]]
  nn_k = idx[b[8]:b[9], 4:4 + K].ravel() - 1
  assert np.isin(nn_k, members).all()
  ps["nn_k"] = _plain_pvalue(np.bincount(np.searchsorted(members, nn_k), minlength=members.size))
  print(ps)
  assert all(1e-4 < p < 1 - 1e-4 for p in ps.values()), ps


def test_positive_neighbour_draws_are_uniform(hub):
  inc = hub
  K = 16
  nq, eq = S._q(inc.N, [(0, 300)]), S._q(inc.E, [(399, 300)])
  ev = inc.col_n[inc.rp_n[0]:inc.rp_n[1]]
  members = inc.col_e[inc.rp_e[399]:inc.rp_e[400]]
  ce = np.zeros(ev.size, np.int64)
  cn = np.zeros(members.size, np.int64)
  for seed in range(14000, 14008):
    idx, _, b = S.stream(inc, "fobe", seed, K, (nq, eq), None, S._t(reject_w=0))
    node_rows = idx[b[2]:b[3]]  # (0, e') for every e' of E(0)
    edge_rows = idx[b[3]:b[4]]  # (u, 399) for every member u
    assert node_rows.shape[0] == 300 and edge_rows.shape[0] == 300
    ne_k = node_rows[:, 4 + K:].ravel() - 1
    nn_k = edge_rows[:, 4:4 + K].ravel() - 1
    assert np.isin(ne_k, ev).all() and np.isin(nn_k, members).all()
    ce += np.bincount(np.searchsorted(ev, ne_k), minlength=ev.size)
    cn += np.bincount(np.searchsorted(members, nn_k), minlength=members.size)
    # the other list of each record comes from the record's own column
    for rec in node_rows[::37]:
      assert np.isin(rec[4:4 + K] - 1, inc.col_e[inc.rp_e[rec[3] - 1]:inc.rp_e[rec[3]]]).all()
  ps = (_plain_pvalue(ce), _plain_pvalue(cn))
  print(ps)
  assert all(1e-4 < p < 1 - 1e-4 for p in ps), ps
