"""The coordinate-descent sweep (hgx_svd_cd_sweep, csrc/hgx_spmm.hip) against
its host statement on identical fp32 operands, and nmf_incidence / EmbedNMF
through the device with the checks of test_nmf_driver_cpu.py against sklearn
(tests/nmf_cases.py has the inputs and the checks)."""

import contextlib

import numpy as np
import pytest

import nmf_cases as C
from hypergraphembedding_amd import EmbedNMF, _hgx, nmf_incidence, synthetic
from hypergraphembedding_amd.runtime import get_context
from hypergraphembedding_amd.svd import NumpyBackend

pytestmark = pytest.mark.gpu

PAD = 16  # panel columns beyond the view
# Both sides do the same float64 arithmetic in another summation order (and
# with FMA contraction): one fp32 rounding may flip in a rare entry and the
# later coordinates of that row carry it on through ratios of order one.
P_TOL = 2.0**-21
V_TOL = 1e-6


@contextlib.contextmanager
def engine(rows):
  """An engine with a side of ``rows`` rows: (engine, side)."""
  n, e, side = {1000: (1000, 65, 1), 65: (1000, 65, 0), 1: (65, 1, 0)}[rows]
  ctx = get_context()
  ctx.upload(C.star_incidence(n, e))
  eng = _hgx.Svd(ctx)
  try:
    assert eng.rows[side] == rows
    yield eng, side
  finally:
    eng.close()


def load(eng, side, P, B, same_slot=False, seed=0):
  """P at PCOL0 of slot 0; B at BCOL0 of slot 1, or right behind P in slot 0;
  every other column random. Returns (bslot, bcol0, {slot: width})."""
  rows, k = P.shape
  rng = np.random.default_rng(seed)
  widths = {0: k + PAD + (k if same_slot else 0)}
  bslot, bcol0 = (0, C.PCOL0 + k) if same_slot else (1, C.BCOL0)
  widths[bslot] = widths[0] if same_slot else k + PAD
  for slot, width in widths.items():
    eng.panel(slot, side, width)
    eng.set(slot, 0, rng.random((rows, width)).astype(np.float32))
  eng.set(0, C.PCOL0, P)
  eng.set(bslot, bcol0, B)
  return bslot, bcol0, widths


def run_parity(rows, k, zero_diag=None, same_slot=False):
  P, B, Q, want, viol = C.sweep_case(rows, k, zero_diag)
  with engine(rows) as (eng, side):
    bslot, bcol0, widths = load(eng, side, P, B, same_slot)
    before = {s: eng.get(s, 0, w) for s, w in widths.items()}
    v = eng.cd_sweep(0, C.PCOL0, bslot, bcol0, Q)
    after = {s: eng.get(s, 0, w) for s, w in widths.items()}
    got = after[0][:, C.PCOL0:C.PCOL0 + k]
    # the same operands again: bitwise the same, violation included
    eng.set(0, C.PCOL0, P)
    v2 = eng.cd_sweep(0, C.PCOL0, bslot, bcol0, Q)
    got2 = eng.get(0, C.PCOL0, k)
    stats = eng.cd_stats()
  dp = np.abs(got.astype(np.float64) - want).max()
  print(f"rows {rows} k {k}: |dP| {dp / np.abs(want).max():.3e} of max|P| "
        f"(bound {P_TOL:.3e}), violation {abs(v - viol) / viol:.3e} relative")
  keep = np.ones(widths[0], bool)
  keep[C.PCOL0:C.PCOL0 + k] = False
  assert np.array_equal(after[0][:, keep], before[0][:, keep])
  if bslot != 0:
    assert np.array_equal(after[1], before[1])
  assert (got >= 0).all()
  assert abs(v - viol) <= V_TOL * viol
  assert dp <= P_TOL * np.abs(want).max()
  assert v2 == v and np.array_equal(got2, got)
  assert stats["sweeps"] == 2 and stats["sweep_ms"] > 0
  return P, got


# k = 1, 3, 8 (several rows per wave), 64 / 65 (one and two coordinates per
# lane), 128, 143 / 144 (the last k with Q in LDS and the first without), 200,
# 256 and the limit 512; 1000 rows are more than one workgroup from k = 2 on,
# 65 rows and 1 row cross the group and wave edges
PARITY = ([(1000, k) for k in (1, 3, 8, 64, 65, 128, 143, 144, 200, 256)] +
          [(65, k) for k in (3, 70, 256, 512)] + [(1, k) for k in (3, 8, 70, 200)])


@pytest.mark.parametrize("rows,k", PARITY)
def test_sweep_parity(rows, k):
  run_parity(rows, k)


def test_sweep_same_slot():
  run_parity(1000, 8, same_slot=True)


@pytest.mark.parametrize("k,zero", [(8, 5), (65, 64)])
def test_sweep_zero_diagonal_keeps_column(k, zero):
  P, got = run_parity(1000, k, zero_diag=zero)
  assert np.array_equal(got[:, zero], P[:, zero])


def test_sweep_rejects():
  P, B, Q, _, _ = C.sweep_case(65, 3)
  with engine(65) as (eng, side):
    eng.panel(0, side, 530)
    eng.panel(1, side, 530)
    eng.panel(2, 1 - side, 8)
    bad = np.array(Q)
    bad[2, 1] = np.nan
    with pytest.raises(ValueError):
      eng.cd_sweep(0, 0, 1, 0, bad)
    with pytest.raises(_hgx.HgxError):  # above the sweep's limit
      eng.cd_sweep(0, 0, 1, 0, np.eye(513))
    with pytest.raises(AssertionError):  # overlapping columns of one slot
      eng.cd_sweep(0, 0, 0, 2, Q)
    with pytest.raises(AssertionError):  # panels of two sides
      eng.cd_sweep(0, 0, 2, 0, Q)
    with pytest.raises(AssertionError):  # outside the panel
      eng.cd_sweep(0, 528, 1, 0, Q)
    with pytest.raises(AssertionError):  # fused: the source is the other side's
      eng.cd_sweep_fused(0, 0, 1, 0, Q)
    assert eng.cd_stats()["sweeps"] == 0


# rows of 1 to about 15 incidences on the node side, about 90 on the edge
# side: odd and even counts for the two-at-a-time gather and its tail
FUSED = [(side, k) for side in (0, 1) for k in (3, 65, 128, 144, 256)]


@pytest.mark.parametrize("side,k", FUSED)
def test_fused_sweep_parity(side, k):
  """hgx_svd_cd_sweep_fused against NumpyBackend.cd_sweep_fused on identical
  operands: the product row is summed in CSR order in float64 on both sides,
  so the bounds of the unfused parity hold."""
  inc = synthetic.random_hypergraph(1000, 65, 6, seed=1)
  rows = (inc.E, inc.N)
  P, _, Q = C.sweep_operands(rows[side], k, seed=7 * k + side)
  rng = np.random.default_rng(k)
  pq = (P.astype(np.float64) @ Q).mean()
  X = (rng.random((rows[1 - side], k)) * 2 * pq * rows[side] / inc.nnz
       ).astype(np.float32)
  wide = rng.random((rows[side], k + PAD)).astype(np.float32)
  xwide = rng.random((rows[1 - side], k + PAD)).astype(np.float32)
  ctx = get_context()
  ctx.upload(inc)
  out = []
  for be in (NumpyBackend(inc), _hgx.Svd(ctx)):
    try:
      be.panel(0, side, k + PAD)
      be.panel(1, 1 - side, k + PAD)
      be.set(0, 0, wide)
      be.set(1, 0, xwide)
      be.set(0, C.PCOL0, P)
      be.set(1, C.BCOL0, X)
      v = be.cd_sweep_fused(0, C.PCOL0, 1, C.BCOL0, Q)
      after, xafter = be.get(0, 0, k + PAD), be.get(1, 0, k + PAD)
      be.set(0, C.PCOL0, P)
      v2 = be.cd_sweep_fused(0, C.PCOL0, 1, C.BCOL0, Q)
      assert v2 == v and np.array_equal(be.get(0, 0, k + PAD), after)
      out.append((v, after, xafter))
    finally:
      be.close()
  (vr, want, xwant), (v, got, xgot) = out
  view = slice(C.PCOL0, C.PCOL0 + k)
  dp = np.abs(got[:, view].astype(np.float64) - want[:, view]).max()
  print(f"fused side {side} k {k}: |dP| {dp / np.abs(want[:, view]).max():.3e} "
        f"of max|P|, violation {abs(v - vr) / vr:.3e} relative")
  changed = want[:, view] != P
  assert (changed & (want[:, view] == 0)).any()
  assert (changed & (want[:, view] > 0)).any()
  keep = np.ones(k + PAD, bool)
  keep[view] = False
  assert np.array_equal(got[:, keep], wide[:, keep])
  assert np.array_equal(xgot, xwant)
  assert abs(v - vr) <= V_TOL * vr
  assert dp <= P_TOL * np.abs(want[:, view]).max()


# ---- the solver ----------------------------------------------------------------
@pytest.mark.parametrize("init", C.INITS)
@pytest.mark.parametrize("name", list(C.CASES))
def test_custom_init_against_sklearn(name, init):
  """The bounds and the CPU figures: test_nmf_driver_cpu.py. Measured on an
  MI355X: DESIGN §4.8."""
  seen = {}

  def solve(inc, k, **kw):
    W, H, info = nmf_incidence(inc, k, **kw)
    seen.update(info)
    return W, H, info

  C.check_custom(name, init, solve)
  assert seen["sweep_ms"] > 0
  # the products are formed inside the sweeps; one for the final error
  assert seen["stats"]["spmm_calls"] == 1


@pytest.mark.parametrize("name", list(C.CASES))
def test_default_init_in_sklearn_spread(name):
  C.check_default(name, EmbedNMF)


def test_reproducible():
  inc, k, _ = C.case("planted4")
  runs = []
  for _ in range(2):
    np.random.seed(7)
    runs.append(nmf_incidence(inc, k))
  (W, H, i1), (W2, H2, i2) = runs
  assert np.array_equal(W, W2) and np.array_equal(H, H2)
  assert i1["violation"] == i2["violation"]


def test_embed_nmf(tiny_hypergraph):
  C.check_embed_nmf(EmbedNMF, nmf_incidence, tiny_hypergraph)
