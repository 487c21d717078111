"""The block primitives of the device SVD (csrc/hgx_spmm.hip, _hgx.Svd) at
the smallest shapes that can go wrong, against float64 numpy / scipy. The
bars are the fp32 summation bounds (terms x 2^-24 x the sum of magnitudes),
so nothing is measured; the kernels sum in float64 and sit far inside."""

import numpy as np
import pytest

from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd.hypergraph_util import Incidence

pytestmark = pytest.mark.gpu

U24 = 2.0**-24
EDGE, NODE = _hgx.Svd.EDGE, _hgx.Svd.NODE
WIDTHS = (1, 3, 4, 17, 64, 136, 264)


def small_incidence():
  """70 nodes x 130 edges with node degrees 0, 1, 2, 63, 64, 65 and 130
  among the rows (the other rows draw 1..40 edges)."""
  rng = np.random.default_rng(0)
  deg = rng.integers(1, 41, 70)
  deg[[0, 5, 11, 20, 33, 47, 69]] = [0, 1, 2, 63, 64, 65, 130]
  cols = [np.sort(rng.choice(130, d, replace=False)) for d in deg]
  rp = np.concatenate([[0], np.cumsum(deg)])
  return Incidence(70, 130, rp, np.concatenate(cols))


# long_row 0: the library's threshold (no row of this matrix is long);
# 16: the rows of 63 / 64 / 65 / 130 incidences are summed in pieces
@pytest.fixture(scope="module", params=[0, 16])
def engine(request):
  inc = small_incidence()
  ctx = _hgx.Context(0)  # its own context: the incidence must stay resident
  ctx.upload(inc)
  svd = _hgx.Svd(ctx, long_row=request.param)
  a = inc.to_scipy()[0].astype(np.float64)
  yield svd, inc, a
  ctx.close()


@pytest.mark.parametrize("b", WIDTHS)
@pytest.mark.parametrize("dst_side", [NODE, EDGE])
def test_spmm(engine, b, dst_side):
  svd, inc, a = engine
  m = a if dst_side == NODE else a.T.tocsr()
  deg = np.diff(m.indptr)
  x = np.random.default_rng(b).standard_normal((m.shape[1], b)).astype(np.float32)
  svd.panel(0, 1 - dst_side, b)
  svd.panel(1, dst_side, b)
  svd.set(0, 0, x)
  svd.spmm(1, 0, 0, 0, b)
  y = svd.get(1, 0, b)
  ref = m @ x.astype(np.float64)
  bound = deg[:, None] * U24 * (m @ np.abs(x.astype(np.float64)))
  assert np.all(np.abs(y - ref) <= bound)
  assert np.all(y[deg == 0] == 0)
  svd.panel(1, dst_side, b)  # zeroed again
  svd.spmm(1, 0, 0, 0, b)
  assert np.array_equal(svd.get(1, 0, b), y)


@pytest.mark.parametrize("b", (1, 5, 64))
@pytest.mark.parametrize("dst_side", [NODE, EDGE])
def test_spmm_on_unaligned_columns(engine, b, dst_side):
  """A column range that does not start on a float4 boundary takes the
  one-column-per-lane form; the columns around the range stay untouched."""
  svd, inc, a = engine
  m = a if dst_side == NODE else a.T.tocsr()
  x = np.random.default_rng(b).standard_normal((m.shape[1], b + 3)).astype(np.float32)
  svd.panel(0, 1 - dst_side, b + 3)
  svd.panel(1, dst_side, b + 7)
  svd.set(0, 0, x)
  svd.spmm(1, 2, 0, 1, b)
  y = svd.get(1, 0, b + 7)
  xs = x[:, 1:1 + b].astype(np.float64)
  bound = np.diff(m.indptr)[:, None] * U24 * (m @ np.abs(xs))
  assert np.all(np.abs(y[:, 2:2 + b] - m @ xs) <= bound)
  assert np.all(y[:, :2] == 0) and np.all(y[:, 2 + b:] == 0)
  # an aligned range next to columns that must survive
  svd.spmm(1, 4, 0, 0, b)
  y2 = svd.get(1, 0, b + 7)
  assert np.array_equal(y2[:, :4], y[:, :4])
  assert np.array_equal(y2[:, 4 + b:], y[:, 4 + b:])
  xs = x[:, :b].astype(np.float64)
  bound = np.diff(m.indptr)[:, None] * U24 * (m @ np.abs(xs))
  assert np.all(np.abs(y2[:, 4:4 + b] - m @ xs) <= bound)


@pytest.fixture(scope="module", params=[1, 63, 64, 65, 4097])
def tall(request):
  """An engine whose node-side panels have n rows."""
  n = request.param
  inc = Incidence(n, 1, np.arange(n + 1), np.zeros(n, np.int32))
  ctx = _hgx.Context(0)
  ctx.upload(inc)
  svd = _hgx.Svd(ctx)
  yield svd, n
  ctx.close()


@pytest.mark.parametrize("p,q", [(1, 1), (24, 8), (136, 264)])
def test_gram_and_apply(tall, p, q):
  svd, n = tall
  rng = np.random.default_rng(1000 * p + q)
  P = rng.standard_normal((n, p)).astype(np.float32)
  Q = rng.standard_normal((n, q)).astype(np.float32)
  M = rng.standard_normal((q, p))
  svd.panel(0, NODE, p)
  svd.panel(1, NODE, q)
  svd.set(0, 0, P)
  svd.set(1, 0, Q)
  P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
  g = svd.gram(0, 0, p, 1, 0, q)
  assert g.dtype == np.float64 and g.shape == (p, q)
  assert np.all(np.abs(g - P64.T @ Q64) <= n * U24 * (np.abs(P64).T @ np.abs(Q64)))
  assert np.array_equal(svd.gram(0, 0, p, 1, 0, q), g)
  # P <- Q M
  svd.apply(0, 0, 1, 0, M)
  r = svd.get(0, 0, p)
  assert np.all(np.abs(r - Q64 @ M) <= q * U24 * (np.abs(Q64) @ np.abs(M)))
  svd.set(0, 0, P)
  svd.apply(0, 0, 1, 0, M)
  assert np.array_equal(svd.get(0, 0, p), r)
  # P <- beta P + Q M: one rounding of a float64 sum of q + 1 terms
  svd.set(0, 0, P)
  svd.apply(0, 0, 1, 0, M, beta=-0.75)
  r = svd.get(0, 0, p)
  mag = 0.75 * np.abs(P64) + np.abs(Q64) @ np.abs(M)
  assert np.all(np.abs(r - (Q64 @ M - 0.75 * P64)) <= (q + 1) * U24 * mag)
  # column scaling: one rounding
  s = rng.standard_normal(q)
  svd.scale(1, 0, s)
  assert np.all(np.abs(svd.get(1, 0, q) - Q64 * s) <= U24 * np.abs(Q64 * s))


def test_views_copy_and_validation(engine):
  svd, inc, _ = engine
  x = np.random.default_rng(5).standard_normal((inc.E, 12)).astype(np.float32)
  svd.panel(0, EDGE, 12)
  svd.panel(1, EDGE, 12)
  svd.panel(2, NODE, 12)
  svd.set(0, 0, x)
  svd.copy(1, 3, 0, 5, 4)
  y = svd.get(1, 0, 12)
  assert np.array_equal(y[:, 3:7], x[:, 5:9]) and np.all(y[:, :3] == 0)
  assert np.all(y[:, 7:] == 0)
  # a Gram of column ranges inside wider panels
  g = svd.gram(0, 2, 5, 1, 3, 4)
  ref = x[:, 2:7].astype(np.float64).T @ x[:, 5:9].astype(np.float64)
  assert np.all(np.abs(g - ref) <= inc.E * U24 * (np.abs(x[:, 2:7]).T.astype(np.float64)
                                                  @ np.abs(x[:, 5:9]).astype(np.float64)))
  with pytest.raises(AssertionError):
    svd.get(0, 10, 3)  # outside the panel
  with pytest.raises(AssertionError):
    svd.apply(0, 0, 0, 2, np.eye(4))  # onto its own source columns
  with pytest.raises(AssertionError):
    svd.spmm(1, 0, 0, 0, 4)  # both on the edge side
  with pytest.raises(AssertionError):
    svd.gram(0, 0, 4, 2, 0, 4)  # two sides
  with pytest.raises(ValueError):
    svd.apply(1, 0, 0, 0, np.full((4, 4), np.nan))
  with pytest.raises(RuntimeError):
    svd.gram(7, 0, 1, 7, 0, 1)  # never allocated
  # the engine is still usable
  svd.spmm(2, 0, 0, 0, 12)
  a = inc.to_scipy()[0].astype(np.float64)
  ref = a @ x.astype(np.float64)
  assert np.all(np.abs(svd.get(2, 0, 12) - ref) <=
                inc.node_degree()[:, None] * U24 * (a @ np.abs(x.astype(np.float64))))


def test_a_replaced_incidence_is_refused():
  """An engine keeps tables of the incidence it was created on: after any
  later upload, even of a matrix with the same N, E and nnz, its calls fail
  with HGX_ESTATE instead of using them."""
  inc = small_incidence()
  ctx = _hgx.Context(0)
  try:
    ctx.upload(inc)
    svd = _hgx.Svd(ctx, long_row=16)
    svd.panel(0, EDGE, 4)
    svd.panel(1, NODE, 4)
    svd.spmm(1, 0, 0, 0, 4)
    ctx.upload(inc)
    with pytest.raises(_hgx.HgxError):
      svd.spmm(1, 0, 0, 0, 4)
    with pytest.raises(_hgx.HgxError):
      svd.panel(2, NODE, 4)
    fresh = _hgx.Svd(ctx, long_row=16)
    fresh.panel(0, EDGE, 4)
    fresh.panel(1, NODE, 4)
    fresh.spmm(1, 0, 0, 0, 4)
  finally:
    ctx.close()
