"""Every kernel instantiation the dense MLP engine's dispatchers can select
(csrc/hgx_mlp.hip: mlp_fwd<NCH>, mlp_bwd<NCH, FH>, mlp_wgrad<NCH>, the label
head's KH forms), and the host loops' second iterations (predict chunks of
4096 rows, loss-partial passes of 1024 batches, the device shuffle), each
bit for bit against the CPU restatement (oracle/mlpref.c).

The restatement orders every sum by position, not by which instantiation
ran, so the bar is test_gpu_mlp.py's: trained weights array_equal, epoch
losses rtol 1e-5 (the device sums loss partials per tile), predictions
array_equal. tests/test_mlp_cases_cpu.py holds the restatement to float64
autograd over whole runs at multi-chunk widths.

mlp_cases.reach() restates the dispatch; test_cases_cover_every_instantiation
asserts that the cases below reach all of mlp_cases.REACHABLE. Every fit
case has at least two batches: with the default prefetch, batch 0 gathers
its input rows and later batches read them densely, so both loaders of each
mlp_fwd<NCH> run.
"""

import numpy as np
import pytest

import oracle as O
from hypergraphembedding_amd import _hgx
from mlp_cases import (REACHABLE, glorot, make_case, reach, run_both,
                       shuffle_perms)

pytestmark = pytest.mark.gpu

# (kind, I, D): the smallest widths found for each target
INSTANTIATIONS = (
    # pre forward <k> and post backward <k>, k = 2..8; the rec layers' loss
    # epilogue over 2k column tiles; fused joint backward <2..5, true>
    [(2, I, 24) for I in (100, 130, 200, 260, 330, 390, 460)] +
    # fused two-term joint backward <6, true>, <7, true>, <8, true>; the
    # mixed-K hidden + post forward at several chunks
    [(2, 390, 100), (2, 260, 150), (2, 200, 250)] +
    # unfused two-term mlp_bwd<8>, mlp_head at KH = 8
    [(2, 60, 300)] +
    # two-term mlp_bwd<0> at 10 chunks
    [(2, 300, 300)] +
    # forward <3>, <4>, <5>, <6>; backward <2, true> / <2>, <3, true> / <3>
    [(1, 130, 70), (1, 260, 150)] +
    # forward <7>, hidden forward <0> at 10 chunks, unfused head at KH = 8,
    # mlp_bwd<5>
    [(1, 390, 300)] +
    # forward <0> at 10, 9 and 18 chunks, the head's loop form, mlp_bwd<0>
    # at 9 chunks
    [(1, 600, 530)] +
    # classifier: forward <4>, <5>, <7> with the node / edge column boundary
    # c1 inside a chunk; KH = 2, KH = 4
    [(0, 100, 0), (0, 130, 0), (0, 200, 0)] +
    # forward <0> at 10 and 19 chunks; KH = 8 and the loop
    [(0, 300, 0), (0, 600, 0)])
N_FIT, BATCH = 600, 256  # three batches, the last of 88 rows

EQUALITY_SHAPES = [(2, 260, 150), (1, 130, 70)]
ROW_EDGE_SHAPE = (2, 40, 24)
ROW_EDGE_BATCHES = (63, 65, 128, 129, 192, 193, 255)
PREDICT_SHAPES = [(0, 40, 0), (1, 40, 24)]
PREDICT_NS = (4096, 4097, 8200)
MANY_BATCH_SHAPES = [(0, 8, 0), (2, 8, 4)]
N_MANY = 1030
SHUFFLE_SHAPES = [(0, 40, 0), (1, 40, 24)]
N_SHUFFLE = 1500


def batch_sizes(n, batch):
  return sorted({min(batch, n - p) for p in range(0, n, batch)})


def launches():
  """(kind, I, D, M, train, fuse_head) of every batch and predict chunk the
  tests of this file run."""
  out = []
  for k, I, D in INSTANTIATIONS:
    out += [(k, I, D, M, True, 1) for M in batch_sizes(N_FIT, BATCH)]
    out += [(k, I, D, N_FIT, False, 1)]
  for k, I, D in EQUALITY_SHAPES:
    out += [(k, I, D, M, True, f) for M in batch_sizes(N_FIT, BATCH) for f in (1, 0)]
  for b in ROW_EDGE_BATCHES:
    out += [ROW_EDGE_SHAPE + (M, True, 1) for M in batch_sizes(2 * b + 1, b)]
  for k, I, D in PREDICT_SHAPES:
    out += [(k, I, D, M, False, 1) for n in PREDICT_NS for M in batch_sizes(n, 4096)]
  for k, I, D in MANY_BATCH_SHAPES:
    out += [(k, I, D, 1, True, 1)]
  for k, I, D in SHUFFLE_SHAPES:
    out += [(k, I, D, M, True, 1) for M in batch_sizes(N_SHUFFLE, BATCH)]
  return out


@pytest.fixture(scope="module")
def ctx():
  c = _hgx.Context(0)
  yield c
  c.close()


def check_fit(gl, cl, wg, wc, epochs):
  assert len(gl) == len(cl) == epochs
  np.testing.assert_allclose(gl, cl, rtol=1e-5)
  diff = np.abs(wg - wc)
  assert diff.max() == 0.0, (diff.max(), int((diff > 0).sum()))
  assert np.isfinite(wc).all()


def check_predict(m, kind, I, D, wc, nt, et, nr, er):
  yg = m.predict(0, nr, er)
  yc = O.mlp_predict(kind, I, D, wc, nt, et, 0, nr, er)
  np.testing.assert_array_equal(yg, yc)
  if kind != 0:
    for out, rows in ((1, np.arange(nt.shape[0])), (2, np.arange(et.shape[0]))):
      a, b = (rows, None) if out == 1 else (None, rows)
      np.testing.assert_array_equal(
          m.predict(out, a, b), O.mlp_predict(kind, I, D, wc, nt, et, out, a, b))


# Adagrad settings. At Keras' (0.01, 1e-7) the first step is lr sign(g) on
# every weight, which at widths of a few hundred saturates the label head
# within a batch or two: at (1, 600, 530) and (0, 600, 0) y (1 - y) is
# exactly 0 from the second batch on and no weight moves again, so batches
# 1..5 (the dense-read forward loaders, the 88-row tail) would compare zeros.
# At (1, 10) the step is about g / 10 and every layer moves in every batch
# (asserted on the restatement: the last batch changes every layer).
SETTINGS = {"keras": (0.01, 1e-7), "prop": (1.0, 10.0)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("kind,I,D", INSTANTIATIONS)
def test_every_instantiation(ctx, kind, I, D, setting):
  lr, eps = SETTINGS[setting]
  m, (nt, et, nr, er), wg, wc, gl, cl = run_both(ctx, kind, I, D, N_FIT, 2,
                                                 batch=BATCH, lr=lr, eps=eps)
  try:
    check_fit(gl, cl, wg, wc, 2)
    check_predict(m, kind, I, D, wc, nt, et, nr, er)
    if setting == "prop":
      # run_both's inputs again (same seed), stopped one batch short
      rng, _, _, _, _, lab = make_case(kind, I, D, N_FIT, 3)
      w0 = glorot(m.shapes, rng, 0.1)
      perms = np.stack([rng.permutation(N_FIT) for _ in range(2)])
      wp, _ = O.mlp_fit(kind, I, D, w0, nt, et, nr, er, lab, perms, batch=BATCH,
                        lr=lr, eps=eps, min_delta=-1e30, seed=77, max_batches=5)
      off = 0
      for k, n in m.shapes:
        sl = slice(off, off + k * n + n)
        off = sl.stop
        assert (wp[sl] != wc[sl]).mean() > 0.25, ((k, n), (wp[sl] != wc[sl]).mean())
  finally:
    m.close()


def test_cases_cover_every_instantiation():
  got = set()
  for k, I, D, M, train, fuse in launches():
    got |= reach(k, I, D, M, train, fuse)
  assert got == set(REACHABLE), (sorted(set(REACHABLE) - got),
                                 sorted(got - set(REACHABLE)))
  # the instantiation cases alone select everything but the one-chunk fused
  # backward (the shuffle and predict tests' kind-1 shape) and mlp_wgrad<1>,
  # <3> (the row-edge test's)
  inst = set()
  for k, I, D in INSTANTIATIONS:
    for M in batch_sizes(N_FIT, BATCH):
      inst |= reach(k, I, D, M, True)
    inst |= reach(k, I, D, N_FIT, False)
  assert set(REACHABLE) - inst == {"mlp_bwd<1,true>", "mlp_wgrad<1>", "mlp_wgrad<3>"}


def fit_with_tuning(ctx, key, value, default, kind, I, D, data, w0, seed):
  nt, et, nr, er, lab = data
  ctx.set_tuning(key, value)
  try:
    m = _hgx.Mlp(ctx, kind, I, D)
    m.set_weights(w0)
    m.set_tables(nt, et)
    m.set_samples(nr, er, lab)
    losses = m.fit(batch=BATCH, max_epochs=2, min_delta=-1e30, seed=seed)
    w = m.get_weights()
    m.close()
  finally:
    ctx.set_tuning(key, default)
  return w, np.asarray(losses)


@pytest.mark.parametrize("kind,I,D", EQUALITY_SHAPES)
def test_fuse_and_prefetch_equalities_at_wide_shapes(ctx, kind, I, D):
  """test_gpu_mlp.py's two equalities at multi-chunk shapes: the label head
  fused into the joint layers' delta launch or in its own launch, and the
  next batch's input rows gathered in the hidden layer's launch, in the
  joint layers' launch, or in place. Weights and losses bit for bit."""
  rng, nt, et, nr, er, lab = make_case(kind, I, D, N_FIT, 5)
  m = _hgx.Mlp(ctx, kind, I, D)
  w0 = glorot(m.shapes, np.random.default_rng(2), 0.1)
  m.close()
  data = (nt, et, nr, er, lab)
  # the defaults (fused head, prefetch 1), then one tuning moved at a time
  res = [fit_with_tuning(ctx, key, v, 1, kind, I, D, data, w0, 4)
         for key, v in (("mlp_fuse_head", 1), ("mlp_fuse_head", 0),
                        ("mlp_prefetch", 2), ("mlp_prefetch", 0))]
  assert not np.array_equal(res[0][0], w0)
  for w, losses in res[1:]:
    np.testing.assert_array_equal(res[0][0], w)
    np.testing.assert_array_equal(res[0][1], losses)


@pytest.mark.parametrize("batch", ROW_EDGE_BATCHES)
def test_batch_row_edges(ctx, batch):
  """Two full batches and a one-row tail: mlp_wgrad<1..4> and the row-tile
  and head row clamps on both sides of their edges."""
  kind, I, D = ROW_EDGE_SHAPE
  m, _, wg, wc, gl, cl = run_both(ctx, kind, I, D, 2 * batch + 1, 2, batch=batch)
  try:
    check_fit(gl, cl, wg, wc, 2)
    assert m.stats()["batches"] == 6
  finally:
    m.close()


@pytest.mark.parametrize("kind,I,D", PREDICT_SHAPES)
def test_predict_chunks(ctx, kind, I, D):
  """hgx_mlp_predict cuts n into chunks of 4096 rows: one full chunk, a
  second chunk of one row, and three chunks."""
  rng, nt, et, _, _, _ = make_case(kind, I, D, 1, 21)
  m = _hgx.Mlp(ctx, kind, I, D)
  try:
    w = glorot(m.shapes, rng, 0.1)
    m.set_weights(w)
    m.set_tables(nt, et)
    nr = rng.integers(0, nt.shape[0], max(PREDICT_NS)).astype(np.int32)
    er = rng.integers(0, et.shape[0], max(PREDICT_NS)).astype(np.int32)
    first = {}
    for n in PREDICT_NS:
      for out in ((0,) if kind == 0 else (0, 1, 2)):
        a = nr[:n] if out != 2 else None
        b = er[:n] if out != 1 else None
        yg = m.predict(out, a, b)
        yc = O.mlp_predict(kind, I, D, w, nt, et, out, a, b)
        assert yg.shape == yc.shape and yg.shape[0] == n
        np.testing.assert_array_equal(yg, yc)
        assert yg.std() > 0
        if n == 4096:
          first[out] = yg
        elif n == 8200:
          np.testing.assert_array_equal(yg[:4096], first[out])
  finally:
    m.close()


@pytest.mark.parametrize("kind,I,D", MANY_BATCH_SHAPES)
def test_more_than_1024_batches(ctx, kind, I, D):
  """hgx_mlp_fit keeps loss partials for 1024 batches at a time: 1030
  batches of one sample cross into the second pass (kind 2: with the rec
  layers' partial slots; the prefetch buffers alternate across it)."""
  m, _, wg, wc, gl, cl = run_both(ctx, kind, I, D, N_MANY, 2, batch=1)
  try:
    check_fit(gl, cl, wg, wc, 2)
    assert m.stats()["batches"] == 2 * N_MANY
  finally:
    m.close()


@pytest.mark.parametrize("kind,I,D", SHUFFLE_SHAPES)
def test_device_shuffle_is_its_keys_order(ctx, kind, I, D):
  """fit(perms=None) (the production path: mlp_shuffle_keys, a 64-bit radix
  sort, mlp_permute) trains in the order its keys define."""
  seed, epochs = 12345, 2
  rng, nt, et, nr, er, lab = make_case(kind, I, D, N_SHUFFLE, 8)
  m = _hgx.Mlp(ctx, kind, I, D)
  try:
    w0 = glorot(m.shapes, rng, 0.1)
    m.set_weights(w0)
    m.set_tables(nt, et)
    m.set_samples(nr, er, lab)
    gl = m.fit(batch=BATCH, max_epochs=epochs, min_delta=-1e30, seed=seed)
    wg = m.get_weights()
  finally:
    m.close()
  perms = shuffle_perms(seed, epochs, N_SHUFFLE)
  assert not np.array_equal(perms[0], perms[1])
  assert not np.array_equal(perms[0], np.arange(N_SHUFFLE))
  wc, cl = O.mlp_fit(kind, I, D, w0, nt, et, nr, er, lab, perms, batch=BATCH,
                     min_delta=-1e30, seed=seed)
  check_fit(gl, cl, wg, wc, epochs)
