"""GPU: the paired-wave form of the trainer step (tuning train_wave_pair).

One record on two waves of a 512-thread workgroup: the node wave owns the
node-table slots, the edge wave the edge-table slots; they exchange P, Q and
y2 through LDS. Nothing about the arithmetic or its order differs from the
one-wave form, so tables and epoch losses are compared bit for bit against
it (same records, initial tables, host permutations), and against the CPU
oracle with the bars of test_gpu_train._check.
"""

import numpy as np
import pytest

import oracle as O
from conftest import golden
from test_gpu_train import _check, _mixed_reuse_records, _run_both

pytestmark = pytest.mark.gpu

PAIRED = (512, 4)  # threads, records per workgroup of the paired form


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.set_tuning("train_wave_pair", -1)
  c.close()


def _widen5(idx, K):
  """The golden streams have K = 3 neighbours and the step is built for the
  default K = 5 only (hgx_train falls back to the two-kernel step, where the
  tuning changes nothing): the same records with both lists padded to five
  by the padding row (id 0), which do take the step."""
  assert K <= 5
  z = np.zeros((idx.shape[0], 5 - K), idx.dtype)
  return np.ascontiguousarray(np.concatenate(
      [idx[:, :4 + K], z, idx[:, 4 + K:], z], axis=1)), 5


def _rows(idx, K):
  nrows = int(idx[:, [0, 2] + list(range(4, 4 + K))].max()) + 2
  erows = int(idx[:, [1, 3] + list(range(4 + K, 4 + 2 * K))].max()) + 2
  return nrows, erows


def _train_both_forms(ctx, idx, tgt, K, d, loss, act, batch, epochs, seed=0):
  """[unpaired, paired] -> (node table, edge table, losses, step geometry,
  path stats, MULTI batches), same init and host permutations."""
  rs = np.random.RandomState(seed)
  nrows, erows = _rows(idx, K)
  nt = rs.uniform(-0.05, 0.05, (nrows, d)).astype(np.float32)
  et = rs.uniform(-0.05, 0.05, (erows, d)).astype(np.float32)
  perms = np.stack([rs.permutation(idx.shape[0]) for _ in range(epochs)])
  ctx.records_set(idx, tgt)
  out = []
  try:
    for pair in (0, 1):
      ctx.set_tuning("train_wave_pair", pair)
      ctx.model_init(d, nrows, erows, node_tab=nt, edge_tab=et)
      gl = ctx.train(batch=batch, max_epochs=epochs, loss=loss, act=act,
                     perms=perms, min_delta=-1.0)
      out.append(ctx.model_get() + (gl, ctx.train_step_geometry(),
                                    ctx.train_path_stats(),
                                    ctx.train_multi_pending()))
  finally:
    ctx.set_tuning("train_wave_pair", -1)
  return out, perms, (nt, et)


def _assert_bitwise(u, p, step=True):
  if step:
    assert u[3][1] > 0 and u[3][0] == 64 * u[3][1], u[3]  # one wave per record
    assert p[3] == PAIRED, p[3]
  assert u[4] == p[4] and u[5] == p[5], (u[4:], p[4:])
  for t in (0, 1):
    ne = u[t] != p[t]
    assert not ne.any(), (t, int(ne.sum()), np.flatnonzero(ne.any(1))[:8],
                          float(np.abs(u[t] - p[t]).max()))
  assert np.array_equal(u[2], p[2]), (u[2], p[2])


HEADS = {"fobe-kld": ("fobe_small_ns.npz", O.LOSS_KLD, O.ACT_SIGMOID),
         "hobe-mse": ("hobe_small.npz", O.LOSS_MSE, O.ACT_RELU)}


@pytest.mark.parametrize("batch", [256, 37, 100])
@pytest.mark.parametrize("heads", sorted(HEADS))
@pytest.mark.parametrize("d", [128, 72, 256, 200])
def test_paired_equals_unpaired_bitwise(ctx, d, heads, batch):
  """Tables and losses of 3 epochs, paired vs one wave per record. d = 72 and
  200 are padded rows; batch 37 and 100 are ragged (workgroups with fewer than
  four records, wave pairs with none). The golden stream as it is (K = 3: no
  step form, the tuning must change nothing) and widened to K = 5 (the step:
  the geometry of both runs is asserted)."""
  name, loss, act = HEADS[heads]
  z = golden(name)
  out, _, _ = _train_both_forms(ctx, z["idx"], z["tgt"], int(z["K"]), d, loss,
                                act, batch, epochs=3)
  _assert_bitwise(*out, step=False)
  idx, K = _widen5(z["idx"], int(z["K"]))
  out, _, init = _train_both_forms(ctx, idx, z["tgt"], K, d, loss, act, batch,
                                   epochs=3)
  _assert_bitwise(*out)
  nb = -(-z["idx"].shape[0] // batch)
  assert out[1][4] == (3 * nb, 0), out[1][4]  # every batch took the step
  assert not np.array_equal(out[1][0], init[0])
  assert not np.array_equal(out[1][1], init[1])


def _k5_synthetic():
  """The generator of test_gpu_train.test_train_k5_synthetic_with_duplicates:
  3,000 records over 29 node and 11 edge rows."""
  rs = np.random.RandomState(7)
  n, K = 3000, 5
  idx = np.zeros((n, 4 + 2 * K), np.int32)
  kind = rs.randint(0, 3, n)
  idx[kind == 0, 0] = rs.randint(1, 30, (kind == 0).sum())
  idx[kind == 0, 2] = rs.randint(1, 30, (kind == 0).sum())
  idx[kind == 1, 1] = rs.randint(1, 12, (kind == 1).sum())
  idx[kind == 1, 3] = rs.randint(1, 12, (kind == 1).sum())
  m = kind == 2
  idx[m, 0] = rs.randint(1, 30, m.sum())
  idx[m, 3] = rs.randint(1, 12, m.sum())
  idx[m, 4:4 + K] = rs.randint(1, 30, (m.sum(), K))
  idx[m, 4 + K:] = rs.randint(1, 12, (m.sum(), K))
  tgt = np.zeros((n, 3), np.float32)
  tgt[np.arange(n), kind] = rs.uniform(0, 1, n).astype(np.float32)
  return idx, tgt, K


def _records_naming_two_deferred(idx, K, perm, batch):
  """Over consecutive batches of one epoch: records of batch b + 1 naming at
  least two distinct rows that batch b defers (a row, of either table, in
  slots of several of its records)."""
  edge = np.array([s in (1, 3) or s >= 4 + K for s in range(4 + 2 * K)])
  keys = idx.astype(np.int64) + edge[None, :] * (1 << 32)  # (table, row)
  keys[idx == 0] = -1  # the padding row has its own path
  count, prev = 0, None
  for b in range(0, perm.size, batch):
    kb = keys[perm[b:b + batch]]
    if prev is not None:
      for rec in kb:
        count += len(set(rec[rec >= 0].tolist()) & prev) >= 2
    seen, deferred = set(), set()
    for rec in kb:
      mine = set(rec[rec >= 0].tolist())
      deferred |= mine & seen
      seen |= mine
    prev = deferred
  return count


@pytest.mark.parametrize("d", [128, 256])
def test_paired_hard_paths_bitwise(ctx, d):
  """29 + 11 rows under 3,584 slots per batch: rows repeated within a record,
  every row deferred, pending slots (several per record: the MULTI form),
  several flush slots per record, the overflow list, a ragged last batch."""
  idx, tgt, K = _k5_synthetic()
  out, perms, _ = _train_both_forms(ctx, idx, tgt, K, d, O.LOSS_MSE, O.ACT_RELU,
                                    256, epochs=2)
  # from the generator alone: the stream does hold MULTI batches
  for p in perms:
    assert _records_naming_two_deferred(idx, K, p, 256) > 0
  _assert_bitwise(*out)
  nb = -(-idx.shape[0] // 256)
  assert out[1][4] == (2 * nb, 0), out[1][4]
  assert out[1][5] > 0, out[1][5]


@pytest.mark.parametrize("name,d,batch", [("hobe_small.npz", 128, 256),
                                          ("fobe_small_ns.npz", 128, 256),
                                          ("hobe_small.npz", 256, 256),
                                          ("fobe_small_ns.npz", 256, 100)])
def test_paired_vs_oracle(ctx, name, d, batch):
  """The golden streams widened to K = 5 (see _widen5: as they are they do not
  reach the step), the oracle on the same widened records."""
  z = golden(name)
  loss, act = ((O.LOSS_MSE, O.ACT_RELU) if name.startswith("hobe")
               else (O.LOSS_KLD, O.ACT_SIGMOID))
  idx, K = _widen5(z["idx"], int(z["K"]))
  ctx.set_tuning("train_wave_pair", 1)
  try:
    o, g, init = _run_both(ctx, idx, z["tgt"], K, d, loss, act, batch, epochs=3)
    assert ctx.train_step_geometry() == PAIRED
  finally:
    ctx.set_tuning("train_wave_pair", -1)
  _check(o, g, init)


@pytest.mark.parametrize("d", [128, 256])
def test_paired_device_shuffle_twice_bitwise(ctx, d):
  """The P / Q / y2 exchange has no race: two device-shuffled runs from the
  same init give the same bits."""
  rs = np.random.RandomState(3)
  idx, tgt = _mixed_reuse_records(rs, 20, 256, 5, hub_batches={7, 8})
  ctx.records_set(idx, tgt)
  out = []
  ctx.set_tuning("train_wave_pair", 1)
  try:
    for _ in range(2):
      ctx.model_init(d, 20002, 20002, seed=9)
      gl = ctx.train(batch=256, max_epochs=2, loss=O.LOSS_MSE, act=O.ACT_RELU,
                     shuffle_seed=5, min_delta=-1.0)
      assert ctx.train_step_geometry() == PAIRED
      assert ctx.train_path_stats() == (40, 0)
      out.append(ctx.model_get() + (gl,))
  finally:
    ctx.set_tuning("train_wave_pair", -1)
  assert np.array_equal(out[0][2], out[1][2])
  assert np.array_equal(out[0][0], out[1][0])
  assert np.array_equal(out[0][1], out[1][1])
