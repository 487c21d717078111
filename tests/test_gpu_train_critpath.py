"""GPU: the trainer step with its record words addressed from preloaded
kernel arguments (the driver forms each batch's bases into the placed
buffers), 1 / records from the host and the divisions by K as div_const.

None of it changes an operation's inputs or its rounding, so the default form
of every row width is compared bit for bit (tables and epoch losses) with the
one-wave form (train_wave_pair 0), which shares the helpers but not the
geometry, and both with the CPU oracle under the bars of test_gpu_train._check
(the oracle divides; a div_const that differed from the division on the device
would show there and in the benchmark's output digests, not in the bitwise
comparison). The batch sizes make 1 / records 1, 1/3, 1/5, 1/7, 1/8, 1/37 and
1/256; a one-batch epoch has q = 0 in every launch, where the padding row is
read from the table and no step is folded.
"""

import numpy as np
import pytest

import oracle as O
from test_gpu_train import _check
from test_gpu_train_pair import _k5_synthetic, _rows

pytestmark = pytest.mark.gpu

QUAD1 = (256, 1)   # threads, records per workgroup: the default at float2 rows
PAIRED = (512, 4)  # the default at float4 rows

HEADS = {"fobe-kld": (O.LOSS_KLD, O.ACT_SIGMOID), "hobe-mse": (O.LOSS_MSE, O.ACT_RELU)}


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.set_tuning("train_wave_pair", -1)
  c.close()


@pytest.fixture(scope="module")
def stream():
  """29 + 11 rows over 3,000 records: pending, deferred and local rows, MULTI
  batches (test_gpu_train_pair._k5_synthetic)."""
  return _k5_synthetic()


def _train_forms(ctx, idx, tgt, K, d, loss, act, batch, epochs, seed=0):
  """[one wave per record, default form] -> (node table, edge table, losses,
  step geometry, path stats, MULTI batches); same init and host permutations."""
  rs = np.random.RandomState(seed)
  nrows, erows = _rows(idx, K)
  nt = rs.uniform(-0.05, 0.05, (nrows, d)).astype(np.float32)
  et = rs.uniform(-0.05, 0.05, (erows, d)).astype(np.float32)
  perms = np.stack([rs.permutation(idx.shape[0]) for _ in range(epochs)])
  ctx.records_set(idx, tgt)
  out = []
  try:
    for pair in (0, -1):
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


def _assert_bitwise(u, p, geometry, nbatches):
  assert u[3][1] > 0 and u[3][0] == 64 * u[3][1], u[3]  # one wave per record
  assert p[3] == geometry, p[3]
  assert u[4] == p[4] == (nbatches, 0), (u[4], p[4])  # every batch took the step
  assert u[5] == p[5], (u[5], p[5])
  for t in (0, 1):
    ne = u[t] != p[t]
    assert not ne.any(), (t, int(ne.sum()), np.flatnonzero(ne.any(1))[:8],
                          float(np.abs(u[t] - p[t]).max()))
  assert np.array_equal(u[2], p[2]), (u[2], p[2])


def _oracle(idx, tgt, K, init, perms, loss, act, batch):
  ont, oet, ol, _, _ = O.train(idx, tgt, K, init[0], init[1], loss, act, batch=batch,
                               max_epochs=perms.shape[0], perms=perms, min_delta=-1.0)
  return ont, oet, ol


@pytest.mark.parametrize("heads", sorted(HEADS))
@pytest.mark.parametrize("d", [128, 72])
def test_default_form_hard_stream_bitwise_and_oracle(ctx, stream, d, heads):
  """The duplicate-heavy stream at batch 256 (ragged last batch of 184), two
  epochs: rows repeated within a record, deferred rows, pending slots (MULTI
  batches), flush slots and the overflow list. d = 72 is a padded row."""
  idx, tgt, K = stream
  loss, act = HEADS[heads]
  out, perms, init = _train_forms(ctx, idx, tgt, K, d, loss, act, 256, epochs=2)
  _assert_bitwise(out[0], out[1], QUAD1, 2 * -(-idx.shape[0] // 256))
  assert out[1][5] > 0, out[1][5]
  _check(_oracle(idx, tgt, K, init, perms, loss, act, 256), out[1][:3], init)


# (batch, records): 1 / records of a launch = 1 / batch, or 1 / tail in the
# last launch of an epoch
BATCHES = [(1, 17), (3, 3 * 13 + 1), (8, 8 * 9 + 3), (5, 5 * 7 + 3), (7, 7 * 5 + 1),
           (37, 37 * 3 + 3), (256, 2 * 256 + 37)]


@pytest.mark.parametrize("batch,n", BATCHES, ids=[f"b{b}-n{n}" for b, n in BATCHES])
@pytest.mark.parametrize("d", [128, 72])
def test_batch_sizes_and_ragged_tails_bitwise_and_oracle(ctx, stream, d, batch, n):
  """Small and ragged batches of the same stream (its first n records), three
  epochs; workgroups without a record where the tail is short."""
  idx, tgt, K = stream
  idx, tgt = np.ascontiguousarray(idx[:n]), np.ascontiguousarray(tgt[:n])
  loss, act = HEADS["hobe-mse"]
  out, perms, init = _train_forms(ctx, idx, tgt, K, d, loss, act, batch, epochs=3)
  _assert_bitwise(out[0], out[1], QUAD1, 3 * -(-n // batch))
  _check(_oracle(idx, tgt, K, init, perms, loss, act, batch), out[1][:3], init)


@pytest.mark.parametrize("n", [256, 100])
def test_one_batch_epochs_read_row0_from_the_table(ctx, stream, n):
  """Every launch is the first batch of its epoch (q = 0): the padding row
  comes from the table, no step is folded into it in the kernel, and
  train_flush applies each epoch's sums. Four epochs, so the row moves."""
  idx, tgt, K = stream
  idx, tgt = np.ascontiguousarray(idx[:n]), np.ascontiguousarray(tgt[:n])
  loss, act = HEADS["hobe-mse"]
  out, perms, init = _train_forms(ctx, idx, tgt, K, 128, loss, act, 256, epochs=4)
  _assert_bitwise(out[0], out[1], QUAD1, 4)
  assert not np.array_equal(out[1][0][0], init[0][0])  # row 0 was trained
  assert not np.array_equal(out[1][1][0], init[1][0])
  _check(_oracle(idx, tgt, K, init, perms, loss, act, 256), out[1][:3], init)


@pytest.mark.parametrize("d", [256, 200])
def test_float4_rows_default_call_unmoved(ctx, stream, d):
  """The shared helpers at float4 rows: the default (paired) form against the
  one-wave form, bit for bit, and the oracle."""
  idx, tgt, K = stream
  loss, act = HEADS["hobe-mse"]
  out, perms, init = _train_forms(ctx, idx, tgt, K, d, loss, act, 256, epochs=2)
  _assert_bitwise(out[0], out[1], PAIRED, 2 * -(-idx.shape[0] // 256))
  _check(_oracle(idx, tgt, K, init, perms, loss, act, 256), out[1][:3], init)
