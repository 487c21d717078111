"""GPU: the trainer's chunk loop with and without the per-chunk host wait.

A merged form of the trainer step is one kernel (the second fold pass and the
slot-by-slot remainder are a wave-uniform runtime branch), so inside an epoch
the driver reads nothing from the device: chunk c + 1's preparation is queued
directly behind chunk c's launches. The paired form at float4 rows (d = 256,
200) is merged; the quad form (d = 128, 72) keeps its light kernel and the
flag path, where the merged kernel measured slower. Either way the MULTI
batches are counted by train_place on the device.

The stream: the duplicate-heavy K = 5 generator (29 + 11 rows) drawn to 8,243
records and trained at batch 8: 1,031 batches in two chunks (1,024 + 7) with
a ragged last batch of 3, so pending and deferred rows, flush slots and MULTI
batches cross the chunk edge and the epoch tail follows a 7-batch chunk. The
one-wave form (train_wave_pair 0) keeps its two kernels and its per-chunk
host wait: it is the reference for the bits and for the MULTI count.
"""

import numpy as np
import pytest

import oracle as O
from conftest import golden
from test_gpu_train import _check
from test_gpu_train_pair import (HEADS, _k5_synthetic, _records_naming_two_deferred,
                                 _rows, _widen5)
from test_gpu_train_quad import (_assert_bitwise, _half_kinds, _local_repeat_records,
                                 _train_forms)

pytestmark = pytest.mark.gpu

BATCH, NREC = 8, 8243
NB = -(-NREC // BATCH)


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.set_tuning("train_wave_pair", -1)
  c.close()


@pytest.fixture(scope="module")
def stream():
  idx, tgt, K = _k5_synthetic()
  sel = np.random.RandomState(21).randint(0, idx.shape[0], NREC)
  return np.ascontiguousarray(idx[sel]), np.ascontiguousarray(tgt[sel]), K


def test_stream_shape(stream):
  assert NB == 1031 and NB > 1024 and NREC % BATCH == 3


@pytest.mark.parametrize("heads", sorted(HEADS))
@pytest.mark.parametrize("d", [128, 72, 256, 200])
def test_chunk_edge_bitwise_and_multi_count(ctx, stream, d, heads):
  """One epoch over two chunks, the default form (quad at float2 rows, one
  record per workgroup; paired at float4 rows) against one wave per record: tables and losses bit for
  bit, the same MULTI count, strictly between 0 and the batch count; and the
  oracle on the same records and order with the bars of _check."""
  idx, tgt, K = stream
  _, loss, act = HEADS[heads]
  out, perms, init = _train_forms(ctx, idx, tgt, K, d, loss, act, BATCH, epochs=1,
                                  arms=(0, -1))
  u, p = out[0], out[-1]
  print("geometry", u[3], p[3], "multi", u[5], p[5], "of", NB)
  assert p[3][0] > 64 * p[3][1], p[3]  # more than one wave per record
  _assert_bitwise(u, p, p[3])
  assert u[4] == p[4] == (NB, 0), (u[4], p[4])
  assert u[5] == p[5] and 0 < p[5] < NB, (u[5], p[5], NB)
  ont, oet, ol, _, _ = O.train(idx, tgt, K, init[0], init[1], loss, act, batch=BATCH,
                               max_epochs=1, perms=perms, min_delta=-1.0)
  _check((ont, oet, ol), p[:3], init)


@pytest.mark.parametrize("d", [128, 256])
def test_two_epochs_device_shuffle_twice_bitwise(ctx, stream, d):
  """The epoch tail and train_flush with no per-chunk wait: two epochs in one
  call on the device shuffle, twice from the same init, the same bits and
  the same counters."""
  idx, tgt, K = stream
  ctx.records_set(idx, tgt)
  nrows, erows = _rows(idx, K)
  out = []
  for _ in range(2):
    ctx.model_init(d, nrows, erows, seed=9)
    gl = ctx.train(batch=BATCH, max_epochs=2, loss=O.LOSS_MSE, act=O.ACT_RELU,
                   shuffle_seed=5, min_delta=-1.0)
    assert len(gl) == 2
    assert ctx.train_path_stats() == (2 * NB, 0)
    out.append(ctx.model_get() + (gl, ctx.train_multi_pending()))
  assert 0 < out[0][3] < 2 * NB, out[0][3]
  assert out[0][3] == out[1][3]
  assert np.array_equal(out[0][2], out[1][2])
  assert np.array_equal(out[0][0], out[1][0])
  assert np.array_equal(out[0][1], out[1][1])


# ---- the quad form at one record per 256-thread workgroup (train_wave_pair 4)

ARM4 = (256, 1)


@pytest.mark.parametrize("batch", [256, 37])
@pytest.mark.parametrize("heads", sorted(HEADS))
@pytest.mark.parametrize("d", [128, 72])
def test_arm4_equals_one_wave_bitwise(ctx, d, heads, batch):
  """test_quad_equals_one_wave_bitwise with one record per workgroup."""
  name, loss, act = HEADS[heads]
  z = golden(name)
  idx, K = _widen5(z["idx"], int(z["K"]))
  out, _, init = _train_forms(ctx, idx, z["tgt"], K, d, loss, act, batch, epochs=3,
                              arms=(0, 4))
  nb = -(-idx.shape[0] // batch)
  _assert_bitwise(out[0], out[4], ARM4)
  assert out[4][4] == (3 * nb, 0), out[4][4]
  assert not np.array_equal(out[4][0], init[0])
  assert not np.array_equal(out[4][1], init[1])


@pytest.mark.parametrize("batch", [256, 37])
@pytest.mark.parametrize("d", [128, 72])
def test_arm4_hard_paths_bitwise(ctx, d, batch):
  """test_quad_hard_paths_bitwise with one record per workgroup."""
  idx, tgt, K = _k5_synthetic()
  out, perms, _ = _train_forms(ctx, idx, tgt, K, d, O.LOSS_MSE, O.ACT_RELU, batch,
                               epochs=2, arms=(0, 4))
  for p in perms:
    assert _records_naming_two_deferred(idx, K, p, batch) > 0
  nb = -(-idx.shape[0] // batch)
  _assert_bitwise(out[0], out[4], ARM4)
  assert out[4][4] == (2 * nb, 0), out[4][4]
  assert out[4][5] > 0, out[4][5]


@pytest.mark.parametrize("batch", [256, 37])
@pytest.mark.parametrize("d", [128, 72])
def test_arm4_local_rows_bitwise(ctx, d, batch):
  """test_quad_local_rows_bitwise with one record per workgroup."""
  idx, tgt, K, rows = _local_repeat_records()
  kinds = _half_kinds(idx, K)
  for kind in (0, 1, 2, 3):
    assert (kinds == kind).sum() >= 100, np.bincount(kinds)
  out, _, init = _train_forms(ctx, idx, tgt, K, d, O.LOSS_MSE, O.ACT_RELU, batch,
                              epochs=2, arms=(0, 4), rows=rows)
  nb = -(-idx.shape[0] // batch)
  _assert_bitwise(out[0], out[4], ARM4)
  assert out[4][4] == (2 * nb, 0), out[4][4]
  assert not np.array_equal(out[4][0], init[0])
