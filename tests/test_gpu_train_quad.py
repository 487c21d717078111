"""GPU: the quad form of the trainer step (tuning train_wave_pair 3).

One record on four waves: each table half of the paired form on a head wave
(hub row H, other head row O, list row T0) and a list wave (T1..T4, and H's
table row to dot them with). The waves exchange their dots and the list
wave's rows through LDS across one barrier; arithmetic and its order are
those of the other forms, so tables and epoch losses are compared bit for
bit against the one-wave form (train_wave_pair 0: same records, initial
tables, host permutations), and against the CPU oracle with the bars of
test_gpu_train._check.

A half in which a list-wave slot repeats a row of its record in a run that
train_prep classes as local (the row is in no other record of the batch) is
not split: its head wave runs the paired form's 7-slot program.

The form exists at float2 rows (padded d = 128), two records per 512-thread
workgroup. The 4-record geometry (tuning value 2 while it was measured) was
slower than the paired form at both row widths and is not built; at float4
rows (d = 256, 200) the tuning selects the paired form, and the same cases
run there against the one-wave form.
"""

import numpy as np
import pytest

import oracle as O
from conftest import golden
from test_gpu_train import _check, _mixed_reuse_records, _run_both
from test_gpu_train_pair import (HEADS, _k5_synthetic,
                                 _records_naming_two_deferred, _rows, _widen5)

pytestmark = pytest.mark.gpu

ARMS = (3,)


def _geometry(arm, d):
  """(threads, records per workgroup): the quad form at float2 rows, the
  paired form at float4 rows. Two records per workgroup cannot be
  bit-identical there: the padding row's gradient is a float sum over the
  workgroup's records, over four in the other forms."""
  return (512, 2) if d <= 128 else (512, 4)


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.set_tuning("train_wave_pair", -1)
  c.close()


def _train_forms(ctx, idx, tgt, K, d, loss, act, batch, epochs, arms, seed=0,
                 rows=None):
  """One run per arm -> (node table, edge table, losses, step geometry, path
  stats, MULTI batches), same init and host permutations."""
  rs = np.random.RandomState(seed)
  nrows, erows = rows or _rows(idx, K)
  nt = rs.uniform(-0.05, 0.05, (nrows, d)).astype(np.float32)
  et = rs.uniform(-0.05, 0.05, (erows, d)).astype(np.float32)
  perms = np.stack([rs.permutation(idx.shape[0]) for _ in range(epochs)])
  ctx.records_set(idx, tgt)
  out = {}
  try:
    for arm in arms:
      ctx.set_tuning("train_wave_pair", arm)
      ctx.model_init(d, nrows, erows, node_tab=nt, edge_tab=et)
      gl = ctx.train(batch=batch, max_epochs=epochs, loss=loss, act=act,
                     perms=perms, min_delta=-1.0)
      out[arm] = ctx.model_get() + (gl, ctx.train_step_geometry(),
                                    ctx.train_path_stats(),
                                    ctx.train_multi_pending())
  finally:
    ctx.set_tuning("train_wave_pair", -1)
  return out, perms, (nt, et)


def _assert_bitwise(u, p, geometry):
  assert u[3][1] > 0 and u[3][0] == 64 * u[3][1], u[3]  # one wave per record
  assert p[3] == geometry, (p[3], geometry)
  assert u[4] == p[4] and u[5] == p[5], (u[4:], p[4:])
  for t in (0, 1):
    ne = u[t] != p[t]
    assert not ne.any(), (t, int(ne.sum()), np.flatnonzero(ne.any(1))[:8],
                          float(np.abs(u[t] - p[t]).max()))
  assert np.array_equal(u[2], p[2]), (u[2], p[2])


@pytest.mark.parametrize("batch", [256, 37, 100])
@pytest.mark.parametrize("heads", sorted(HEADS))
@pytest.mark.parametrize("d", [128, 72, 256, 200])
def test_quad_equals_one_wave_bitwise(ctx, d, heads, batch):
  """Tables and losses of 3 epochs, the quad form vs one wave per record, on
  the golden streams widened to K = 5. d = 72 and 200 are padded rows (200:
  float4 rows, where the tuning selects the paired form); batch 37 and 100
  are ragged (workgroups with fewer records than groups, wave quads with
  none)."""
  name, loss, act = HEADS[heads]
  z = golden(name)
  idx, K = _widen5(z["idx"], int(z["K"]))
  out, _, init = _train_forms(ctx, idx, z["tgt"], K, d, loss, act, batch,
                              epochs=3, arms=(0,) + ARMS)
  nb = -(-idx.shape[0] // batch)
  for arm in ARMS:
    _assert_bitwise(out[0], out[arm], _geometry(arm, d))
    assert out[arm][4] == (3 * nb, 0), out[arm][4]  # every batch took the step
    assert not np.array_equal(out[arm][0], init[0])
    assert not np.array_equal(out[arm][1], init[1])


def _half_kinds(idx, K):
  """Per table half of the list records: 1 no row repeated in the half, 2 a
  repeat spanning head-wave slots (H, O, T0) and list-wave slots (T1..), 3
  repeats in list-wave slots only, 0 anything else (a repeat inside the head
  wave's slots alone)."""
  kinds = []
  for rec in idx[(idx[:, 4:] != 0).any(1)]:
    for hub, other, t0 in ((0, 2, 4), (3, 1, 4 + K)):
      head = [rec[hub], rec[other], rec[t0]]
      lst = list(rec[t0 + 1:t0 + K])
      head = [r for r in head if r]
      lst = [r for r in lst if r]
      rep_h = len(set(head)) < len(head)
      rep_l = len(set(lst)) < len(lst)
      span = bool(set(head) & set(lst))
      kinds.append(2 if span else 3 if rep_l else 0 if rep_h else 1)
  return np.array(kinds)


@pytest.mark.parametrize("d", [128, 256])
def test_quad_hard_paths_bitwise(ctx, d):
  """29 + 11 rows under 3,584 slots per batch: rows repeated within a record,
  every row deferred, pending slots (several per record: the MULTI form),
  several flush slots per record, the overflow list, a ragged last batch."""
  idx, tgt, K = _k5_synthetic()
  # from the generator alone: all three kinds of half occur, and MULTI batches
  kinds = _half_kinds(idx, K)
  for kind in (1, 2, 3):
    assert (kinds == kind).sum() > 0, (kind, np.bincount(kinds))
  out, perms, _ = _train_forms(ctx, idx, tgt, K, d, O.LOSS_MSE, O.ACT_RELU,
                               256, epochs=2, arms=(0,) + ARMS)
  for p in perms:
    assert _records_naming_two_deferred(idx, K, p, 256) > 0
  nb = -(-idx.shape[0] // 256)
  for arm in ARMS:
    _assert_bitwise(out[0], out[arm], _geometry(arm, d))
    assert out[arm][4] == (2 * nb, 0), out[arm][4]
    assert out[arm][5] > 0, out[arm][5]


def _local_repeat_records(n=600, K=5):
  """Records over disjoint rows (record i draws from its own block of 8 node
  and 8 edge rows, so no row is in two records and every repeat within a
  record is a local run), the repeats by i % 6: none; T2 = H in the node half
  (spans the two waves); T3 = T4 in the edge half (list wave only); T0 = H in
  the node half (head wave only: split, summed there); a triple in the list
  wave's node slots and H = T0 = T4 in the edge half; a list-less record with
  Nl = Nr."""
  rs = np.random.RandomState(11)
  idx = np.zeros((n, 4 + 2 * K), np.int32)
  tgt = np.zeros((n, 3), np.float32)
  for i in range(n):
    nr = 1 + 8 * i + np.arange(8)
    er = 1 + 8 * i + np.arange(8)
    pat = i % 6
    if pat == 5:
      idx[i, 0] = idx[i, 2] = nr[0]
      tgt[i, 0] = rs.uniform(0, 1)
      continue
    idx[i, 0], idx[i, 3] = nr[0], er[0]
    idx[i, 4:4 + K] = nr[1:1 + K]
    idx[i, 4 + K:] = er[1:1 + K]
    if pat == 1:
      idx[i, 4 + 2] = nr[0]
    elif pat == 2:
      idx[i, 4 + K + 3] = idx[i, 4 + K + 4]
    elif pat == 3:
      idx[i, 4] = nr[0]
    elif pat == 4:
      idx[i, 4 + 1] = idx[i, 4 + 2] = idx[i, 4 + 3]
      idx[i, 4 + K] = idx[i, 4 + K + 4] = er[0]
    tgt[i, 2] = rs.uniform(0, 1)
  return idx, tgt, K, (8 * n + 2, 8 * n + 2)


@pytest.mark.parametrize("d", [128, 256])
def test_quad_local_rows_bitwise(ctx, d):
  """The unsplit fallback and the head wave's own local runs, taken for
  certain: rows repeated within a record and in no other record."""
  idx, tgt, K, rows = _local_repeat_records()
  kinds = _half_kinds(idx, K)
  for kind in (0, 1, 2, 3):
    assert (kinds == kind).sum() >= 100, np.bincount(kinds)
  out, _, init = _train_forms(ctx, idx, tgt, K, d, O.LOSS_MSE, O.ACT_RELU, 256,
                              epochs=2, arms=(0,) + ARMS, rows=rows)
  nb = -(-idx.shape[0] // 256)
  for arm in ARMS:
    _assert_bitwise(out[0], out[arm], _geometry(arm, d))
    assert out[arm][4] == (2 * nb, 0), out[arm][4]
    assert not np.array_equal(out[arm][0], init[0])


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("name,d,batch", [("hobe_small.npz", 128, 256),
                                          ("fobe_small_ns.npz", 128, 256),
                                          ("hobe_small.npz", 256, 256),
                                          ("fobe_small_ns.npz", 256, 100)])
def test_quad_vs_oracle(ctx, name, d, batch, arm):
  """The golden streams widened to K = 5, the oracle on the same records."""
  z = golden(name)
  loss, act = ((O.LOSS_MSE, O.ACT_RELU) if name.startswith("hobe")
               else (O.LOSS_KLD, O.ACT_SIGMOID))
  idx, K = _widen5(z["idx"], int(z["K"]))
  ctx.set_tuning("train_wave_pair", arm)
  try:
    o, g, init = _run_both(ctx, idx, z["tgt"], K, d, loss, act, batch, epochs=3)
    assert ctx.train_step_geometry() == _geometry(arm, d)
  finally:
    ctx.set_tuning("train_wave_pair", -1)
  _check(o, g, init)


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("d", [128, 256])
def test_quad_device_shuffle_twice_bitwise(ctx, d, arm):
  """The exchange of dots and rows has no race: two device-shuffled runs from
  the same init give the same bits."""
  rs = np.random.RandomState(3)
  idx, tgt = _mixed_reuse_records(rs, 20, 256, 5, hub_batches={7, 8})
  ctx.records_set(idx, tgt)
  out = []
  ctx.set_tuning("train_wave_pair", arm)
  try:
    for _ in range(2):
      ctx.model_init(d, 20002, 20002, seed=9)
      gl = ctx.train(batch=256, max_epochs=2, loss=O.LOSS_MSE, act=O.ACT_RELU,
                     shuffle_seed=5, min_delta=-1.0)
      assert ctx.train_step_geometry() == _geometry(arm, d)
      assert ctx.train_path_stats() == (40, 0)
      out.append(ctx.model_get() + (gl,))
  finally:
    ctx.set_tuning("train_wave_pair", -1)
  assert np.array_equal(out[0][2], out[1][2])
  assert np.array_equal(out[0][0], out[1][0])
  assert np.array_equal(out[0][1], out[1][1])
