"""The trainer restatement (oracle/hgref.c hgref_train, both duplicate-row
summation orders, and its multithreaded twin cpu_train_mt.c) against an
independent float64 autograd formulation of the same Keras models
(tests/hg2v_autograd.py): 3 batches (the last ragged), 2 epochs.

Three Adagrad settings. Keras' defaults (0.01, 1e-7) make the step
lr g / sqrt(sum g^2): a constant factor on every gradient cancels. (1, 10)
makes the step proportional to the gradient. lr = 0.01 with eps of the size
of sqrt(a) shows both the gradient's scale and the accumulator.

Bar: table error <= 1e-6 of the table's largest single Adagrad step plus
2 ulp32 of the largest |p| (the float32 parameter rounding, which dominates
where the steps are small); epoch losses <= 1e-6 relative.

Sensitivity: the reference with each of three deliberate mistakes (every
gradient x 2; 1 / batch on the ragged last batch; the ne head's backward
pass without 1 / K) is > 100 x the bar away from hgref_train at (1, 10),
and the x 2 variant is inside the bar at (0.01, 1e-7): the gap the default
setting leaves.
"""

import numpy as np
import pytest

import hg2v_autograd as A
import oracle as O

MODELS = {"boolean": (O.LOSS_KLD, O.ACT_SIGMOID),
          "float": (O.LOSS_MSE, O.ACT_RELU)}
K, BATCH, N_REC, ROWS, EPOCHS = 5, 32, 75, 24, 2


def _case(model, d, seed=1, no_cancel=False, rows=ROWS):
  """24-row tables, 75 records in three in-order batches of 32, 32 and 11.
  Three things keep the float32 floor of a CORRECT trainer under the bar,
  by construction and not by looking at the oracle:
  - duplicate-row sums: a sequential float32 sum of m terms is off by about
    sqrt(m) 2^-24 of the sum; the padding row collects ~11 slots per record,
    ~350 at 32 records: 1.1e-6, the bar's relative term (at 256 records the
    emit-order sum alone is 3e-6 off, the float64-summed variant is not);
  - parameter rounding: every Adagrad step rounds p once (<= 0.5 ulp), so a
    row may be updated at most four times for 2 ulp: batch b names no row
    with r % 3 == b % 3 (two updates per epoch), and the padding row, which
    every batch updates, is scaled into the binade below (6 x 0.25 ulp);
  - no_cancel (the eps = 1e-7 setting): there a gradient element that nearly
    cancels over the batch (|g| ~ eps) turns an absolute float32 rounding
    error dg into a step error lr dg / eps = 1e5 dg, so the inputs keep
    every contribution to an element of one sign: sigmoid + KLD has dz < 0
    throughout, so all rows share the sign s = +1; relu + MSE keeps both
    signs (opposite-sign pairs are inactive) with every active output above
    its target (|u|^2 = 3 + 0.03 d against nn / ee targets <= 1, ne targets
    <= 0.05 below the smallest non-zero P Q ~ 0.08), so dz > 0 throughout."""
  loss, act = MODELS[model]
  rs = np.random.RandomState(seed)
  kw = dict(thirds_batch=BATCH)
  if not no_cancel:
    nt, et = A.signed_tables(rs, rows, rows, d, A.amp_for(loss, act, d),
                             row0=0.45)
  elif act == O.ACT_SIGMOID:
    nt, et = A.signed_tables(rs, rows, rows, d, np.sqrt(1.5 / d),
                             both_signs=False, row0=0.45)
  else:
    nt, et = A.signed_tables(rs, rows, rows, d, np.sqrt((3 + 0.03 * d) / d),
                             row0=0.45)
    kw["ne_tgt"] = (0.01, 0.05)
  idx, tgt = A.random_records(rs, N_REC, K, rows, rows, **kw)
  return idx, tgt, nt, et, loss, act


def _settings(idx, tgt, nt, et, loss, act, batch=BATCH, k=K):
  e3, med = A.mid_eps(idx, tgt, k, nt, et, loss, act, batch)
  # the third setting's condition: eps within a factor of 10 of the median
  # sqrt(a) over touched elements after batch 1
  assert med / 10 <= e3 <= med * 10, (e3, med)
  return {"keras": (0.01, 1e-7), "prop": (1.0, 10.0), "mid": (0.01, e3)}


def _bar(ref, init, t):
  p = (ref.nt, ref.et)[t]
  return 1e-6 * ref.max_step[t] + 2 * A.ulp32(np.abs(p).max())


def _oracles(idx, tgt, k, nt, et, loss, act, batch, lr, eps, epochs):
  kw = dict(batch=batch, lr=lr, eps=eps)
  perms = np.tile(np.arange(idx.shape[0]), (epochs, 1))
  out = {}
  for name, f64 in (("fp32-order", False), ("f64-dups", True)):
    o = O.train(idx, tgt, k, nt, et, loss, act, max_epochs=epochs, perms=perms,
                min_delta=-1.0, dup_f64=f64, **kw)
    out[name] = (o[0], o[1], o[2].astype(np.float64))
  m = O.train_mt(idx, tgt, k, nt, et, loss, act, epochs=epochs, exact=True,
                 threads=2, **kw)
  out["mt"] = (m[0], m[1], m[2])  # the mean of the epoch losses
  return out


def _assert_within(out, ref, init, tag):
  for name, (ont, oet, ol) in out.items():
    for t, (o, r) in enumerate(((ont, ref.nt), (oet, ref.et))):
      err = np.abs(o.astype(np.float64) - r).max()
      bar = _bar(ref, init, t)
      print(f"{tag} {name} table {t}: err {err:.3g} bar {bar:.3g} "
            f"(step {ref.max_step[t]:.3g})")
      assert err <= bar, (tag, name, t, err, bar)
    want = ref.losses.mean() if name == "mt" else ref.losses
    assert np.allclose(ol, want, rtol=1e-6, atol=0), (tag, name, ol, want)


@pytest.mark.parametrize("d", [8, 128])
@pytest.mark.parametrize("setting", ["keras", "prop", "mid"])
@pytest.mark.parametrize("model", list(MODELS))
def test_oracle_vs_autograd(model, setting, d):
  idx, tgt, nt, et, loss, act = _case(model, d, no_cancel=setting == "keras")
  lr, eps = _settings(idx, tgt, nt, et, loss, act)[setting]
  ref = A.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, lr=lr, eps=eps,
                epochs=EPOCHS)
  if act == O.ACT_RELU:
    assert A.relu_margin(ref, d) >= 1.0
  assert len(ref.losses) == EPOCHS
  out = _oracles(idx, tgt, K, nt, et, loss, act, BATCH, lr, eps, EPOCHS)
  _assert_within(out, ref, (nt, et), f"{model} {setting} d={d}")


@pytest.mark.parametrize("model", list(MODELS))
def test_oracle_vs_autograd_shuffled_epochs(model):
  """Per-epoch permutations (hgref_train only: the multithreaded twin takes
  the records in order)."""
  idx, tgt, nt, et, loss, act = _case(model, 16, seed=2)
  rs = np.random.RandomState(5)
  # whole batches change places and their records are shuffled (the row
  # thirds of _case stay together); the ragged batch stays last
  blocks = [np.arange(0, BATCH), np.arange(BATCH, 2 * BATCH),
            np.arange(2 * BATCH, N_REC)]
  perms = np.stack([np.concatenate([rs.permutation(blocks[b]) for b in o])
                    for o in ((1, 0, 2), (0, 1, 2))])
  ref = A.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, lr=1.0, eps=10.0,
                epochs=EPOCHS, perms=perms)
  if act == O.ACT_RELU:
    assert A.relu_margin(ref, 16) >= 1.0
  o = O.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, lr=1.0, eps=10.0,
              max_epochs=EPOCHS, perms=perms, min_delta=-1.0)
  _assert_within({"fp32-order": (o[0], o[1], o[2].astype(np.float64))}, ref,
                 (nt, et), f"{model} shuffled")


@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("setting", ["keras", "prop"])
@pytest.mark.parametrize("pair", [(0, 0), (1, 1), (0, 1), (1, 0)],
                         ids=["kld-sig", "mse-relu", "kld-relu", "mse-sig"])
def test_oracle_edge_records_vs_autograd(pair, setting, d):
  """The constructed batch (hg2v_autograd.edge_batch): exact relu kinks,
  clipped KLD heads, saturated sigmoids, repeated and self neighbours."""
  loss, act = pair
  idx, tgt, nt, et = A.edge_batch(np.random.RandomState(3), d, K, loss, act)
  lr, eps = {"keras": (0.01, 1e-7), "prop": (1.0, 10.0)}[setting]
  ref = A.train(idx, tgt, K, nt, et, loss, act, batch=256, lr=lr, eps=eps)
  if act == O.ACT_RELU:
    z = np.concatenate(ref.relu_z)
    assert (z == 0.0).sum() >= 2 + 2 * K and (z == 2.0 ** -20).sum() == 2
    assert A.relu_margin(ref, d) >= 1.0
  out = _oracles(idx, tgt, K, nt, et, loss, act, 256, lr, eps, 1)
  _assert_within(out, ref, (nt, et), f"edge {pair} {setting} d={d}")
  if loss == O.LOSS_KLD and act == O.ACT_SIGMOID:
    # the clipped heads: sigmoid(-20) < 1e-7 -> loss yt log(yt / 1e-7), no
    # gradient through the nn head (rows 14, 15 move only through the ne
    # head's padding slots, as in the reference)
    one = A.train(idx[8:9], tgt[8:9], K, nt, et, loss, act, batch=1)
    yt = np.float64(np.float32(0.7))
    clip = yt * np.log(yt / A.KEPS)
    # (+ the inactive heads' terms 1e-7 log(1e-7 / y), a few 1e-6 below 0)
    assert abs(one.losses[0] - clip) < 1e-5
    o1 = O.train(idx[8:9], tgt[8:9], K, nt, et, loss, act, batch=1,
                 max_epochs=1)
    assert np.isclose(o1[2][0], one.losses[0], rtol=1e-6)


BUG_CASES = [(m, b) for m in MODELS for b in A.BUGS]


@pytest.mark.parametrize("model,bug", BUG_CASES)
def test_sensitivity_proportional_setting_sees_each_mistake(model, bug):
  idx, tgt, nt, et, loss, act = _case(model, 8)
  ref = A.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, lr=1.0, eps=10.0,
                epochs=EPOCHS)
  bad = A.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, lr=1.0, eps=10.0,
                epochs=EPOCHS, bug=bug)
  o = O.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, lr=1.0, eps=10.0,
              max_epochs=EPOCHS, perms=np.tile(np.arange(N_REC), (EPOCHS, 1)),
              min_delta=-1.0)
  worst = 0.0
  for t, (ot, bt) in enumerate(((o[0], bad.nt), (o[1], bad.et))):
    worst = max(worst, np.abs(ot - bt).max() / _bar(ref, (nt, et), t))
  print(f"{model} {bug}: {worst:.3g} x the bar")
  assert worst > 100.0, (model, bug, worst)


@pytest.mark.parametrize("model", list(MODELS))
def test_sensitivity_default_setting_hides_gradient_scale(model):
  """At Keras' defaults a trainer whose every gradient is doubled is inside
  the bar: what the other two settings are for. (Doubling g moves the step
  lr g / (|g| + eps) by lr eps / 2|g|, under the bar where |g| >~ 4e-3: seven
  rows, so that every row collects about thirty records' gradients, and
  d = 2, where the elements are largest.)"""
  idx, tgt, nt, et, loss, act = _case(model, 2, no_cancel=True, rows=7)
  ref = A.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, epochs=EPOCHS)
  bad = A.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, epochs=EPOCHS,
                bug="grad_x2")
  o = O.train(idx, tgt, K, nt, et, loss, act, batch=BATCH, max_epochs=EPOCHS,
              perms=np.tile(np.arange(N_REC), (EPOCHS, 1)), min_delta=-1.0)
  for t, (ot, bt) in enumerate(((o[0], bad.nt), (o[1], bad.et))):
    assert np.abs(ot - bt).max() <= _bar(ref, (nt, et), t)
