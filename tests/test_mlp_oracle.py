"""The MLP restatement (oracle/mlpref.c) against an independent float64
autograd formulation of the same Keras models (torch on the CPU): forward
values, the gradient of the Keras loss (sum over outputs of the weighted
batch mean of the per-sample mean squared error) and the Adagrad step.
A large Adagrad epsilon makes the step proportional to the gradient, so a
wrong gradient scale shows (with eps = 1e-7 Adagrad's first step is
lr * sign(g)). The dropout masks are the shared counter-based ones."""

import numpy as np
import pytest

import mlp_autograd as A
import oracle as O
from mlp_autograd import shapes_of
from mlp_cases import mix64, rand64  # noqa: F401 (their home is mlp_cases)


def torch_step(kind, I, D, flat, nt, et, nr, er, lab, seed, lr, eps):
  """One Keras batch in float64 autograd; returns (new flat weights, loss)."""
  r = A.fit(kind, I, D, flat, nt, et, nr, er, lab, np.arange(len(nr))[None, :],
            batch=len(nr), lr=lr, eps=eps, seed=seed)
  return r.w, float(r.losses[0])


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_one_batch_matches_autograd(kind):
  I, D, M = 12, 6, 40
  rng = np.random.default_rng(kind)
  shapes = shapes_of(kind, I, D)
  flat = np.concatenate([np.concatenate([
      rng.uniform(-1, 1, k * n) * np.sqrt(6 / (k + n)),
      rng.normal(0, 0.2, n)]) for k, n in shapes]).astype(np.float32)
  assert flat.size == O.mlp_num_weights(kind, I, D)
  nt = rng.random((30, I)).astype(np.float32)
  et = rng.random((20, I)).astype(np.float32)
  nr = rng.integers(0, 30, M).astype(np.int32)
  er = rng.integers(0, 20, M).astype(np.int32)
  lab = (rng.random(M) < 0.4).astype(np.float32)
  # lr 1, eps 10: the step ~ g/10 is far above the f32 spacing of w
  seed, lr, eps = 1234, 1.0, 10.0
  w, losses = O.mlp_fit(kind, I, D, flat, nt, et, nr, er, lab,
                        np.arange(M)[None, :], batch=M, lr=lr, eps=eps,
                        seed=seed)
  ref, ref_loss = torch_step(kind, I, D, flat.astype(np.float64), nt, et, nr, er,
                             lab, seed, lr, eps)
  assert abs(losses[0] - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
  step_ref = ref - flat
  step = w - flat
  # the step is ~lr*g/eps: compare it relative to its own scale
  assert np.abs(step - step_ref).max() <= 1e-3 * np.abs(step_ref).max()
  assert np.abs(step_ref).max() > 0


def test_early_stopping_and_epoch_loss():
  """EarlyStopping(monitor=loss, min_delta, patience=0): stops at the first
  epoch that does not improve the best loss by more than min_delta."""
  kind, I, D, n = 0, 8, 0, 600
  rng = np.random.default_rng(7)
  shapes = shapes_of(kind, I, D)
  flat = np.concatenate([np.concatenate([
      rng.uniform(-1, 1, k * n_) * np.sqrt(6 / (k + n_)), np.zeros(n_)])
      for k, n_ in shapes]).astype(np.float32)
  nt = rng.random((40, I)).astype(np.float32)
  et = rng.random((25, I)).astype(np.float32)
  nr = rng.integers(0, 40, n).astype(np.int32)
  er = rng.integers(0, 25, n).astype(np.int32)
  lab = (rng.random(n) < 0.5).astype(np.float32)
  perms = np.stack([rng.permutation(n) for _ in range(30)])
  _, l_all = O.mlp_fit(kind, I, 0, flat, nt, et, nr, er, lab, perms,
                       min_delta=-1e30)
  assert len(l_all) == 30
  _, l_stop = O.mlp_fit(kind, I, 0, flat, nt, et, nr, er, lab, perms,
                        min_delta=1e-3)
  k = len(l_stop)
  np.testing.assert_array_equal(l_stop, l_all[:k])
  best = np.minimum.accumulate(l_all)
  # every epoch before the stop improved on the best by more than 1e-3
  for e in range(1, k - 1):
    assert l_all[e] + 1e-3 < best[e - 1]
  if k < 30:
    assert not l_all[k - 1] + 1e-3 < best[k - 2]
