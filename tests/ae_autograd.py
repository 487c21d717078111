"""Float64 autograd reference of the auto-encoder baseline (torch, CPU).

Written from the reference's model definition (auto_encoder.py:20-84) and
Keras' formulas:

  x (C) -> Dense(d, relu) [W1 C x d, b1] -> Dense(C, softmax) [W2 d x C, b2];
  a sample (row, drop) of a row with support S, n = |S|: target y = 1_S / n,
  input x = y (drop = -1) or 1_{S \\ drop} / (n - 1), both float32 values as
  Keras is fed them;
  kullback_leibler_divergence: sum_c yt' log(yt' / yp') with clip(., 1e-7, 1)
  on both, batch mean;
  Adagrad (Keras 2.x): a += g^2; p -= lr g / (sqrt(a) + eps), a0 = 0;
  gradients by torch.autograd.grad.

Batches are explicit (row, drop) lists. A helper module for the tests, not a
conftest; it takes nothing from the package under test.
"""

import numpy as np
import torch

# Keras' epsilon as its float32 graph sees it
KEPS = float(np.float32(1e-7))


class Result:
  """Weights and accumulators (float64, order W1, b1, W2, b2), batch losses,
  the accumulators after the first batch, and per batch the relu
  pre-activations z with sum |terms| and the term count of each."""

  def __init__(self):
    self.w = self.a = self.acc1 = None
    self.losses = []
    self.relu_z, self.relu_s, self.relu_n = [], [], []


def dense_batch(rp, col, C, row, drop):
  """X (inputs) and Y (targets), M x C float64 holding the float32 values."""
  M = len(row)
  X, Y = np.zeros((M, C), np.float32), np.zeros((M, C), np.float32)
  for m, (r, dr) in enumerate(zip(row, drop)):
    cs = col[rp[r]:rp[r + 1]]
    Y[m, cs] = np.float32(1.0 / cs.size)
    if dr >= 0:
      assert cs.size > 1 and dr in cs
      X[m, cs] = np.float32(1.0 / (cs.size - 1))
      X[m, dr] = 0
    else:
      X[m] = Y[m]
  return X.astype(np.float64), Y.astype(np.float64)


def forward(w, X):
  H = torch.relu(X @ w[0] + w[1])
  return H, torch.softmax(H @ w[2] + w[3], dim=1)


def kld(Y, P):
  yc, pc = torch.clamp(Y, KEPS, 1.0), torch.clamp(P, KEPS, 1.0)
  return (yc * torch.log(yc / pc)).sum(1)


def train(rp, col, C, weights, batches, lr=0.01, eps=1e-7):
  """One Adagrad step per (row, drop) batch, in order."""
  w = [torch.tensor(np.asarray(p, np.float64)) for p in weights]
  a = [torch.zeros_like(p) for p in w]
  res = Result()
  for row, drop in batches:
    X, Y = (torch.tensor(t) for t in dense_batch(rp, col, C, row, drop))
    for p in w:
      p.requires_grad_(True)
    H, P = forward(w, X)
    loss = kld(Y, P).mean()
    g = torch.autograd.grad(loss, w)
    with torch.no_grad():
      res.relu_z.append((X @ w[0] + w[1]).numpy().copy())
      res.relu_s.append((X @ w[0].abs() + w[1].abs()).numpy().copy())
      res.relu_n.append(np.repeat((X.numpy() != 0).sum(1) + 1,
                                  w[1].numel()).reshape(len(row), -1))
      for p, acc, gp in zip(w, a, g):
        acc += gp * gp
        p -= lr * gp / (torch.sqrt(acc) + eps)
    for p in w:
      p.requires_grad_(False)
    res.losses.append(float(loss.detach()))
    if res.acc1 is None:
      res.acc1 = [t.numpy().copy() for t in a]
  res.w = [p.numpy().copy() for p in w]
  res.a = [t.numpy().copy() for t in a]
  res.losses = np.array(res.losses)
  return res


def encode(rp, col, C, weights, rows):
  """relu(1_S / n . W1 + b1) of the listed rows, float64."""
  w = [torch.tensor(np.asarray(p, np.float64)) for p in weights]
  X, _ = dense_batch(rp, col, C, rows, [-1] * len(rows))
  return torch.relu(torch.tensor(X) @ w[0] + w[1]).numpy()


def relu_margin(res):
  """min over every relu pre-activation the reference saw of
  |z| / (16 deg 2^-24 sum |terms|), deg = the number of terms (the input's
  columns and the bias); z == 0 with sum |terms| == 0 is exact by
  construction and excluded. >= 1 is the input condition."""
  worst = np.inf
  for z, s, n in zip(res.relu_z, res.relu_s, res.relu_n):
    lim = 16.0 * n * 2.0 ** -24 * s
    m = lim > 0
    assert (z[~m] == 0).all()
    if m.any():
      worst = min(worst, float((np.abs(z[m]) / lim[m]).min()))
  return worst


def mid_eps(rp, col, C, weights, batches):
  """An Adagrad epsilon of the size of sqrt(a) after the first batch (the
  power of ten nearest the median over touched elements), with that median."""
  r = train(rp, col, C, weights, batches[:1])
  a = np.concatenate([t.ravel() for t in r.acc1])
  med = float(np.median(np.sqrt(a[a > 0])))
  return float(10.0 ** np.round(np.log10(med))), med


def ulp32(x):
  return float(np.spacing(np.float32(abs(x))))
