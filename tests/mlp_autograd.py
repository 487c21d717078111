"""A float64 (on request float32) autograd fit of the three Keras models of
the dense MLP engine (torch on the CPU): the reference of test_mlp_oracle.py
and test_mlp_cases_cpu.py. A helper module, not a conftest.

Independent of oracle/mlpref.c and of the device: plain matrix products, the
gradient from autograd, Adagrad written once (a += g^2; p -= lr g / (sqrt(a)
+ eps), accumulators from zero). Shared with both are only the statement of
the model (evaluation_util.py:471-505, combine_embeddings_util.py:80-174) and
the counter-based dropout bits: keep = bit (k & 63) of rand64(seed, stream,
p w64 + (k >> 6)) with p the sample's position in the epoch's order, w64 =
ceil(ru(I, 4) / 64) and stream = 0x44000000 + 4 ep (+ 1 on the edge side).

Flat weights: per layer in Keras creation order, the kernel (K x N, row
major) then the bias (N)."""

import numpy as np
import torch

from mlp_cases import rand64


def ulp32(x):
  return float(np.spacing(np.float32(abs(x))))


def shapes_of(kind, I, D):
  if kind == 0:
    return [(2 * I, I), (I, 1)]
  H = (I + D) // 2
  s = [(I, H), (I, H), (H, D), (H, D)]
  if kind == 2:
    s += [(D, H), (D, H), (H, I), (H, I)]
  return s + [(2 * D, D), (D, 1)]


def layer_names(kind):
  if kind == 0:
    return ["pre", "label"]
  n = ["pre_n", "pre_e", "joint_n", "joint_e"]
  if kind == 2:
    n += ["post_n", "post_e", "rec_n", "rec_e"]
  return n + ["hidden", "label"]


def layer_slices(kind, I, D):
  """(name, slice of the flat vector) per layer, kernel and bias together."""
  out, off = [], 0
  for name, (k, n) in zip(layer_names(kind), shapes_of(kind, I, D)):
    out.append((name, slice(off, off + k * n + n)))
    off += k * n + n
  return out


def drop_mask(seed, stream, p0, M, width):
  """[M x width] of 2.0 (kept) / 0.0 (dropped) for epoch positions p0 ..
  p0 + M - 1."""
  w64 = ((width + 3) // 4 * 4 + 63) // 64
  mask = np.zeros((M, width), np.float64)
  for m in range(M):
    for j in range(w64):
      r = rand64(seed, stream, (p0 + m) * w64 + j)
      ks = np.arange(64 * j, min(width, 64 * j + 64))
      bits = np.array([(r >> int(k & 63)) & 1 for k in ks], np.float64)
      mask[m, ks] = 2.0 * bits
  return mask


def unflatten(kind, I, D, flat, dtype, grad=False):
  params, off = [], 0
  for k, n in shapes_of(kind, I, D):
    W = torch.tensor(np.asarray(flat[off:off + k * n], np.float64).reshape(k, n),
                     dtype=dtype, requires_grad=grad)
    off += k * n
    b = torch.tensor(np.asarray(flat[off:off + n], np.float64), dtype=dtype,
                     requires_grad=grad)
    off += n
    params += [W, b]
  assert off == len(flat)
  return params


def flatten(params):
  return np.concatenate([p.detach().numpy().astype(np.float64).ravel()
                         for p in params])


def model(kind, params, xn, xe, mn=None, me=None, pre=None):
  """The forward pass. mn / me: dropout masks (training) or None. Returns
  (label output y [M], joint_n, joint_e, rec_n, rec_e); the pre-activation
  of every relu layer is appended to ``pre`` as (layer name, z)."""
  names = layer_names(kind)

  def dense(x, q, act):
    z = x @ params[2 * q] + params[2 * q + 1]
    if act is torch.relu and pre is not None:
      pre.append((names[q], z.detach().numpy().astype(np.float64)))
    return act(z)

  relu, sig = torch.relu, torch.sigmoid
  if kind == 0:
    h = dense(torch.cat([xn, xe], 1), 0, relu)
    return dense(h, 1, sig)[:, 0], None, None, None, None
  dn = xn if mn is None else xn * mn
  de = xe if me is None else xe * me
  jn = dense(dense(dn, 0, relu), 2, sig)
  je = dense(dense(de, 1, relu), 3, sig)
  q = 4 if kind == 1 else 8
  y = dense(dense(torch.cat([jn, je], 1), q, relu), q + 1, sig)[:, 0]
  rn = re = None
  if kind == 2:  # creation order: post_n 4, post_e 5, rec_n 6, rec_e 7
    rn = dense(dense(jn, 4, relu), 6, relu)
    re = dense(dense(je, 5, relu), 7, relu)
  return y, jn, je, rn, re


class Run:
  """w: flat weights after training (float64 array); acc: the Adagrad
  accumulators in the same layout; losses: per epoch; batch_losses: per
  batch; pre: per batch, the (name, z) list of model(); acc1: the
  accumulators after the first batch."""


def fit(kind, I, D, flat, nt, et, nr, er, lab, perms, batch=256, lr=0.01,
        eps=1e-7, seed=0, dtype=torch.float64, max_batches=0):
  """Keras fit: per epoch the batches perms[ep][b0:b0 + batch]; the loss is
  the sum over outputs of the weighted batch mean of the per-sample mean
  squared error (weights 1, or [4, 1, 1] for kind 2); the epoch loss is the
  batch-size-weighted mean of the batch losses."""
  params = unflatten(kind, I, D, flat, dtype, grad=True)
  acc = [torch.zeros_like(p) for p in params]
  T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
  mse = lambda y, t: ((y - t) ** 2).mean(dim=-1).mean()
  perms = np.asarray(perms)
  n = perms.shape[1]
  r = Run()
  r.losses, r.batch_losses, r.pre, r.acc1 = [], [], [], None
  done = 0
  for ep in range(perms.shape[0]):
    stream = 0x44000000 + 4 * ep
    tot = 0.0
    for b0 in range(0, n, batch):
      s = perms[ep][b0:b0 + batch]
      M = len(s)
      xn, xe, t = T(nt[nr[s]]), T(et[er[s]]), T(lab[s])
      mn = me = None
      if kind != 0:
        mn = T(drop_mask(seed, stream, b0, M, I))
        me = T(drop_mask(seed, stream + 1, b0, M, I))
      pre = []
      y, _, _, rn, re = model(kind, params, xn, xe, mn, me, pre)
      loss = mse(y[:, None], t[:, None])
      if kind == 2:
        loss = 4 * loss + mse(rn, xn) + mse(re, xe)
      grads = torch.autograd.grad(loss, params)
      with torch.no_grad():
        for p, a, g in zip(params, acc, grads):
          a += g * g
          p -= lr * g / (torch.sqrt(a) + eps)
      r.pre.append(pre)
      r.batch_losses.append(float(loss.detach()))
      tot += r.batch_losses[-1] * M
      done += 1
      if r.acc1 is None:
        r.acc1 = flatten(acc)
      if max_batches and done >= max_batches:
        break
    r.losses.append(tot / n)
    if max_batches and done >= max_batches:
      break
  r.w, r.acc = flatten(params), flatten(acc)
  r.losses = np.array(r.losses)
  return r


def predict(kind, I, D, flat, nt, et, output, nr=None, er=None,
            dtype=torch.float64):
  """Inference (no dropout): output 0 the label, 1 / 2 the node / edge side's
  joint embedding of the given rows."""
  params = unflatten(kind, I, D, flat, dtype)
  T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
  n = len(nr if nr is not None else er)
  xn = T(nt[nr]) if nr is not None else torch.zeros((n, I), dtype=dtype)
  xe = T(et[er]) if er is not None else torch.zeros((n, I), dtype=dtype)
  with torch.no_grad():
    y, jn, je, _, _ = model(kind, params, xn, xe)
  out = (y, jn, je)[output]
  return out.numpy().astype(np.float64)


def mid_eps(kind, I, D, flat, nt, et, nr, er, lab, perms, batch, seed):
  """An Adagrad epsilon of the size of sqrt(a) after the first batch (the
  power of ten nearest the median over touched elements), with that median:
  there the gradient's scale and the accumulator both show in the step."""
  r = fit(kind, I, D, flat, nt, et, nr, er, lab, perms, batch=batch, seed=seed,
          max_batches=1)
  a = r.acc1
  med = float(np.median(np.sqrt(a[a > 0])))
  return float(10.0 ** np.round(np.log10(med))), med


def relu_sides(run):
  """Per batch and relu layer, the boolean z > 0 array."""
  return [[(name, z > 0) for name, z in pre] for pre in run.pre]
