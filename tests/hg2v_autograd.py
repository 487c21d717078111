"""Float64 autograd reference of the hypergraph2vec trainer (torch, CPU).

Written from the reference's model definition (hg2v_model.py:51-203:
BooleanModel = sigmoid heads + KLD, UnweightedFloatModel = relu heads + MSE)
and Keras' formulas, independently of oracle/hgref.c:

  two embedding tables N, E (row 0 = the padding row, trained like any other);
  nn = act(N[ln] . N[rn]);  ee = act(E[le] . E[re]);
  ne = Average_k act(N[nn_k] . N[ln]) * Average_k act(E[ne_k] . E[re]);
  kullback_leibler_divergence: yt' log(yt' / yp') with clip(., 1e-7, 1) on both;
  mean_squared_error: (yp - yt)^2;
  model loss = sum over the three outputs of the batch mean (actual batch
  size: the last batch is ragged);
  Adagrad (Keras 2.x) on whole tables: a += g^2; p -= lr g / (sqrt(a) + eps),
  a0 = 0; gradients by torch.autograd.grad;
  epoch loss = sum of the per-record losses / n (BaseLogger).

`loss` and `act` are independent (0 = KLD / sigmoid, 1 = MSE / relu), any K
and d. A helper module for the tests, not a conftest.
"""

import numpy as np
import torch

LOSS_KLD, LOSS_MSE = 0, 1
ACT_SIGMOID, ACT_RELU = 0, 1

# Keras' epsilon as its float32 graph sees it
KEPS = float(np.float32(1e-7))

# deliberate mistakes for the sensitivity checks (keyword `bug`)
BUGS = ("grad_x2", "ragged_inv_batch", "ne_no_inv_k")


def _act(act, z):
  return torch.sigmoid(z) if act == ACT_SIGMOID else torch.relu(z)


def _head_loss(loss, y, yt):
  if loss == LOSS_KLD:
    ytc = torch.clamp(yt, KEPS, 1.0)
    ypc = torch.clamp(y, KEPS, 1.0)
    return ytc * torch.log(ytc / ypc)
  return (y - yt) ** 2


def _scale_grad(x, s):
  """x in the forward pass, s * dx in the backward pass."""
  return x.detach() + s * (x - x.detach())


class Result:
  """Tables / accumulators (float64), epoch losses, per table the largest
  single Adagrad step, the accumulators after the first batch, and for relu
  heads per batch the pre-activations z with their sum |a_i b_i|."""

  def __init__(self):
    self.nt = self.et = self.na = self.ea = None
    self.losses = None
    self.max_step = [0.0, 0.0]
    self.acc1 = None
    self.relu_z = []
    self.relu_s = []


def train(idx, tgt, K, node_tab, edge_tab, loss, act, batch=256, lr=0.01,
          eps=1e-7, epochs=1, perms=None, bug=None, max_batches=None):
  assert bug is None or bug in BUGS
  idx = np.asarray(idx, np.int64)
  n = idx.shape[0]
  assert idx.shape[1] == 4 + 2 * K
  N = torch.tensor(np.asarray(node_tab, np.float64))
  E = torch.tensor(np.asarray(edge_tab, np.float64))
  aN, aE = torch.zeros_like(N), torch.zeros_like(E)
  T = torch.tensor(np.asarray(tgt, np.float64))
  I = torch.tensor(idx)
  res = Result()
  losses, done = [], 0
  for ep in range(epochs):
    order = torch.arange(n) if perms is None else torch.tensor(
        np.asarray(perms[ep], np.int64))
    total = 0.0
    for b0 in range(0, n, batch):
      if max_batches is not None and done >= max_batches:
        break
      sel = order[b0:b0 + batch]
      r, yt = I[sel], T[sel]
      nb = r.shape[0]
      N.requires_grad_(True)
      E.requires_grad_(True)
      Nl, Nr = N[r[:, 0]], N[r[:, 2]]
      El, Er = E[r[:, 1]], E[r[:, 3]]
      Nk, Ek = N[r[:, 4:4 + K]], E[r[:, 4 + K:]]
      z1 = (Nl * Nr).sum(1)
      z2 = (El * Er).sum(1)
      za = (Nk * Nl[:, None, :]).sum(2)
      zb = (Ek * Er[:, None, :]).sum(2)
      P, Q = _act(act, za).mean(1), _act(act, zb).mean(1)
      if bug == "ne_no_inv_k":  # the backward pass loses the Average's 1/K
        P, Q = _scale_grad(P, K), _scale_grad(Q, K)
      per = (_head_loss(loss, _act(act, z1), yt[:, 0]) +
             _head_loss(loss, _act(act, z2), yt[:, 1]) +
             _head_loss(loss, P * Q, yt[:, 2]))
      denom = batch if bug == "ragged_inv_batch" else nb
      gN, gE = torch.autograd.grad(per.sum() / denom, [N, E])
      if bug == "grad_x2":
        gN, gE = 2 * gN, 2 * gE
      total += float(per.sum().detach())
      if act == ACT_RELU:
        with torch.no_grad():
          s = torch.cat([(Nl * Nr).abs().sum(1), (El * Er).abs().sum(1),
                         (Nk * Nl[:, None, :]).abs().sum(2).ravel(),
                         (Ek * Er[:, None, :]).abs().sum(2).ravel()])
          z = torch.cat([z1, z2, za.ravel(), zb.ravel()])
        res.relu_z.append(z.detach().numpy().copy())
        res.relu_s.append(s.numpy().copy())
      with torch.no_grad():
        for t, (p, a, g) in enumerate(((N, aN, gN), (E, aE, gE))):
          a += g * g
          step = lr * g / (torch.sqrt(a) + eps)
          res.max_step[t] = max(res.max_step[t], float(step.abs().max()))
          p -= step
      N.requires_grad_(False)
      E.requires_grad_(False)
      done += 1
      if done == 1:
        res.acc1 = (aN.numpy().copy(), aE.numpy().copy())
    losses.append(total / n)
  res.nt, res.et = N.numpy().copy(), E.numpy().copy()
  res.na, res.ea = aN.numpy().copy(), aE.numpy().copy()
  res.losses = np.array(losses)
  return res


def mid_eps(idx, tgt, K, node_tab, edge_tab, loss, act, batch):
  """An Adagrad epsilon of the size of sqrt(a) after the first batch (the
  power of ten nearest the median over touched elements), with that median:
  there the gradient's scale and the accumulator both show in the step."""
  r = train(idx, tgt, K, node_tab, edge_tab, loss, act, batch=batch,
            max_batches=1)
  a = np.concatenate([r.acc1[0].ravel(), r.acc1[1].ravel()])
  med = float(np.median(np.sqrt(a[a > 0])))
  return float(10.0 ** np.round(np.log10(med))), med


def ulp32(x):
  return float(np.spacing(np.float32(abs(x))))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def signed_tables(rs, nrows, erows, d, amp, noise=0.25, both_signs=True,
                  row0=1.0):
  """Rows s_r (u + noise) with s_r = +-1 and a shared direction u of
  per-element size amp: every dot product of two rows is about +-|u|^2, far
  from 0 relative to sum |a_i b_i|, with both signs present (relu heads on
  both sides, none near its kink). both_signs=False: every s_r = +1. row0
  scales the padding row."""
  out = []
  for rows in (nrows, erows):
    u = amp * rs.choice([-1.0, 1.0], d)
    s = rs.choice([-1.0, 1.0], rows) if both_signs else np.ones(rows)
    s[0] = row0
    t = s[:, None] * (u[None, :] * (1.0 + noise * rs.uniform(-1, 1, (rows, d))))
    out.append(t.astype(np.float32))
  return out


def amp_for(loss, act, d):
  """Per-element size of u. relu + MSE: at least 0.1 (0.08 for d > 512, where
  |u|^2 = 0.01 d makes the (1, 10) setting's steps as large as the
  elements), so six Adagrad steps of lr = 0.01 cannot turn an element's sign
  before the last forward pass (|u|^2 >= 0.5, grows with d); relu + KLD:
  |u|^2 = 0.5, inside the clip range; sigmoid: |u|^2 = 1.5."""
  if act == ACT_RELU:
    a = np.sqrt(0.5 / d)
    return max(a, 0.08 if d > 512 else 0.1) if loss == LOSS_MSE else a
  return np.sqrt(1.5 / d)


def random_records(rs, n, K, nrows, erows, all_three=0.15, ne_tgt=(0.3, 1.0),
                   thirds_batch=0):
  """Records of the three kinds (node-node, edge-edge, node-edge) with row 0
  in every inactive slot, plus: ln == rn / le == re, a neighbour equal to ln,
  a neighbour repeated within a list, short neighbour lists (row 0 tails),
  and records with all three targets non-zero. thirds_batch = B: the records
  of in-order batch b name only rows r with r % 3 != b % 3, so over three
  batches a row other than row 0 is updated at most twice."""
  idx = np.zeros((n, 4 + 2 * K), np.int32)
  tgt = np.zeros((n, 3), np.float32)
  kind = rs.randint(0, 3, n)
  draw = rs.randint
  for q in range(n):
    k = kind[q]
    if thirds_batch:
      skip = (q // thirds_batch) % 3

      def draw(lo, hi, size=None, skip=skip):
        ok = np.array([r for r in range(lo, hi) if r % 3 != skip])
        return ok[rs.randint(0, ok.size, size)]
    full = rs.uniform() < all_three
    if k == 0 or full:
      idx[q, 0], idx[q, 2] = draw(1, nrows, 2)
      tgt[q, 0] = rs.uniform(0.3, 1.0)
    if k == 1 or full:
      idx[q, 1], idx[q, 3] = draw(1, erows, 2)
      tgt[q, 1] = rs.uniform(0.3, 1.0)
    if k == 2 or full:
      if idx[q, 0] == 0:
        idx[q, 0] = draw(1, nrows)
      if idx[q, 3] == 0:
        idx[q, 3] = draw(1, erows)
      kn, ke = rs.randint(1, K + 1, 2)
      idx[q, 4:4 + kn] = draw(1, nrows, kn)
      idx[q, 4 + K:4 + K + ke] = draw(1, erows, ke)
      tgt[q, 2] = rs.uniform(*ne_tgt)
    e = q % 16
    if e == 3 and idx[q, 0]:
      idx[q, 2] = idx[q, 0]  # ln == rn
    if e == 5 and idx[q, 1]:
      idx[q, 3] = idx[q, 1]  # le == re
    if e == 7 and idx[q, 4]:
      idx[q, 4] = idx[q, 0]  # a neighbour equal to ln
    if e == 9 and idx[q, 4] and K > 1:
      idx[q, 5] = idx[q, 4]  # a neighbour repeated within the list
      idx[q, 4 + K + 1] = idx[q, 4 + K]
  return idx, tgt


def relu_margin(res, d):
  """min over every relu pre-activation the reference saw of
  |z| / (16 d 2^-24 sum |a_i b_i|), exact constructed values (z == 0 with
  sum == 0 terms aside, z == 2^-20) excluded; >= 1 is the input condition."""
  worst = np.inf
  for z, s in zip(res.relu_z, res.relu_s):
    exact = (z == 0.0) | (z == 2.0 ** -20)
    lim = 16.0 * d * 2.0 ** -24 * s
    m = ~exact & (lim > 0)
    if m.any():
      worst = min(worst, float((np.abs(z[m]) / lim[m]).min()))
  return worst


def edge_batch(rs, d, K, loss, act):
  """One batch of constructed records on 24-row tables (d >= 2). Rows 1-4
  have sign +, 5-7 sign -, rows 8-17 are built per case and appear in no
  other record, so every constructed pre-activation holds exactly:
    rows 10, 11: disjoint support -> z == 0 in every summation order (nn / ee
                 head, and all K slots of an ne list: P == 0, dQ == 0);
    rows 12, 13: 2^-10 e_0 each -> z == 2^-20 exactly (relu gradient 1);
    ln row 1 with K sign - neighbours: every relu pre-activation < 0, P == 0;
    rows 14, 15: z ~ -20 (sigmoid < 1e-7: KLD gradient 0, loss
                 yt log(yt / 1e-7));
    rows 8, 9:   z ~ +40 (sigmoid == 1 in float32 and in float64);
    rows 16, 17: z ~ -8.5 in all K slots of both lists (P Q ~ 4e-8 < 1e-7);
  plus ln == rn, le == re, a neighbour equal to ln, a repeated neighbour and
  a record with all three targets, on the generic rows.
  Returns idx, tgt, node_tab, edge_tab."""
  assert d >= 2
  amp = amp_for(loss, act, d)
  tabs = []
  for _ in range(2):
    u = amp * rs.choice([-1.0, 1.0], d)
    sign = np.ones(24)
    sign[5:8] = -1.0
    t = sign[:, None] * (u[None, :] * (1.0 + 0.25 * rs.uniform(-1, 1, (24, d))))
    h = d // 2
    t[10, h:] = 0.0
    t[11, :h] = 0.0
    t[12:14] = 0.0
    t[12:14, 0] = 2.0 ** -10
    un = u / np.linalg.norm(u)
    t[14], t[15] = np.sqrt(20.0) * un, -np.sqrt(20.0) * un
    t[8], t[9] = np.sqrt(40.0) * un, np.sqrt(40.0) * un
    t[16], t[17] = np.sqrt(8.5) * un, -np.sqrt(8.5) * un
    tabs.append(t.astype(np.float32))
  R = 4 + 2 * K
  neg = [5 + (k % 3) for k in range(K)]
  pos = [1 + (k % 4) for k in range(K)]
  rec = []

  def add(ln=0, le=0, rn=0, re=0, nn=(), ne=(), t=(0, 0, 0)):
    r = np.zeros(R, np.int32)
    r[:4] = ln, le, rn, re
    r[4:4 + len(nn)] = nn
    r[4 + K:4 + K + len(ne)] = ne
    rec.append((r, np.array(t, np.float32)))

  add(ln=10, rn=11, t=(.5, 0, 0))
  add(le=10, re=11, t=(0, .5, 0))
  add(ln=12, rn=13, t=(.5, 0, 0))
  add(le=12, re=13, t=(0, .5, 0))
  add(ln=10, re=1, nn=[11] * K, ne=pos, t=(0, 0, .5))
  add(ln=2, re=10, nn=pos, ne=[11] * K, t=(0, 0, .5))
  add(ln=1, re=2, nn=neg, ne=pos, t=(0, 0, .5))
  add(ln=3, re=1, nn=pos, ne=neg, t=(0, 0, .5))
  add(ln=14, rn=15, t=(.7, 0, 0))
  add(le=14, re=15, t=(0, .7, 0))
  add(ln=8, rn=9, t=(.6, 0, 0))
  add(le=8, re=9, t=(0, .6, 0))
  add(ln=16, re=16, nn=[17] * K, ne=[17] * K, t=(0, 0, .4))
  add(ln=2, rn=2, t=(.8, 0, 0))
  add(le=3, re=3, t=(0, .8, 0))
  add(ln=4, re=4, nn=[4] + pos[1:], ne=pos, t=(0, 0, .6))
  add(ln=1, re=2, nn=[3] * min(K, 2), ne=[4] * min(K, 2), t=(0, 0, .6))
  add(ln=1, le=2, rn=3, re=4, nn=pos[:max(1, K - 1)], ne=pos[:1],
      t=(.9, .35, .6))
  idx = np.stack([r for r, _ in rec])
  tgt = np.stack([t for _, t in rec])
  return idx, tgt, tabs[0], tabs[1]
