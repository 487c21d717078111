"""Auto-encoder baseline on the device (reference: ``EmbedAutoEncoder``,
hypergraph_embedding/auto_encoder.py:20-115, a Keras model per side trained
on the CPU from dense perturbed rows).

Per side of the incidence (rows x C) the model is

  x (C) -> Dense(d, relu) [W1 C x d, b1] -> Dense(C, softmax) [W2 d x C, b2]

with glorot-uniform kernels, zero biases, ``kullback_leibler_divergence``
and Adagrad (lr 0.01, eps 1e-7). A sample of a row with support S, n = |S|,
is a pair ``(row, drop)``: the target is 1_S / n, the input 1_S / n
(``drop = -1``) or, for each of ``min(n, samples_per_idx)`` distinct columns
c of a row of more than one column, 1_{S \\ c} / (n - 1). Per epoch the rows
are permuted and split by ``numpy.array_split`` into
``max(1, int(rows / idx_per_batch))`` sections; every section is one
``train_on_batch`` on all its rows' samples. The embedding of a row is
``relu(1_S / n . W1 + b1)``.

The device engine (``_hgx.Ae``, csrc/hgx_ae.hip) never forms a dense input or
target: DESIGN §4.9. ``NumpyBackend`` restates it in float32 on the host with
the same protocol (set_weights, get_weights, draw, step, encode), so the
driver runs without a GPU.
"""

import numpy as np

from . import _hgx
from .hypergraph_util import Incidence

NODE, EDGE = 0, 1
MAX_DIM = 512  # hgx_ae_create's limit (include/hgx.h)
KEPS = np.float32(1e-7)  # Keras' epsilon in its float32 graph
_M64 = (1 << 64) - 1


def side_csr(inc, side):
  """(rows, C, rowptr, columns) of the side's matrix: node rows over edge
  columns (NODE) or edge rows over node columns (EDGE)."""
  if side == NODE:
    return inc.N, inc.E, np.asarray(inc.rp_n), np.asarray(inc.col_n)
  assert side == EDGE
  return inc.E, inc.N, np.asarray(inc.rp_e), np.asarray(inc.col_e)


def glorot_uniform(fan_in, fan_out):
  """Keras' default Dense kernel from numpy's global RandomState."""
  lim = np.sqrt(6.0 / (fan_in + fan_out))
  return np.random.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32)


def sections(perm, idx_per_batch):
  """The reference's batches of one epoch (auto_encoder.py:64-66)."""
  perm = np.asarray(perm)
  return np.array_split(perm, max(1, int(len(perm) / idx_per_batch)))


# ---- the library's counter-based generator (csrc/hgx_internal.h) ------------
def _mix64(z):
  z = (z + 0x9e3779b97f4a7c15) & _M64
  z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & _M64
  z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & _M64
  return z ^ (z >> 31)


def _rand64_key(seed, stream):
  return _mix64((seed & _M64) ^ _mix64((stream + 0x632be59bd9b4e019) & _M64))


def draw_row(cols, samples_per_idx, seed, row, epoch):
  """The drops hgx_ae_draw gives a row with the columns ``cols``: none for a
  row of one column, every column when there are at most ``samples_per_idx``,
  else selection sampling keyed by (seed, row, epoch)."""
  n = len(cols)
  if n <= 1:
    return []
  k = min(n, samples_per_idx)
  if n <= k:
    return [int(c) for c in cols]
  key = _rand64_key(seed, (epoch << 32) | row)
  out = []
  for j in range(n):
    if len(out) == k:
      break
    if (_mix64((key + j) & _M64) * (n - j)) >> 64 < k - len(out):
      out.append(int(cols[j]))
  return out


class NumpyBackend:
  """Float32 host restatement of the engine on one side of ``inc``.
  ``reverse=True`` runs every batch over its sample list reversed, which
  reverses each sum over samples: the distance between the two orders is the
  float32 floor the device tests take their bar from."""

  def __init__(self, inc, side, dim, reverse=False):
    self.side, self.dim, self.reverse = side, int(dim), bool(reverse)
    self.R, self.C, self.rp, self.col = side_csr(inc, side)
    d, C = self.dim, self.C
    self.set_weights(np.zeros((C, d)), np.zeros(d), np.zeros((d, C)),
                     np.zeros(C))
    self._ms = 0.0
    self._samples = self._batches = 0

  def close(self):
    pass

  def set_weights(self, W1, b1, W2, b2):
    d, C = self.dim, self.C
    self.W = [np.array(W1, np.float32).reshape(C, d),
              np.array(b1, np.float32).reshape(d),
              np.array(W2, np.float32).reshape(d, C),
              np.array(b2, np.float32).reshape(C)]
    self.A = [np.zeros_like(w) for w in self.W]

  def get_weights(self):
    return tuple(w.copy() for w in self.W)

  def draw(self, rows, samples_per_idx, seed, epoch):
    row, drop = [], []
    for r in np.asarray(rows).ravel():
      r = int(r)
      d = draw_row(self.col[self.rp[r]:self.rp[r + 1]], samples_per_idx, seed,
                   r, epoch)
      row.extend([r] * (1 + len(d)))
      drop.extend([-1] + d)
    return np.array(row, np.int32), np.array(drop, np.int32)

  def _pairs(self, row, drop):
    """(sample, column) of every non-zero input entry, the input's value per
    sample, and the pairs of the targets' supports."""
    pm, pc, tm, tc = [], [], [], []
    v = np.empty(len(row), np.float32)
    for m, (r, dr) in enumerate(zip(row, drop)):
      assert 0 <= r < self.R
      cs = self.col[self.rp[r]:self.rp[r + 1]]
      tm.append(np.full(cs.size, m))
      tc.append(cs)
      if dr >= 0:
        assert cs.size > 1 and dr in cs
        cs = cs[cs != dr]
      pm.append(np.full(cs.size, m))
      pc.append(cs)
      v[m] = np.float32(1.0) / np.float32(cs.size)
    cat = np.concatenate
    return cat(pm), cat(pc), v, cat(tm), cat(tc)

  def _hidden(self, pm, pc, v, M):
    W1, b1 = self.W[0], self.W[1]
    hs = np.zeros((M, self.dim), np.float32)
    np.add.at(hs, pm, W1[pc])
    return np.maximum(v[:, None] * hs + b1, np.float32(0))

  def step(self, row, drop, lr=0.01, eps=1e-7):
    import time
    t0 = time.perf_counter()
    row = np.asarray(row, np.int64).ravel()
    drop = np.asarray(drop, np.int64).ravel()
    assert row.size == drop.size and row.size > 0
    if self.reverse:
      row, drop = row[::-1], drop[::-1]
    M, C = row.size, self.C
    W1, b1, W2, b2 = self.W
    pm, pc, v, tm, tc = self._pairs(row, drop)
    H = self._hidden(pm, pc, v, M)
    Z = H @ W2 + b2
    e = np.exp(Z - Z.max(1, keepdims=True))
    P = e / e.sum(1, keepdims=True)
    yt = np.full((M, C), KEPS, np.float32)
    yt[tm, tc] = (np.float32(1.0) /
                  (self.rp[row + 1] - self.rp[row]).astype(np.float32))[tm]
    pcl = np.maximum(P, KEPS)
    loss = float((yt * np.log(yt / pcl)).sum(1, dtype=np.float64).sum() / M)
    u = P >= KEPS
    ytu = np.where(u, yt, np.float32(0))
    T = ytu.sum(1)
    dZ = (P * T[:, None] - ytu) * (np.float32(1.0) / np.float32(M))
    gW2 = H.T @ dZ
    gb2 = dZ.sum(0)
    dH = (dZ @ W2.T) * (H > 0)
    gb1 = dH.sum(0)
    gW1 = np.zeros_like(W1)
    np.add.at(gW1, pc, (v[:, None] * dH)[pm])
    lr, eps = np.float32(lr), np.float32(eps)
    for p, a, g in zip(self.W, self.A, (gW1, gb1, gW2, gb2)):
      a += g * g
      p -= lr * g / (np.sqrt(a) + eps)
    self._ms = (time.perf_counter() - t0) * 1e3
    self._samples, self._batches = M, 1
    return loss

  def encode(self, rows):
    rows = np.asarray(rows, np.int64).ravel()
    pm, pc, v, _, _ = self._pairs(rows, np.full(rows.size, -1))
    return self._hidden(pm, pc, v, rows.size)

  def stats(self):
    return {"ms": self._ms, "samples": self._samples,
            "batches": self._batches,
            "flops": 6.0 * self._samples * self.C * self.dim}


def _fit_loop(be, epochs, idx_per_batch, samples_per_idx, lr, eps, seed, perms):
  """hgx_ae_fit as a host loop of draw + step (any backend)."""
  losses = []
  for ep in range(epochs):
    losses.append([be.step(*be.draw(sec, samples_per_idx, seed, ep), lr=lr,
                           eps=eps)
                   for sec in sections(perms[ep], idx_per_batch)])
  return np.array(losses, np.float32).reshape(epochs, -1)


def _fit_mt19937(be, rp, col, rows, epochs, idx_per_batch, samples_per_idx, lr,
                 eps):
  """The reference's own draws in the reference's order from numpy's global
  RandomState (auto_encoder.py:20-37, 61-76): per epoch the permutation, then
  per row of each section, as its batch is built, ``np.random.choice`` of
  ``min(n, samples_per_idx)`` of its columns without replacement."""
  losses = []
  for _ in range(epochs):
    ep = []
    for sec in sections(np.random.permutation(rows), idx_per_batch):
      row, drop = [], []
      for r in sec:
        cs = col[rp[r]:rp[r + 1]]
        row.append(r)
        drop.append(-1)
        if cs.size > 1:
          for c in np.random.choice(cs, min(cs.size, samples_per_idx),
                                    replace=False):
            row.append(r)
            drop.append(c)
      ep.append(be.step(np.array(row, np.int32), np.array(drop, np.int32),
                        lr=lr, eps=eps))
    losses.append(ep)
  return np.array(losses, np.float32).reshape(epochs, -1)


def auto_encoder_incidence(inc, side, dimension, *, epochs=5,
                           idx_per_batch=200, samples_per_idx=100, lr=0.01,
                           eps=1e-7, rng="device", kernels=None, ctx=None,
                           backend=None):
  """Train the reference's auto-encoder on one side of ``inc`` (``NODE``: a
  row per node over the edges, ``EDGE``: a row per edge over the nodes) and
  return ``(embedding rows x dimension float32, info)``.

  Host draws come from numpy's global RandomState, in this order: the glorot
  kernels W1 then W2 (unless ``kernels=(W1, W2)`` is given), then with
  ``rng="device"`` one ``np.random.permutation(rows)`` per epoch and one seed
  for the device's sample draw; after ``np.random.seed`` a run is
  reproducible bit for bit. ``rng="mt19937"`` makes the reference's own
  ``permutation`` / ``choice`` calls in the reference's order instead and
  trains through ``step`` on those explicit lists: the batches are the
  reference's given the stream position at the start of the fit (Keras
  consumes draws of its own when it builds a model, which is not restated).

  ``info``: ``batch_loss`` (epochs x sections), ``sections``, ``stats`` of
  the backend's last call. ``ctx`` is the device context (the process-wide
  one by default; its resident incidence is replaced by ``inc``);
  ``backend`` is any object with the engine's protocol instead, e.g.
  ``NumpyBackend(inc, side, dimension)``.
  """
  d = int(dimension)
  assert d > 0
  assert epochs >= 0 and idx_per_batch > 0 and samples_per_idx >= 0
  if rng not in ("device", "mt19937"):
    raise ValueError("auto_encoder_incidence: rng %r is not 'device' or "
                     "'mt19937'" % (rng,))
  if d > MAX_DIM:
    raise _hgx.HgxError("auto_encoder_incidence: dimension %d is above the "
                        "%d the device engine takes" % (d, MAX_DIM))
  R, C, rp, col = side_csr(inc, side)
  own = backend is None
  if own:
    from .runtime import get_context
    ctx = ctx or get_context()
    ctx.upload(inc)
    backend = _hgx.Ae(ctx, side, d)
  be = backend
  try:
    W1, W2 = kernels if kernels is not None else (glorot_uniform(C, d),
                                                  glorot_uniform(d, C))
    be.set_weights(W1, np.zeros(d, np.float32), W2, np.zeros(C, np.float32))
    if rng == "mt19937":
      losses = _fit_mt19937(be, rp, col, R, epochs, idx_per_batch,
                            samples_per_idx, lr, eps)
    else:
      perms = np.array([np.random.permutation(R) for _ in range(epochs)],
                       np.int64).reshape(epochs, R)
      seed = int(np.random.randint(0, 2**31 - 1))
      if hasattr(be, "fit"):
        losses = be.fit(epochs, idx_per_batch, samples_per_idx, lr, eps, seed,
                        perms)
      else:
        losses = _fit_loop(be, epochs, idx_per_batch, samples_per_idx, lr, eps,
                           seed, perms)
    emb = be.encode(np.arange(R, dtype=np.int32))
    stats = be.stats()
  finally:
    if own:
      be.close()
  info = {"batch_loss": losses, "sections": max(1, int(R / idx_per_batch)),
          "stats": stats, "rng": rng}
  return emb, info


def EmbedAutoEncoder(hypergraph, dimension, num_samples=100, epochs=5,
                     idx_per_batch=200, run_in_parallel=True,
                     disable_pbar=False, *, rng="device", ctx=None,
                     backend_factory=None, info=None):
  """auto_encoder.py:87-115: node vector = the node model's encoding of the
  node's normalised row, edge vector = the edge model's, keyed by the
  original ids. The reference compresses the id range first
  (``CompressRange``), which is the matrix of the compressed ``Incidence``
  (also accepted as input). ``run_in_parallel`` and ``disable_pbar`` are the
  reference's and change nothing here. The four glorot kernels are drawn
  first (W1 then W2, node model then edge model), then each model's
  permutations and seed (``auto_encoder_incidence``). ``backend_factory`` (a
  callable: (Incidence, side, dimension) -> backend, e.g. ``NumpyBackend``)
  replaces the device; a dict passed as ``info`` receives the two sides'
  info under "node" and "edge"."""
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension > 0
  assert num_samples >= 0
  assert epochs >= 0
  assert idx_per_batch > 0
  from .algebraic_distance import coords_to_embedding
  kernels = [(glorot_uniform(C, dimension), glorot_uniform(dimension, C))
             for C in (inc.E, inc.N)]
  out = []
  for side, name in ((NODE, "node"), (EDGE, "edge")):
    emb, i = auto_encoder_incidence(
        inc, side, dimension, epochs=epochs, idx_per_batch=idx_per_batch,
        samples_per_idx=num_samples, rng=rng, kernels=kernels[side], ctx=ctx,
        backend=(backend_factory(inc, side, dimension) if backend_factory
                 else None))
    out.append(emb)
    if info is not None:
      info[name] = i
  return coords_to_embedding(inc, out[0], out[1], dimension, "AutoEncoder")


__all__ = ["auto_encoder_incidence", "EmbedAutoEncoder", "NumpyBackend",
           "draw_row", "sections", "glorot_uniform", "NODE", "EDGE"]
