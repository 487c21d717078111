"""Truncated SVD of the incidence matrix on the device (reference:
``EmbedSvd``, hypergraph_embedding/embedding.py:110-126, which calls
``scipy.sparse.linalg.svds``) and the ``EmbedRandom`` baseline (:129-140).

``svd_incidence`` is a thick-restart block Lanczos on the Gram operator of
the smaller side (A^T A when E <= N, otherwise A A^T):

* block width b = k + oversample; a cycle multiplies ``steps`` blocks, each
  product two sparse x tall-skinny products (A V, then A^T (A V)) on fp32
  panels, each row summed in float64 and rounded once;
* every new block is projected twice against the whole basis (kept Ritz
  vectors included), normalised, projected once more and orthonormalised
  again (Gram on the device; its
  eigen / Cholesky factor in float64 with numpy; directions whose norm is
  at the products' rounding level are dropped, so a rank-deficient or
  exhausted Krylov space shrinks the block instead of breaking down);
* the projected matrix T = V^T G V is assembled from those explicit float64
  Grams, Rayleigh-Ritz is ``numpy.linalg.eigh`` in float64, and a restart
  keeps the top b Ritz vectors plus the residual block;
* when the Ritz estimate passes ``tol`` the k wanted vectors are finished:
  orthonormalised once more, B = A V formed, the k x k problem B^T B solved
  (so U = B S / sigma and V S are both orthonormal to fp32 rounding), and
  the residuals ``|G v_j - lambda_j v_j| / lambda_1`` measured with one more
  product. Only that measured figure ends the solve.

The driver talks to a backend with the protocol of ``_hgx.Svd`` (panel, set,
get, copy, spmm, gram, apply, scale, stats, close and ``rows``; nmf.py adds
cd_sweep, cd_sweep_fused and cd_stats);
``NumpyBackend`` restates it with numpy / scipy (fp32 panels, float64 sums) so
that the same driver runs without a GPU in the tests.
"""

import random as _pyrandom

import numpy as np

from . import _hgx
from .hypergraph_util import Incidence
from .proto import HypergraphEmbedding

EDGE, NODE = 0, 1
# panel slots: the Krylov basis and two block-sized work panels on the
# smaller side, one work panel on the larger side, the two result panels
BASIS, P1, P2, WORK, RES_S, RES_L = 0, 1, 2, 3, 4, 5
MAX_SMALL = 1056  # largest Gram / apply dimension of the device primitives
# A direction of a new block is dropped when its norm is below this times
# the norm of the product it came from: 16 ulp of fp32, about ten times the
# rounding error of one fp32 product column.
DROP = 16 * 2.0**-24
# Default stopping tolerance: ten times the worst residual floor measured on
# the device over the three test inputs (5.6e-8).
DEFAULT_TOL = 6e-7


class NumpyBackend:
  """The block primitives of ``_hgx.Svd`` on the host: fp32 panels, sparse
  products, Gram and apply summed in float64 and rounded once to fp32. For the non-GPU tests and as the statement of what the device
  computes."""

  def __init__(self, inc):
    import scipy.sparse as sp
    one = np.ones(inc.nnz, np.float64)
    self.a = sp.csr_matrix((one, inc.col_n, inc.rp_n), shape=(inc.N, inc.E))
    self.at = sp.csr_matrix((one, inc.col_e, inc.rp_e), shape=(inc.E, inc.N))
    self.rows = (inc.E, inc.N)
    self.nnz = inc.nnz
    self.p = {}
    self.side = {}
    self._st = {"spmm_ms": 0.0, "spmm_bytes": 0.0, "spmm_calls": 0,
                "spmm_cols": 0, "dense_calls": 0}

  def close(self):
    self.p = {}

  def panel(self, slot, side, width):
    self.p[slot] = np.zeros((self.rows[side], width), np.float32)
    self.side[slot] = side

  def set(self, slot, col0, host):
    self.p[slot][:, col0:col0 + host.shape[1]] = host

  def get(self, slot, col0, ncols):
    return self.p[slot][:, col0:col0 + ncols].copy()

  def copy(self, dst, dcol0, src, scol0, ncols):
    self.p[dst][:, dcol0:dcol0 + ncols] = self.p[src][:, scol0:scol0 + ncols]

  def spmm(self, dst, dcol0, src, scol0, ncols):
    assert self.side[dst] != self.side[src]
    m = self.a if self.side[dst] == NODE else self.at
    x = self.p[src][:, scol0:scol0 + ncols].astype(np.float64)
    self.p[dst][:, dcol0:dcol0 + ncols] = m @ x
    self._st["spmm_calls"] += 1
    self._st["spmm_cols"] += ncols
    self._st["spmm_bytes"] += (4.0 * self.nnz + 4.0 * ncols * self.nnz +
                               4.0 * ncols * self.rows[self.side[dst]])

  def gram(self, pslot, pcol0, p, qslot, qcol0, q):
    self._st["dense_calls"] += 1
    return (self.p[pslot][:, pcol0:pcol0 + p].astype(np.float64).T @
            self.p[qslot][:, qcol0:qcol0 + q].astype(np.float64))

  def apply(self, dst, dcol0, src, scol0, M, beta=0.0):
    M = np.asarray(M, np.float64)
    q, p = M.shape
    r = self.p[src][:, scol0:scol0 + q].astype(np.float64) @ M
    if beta != 0.0:
      r += beta * self.p[dst][:, dcol0:dcol0 + p]
    self.p[dst][:, dcol0:dcol0 + p] = r
    self._st["dense_calls"] += 1

  def scale(self, slot, col0, scale):
    s = np.asarray(scale, np.float64)
    self.p[slot][:, col0:col0 + s.size] = (
        self.p[slot][:, col0:col0 + s.size].astype(np.float64) * s)
    self._st["dense_calls"] += 1

  def stats(self):
    return dict(self._st)

  def cd_sweep(self, pslot, pcol0, bslot, bcol0, Q):
    """hgx_svd_cd_sweep: one non-negative coordinate-descent sweep of the k
    columns from pcol0 of pslot (P) against the k columns from bcol0 of bslot
    (B) and the k x k float64 matrix Q. Every row i on its own, t = 0..k-1 in
    order, in float64: g = Q[t] . P[i] - B[i][t]; the violation grows by |g|
    (|min(g, 0)| where P[i][t] == 0); P[i][t] becomes max(P[i][t] - g /
    Q[t][t], 0) rounded to fp32 (unless Q[t][t] == 0), and the later
    coordinates see the rounded value. Returns the summed violation."""
    k = np.shape(Q)[0]
    assert self.side[pslot] == self.side[bslot]
    assert pslot != bslot or pcol0 + k <= bcol0 or bcol0 + k <= pcol0
    return self._sweep(pslot, pcol0, Q,
                       self.p[bslot][:, bcol0:bcol0 + k].astype(np.float64))

  def cd_sweep_fused(self, pslot, pcol0, xslot, xcol0, Q):
    """hgx_svd_cd_sweep_fused: cd_sweep with B = A X (factor on the node
    side) or A^T X formed in float64 from the k columns from xcol0 of xslot,
    a panel of the other side, and used without rounding it to fp32."""
    k = np.shape(Q)[0]
    assert self.side[pslot] != self.side[xslot]
    m = self.a if self.side[pslot] == NODE else self.at
    return self._sweep(pslot, pcol0, Q,
                       m @ self.p[xslot][:, xcol0:xcol0 + k].astype(np.float64))

  def _sweep(self, pslot, pcol0, Q, B):
    import time
    t0 = time.perf_counter()
    Q = np.asarray(Q, np.float64)
    k = Q.shape[0]
    assert Q.shape == (k, k)
    if not np.isfinite(Q).all():
      raise ValueError("cd_sweep: the matrix holds a non-finite value")
    P = self.p[pslot][:, pcol0:pcol0 + k]
    W = P.astype(np.float64)
    viol = 0.0
    for t in range(k):
      g = W @ Q[t] - B[:, t]
      pt = W[:, t]
      viol += float(np.abs(np.where(pt == 0.0, np.minimum(g, 0.0), g)).sum())
      if Q[t, t] != 0.0:
        W[:, t] = np.maximum(pt - g / Q[t, t], 0.0).astype(np.float32)
    P[:] = W
    self._cd_ms = getattr(self, "_cd_ms", 0.0) + (time.perf_counter() - t0) * 1e3
    self._cd_n = getattr(self, "_cd_n", 0) + 1
    return viol

  def cd_stats(self):
    """Host wall time of the sweeps so far (ms) and their count."""
    return {"sweep_ms": getattr(self, "_cd_ms", 0.0),
            "sweeps": getattr(self, "_cd_n", 0)}


def _inv_factor(C):
  """M with M^T C M = I for a symmetric positive definite C: the inverse
  transpose of its Cholesky factor, or, when the factorisation fails, the
  same from the eigen decomposition with a floor (the shifted retry)."""
  C = (C + C.T) * 0.5
  try:
    L = np.linalg.cholesky(C)
    return np.linalg.inv(L).T
  except np.linalg.LinAlgError:
    ev, Q = np.linalg.eigh(C)
    ev = np.maximum(ev, ev[-1] * 1e-12)
    return Q / np.sqrt(ev)


class _Solver:
  """One solve's state. Every gram returns a small matrix to the host and
  every apply sends one, so a cycle is a chain of host round trips: at the
  100k / 50k graph (k = 128) those, with the host eigh, are 98% of the wall
  time and the sparse products 2%."""

  def __init__(self, be, small, k, b, steps, tol):
    self.be, self.small, self.large = be, small, 1 - small
    self.n = be.rows[small]
    self.k, self.b, self.steps, self.tol = k, b, steps, tol
    self.cap = min((steps + 2) * b, self.n)
    if self.cap > MAX_SMALL:
      raise _hgx.HgxError(
          "svd_incidence: a basis of %d columns (k + oversample = %d, %d "
          "steps) is above the %d the device's block algebra takes" %
          (self.cap, b, steps, MAX_SMALL))
    be.panel(BASIS, small, self.cap)
    be.panel(P1, small, b)
    be.panel(P2, small, b)
    be.panel(WORK, self.large, b)
    be.panel(RES_S, small, k)
    be.panel(RES_L, self.large, k)
    self.T = np.zeros((self.cap, self.cap))
    self.cnt = 0          # basis columns, the unmultiplied block included
    self.blk = (0, 0)     # the unmultiplied block (first column, width)
    self.last = (0, 0)    # the block multiplied last
    self.Rc = np.zeros((0, 0))  # P1 after projection = new block @ Rc
    self.products = 0
    self.history = []     # largest measured residual of every finish

  def _orthonormalise(self, w, scale):
    """P1[:, :w] (already orthogonal to the basis) -> orthonormal columns
    appended to the basis; returns their count and the factor Rc."""
    be, cnt = self.be, self.cnt
    C = be.gram(P1, 0, w, P1, 0, w)
    C = (C + C.T) * 0.5
    ev, Q = np.linalg.eigh(C)
    if scale is None:
      scale = np.sqrt(max(ev[-1], 0.0))
    keep = ev > (DROP * scale)**2
    room = self.cap - cnt
    if keep.sum() > room:
      keep[:keep.size - room] = False  # eigh is ascending: keep the largest
    wn = int(keep.sum())
    if wn == 0:
      return 0, np.zeros((0, w))
    M1 = Q[:, keep] / np.sqrt(ev[keep])
    be.apply(P2, 0, P1, 0, M1)
    if cnt:
      # a direction much shorter than the block's columns carries their
      # rounding (absolute, in every direction) at full size once it is
      # normalised: project the normalised block once more
      be.apply(P2, 0, BASIS, 0, -be.gram(BASIS, 0, cnt, P2, 0, wn), beta=1.0)
    M2 = _inv_factor(be.gram(P2, 0, wn, P2, 0, wn))
    be.apply(BASIS, cnt, P2, 0, M2)
    Rc = np.linalg.solve(M2, np.sqrt(ev[keep])[:, None] * Q[:, keep].T)
    return wn, Rc

  def start(self):
    x = np.random.standard_normal((self.n, self.b)).astype(np.float32)
    self.be.set(P1, 0, x)
    wn, _ = self._orthonormalise(self.b, None)
    self.blk, self.cnt = (0, wn), wn

  def multiply(self):
    """G times the unmultiplied block: its column of T, and the next block."""
    be, cnt = self.be, self.cnt
    c0, w = self.blk
    be.spmm(WORK, 0, BASIS, c0, w)
    be.spmm(P1, 0, WORK, 0, w)
    self.products += 2
    H = be.gram(BASIS, 0, cnt, P1, 0, w)
    be.apply(P1, 0, BASIS, 0, -H, beta=1.0)
    H2 = be.gram(BASIS, 0, cnt, P1, 0, w)
    be.apply(P1, 0, BASIS, 0, -H2, beta=1.0)
    H += H2
    T = self.T
    T[:cnt, c0:c0 + w] = H
    T[c0:c0 + w, :cnt] = H.T
    d = T[c0:c0 + w, c0:c0 + w]
    T[c0:c0 + w, c0:c0 + w] = (d + d.T) * 0.5
    scale = np.sqrt((H * H).sum(0).max())
    wn, Rc = self._orthonormalise(w, scale)
    self.last, self.Rc = (c0, w), Rc
    self.blk, self.cnt = (cnt, wn), cnt + wn

  def ritz(self):
    qm = self.blk[0]
    th, S = np.linalg.eigh(self.T[:qm, :qm])
    c0, w = self.last
    if self.blk[1]:
      est = np.linalg.norm(self.Rc @ S[c0:c0 + w, :], axis=0) / th[-1]
    else:
      est = np.zeros(qm)  # the basis spans an invariant subspace
    return th, S, est

  def restart(self, th, S):
    be = self.be
    qm, (r0, wr) = self.blk[0], self.blk
    nk = min(self.b, qm)
    be.apply(P2, 0, BASIS, 0, S[:, qm - nk:])
    if wr:
      be.copy(P1, 0, BASIS, r0, wr)
    be.copy(BASIS, 0, P2, 0, nk)
    if wr:
      be.copy(BASIS, nk, P1, 0, wr)
    self.T[:] = 0.0
    self.T[:nk, :nk] = np.diag(th[qm - nk:])
    self.blk, self.cnt = (nk, wr), nk + wr

  def finish(self, S):
    """The k wanted Ritz vectors -> result panels; returns (sigma ascending,
    measured residuals |G v - lambda v| / lambda_1)."""
    be, k = self.be, self.k
    qm = self.blk[0]
    be.apply(P2, 0, BASIS, 0, S[:, qm - k:])
    M = _inv_factor(be.gram(P2, 0, k, P2, 0, k))
    be.apply(P1, 0, P2, 0, M)
    be.spmm(WORK, 0, P1, 0, k)
    ev, S2 = np.linalg.eigh(be.gram(WORK, 0, k, WORK, 0, k))
    sig = np.sqrt(np.maximum(ev, 0.0))
    be.apply(RES_S, 0, P2, 0, M @ S2)  # one rounding, not two through P1
    live = sig > 1e-6 * sig[-1]
    # U = B S2 diag(1 / sigma) in one apply: a separate column scaling
    # (backend.scale) would round every entry of U a second time
    be.apply(RES_L, 0, WORK, 0,
             S2 * np.where(live, 1.0 / np.where(live, sig, 1.0), 0.0))
    be.spmm(P2, 0, RES_L, 0, k)
    be.apply(P2, 0, RES_S, 0, -np.diag(sig), beta=1.0)
    self.products += 2
    r = np.sqrt(np.maximum(np.diag(be.gram(P2, 0, k, P2, 0, k)), 0.0))
    res = sig * r / sig[-1]**2
    self.history.append(float(res.max()))
    return sig, live, res


def _no_convergence(msg, sv, restarts):
  e = _hgx.HgxError("svd_incidence: " + msg)
  e.info = {"restarts": restarts, "products": sv.products, "converged": False,
            "measured": list(sv.history)}
  return e


def svd_incidence(inc, k, tol=None, max_restarts=300, oversample=8, steps=None,
                  ctx=None, backend=None):
  """The k largest singular triplets of the N x E 0/1 incidence matrix.

  Returns ``(U, s, Vt, info)``: ``s`` ascending as ``scipy.sparse.linalg.svds``
  returns it, ``U`` N x k and ``Vt`` k x E in float32, each pair's sign chosen
  so that the largest-magnitude entry of ``v_j`` (the lowest index on ties) is
  positive. ``info`` holds ``restarts``, ``products`` (block products applied),
  ``product_columns``, ``residuals`` (the measured ``|G v_j - lambda_j v_j| /
  lambda_1`` of the returned pairs), ``estimate``, ``converged``, ``tol``,
  ``block``, ``steps``, ``measured`` (the largest measured residual of every
  finish tried) and the backend's ``stats``; the error raised on failure
  carries the same counters as ``.info``.

  The solve stops when the largest measured residual is at most ``tol``. The
  default, 6e-7, is ten times the residual floor the device reaches on the
  project's three test inputs (3.5e-8 to 5.6e-8 measured on an MI355X;
  further restarts do not lower it). The floor is that of fp32
  panels: the sparse products, the Gram sums and the Rayleigh-Ritz step all
  sum in float64 (with fp32 row sums the numpy backend cannot get below
  1.7e-5 on the input whose edges have thousands of members). If ``max_restarts`` runs out, or the
  Krylov space is exhausted above ``tol``, ``_hgx.HgxError`` (a RuntimeError,
  as scipy's ArpackNoConvergence is) is raised.

  Rank-deficient tail: a pair with ``s_j <= 1e-6 s_max`` is returned with
  ``u_j = 0`` and a unit ``v_j`` orthogonal to the other right vectors (a
  null vector of the matrix), and ``s_j`` as computed (about 0).

  The start block comes from numpy's global RandomState, so ``np.random.seed``
  makes a run reproducible bit for bit. ``ctx`` is the device context (the
  process-wide one by default; its resident incidence is replaced by
  ``inc``); ``backend`` is any object with ``_hgx.Svd``'s protocol instead,
  e.g. ``NumpyBackend(inc)``.
  """
  k = int(k)
  assert 0 < k < min(inc.N, inc.E)
  tol = DEFAULT_TOL if tol is None else float(tol)
  own = backend is None
  if own:
    from .runtime import get_context
    ctx = ctx or get_context()
    ctx.upload(inc)
    backend = _hgx.Svd(ctx)
  try:
    small = EDGE if inc.E <= inc.N else NODE
    n = backend.rows[small]
    b = min(k + int(oversample), n)
    if steps is None:
      steps = max(2, min(6, MAX_SMALL // b - 2))
    sv = _Solver(backend, small, k, b, int(steps), tol)
    sv.start()
    restarts = 0
    first = True
    while True:
      for _ in range(sv.steps + (1 if first else 0)):
        # a product needs room for a whole residual block, unless the basis
        # is about to span the whole space
        if sv.blk[1] == 0 or (sv.cap - sv.cnt < sv.blk[1] and sv.cap < sv.n):
          break
        sv.multiply()
      first = False
      th, S, est = sv.ritz()
      est_k = est[-k:]
      if est_k.max() <= tol:
        sig, live, res = sv.finish(S)
        if res.max() <= tol:
          break
        if sv.blk[1] == 0:
          raise _no_convergence(
              "the Krylov space is exhausted at residual %.3g, above tol = "
              "%.3g" % (res.max(), tol), sv, restarts)
      elif sv.blk[1] == 0:
        raise _no_convergence("breakdown before convergence", sv, restarts)
      if restarts >= max_restarts:
        raise _no_convergence(
            "no convergence in %d restarts (estimate %.3g, tol %.3g)" %
            (restarts, est_k.max(), tol), sv, restarts)
      sv.restart(th, S)
      restarts += 1
    xs = backend.get(RES_S, 0, k)
    xl = backend.get(RES_L, 0, k)
    stats = backend.stats()
  finally:
    if own:
      backend.close()
  U, V = (xl, xs) if small == EDGE else (xs, xl)
  if small == NODE and not live.all():
    # the computed vectors of a zero singular value are left null vectors:
    # return u_j = 0 and a right null vector instead
    V, U = V.astype(np.float64), U.copy()
    for j in np.flatnonzero(~live):
      others = np.delete(V, j, axis=1)
      v = np.random.standard_normal(V.shape[0])
      for _ in range(2):
        v -= others @ (others.T @ v)
      V[:, j] = v / np.linalg.norm(v)
      U[:, j] = 0.0
    V = V.astype(np.float32)
  top = np.abs(V).argmax(axis=0)
  flip = np.where(V[top, np.arange(k)] < 0, -1.0, 1.0).astype(np.float32)
  U, V = U * flip, V * flip
  info = {"restarts": restarts, "products": sv.products,
          "product_columns": stats["spmm_cols"], "residuals": res,
          "estimate": est_k, "converged": True, "tol": tol, "block": b,
          "measured": list(sv.history),
          "steps": sv.steps, "side": "edge" if small == EDGE else "node",
          "stats": stats}
  return (np.ascontiguousarray(U), sig.astype(np.float32),
          np.ascontiguousarray(V.T), info)


def EmbedSvd(hypergraph, dimension, *, tol=None, max_restarts=300, ctx=None,
             backend_factory=None):
  """embedding.py:110-126: node vector = row of U, edge vector = column of
  V^T of the ``dimension`` largest singular triplets (unit-norm columns, not
  scaled by the singular values), keyed by the original ids. The reference
  builds its matrix on the raw ids; ids that are absent are zero rows and
  columns there and change nothing for the ids present, so the compressed
  ``Incidence`` (also accepted as input) gives the same vectors.
  ``backend_factory`` (a callable: Incidence -> backend object, e.g.
  ``NumpyBackend``) replaces the device, as ``backend`` does in
  ``svd_incidence``."""
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension < inc.N
  assert dimension < inc.E
  assert dimension > 0
  from .algebraic_distance import coords_to_embedding
  U, _, Vt, _ = svd_incidence(inc, dimension, tol=tol,
                              max_restarts=max_restarts, ctx=ctx,
                              backend=(backend_factory(inc) if backend_factory
                                       else None))
  return coords_to_embedding(inc, U, Vt.T, dimension, "SVD")


def EmbedRandom(hypergraph, dimension):
  """embedding.py:129-140: ``dimension`` draws of Python's global
  ``random.random()`` per node in the node map's iteration order, then the
  same for the edges (stored as float32, as the message stores them)."""
  assert dimension > 0
  embedding = HypergraphEmbedding()
  embedding.dim = dimension
  embedding.method_name = "RANDOM"
  if isinstance(hypergraph, Incidence):
    nodes, edges = hypergraph.node_ids.tolist(), hypergraph.edge_ids.tolist()
  else:
    nodes, edges = hypergraph.node, hypergraph.edge
  rnd = _pyrandom.random
  for node_idx in nodes:
    embedding.node[node_idx].values.extend([rnd() for _ in range(dimension)])
  for edge_idx in edges:
    embedding.edge[edge_idx].values.extend([rnd() for _ in range(dimension)])
  return embedding


__all__ = ["svd_incidence", "EmbedSvd", "EmbedRandom", "NumpyBackend"]
