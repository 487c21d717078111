"""Non-negative matrix factorisation of the incidence matrix on the device
(reference: ``EmbedNMF``, hypergraph_embedding/embedding.py:143-162, which
calls ``sklearn.decomposition.NMF(dimension)`` on ``matrix.todense()``).

``nmf_incidence`` is sklearn's default solver, coordinate descent on the
Frobenius loss without regularisation or shuffle (``_fit_coordinate_descent``
/ ``_update_cdnmf_fast``), restated on the panel engine of svd.py so that the
N x E matrix is never densified. W (N x k) and H^T (E x k) are fp32 panels;
an iteration is

  Q = H H^T (gram)   v  = cd_sweep_fused(W,   H^T, Q)    with Bn = A H^T
  Q = W^T W (gram)   v += cd_sweep_fused(H^T, W,   Q)    with Be = A^T W

and the solve stops when ``v / v_first <= tol``. The sweep (the new device
kernel, csrc/hgx_spmm.hip; ``NumpyBackend`` states it on the host) does the
per-row coordinate updates in float64 and rounds every coordinate to fp32 as
it is stored. Its fused form sums the row of the product Bn / Be it needs in
float64 inside the kernel and never rounds it: with the products stored in
fp32 panels (``spmm`` then ``cd_sweep``) a badly scaled component, whose
gradient cancels the product against the Gram terms, put one test input
1.09e-5 of ``max(W, H)`` away from sklearn's float64 solve after 200
iterations; fused it is 2.9e-6.

The driver talks to the backend protocol of svd.py only (panel, set, get,
spmm, gram, cd_sweep_fused, stats, cd_stats, close), so ``NumpyBackend`` runs
it without a GPU.
"""

import warnings

import numpy as np

from . import _hgx
from .hypergraph_util import Incidence
from .svd import EDGE, NODE, svd_incidence

# panel slots: the two factors, and the product A H^T of the final error
W_, HT_, BN_ = 0, 1, 2
MAX_K = 512  # the sweep's limit (hgx_svd_cd_sweep, include/hgx.h)
EPS = float(np.finfo(np.float64).eps)


def nndsvd_init(U, s, Vt, fill=None):
  """sklearn's ``_initialize_nmf`` (NNDSVD, Boutsidis & Gallopoulos 2008) from
  the triplets ``U`` (N x k), ``s`` (k), ``Vt`` (k x E), largest first, in
  float64: the first pair by absolute value, every other pair by the larger
  of its positive and negative parts; entries below eps become 0 and, with
  ``fill`` (nndsvda: the matrix mean), zeros become ``fill``. A triplet whose
  parts all have zero norm (``u_j = 0``: the rank-deficient tail of
  svd_incidence) gives a zero column and row where sklearn would divide 0 by
  0. The result does not depend on the sign of a pair."""
  U = np.asarray(U, np.float64)
  Vt = np.asarray(Vt, np.float64)
  s = np.asarray(s, np.float64)
  k = s.size
  W, H = np.zeros_like(U), np.zeros_like(Vt)
  W[:, 0] = np.sqrt(s[0]) * np.abs(U[:, 0])
  H[0] = np.sqrt(s[0]) * np.abs(Vt[0])
  for j in range(1, k):
    x, y = U[:, j], Vt[j]
    xp, yp = np.maximum(x, 0), np.maximum(y, 0)
    xn, yn = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
    xpn, ypn = np.linalg.norm(xp), np.linalg.norm(yp)
    xnn, ynn = np.linalg.norm(xn), np.linalg.norm(yn)
    mp, mn = xpn * ypn, xnn * ynn
    if mp > mn:
      u, v, sigma = xp / xpn, yp / ypn, mp
    elif mn > 0:
      u, v, sigma = xn / xnn, yn / ynn, mn
    else:
      continue
    lbd = np.sqrt(s[j] * sigma)
    W[:, j] = lbd * u
    H[j] = lbd * v
  W[W < EPS] = 0
  H[H < EPS] = 0
  if fill is not None:
    W[W == 0] = fill
    H[H == 0] = fill
  return W, H


def _check_custom(inc, k, W0, H0):
  if W0 is None or H0 is None:
    raise ValueError("nmf_incidence: init='custom' needs W0 and H0")
  W0, H0 = np.asarray(W0), np.asarray(H0)
  for name, m, shape in (("W0", W0, (inc.N, k)), ("H0", H0, (k, inc.E))):
    if m.shape != shape:
      raise ValueError("nmf_incidence: %s has shape %s, not %s" %
                       (name, m.shape, shape))
    if not np.isfinite(m).all():
      raise ValueError("nmf_incidence: %s holds a non-finite value" % name)
    if (m < 0).any():
      raise ValueError("nmf_incidence: %s holds a negative value" % name)
  return W0, H0


def nmf_incidence(inc, k, *, init="nndsvda", W0=None, H0=None, tol=1e-4,
                  max_iter=200, ctx=None, backend=None):
  """A ~ W H for the N x E 0/1 incidence matrix, W >= 0 (N x k) and H >= 0
  (k x E) in float32: ``sklearn.decomposition.NMF(k)`` with its defaults
  (solver "cd", Frobenius loss, no regularisation, ``tol`` 1e-4, ``max_iter``
  200), on the sparse matrix.

  ``init``: "nndsvda" (what ``NMF(k)`` picks for k < min(N, E)) or "nndsvd"
  follow sklearn's ``_initialize_nmf`` on the k largest triplets of
  ``svd_incidence(inc, k)``, run on the same engine. sklearn takes them from
  an approximate randomized SVD under its ``random_state``; these are the
  converged ones, so the start, and with it the factors, differ slightly from
  any one sklearn run (the reconstruction error lands inside sklearn's own
  seed-to-seed spread). The SVD's start block comes from numpy's
  global RandomState: after ``np.random.seed`` a run is reproducible bit for
  bit. "custom" starts from ``W0`` (N x k) and ``H0`` (k x E), which must be
  finite and non-negative (``ValueError`` otherwise; they are rounded to
  float32).

  Returns ``(W, H, info)``. ``info``: ``n_iter``; ``converged`` (the stop
  test ``violation / violation_init <= tol`` fired; when ``max_iter`` ends
  the solve instead a ``RuntimeWarning`` is emitted, as sklearn warns and
  does not raise); ``violation`` (that ratio after every iteration) and
  ``violation_init``; ``reconstruction_err`` = ``|A - W H|_F`` (sklearn's
  ``reconstruction_err_``) from nnz - 2 tr(W^T A H^T) + sum(W^T W o H H^T),
  without forming W H; ``sweep_ms`` (time inside the coordinate sweeps:
  device time from HIP events, host wall time for the numpy backend), the
  backend's ``stats`` and ``init``.

  ``ctx`` is the device context (the process-wide one by default; its
  resident incidence is replaced by ``inc``); ``backend`` is any object with
  the engine's protocol instead, e.g. ``svd.NumpyBackend(inc)``.
  """
  k = int(k)
  assert 0 < k < min(inc.N, inc.E)
  if init not in ("nndsvda", "nndsvd", "custom"):
    raise ValueError("nmf_incidence: init %r is not one of 'nndsvda', "
                     "'nndsvd', 'custom'" % (init,))
  if k > MAX_K:
    raise _hgx.HgxError(
        "nmf_incidence: k = %d is above the %d the device's coordinate sweep "
        "takes" % (k, MAX_K))
  if init == "custom":
    W0, H0 = _check_custom(inc, k, W0, H0)
  tol, max_iter = float(tol), int(max_iter)
  own = backend is None
  if own:
    from .runtime import get_context
    ctx = ctx or get_context()
    ctx.upload(inc)
    backend = _hgx.Svd(ctx)
  be = backend
  try:
    if init != "custom":
      U, s, Vt, _ = svd_incidence(inc, k, backend=be)
      fill = inc.nnz / (float(inc.N) * inc.E) if init == "nndsvda" else None
      W0, H0 = nndsvd_init(U[:, ::-1], s[::-1], Vt[::-1], fill)
    be.panel(W_, NODE, k)
    be.panel(HT_, EDGE, k)
    be.panel(BN_, NODE, k)
    be.set(W_, 0, np.ascontiguousarray(W0, np.float32))
    be.set(HT_, 0, np.ascontiguousarray(np.asarray(H0).T, np.float32))
    ms0 = be.cd_stats()["sweep_ms"]
    ratios, v0, n_iter, converged = [], 0.0, 0, False
    for n_iter in range(1, max_iter + 1):
      v = be.cd_sweep_fused(W_, 0, HT_, 0, be.gram(HT_, 0, k, HT_, 0, k))
      v += be.cd_sweep_fused(HT_, 0, W_, 0, be.gram(W_, 0, k, W_, 0, k))
      if n_iter == 1:
        v0 = v
      if v0 == 0:
        ratios.append(0.0)
        converged = True
        break
      ratios.append(v / v0)
      if v / v0 <= tol:
        converged = True
        break
    # |A - W H|_F^2 = nnz - 2 tr(W^T (A H^T)) + sum(W^T W o H H^T)
    be.spmm(BN_, 0, HT_, 0, k)
    cross = np.trace(be.gram(W_, 0, k, BN_, 0, k))
    wh = (be.gram(W_, 0, k, W_, 0, k) * be.gram(HT_, 0, k, HT_, 0, k)).sum()
    err = float(np.sqrt(max(inc.nnz - 2.0 * cross + wh, 0.0)))
    W = be.get(W_, 0, k)
    H = np.ascontiguousarray(be.get(HT_, 0, k).T)
    sweep_ms = be.cd_stats()["sweep_ms"] - ms0
    stats = be.stats()
  finally:
    if own:
      be.close()
  if not converged:
    warnings.warn("nmf_incidence: maximum number of iterations %d reached; "
                  "increase max_iter or tol" % max_iter, RuntimeWarning,
                  stacklevel=2)
  info = {"n_iter": n_iter, "converged": converged, "violation": ratios,
          "violation_init": v0, "reconstruction_err": err, "tol": tol,
          "sweep_ms": sweep_ms, "stats": stats, "init": init}
  return W, H, info


def EmbedNMF(hypergraph, dimension, *, tol=1e-4, max_iter=200, init="nndsvda",
             ctx=None, backend_factory=None):
  """embedding.py:143-162: node vector = row of W, edge vector = column of H
  of ``NMF(dimension)`` of the incidence matrix, keyed by the original ids.
  The reference compresses the id range first (``CompressRange``), which is
  the matrix of the compressed ``Incidence`` (also accepted as input).
  ``backend_factory`` (a callable: Incidence -> backend object, e.g.
  ``svd.NumpyBackend``) replaces the device."""
  inc = (hypergraph if isinstance(hypergraph, Incidence)
         else Incidence.from_hypergraph(hypergraph))
  assert dimension < inc.N
  assert dimension < inc.E
  assert dimension > 0
  from .algebraic_distance import coords_to_embedding
  W, H, _ = nmf_incidence(inc, dimension, init=init, tol=tol,
                          max_iter=max_iter, ctx=ctx,
                          backend=(backend_factory(inc) if backend_factory
                                   else None))
  return coords_to_embedding(inc, W, H.T, dimension, "NMF")


__all__ = ["nmf_incidence", "EmbedNMF", "nndsvd_init"]
