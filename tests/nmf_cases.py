"""Inputs and checks shared by test_nmf_driver_cpu.py (numpy backend) and
test_gpu_nmf.py (device): nmf_incidence against sklearn.decomposition.NMF in
float64 on the dense matrix, and the operands of the sweep parity tests."""

import functools
import warnings

import numpy as np

import svd_cases
from hypergraphembedding_amd import synthetic
from hypergraphembedding_amd.hypergraph_util import Incidence

# name -> (incidence builder, k). planted4 is the one case where the stop
# test fires (8 iterations); the other two run all 200.
CASES = {
    "planted4": (lambda: svd_cases.planted_hypergraph(600, 150, 4), 4),
    "planted8": (svd_cases.planted_hypergraph, 8),
    "random70": (lambda: synthetic.random_hypergraph(400, 300, 5, seed=0), 70),
}
INITS = ("nndsvda", "nndsvd")
# Factors against sklearn's float64 solve from the same start, relative to
# max(W_sk, H_sk): 6 x the largest deviation measured for fp32 panels with
# float64 arithmetic (1.7e-6) when the solver was specified.
FACTOR_TOL = 1e-5
ERR_TOL = 1e-6


@functools.lru_cache(maxsize=None)
def case(name):
  """(incidence, k, A dense float64)."""
  build, k = CASES[name]
  inc = build()
  return inc, k, inc.to_scipy()[0].astype(np.float64).toarray()


def _sklearn_nmf(k, **kw):
  from sklearn.decomposition import NMF
  return NMF(k, **kw)


@functools.lru_cache(maxsize=None)
def custom_reference(name, init):
  """sklearn's own start for ``init`` (W0, H0) and its float64 solve from it:
  (W0, H0, W_sk, H_sk, n_iter, reconstruction_err)."""
  from sklearn.decomposition._nmf import _initialize_nmf
  _, k, a = case(name)
  W0, H0 = _initialize_nmf(a, k, init=init, random_state=0)
  m = _sklearn_nmf(k, init="custom")
  with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    W = m.fit_transform(a, W=W0.copy(), H=H0.copy())
  for x in (W0, H0, W, m.components_):
    x.setflags(write=False)
  return W0, H0, W, m.components_, m.n_iter_, m.reconstruction_err_


@functools.lru_cache(maxsize=None)
def default_reference(name):
  """reconstruction_err_ of NMF(k) under np.random.seed(0..4)."""
  _, k, a = case(name)
  errs = []
  state = np.random.get_state()
  try:
    for seed in range(5):
      np.random.seed(seed)
      m = _sklearn_nmf(k)
      with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(a)
      errs.append(m.reconstruction_err_)
  finally:
    np.random.set_state(state)
  return tuple(errs)


def check_custom(name, init, solve, out=print):
  """``solve(inc, k, **kw) -> (W, H, info)`` from sklearn's start against
  sklearn's solve. Returns the measured figures."""
  inc, k, _ = case(name)
  W0, H0, Wr, Hr, n_iter, err = custom_reference(name, init)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)
    W, H, info = solve(inc, k, init="custom", W0=W0, H0=H0)
  assert W.shape == (inc.N, k) and H.shape == (k, inc.E)
  assert W.dtype == H.dtype == np.float32
  scale = max(Wr.max(), Hr.max())
  dw = np.abs(W - Wr).max() / scale
  dh = np.abs(H - Hr).max() / scale
  de = abs(info["reconstruction_err"] - err) / err
  out(f"{name}/{init}: n_iter {info['n_iter']} (sklearn {n_iter}), "
      f"|dW| {dw:.3e} |dH| {dh:.3e} of max(W, H), err {de:.3e} relative, "
      f"last ratios {info['violation'][-2:]}")
  assert info["n_iter"] == n_iter
  assert info["converged"] == (n_iter < 200)
  assert dw <= FACTOR_TOL and dh <= FACTOR_TOL
  assert de <= ERR_TOL
  assert (W >= 0).all() and (H >= 0).all()
  return dw, dh, de


def dense_err(a, W, H):
  return float(np.linalg.norm(a - W.astype(np.float64) @ H.astype(np.float64)))


def check_default(name, embed, out=print):
  """``embed(inc, k) -> HypergraphEmbedding`` (EmbedNMF, nndsvda from the
  converged SVD): its reconstruction error lies in sklearn's seed-to-seed
  range widened by that range (or 1e-6 relative) on either side."""
  inc, k, a = case(name)
  errs = default_reference(name)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)
    np.random.seed(0)
    emb = embed(inc, k)
  W = np.array([emb.node[int(i)].values for i in inc.node_ids], np.float32)
  H = np.array([emb.edge[int(j)].values for j in inc.edge_ids], np.float32).T
  err = dense_err(a, W, H)
  lo, hi = min(errs), max(errs)
  m = max(hi - lo, 1e-6 * hi)
  out(f"{name}: err {err:.9g}, sklearn seeds 0..4 [{lo:.9g}, {hi:.9g}]")
  assert lo - m <= err <= hi + m


def check_embed_nmf(embed, nmf, hg):
  """EmbedNMF on youtube_tiny: keys, dim, method name, vectors = rows of W
  and columns of H of nmf_incidence, and the reference's assertions."""
  import pytest
  inc = Incidence.from_hypergraph(hg)
  with warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)
    np.random.seed(5)
    emb = embed(hg, 6, max_iter=20)
    np.random.seed(5)
    W, H, _ = nmf(inc, 6, max_iter=20)
  assert emb.dim == 6 and emb.method_name == "NMF"
  assert set(emb.node) == set(hg.node) and set(emb.edge) == set(hg.edge)
  for i, idx in enumerate(inc.node_ids):
    assert np.array_equal(np.float32(emb.node[int(idx)].values), W[i])
  for j, idx in enumerate(inc.edge_ids):
    assert np.array_equal(np.float32(emb.edge[int(idx)].values), H[:, j])
  for bad in (0, len(hg.edge), len(hg.edge) + 5):
    with pytest.raises(AssertionError):
      embed(hg, bad)


# ---- sweep parity operands ---------------------------------------------------
PCOL0, BCOL0 = 4, 8  # the column views inside wider panels


def star_incidence(n_nodes, n_edges):
  """Every node in edge (node mod n_edges): any row counts, E = 1 included."""
  return Incidence(n_nodes, n_edges, np.arange(n_nodes + 1),
                   np.arange(n_nodes) % n_edges)


def sweep_operands(rows, k, seed, zero_diag=None):
  """(P, B, Q): Q the float64 Gram of a random non-negative k-column matrix
  (comparable diagonals), P >= 0 in fp32 with about 30% exact zeros, B = P Q
  plus a perturbation of the size of its entries, so that updates are both
  clamped and free and g takes both signs at the zero entries. ``zero_diag``
  zeroes that row and column of Q."""
  rng = np.random.default_rng(seed)
  M = rng.random((max(2 * k, 8), k))
  Q = M.T @ M
  if zero_diag is not None:
    Q[zero_diag, :] = 0.0
    Q[:, zero_diag] = 0.0
  P = rng.random((rows, k)).astype(np.float32)
  P[rng.random((rows, k)) < 0.3] = 0.0
  PQ = P.astype(np.float64) @ Q
  B = (PQ + rng.standard_normal((rows, k)) * PQ.std()).astype(np.float32)
  return P, B, Q


@functools.lru_cache(maxsize=None)
def sweep_case(rows, k, zero_diag=None):
  """Operands and the stated result: (P, B, Q, P after the sweep, violation)."""
  P, B, Q = sweep_operands(rows, k, seed=1000 * k + rows, zero_diag=zero_diag)
  want, viol = sweep_fresh(P, B, Q)
  for x in (P, B, Q, want):
    x.setflags(write=False)
  return P, B, Q, want, viol


def sweep_fresh(P, B, Q):
  """The sweep as stated (a fresh dot per coordinate), rows vectorised."""
  W, B = P.astype(np.float64), B.astype(np.float64)
  viol = 0.0
  for t in range(Q.shape[0]):
    g = W @ Q[t] - B[:, t]
    viol += np.abs(np.where(W[:, t] == 0, np.minimum(g, 0), g)).sum()
    if Q[t, t] != 0:
      W[:, t] = np.maximum(W[:, t] - g / Q[t, t], 0).astype(np.float32)
  return W.astype(np.float32), viol


def sweep_rank1(P, B, Q):
  """The same sweep with the gradient kept up to date by rank-1 updates (the
  device kernel's form): another summation order, the same arithmetic."""
  W, g = P.astype(np.float64), -B.astype(np.float64)
  k = Q.shape[0]
  for t in range(k):
    g += W[:, t:t + 1] * Q[:, t]
  viol = 0.0
  for t in range(k):
    gt, pt = g[:, t].copy(), W[:, t].copy()
    viol += np.abs(np.where(pt == 0, np.minimum(gt, 0), gt)).sum()
    if Q[t, t] != 0:
      W[:, t] = np.maximum(pt - gt / Q[t, t], 0).astype(np.float32)
      g += (W[:, t] - pt)[:, None] * Q[:, t]
  return W.astype(np.float32), viol
