"""svd_incidence and EmbedSvd through the device (csrc/hgx_spmm.hip): the
checks of test_svd_driver_cpu.py against scipy.sparse.linalg.svds in float64
(tests/svd_cases.py has the inputs and the derived bounds)."""

import numpy as np
import pytest

import svd_cases as C
from hypergraphembedding_amd import EmbedSvd, _hgx, svd_incidence

pytestmark = pytest.mark.gpu


def solve(inc, k, seed=11, **kw):
  np.random.seed(seed)
  return svd_incidence(inc, k, **kw)


@pytest.fixture(scope="module", params=list(C.CASES))
def solved(request):
  inc, k = C.case(request.param)[:2]
  return request.param, inc, k, solve(inc, k, tol=C.TOL)


def test_against_scipy(solved):
  name, _, _, (U, s, Vt, info) = solved
  C.check_against_scipy(name, U, s, Vt, C.TOL)
  assert info["converged"] and info["residuals"].max() <= C.TOL
  assert info["stats"]["spmm_calls"] >= info["products"]


def test_default_tolerance(solved):
  name, inc, k, _ = solved
  U, s, Vt, info = solve(inc, k)
  C.check_against_scipy(name, U, s, Vt, info["tol"])


def test_reproducible(solved):
  _, inc, k, (U, s, Vt, _) = solved
  U2, s2, Vt2, _ = solve(inc, k, tol=C.TOL)
  assert np.array_equal(U, U2) and np.array_equal(s, s2)
  assert np.array_equal(Vt, Vt2)


def test_rank_deficient():
  U, s, Vt, _ = solve(C.rank2_incidence(), 3)
  C.check_rank_deficient(U, s, Vt)
  C.check_sign(Vt)


def test_no_convergence_raises():
  inc, k = C.case("random")[:2]
  with pytest.raises(_hgx.HgxError) as ei:
    solve(inc, k, tol=1e-9, max_restarts=2)
  assert ei.value.info["restarts"] == 2


def test_embed_svd(tiny_hypergraph):
  C.check_embed_svd(EmbedSvd, svd_incidence, tiny_hypergraph)
