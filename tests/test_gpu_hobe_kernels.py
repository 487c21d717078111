"""GPU: every data-dependent branch of hgx_hobe.hip against the float64
reference, the derived float32 bound, the oracle and the exact max / min
composition of hobe_cases.py, on the planted graph and under every input set
(k = 1 ... 257; [0, 1), [-1, 1), [100, 101); the exact-zero set).

Which branch a pair takes is established on the CPU (test_hobe_cases_cpu.py:
the restated predicate, asserted per labelled pair and input set), not read
from the device. Here every pair list goes to the device in one call, so a
four-wave workgroup holds pairs of different branches side by side, and the
result must equal

  * the composition of the DEVICE's own weights, bit for bit (a branch that
    drops or adds a shared target shows here whatever the weights are);
  * the oracle, bit for bit (the arithmetic of the weights: numpy's norm, the
    tail loop below k = 32 and the blocked kernel from 32 on);
  * the float64 reference within the derived bound (what the oracle and the
    device could share by mistake).

Every check against the reference is |device - reference| <= bound
elementwise; a NaN never passes. The bound is derived in hobe_cases.py, not
measured here. Each test prints one RATIO line: the worst |device -
reference| / bound it met. The lines of one MI355X run are kept in
profiles/hobe/gpu_test_ratios.txt; they are records, not bars.

Not covered, and why:
  * the grid-stride loop of hobe_weight_kernel: the grid is capped at 65,536
    workgroups of 256 incidences, so a second trip needs more than 16.7M
    incidences;
  * the records path of get_pair (pairs read from the sampler's records):
    the sampler tests (test_gpu_samplers.py) exercise it against the oracle.
"""

import numpy as np
import pytest
# before libhgx loads, so that both use one HIP runtime (torch brings its own)
import torch  # noqa: F401

import hobe_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

KINDS = (C.NN, C.EE, C.NE)
_REF = {}


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  c.upload(C.graph())
  yield c
  c.close()


def _sets(k):
  """The input sets of one k: the three distributions, and zero4 at k = 4."""
  return [(d, k) for d in C.DISTS] + ([C.ZERO4] if k == 4 else [])


def _reference(dist, k):
  """Inputs, the oracle's weights, the float64 weights and their bound;
  computed once per module and left unchanged."""
  if (dist, k) not in _REF:
    inc = C.graph()
    x, y = C.inputs(inc, dist, k)
    w64, rel = C.ref_weights(inc, x, y)
    _REF[dist, k] = dict(x=x, y=y, wo=O.hobe_weights(inc, x, y), w64=w64,
                         bw=C.weight_bound(k, w64, rel), probs={})
  return _REF[dist, k]


def _ref_probs(dist, k, kind):
  r = _reference(dist, k)
  if kind not in r["probs"]:
    inc = C.graph()
    a, b, _ = C.pair_arrays(inc, kind)
    r["probs"][kind] = (C.ref_probs(inc, r["w64"], kind, a, b),
                        C.prob_bound(inc, r["bw"], kind, a, b),
                        O.hobe_probs(kind, a, b, inc, r["x"], r["y"]))
  return r["probs"][kind]


class Worst:
  """Checks against the bound and keeps the worst err / bound of a test."""

  def __init__(self, name):
    self.name, self.ratio, self.where = name, 0.0, None

  def check(self, got, want, b, where):
    assert got.shape == want.shape, where
    assert np.isfinite(got).all(), where
    r = np.abs(got.astype(np.float64) - want) / b
    if r.size and r.max() > self.ratio:
      self.ratio, self.where = float(r.max()), where
    assert np.all(r <= 1.0), (where, float(r.max()))

  def report(self):
    print(f"\nRATIO {self.name}: worst err/bound {self.ratio:.3f} at {self.where}")


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check_weights(ctx, w, dist, k, tag=""):
  inc = C.graph()
  r = _reference(dist, k)
  ctx.alg_set(r["x"], r["y"])
  wn, we = ctx.incidence_weights(2)
  where = (dist, k, tag)
  w.check(wn, r["w64"], r["bw"], where + ("node-major",))
  w.check(we, r["w64"][inc.t_order], r["bw"][inc.t_order], where + ("edge-major",))
  # one weight per incidence serves both orientations
  assert np.array_equal(_bits(we), _bits(wn[inc.t_order])), where
  assert np.array_equal(_bits(wn), _bits(r["wo"])), where
  return wn, we


@pytest.mark.parametrize("k", C.KS)
def test_weights(ctx, k):
  """hobe_weight_kernel, both instantiations (k < 32: the tail loop; k >= 32:
  norm32), both orientations."""
  w = Worst(f"weights k={k}")
  for dist, k_ in _sets(k):
    wn, we = _check_weights(ctx, w, dist, k_)
    if dist == "zero4":
      e = C.graph().edge["ZERO"]
      z = we[C.graph().rp_e[e]:C.graph().rp_e[e + 1]]
      assert np.all(_bits(z) == 0)  # exactly +0
  w.report()


def test_weights_row_width_tuning(ctx):
  """k = 10 in rows of 16 and 20 floats (the alg_ks tuning changes KS, the
  stride of the coordinate rows the weight kernel reads)."""
  w = Worst("weights alg_ks")
  try:
    for ks in (16, 20):
      ctx.set_tuning("alg_ks", ks)
      for dist in C.DISTS:
        _check_weights(ctx, w, dist, 10, f"alg_ks={ks}")
  finally:
    ctx.set_tuning("alg_ks", 0)
  w.report()


@pytest.mark.parametrize("k", C.KS)
def test_row_maxima(ctx, k):
  """hw_self through hobe_probs(1, e, e) for every edge: max(0, max of the
  device's edge-major weights of e), bit for bit: whole waves in one row
  (wave reduction), waves over several rows and the ragged last wave (lane
  atomics), rows whose weights are all negative or all +0."""
  inc = C.graph()
  ids = np.arange(inc.E, dtype=np.int32)
  for dist, k_ in _sets(k):
    r = _reference(dist, k_)
    ctx.alg_set(r["x"], r["y"])
    _, we = ctx.incidence_weights(2)
    got = ctx.hobe_probs(C.EE, ids, ids)
    assert np.array_equal(_bits(got), _bits(C.self_from(inc, we))), (dist, k_)
    far = inc.edge["FAR"]
    assert _bits(got)[far] == 0 and we[inc.rp_e[far]:inc.rp_e[far + 1]].max() < 0
    if dist == "zero4":
      assert _bits(got)[inc.edge["ZERO"]] == 0


@pytest.mark.parametrize("k", C.KS)
def test_probabilities(ctx, k):
  """nn / ee / ne of the labelled pair lists, each list in one call."""
  inc = C.graph()
  w = Worst(f"probabilities k={k}")
  for dist, k_ in _sets(k):
    r = _reference(dist, k_)
    ctx.alg_set(r["x"], r["y"])
    wn, we = ctx.incidence_weights(2)
    for kind in KINDS:
      a, b, lab = C.pair_arrays(inc, kind)
      want, bound, orc = _ref_probs(dist, k_, kind)
      got = ctx.hobe_probs(kind, a, b)
      where = (dist, k_, ("nn", "ee", "ne")[kind])
      comp = C.probs_from_weights(inc, wn, we, kind, a, b)
      bad = np.flatnonzero(_bits(got) != _bits(comp))
      assert bad.size == 0, (where, [(lab[q], got[q], comp[q]) for q in bad[:5]])
      bad = np.flatnonzero(_bits(got) != _bits(orc))
      assert bad.size == 0, (where, [(lab[q], got[q], orc[q]) for q in bad[:5]])
      w.check(got, want, bound, where)
      nothing = np.array([l.endswith("_nothing") for l in lab])
      assert nothing.any() and np.all(_bits(got)[nothing] == 0), where
      assert np.array_equal(_bits(ctx.hobe_probs(kind, a, b)), _bits(got)), where
  w.report()


@pytest.mark.parametrize("dist,k", [("u01", 10), ("sym", 33), C.ZERO4],
                         ids=lambda v: str(v))
def test_partial_workgroups(ctx, dist, k):
  """The same lists as calls of one pair and of five: a workgroup of four
  waves with one or three idle (wave kernel), a block of 256 lanes with one
  or five live (nn kernel)."""
  inc = C.graph()
  r = _reference(dist, k)
  ctx.alg_set(r["x"], r["y"])
  for kind in KINDS:
    a, b, lab = C.pair_arrays(inc, kind)
    whole = ctx.hobe_probs(kind, a, b)
    assert np.array_equal(_bits(whole), _bits(_ref_probs(dist, k, kind)[2]))
    for n in (1, 5):
      got = np.concatenate([ctx.hobe_probs(kind, a[q:q + n], b[q:q + n])
                            for q in range(0, len(a), n)])
      assert np.array_equal(_bits(got), _bits(whole)), (kind, n)
