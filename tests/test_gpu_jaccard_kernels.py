"""GPU: every data-dependent branch of hgx_jaccard.hip against the oracle
(bit for bit), the float64 reference of jaccard_cases.py (within the derived
float32 bound, elementwise) and the exact properties (support, symmetry,
power-of-two rescaling, a == b), on the planted cases and under the three
feature ranges (all ones; [0.01, 1) and [1, 1000) with stored zeros).

Which branch a row or a pair takes is established on the CPU
(test_jaccard_cases_cpu.py: the restated selection, asserted per label and
for REQUIRED_BRANCHES as a whole), not read from the device. Which case
reaches what:

  case      reaches
  small     degree 0 / 1 / many on both sides; the record fill (jac_fill) of
            every kind at K = 1, 5, 16 with each block empty in turn; one
            jac_pairs call of 1,048,876 pairs (its grid stride); the
            rebuild after a second features_set; the state after upload;
            the numpy-seeded sampler's fill.
  planted   every swj branch by label (left-only, right-only, x < y, x > y,
            x == y, both tails, one / both operands empty, all stored values
            zero, a == b, disjoint, a stored zero against a value); feature
            rows of 255, 256, 257 and 600 entries (the z += 256 loop); 20
            columns (one partial bitmap word) and 20 rows (fewer than the
            1024 workgroups) on the edge side; 2400 rows on the node side (a
            workgroup reuses its accumulator and bitmap for a third row);
            zero-mean columns between kept ones of one word, a whole word
            of them; centroid rows of up to 1365 entries (compact_rows'
            stride of 64); kind 2 with an empty centroid row, a node in the
            edge, a node not in it.
  c8192     8192 columns (one compaction pass, 256 words exactly) and 8193
            (two; the second holds the last column alone); kept columns in
            all four waves of a pass.
  c3pass    16,390 columns (three passes, s_base carried twice); kept
            columns in passes 1 and 3 only; the last kept column the last.
  rows70k   70,001 rows: compact_rows' grid stride beyond 65,536; nine
            passes.
  shrink    473,485 columns: build_centroids halves its workgroups to 512
            (own Context, closed afterwards: about 1 GB of scratch);
            centroids and 3000 pairs per kind.
  fill_big  a node-node block of 1.1M records: jac_fill's grid stride and
            its 64-bit i * R.

Every check against the reference is |device - reference| <= bound
elementwise; where the reference is 0 the device must be exactly 0; a NaN
never passes. The bound is derived in jaccard_cases.py, not measured here.
Each test prints RATIO lines: the worst |device - reference| / bound per
case and kind. The lines of one MI355X run are kept in
profiles/jaccard/gpu_test_ratios.txt; they are records, not bars.

Not asserted here: which pairs the sampler draws (test_gpu_sampler_kernels.py
restates that exactly).
"""

import numpy as np
import pytest
# before libhgx loads, so that both use one HIP runtime (torch brings its own)
import torch  # noqa: F401

import jaccard_cases as C
import oracle as O

pytestmark = pytest.mark.gpu

KINDS = (C.NN, C.EE, C.NE)
KIND_NAME = ("nn", "ee", "ne")
N_RANDOM = 3000
_REF = {}


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.close()


def _reference(name, rng):
  """Features, the float64 reference, the oracle's centroids and (on demand)
  the pair lists with both references; computed once and left unchanged."""
  if (name, rng) not in _REF:
    inc = C.case(name)
    fn, fe = C.features(inc, rng)
    _REF[name, rng] = dict(
        inc=inc, fn=fn, fe=fe, ref=C.Reference(inc, fn, fe), pairs={},
        cen=[O.centroids(*C.centroid_args(inc, w, fn, fe)) for w in (0, 1)])
  return _REF[name, rng]


def _pairs(name, rng, kind):
  r = _reference(name, rng)
  if kind not in r["pairs"]:
    a, b, lab = C.pair_arrays(r["inc"], kind, N_RANDOM)
    want, bound = r["ref"].bound(kind, a, b)
    r["pairs"][kind] = (a, b, lab, want, bound,
                        O.jaccard_probs(kind, a, b, r["inc"], r["fn"], r["fe"]))
  return r["pairs"][kind]


class Worst:
  """Checks against the bound and keeps the worst err / bound per key."""

  def __init__(self):
    self.worst, self.count = {}, {}

  def check(self, key, got, want, bound, where):
    assert got.shape == want.shape, where
    assert np.isfinite(got).all(), where
    err = np.abs(got.astype(np.float64) - want)
    nz = bound > 0
    assert np.all(err[~nz] == 0), (where, "not exactly 0 where the reference is")
    r = err[nz] / bound[nz]
    top = float(r.max()) if r.size else 0.0
    self.worst[key] = max(self.worst.get(key, 0.0), top)
    self.count[key] = self.count.get(key, 0) + got.size
    assert np.all(r <= 1.0), (where, top)

  def report(self):
    for key in sorted(self.worst):
      print(f"\nRATIO {key}: worst err/bound {self.worst[key]:.3f} "
            f"over {self.count[key]} values")


def _same(got, want, where):
  bad = np.flatnonzero(C.bits(got) != C.bits(want))
  assert bad.size == 0, (where, bad[:5], got[bad[:5]], want[bad[:5]])


def _check_centroids(ctx, w, key, r, where):
  inc, fn, fe, ref = r["inc"], r["fn"], r["fe"], r["ref"]
  for which in (0, 1):
    p, j, v = ctx.jaccard_centroids(which)
    op, oj, ov = r["cen"][which]
    assert np.array_equal(p, op) and np.array_equal(j, oj), where + (which,)
    _same(v, ov, where + (which,))
    rp_, rj, rv = ref.cen[which]
    C.check_support(p, j, rp_, rj, where + (which,))
    w.check(key, v, rv, C.centroid_bound(inc, which, rp_, rv), where + (which,))
    C.check_degree_one(inc, which, p, j, v, fn, fe, where + (which,))
    p2, j2, v2 = ctx.jaccard_centroids(which)
    assert np.array_equal(p2, p) and np.array_equal(j2, j), where
    _same(v2, v, where + (which, "second call"))


@pytest.mark.parametrize("name", C.CASES)
def test_centroids(ctx, name):
  """build_centroids (centroid_caps, centroid_rows, compact_rows), both
  sides, every range."""
  w = Worst()
  ctx.upload(C.case(name))
  for rng in C.RANGES:
    r = _reference(name, rng)
    ctx.features_set(r["fn"], r["fe"])
    _check_centroids(ctx, w, f"centroids {name}", r, (name, rng))
  w.report()


@pytest.mark.parametrize("name", C.CASES)
def test_probabilities(ctx, name):
  """jac_pairs of the labelled pairs and N_RANDOM random ones per kind."""
  w = Worst()
  inc = C.case(name)
  ctx.upload(inc)
  for rng in C.RANGES:
    r = _reference(name, rng)
    fn, fe = r["fn"], r["fe"]
    ctx.features_set(fn, fe)
    got = {}
    # kinds 0 and 1 before any centroid is built, then kind 2, then again
    for kind in (C.NN, C.EE, C.NE, C.NN, C.EE):
      a, b, lab, want, bound, orc = _pairs(name, rng, kind)
      p = ctx.jaccard_probs(kind, a, b)
      where = (name, rng, KIND_NAME[kind])
      if kind in got:
        _same(p, got[kind], where + ("after the centroids",))
        continue
      got[kind] = p
      bad = np.flatnonzero(C.bits(p) != C.bits(orc))
      assert bad.size == 0, (where, [(lab[q], p[q], orc[q]) for q in bad[:5]])
      w.check(f"probabilities {name} {KIND_NAME[kind]}", p, want, bound, where)
      if kind != C.NE:
        C.check_symmetric(p, ctx.jaccard_probs(kind, b, a), where)
        C.check_same_is_one(inc, kind, a, b, p, fn, fe, where)
    for s in (8.0, 0.125):
      ctx.features_set(fn * np.float32(s), fe * np.float32(s))
      for kind in KINDS:
        a, b = _pairs(name, rng, kind)[:2]
        C.check_scale_invariant(got[kind], ctx.jaccard_probs(kind, a, b),
                                (name, rng, KIND_NAME[kind], s))
  w.report()


def test_pairs_grid_stride(ctx):
  """One call of 1,048,576 + 300 pairs per kind (jac_pairs loops), drawn
  with replacement on the small case; the references on the distinct pairs."""
  w = Worst()
  name, rng = "small", "small"
  r = _reference(name, rng)
  inc = r["inc"]
  ctx.upload(inc)
  ctx.features_set(r["fn"], r["fe"])
  gen = np.random.default_rng(51)
  for kind in KINDS:
    na = inc.E if kind == C.EE else inc.N
    nb = inc.N if kind == C.NN else inc.E
    a = gen.integers(0, na, C.PAIRS_LOOP).astype(np.int32)
    b = gen.integers(0, nb, C.PAIRS_LOOP).astype(np.int32)
    got = ctx.jaccard_probs(kind, a, b)
    uniq, inv = np.unique(a.astype(np.int64) * nb + b, return_inverse=True)
    ua, ub = (uniq // nb).astype(np.int32), (uniq % nb).astype(np.int32)
    where = (name, rng, KIND_NAME[kind], "grid stride")
    _same(got, O.jaccard_probs(kind, ua, ub, inc, r["fn"], r["fe"])[inv], where)
    want, bound = r["ref"].bound(kind, ua, ub)
    w.check(f"pairs grid stride {KIND_NAME[kind]}", got, want[inv], bound[inv], where)
  w.report()


def test_state(ctx):
  """A second features_set on the same upload gives that set's centroids
  and kind-2 probabilities; a new upload forgets the features."""
  from hypergraphembedding_amd._hgx import HgxError
  w = Worst()
  name = "small"
  inc = C.case(name)
  ctx.upload(inc)
  first = None
  for rng in ("small", "big", "small"):
    r = _reference(name, rng)
    ctx.features_set(r["fn"], r["fe"])
    _check_centroids(ctx, w, "state centroids", r, (name, rng, "state"))
    a, b, lab, want, bound, orc = _pairs(name, rng, C.NE)
    p = ctx.jaccard_probs(C.NE, a, b)
    _same(p, orc, (name, rng, "state"))
    w.check("state ne", p, want, bound, (name, rng, "state"))
    if first is None:
      first = p
    elif rng == "big":
      assert np.any(C.bits(p) != C.bits(first))  # the sets do differ
    else:
      _same(p, first, (name, rng, "the first set again"))
  ctx.upload(inc)
  a, b = _pairs(name, "small", C.NE)[:2]
  for kind in KINDS:
    with pytest.raises(HgxError):
      ctx.jaccard_probs(kind, a[:4], b[:4])
  with pytest.raises(HgxError):
    ctx.jaccard_centroids(0)
  r = _reference(name, "small")
  ctx.features_set(r["fn"], r["fe"])
  _same(ctx.jaccard_probs(C.NE, a, b), first, (name, "after the new upload"))
  w.report()


def _check_records(ctx, w, key, r, n, K, where):
  """Every record's own tgt column against the oracle (bit for bit) and the
  float64 reference for the device's own pair; the other two exactly 0.
  Returns the three block sizes."""
  inc, fn, fe = r["inc"], r["fn"], r["fe"]
  idx, tgt = ctx.records_get()
  blk = ctx.records_blocks()
  assert idx.shape == (n, 4 + 2 * K) and blk.size == 5 and blk[4] == n, where
  sizes = []
  for kind, lo, hi, lc, rc in ((C.NN, blk[0], blk[1], 0, 2),
                               (C.EE, blk[1], blk[2], 1, 3),
                               (C.NE, blk[2], blk[4], 0, 3)):
    a, b = idx[lo:hi, lc] - 1, idx[lo:hi, rc] - 1
    sizes.append(int(hi - lo))
    assert np.all(a >= 0) and np.all(b >= 0), where
    got = np.ascontiguousarray(tgt[lo:hi, kind])
    kw = where + (KIND_NAME[kind],)
    _same(got, O.jaccard_probs(kind, a, b, inc, fn, fe), kw)
    want, bound = r["ref"].bound(kind, a, b)
    w.check(f"{key} {KIND_NAME[kind]}", got, want, bound, kw)
    rest = np.ascontiguousarray(np.delete(tgt[lo:hi], kind, axis=1))
    assert np.all(C.bits(rest) == 0), kw
  return sizes


@pytest.mark.parametrize("K", [1, 5, 16])
def test_record_fill(ctx, K):
  """jac_fill through sample_jaccard: all three blocks, then each empty in
  turn (no node quota: no nn block; no edge quota: no ee block; quotas on
  rows without neighbours only: no record at all, the only way the
  sampler's rules leave the node-edge block empty)."""
  w = Worst()
  name, rng = "small", "big"
  r = _reference(name, rng)
  inc = r["inc"]
  ctx.upload(inc)
  ctx.features_set(r["fn"], r["fe"])
  zn, ze = np.zeros(inc.N, np.int32), np.zeros(inc.E, np.int32)
  lone_n = (inc.node_degree() == 0).astype(np.int32) * 3
  lone_e = (inc.edge_size() == 0).astype(np.int32) * 3
  assert lone_n.any() and lone_e.any()
  seen = []
  for tag, nq, eq in (("all", zn + 3, ze + 3), ("no nn", zn, ze + 3),
                      ("no ee", zn + 3, ze), ("none", lone_n, lone_e)):
    n = ctx.sample_jaccard(17 + K, K, nq, eq)
    sizes = _check_records(ctx, w, f"record fill K={K}", r, n, K, (name, rng, K, tag))
    seen.append([s > 0 for s in sizes])
  assert seen == [[True, True, True], [False, True, True], [True, False, True],
                  [False, False, False]]
  w.report()


def test_record_fill_grid_stride(ctx):
  """A node-node block above 1,048,576 records: jac_fill loops."""
  w = Worst()
  name, rng = "fill_big", "small"
  r = _reference(name, rng)
  inc = r["inc"]
  ctx.upload(inc)
  ctx.features_set(r["fn"], r["fe"])
  n = ctx.sample_jaccard(5, 1, np.full(inc.N, 1000, np.int32),
                         np.zeros(inc.E, np.int32))
  sizes = _check_records(ctx, w, "record fill grid stride", r, n, 1, (name, rng))
  assert sizes[0] > C.FILL_LOOP and sizes[1] == 0 and sizes[2] > 0
  w.report()


def test_numpy_seeded_path(ctx):
  """sample_jaccard_mt (hgx_mt.hip's stream, the same jac_fill) on the small
  case with stored zeros."""
  w = Worst()
  name, rng = "small", "small"
  r = _reference(name, rng)
  inc = r["inc"]
  assert (r["fn"] == 0).any() and (r["fe"] == 0).any()
  ctx.upload(inc)
  ctx.features_set(r["fn"], r["fe"])
  np.random.seed(9)
  n = ctx.sample_jaccard_mt(2, np.full(inc.N, 3, np.int32), np.full(inc.E, 3, np.int32))
  sizes = _check_records(ctx, w, "numpy-seeded fill", r, n, 2, (name, rng, "mt"))
  assert all(s > 0 for s in sizes)
  w.report()


def test_large_case_workgroup_shrink():
  """473,485 columns: the node side runs on 512 workgroups. Centroids and
  N_RANDOM pairs per kind, on a Context of its own."""
  from hypergraphembedding_amd import _hgx
  w = Worst()
  name, rng = C.LARGE, "small"
  inc = C.case(name)
  assert C.workgroups(inc.N) < 1024
  r = _reference(name, rng)
  c = _hgx.Context(0)
  try:
    c.upload(inc)
    c.features_set(r["fn"], r["fe"])
    _check_centroids(c, w, f"centroids {name}", r, (name, rng))
    for kind in KINDS:
      a, b, lab, want, bound, orc = _pairs(name, rng, kind)
      p = c.jaccard_probs(kind, a, b)
      _same(p, orc, (name, rng, KIND_NAME[kind]))
      w.check(f"probabilities {name} {KIND_NAME[kind]}", p, want, bound,
              (name, rng, KIND_NAME[kind]))
  finally:
    c.close()
    del _REF[name, rng]
  w.report()
