"""CPU: the weighted-Jaccard cases are what they claim (jaccard_cases.py):
every planted size, degree and support exists, every labelled pair takes its
branch and every label of REQUIRED_BRANCHES is reached by some case and
range (decided by the restated branch selection, not by the oracle); the
oracle agrees with the float64 reference within the derived bound and has
the exact properties on every case; every wrong variant of the reference
moves every member of the class it is aimed at by at least twice the bound
or changes the support; and the oracle still equals the reference's own
outputs (tests/golden/jaccard_small.npz), on which the float64 reference is
within the bound too.

The variant condition is a condition on the CASES: a variant that moves
nothing is a failure of the cases.
"""

import numpy as np
import pytest

import jaccard_cases as C
import oracle as O
from conftest import golden

N_RANDOM = 400
ALL = C.CASES + ("fill_big",)
_REF = {}


def _ref(name, rng):
  """(inc, fn, fe, Reference); built once and left unchanged."""
  if (name, rng) not in _REF:
    inc = C.case(name)
    fn, fe = C.features(inc, rng)
    _REF[name, rng] = (inc, fn, fe, C.Reference(inc, fn, fe))
  return _REF[name, rng]


def test_cases_are_as_stated():
  for name in ALL + (C.LARGE,):
    inc = C.case(name)
    for rp, col in ((inc.rp_n, inc.col_n), (inc.rp_e, inc.col_e)):
      row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
      assert np.all(np.diff(col.astype(np.int64))[row[1:] == row[:-1]] > 0), name
  inc = C.case("planted")
  deg, size = inc.node_degree(), inc.edge_size()
  assert (inc.N, inc.E) == (2400, 20) and inc.N > 2048 and inc.E < 1024
  assert size[0] == 0 and size[1] == 1
  assert [size[e] for e in (2, 3, 4, 5)] == [255, 256, 257, 600]
  assert deg[list(C.PLANTED_EMPTY)].tolist() == [0, 0]
  assert deg[C.PLANTED_HUB] == 4 and deg[33] == 1 and deg[100] == 2
  for e, first in inc.first_private.items():
    assert deg[first] == 1 and inc.col_n[inc.rp_n[first]] == e
  inc = C.case("c8192")
  assert (inc.N, inc.E) == (C.PASS_COLS + 1, C.PASS_COLS)
  inc = C.case("c3pass")
  assert inc.N >= 2 * C.PASS_COLS + 1
  assert inc.col_e[inc.rp_e[0]:inc.rp_e[1]].tolist() == [10, 5000, 16385, 16389]
  assert inc.node_degree()[[10, 5000, 16385, 16389]].tolist() == [1] * 4
  inc = C.case("rows70k")
  assert inc.N > 65536 and inc.node_degree().max() <= 2
  inc = C.case(C.LARGE)
  assert inc.N == C.N_SHRINK and C.workgroups(inc.N) == 512
  assert C.workgroups(inc.E) == 1024  # only the node side shrinks
  assert inc.node_degree().max() <= 2 and inc.edge_size().max() <= 2
  # the scratch of the shrunk launch: about 1 GB
  assert 0.9e9 < 512 * (4 * inc.N + 4 * -(-inc.N // 32)) < 1.1e9
  inc = C.case("fill_big")
  a, at = inc.to_scipy()
  nn_rows = np.diff((a.astype(np.int32) @ at.astype(np.int32)).tocsr().indptr)
  assert np.minimum(nn_rows, 1000).sum() > C.FILL_LOOP
  assert C.PAIRS_LOOP > 4096 * 256


def _pair_branches(inc, ref, kind, a, b, fn, fe):
  """The labels one pair reaches (restated swj; the kind-2 labels)."""
  if kind in (C.NN, C.EE):
    f = fn if kind == C.NN else fe
    ra = C.row_of(inc, kind, a, fn, fe)
    rb = C.row_of(inc, kind, b, fn, fe)
    rp = inc.rp_n if kind == C.NN else inc.rp_e
    seen, p32 = C.swj_branches(ra[0], f[rp[a]:rp[a + 1]], rb[0], f[rp[b]:rp[b + 1]])
    return seen, p32
  cen = lambda w, r: (ref.cen[w][1][ref.cen[w][0][r]:ref.cen[w][0][r + 1]],
                      ref.cen[w][2][ref.cen[w][0][r]:ref.cen[w][0][r + 1]])
  s1, _ = C.swj_branches(*C.row_of(inc, 0, a, fn, fe), *cen(1, b))
  s2, _ = C.swj_branches(*C.row_of(inc, 1, b, fn, fe), *cen(0, a))
  seen = s1 | s2
  ev = inc.col_n[inc.rp_n[a]:inc.rp_n[a + 1]]
  empty = (ref.cen[0][0][a + 1] == ref.cen[0][0][a]
           or ref.cen[1][0][b + 1] == ref.cen[1][0][b])
  seen.add("ne_empty_centroid" if empty else
           "ne_node_in_edge" if b in ev else "ne_node_not_in_edge")
  return seen, None


def test_every_required_branch_is_reached():
  reached = set()
  for name in ALL + (C.LARGE,):
    for rng in C.RANGES if name != C.LARGE else ("small",):
      inc, fn, fe, ref = _ref(name, rng)
      for w in (0, 1):
        reached |= C.centroid_branches(inc, w, fn, fe, ref.cen[w])
      for kind in (C.NN, C.EE, C.NE):
        a, b, lab = C.labelled_pairs(inc, kind)
        for i, j, l in zip(a, b, lab):
          seen, p32 = _pair_branches(inc, ref, kind, int(i), int(j), fn, fe)
          reached |= seen
          if rng != "ones" or l not in C.NEEDS_VALUES:
            assert l in seen, (name, rng, kind, int(i), int(j), l, seen)
      if name == C.LARGE:
        del _REF[name, rng]
  assert set(C.REQUIRED_BRANCHES) <= reached, set(C.REQUIRED_BRANCHES) - reached
  # the planted rows, one by one ("small": zeros are planted)
  inc, fn, fe, ref = _ref("planted", "small")
  p, j, v = ref.cen[0]
  row = lambda r: j[p[r]:p[r + 1]].tolist()
  assert row(10) == []                                  # degree 0
  r33 = row(33)                                         # degree 1, edge 6
  assert 39 in r33 and 42 in r33 and 40 not in r33 and 41 not in r33
  assert not set(range(64, 96)) & set(r33) and 100 in r33
  r100 = row(100)                                       # degree 2, edges 6 and 7
  assert 40 not in r100 and not set(range(64, 96)) & set(r100) and 42 in r100
  assert len(row(C.PLANTED_HUB)) > 1200                 # four long feature rows
  pe, je, _ = ref.cen[1]
  assert je[pe[0]:pe[1]].tolist() == [] and je[pe[1]:pe[2]].tolist() == [1, 8, 10]
  inc, fn, fe, ref = _ref("c3pass", "big")
  p, j, _ = ref.cen[0]
  assert j[p[10]:p[11]].tolist() == [10, 5000, 16385, 16389]
  assert j[p[100]:p[101]].tolist() == [100, 2148, 4196, 6244]
  inc, fn, fe, ref = _ref("c8192", "ones")
  p, j, _ = ref.cen[0]
  assert j[p[1] - 1] == 8192 and j[p[1] - 2] < 8192  # alone in the second pass


def _check_centroids(inc, fn, fe, ref, where):
  worst, ones = 0.0, 0
  for w in (0, 1):
    p, j, v = O.centroids(*C.centroid_args(inc, w, fn, fe))
    rp_, rj, rv = ref.cen[w]
    C.check_support(p, j, rp_, rj, where + (w,))
    r = np.abs(v.astype(np.float64) - rv) / C.centroid_bound(inc, w, rp_, rv)
    assert np.all(r <= 1), (where, w, r.max())
    worst = max(worst, float(r.max()) if r.size else 0.0)
    ones += C.check_degree_one(inc, w, p, j, v, fn, fe, where)
  assert ones > 0, where  # every case has degree-1 rows
  return worst


@pytest.mark.parametrize("name", ALL)
def test_oracle_is_within_the_bound_of_the_reference(name, capsys):
  worst = (0.0, None)
  for rng in C.RANGES:
    inc, fn, fe, ref = _ref(name, rng)
    where = (name, rng)
    worst = max(worst, (_check_centroids(inc, fn, fe, ref, where), where + ("centroid",)))
    for kind in (C.NN, C.EE, C.NE):
      a, b, lab = C.pair_arrays(inc, kind, N_RANDOM)
      got = O.jaccard_probs(kind, a, b, inc, fn, fe)
      want, bound = ref.bound(kind, a, b)
      assert np.isfinite(got).all()
      err = np.abs(got.astype(np.float64) - want)
      assert np.all(err <= bound), (where, kind, (err / np.maximum(bound, 1e-300)).max())
      r = err[bound > 0] / bound[bound > 0]
      if r.size:
        worst = max(worst, (float(r.max()), where + (kind,)))
      # the vectorised reference is the plain one
      nl = len(C.labelled_pairs(inc, kind)[0]) + 20
      for q in range(nl):
        one = C.pair_prob64(inc, ref, kind, int(a[q]), int(b[q]), fn, fe)
        assert abs(one - want[q]) <= 1e-14 * max(one, 1e-300), (where, kind, q)
      # exact properties
      for s in (8.0, 0.125):
        scaled = O.jaccard_probs(kind, a, b, inc, fn * np.float32(s), fe * np.float32(s))
        C.check_scale_invariant(got, scaled, where + (kind, s))
      if kind != C.NE:
        C.check_symmetric(got, O.jaccard_probs(kind, b, a, inc, fn, fe), where + (kind,))
        ids = np.arange(inc.N if kind == C.NN else inc.E, dtype=np.int32)
        same = O.jaccard_probs(kind, ids, ids, inc, fn, fe)
        assert C.check_same_is_one(inc, kind, ids, ids, same, fn, fe, where) == ids.size
        # the restated float32 merge is the oracle's
        for q in range(len(C.labelled_pairs(inc, kind)[0])):
          _, p32 = _pair_branches(inc, ref, kind, int(a[q]), int(b[q]), fn, fe)
          assert C.bits(p32) == C.bits(got[q]), (where, kind, q)
  with capsys.disabled():
    print(f"\nworst |oracle - float64 reference| / bound, {name}: "
          f"{worst[0]:.3f} at {worst[1]}")


def test_oracle_centroids_on_the_large_case(capsys):
  inc, fn, fe, ref = _ref(C.LARGE, "small")
  worst = _check_centroids(inc, fn, fe, ref, (C.LARGE, "small"))
  del _REF[C.LARGE, "small"]
  with capsys.disabled():
    print(f"\nworst |oracle - float64 reference| / bound, {C.LARGE} centroids: {worst:.3f}")


def _labelled(inc, kind, labels):
  a, b, lab = C.labelled_pairs(inc, kind)
  sel = np.array([l in labels for l in lab])
  assert sel.any(), labels
  return a[sel], b[sel]


@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_every_wrong_variant_moves_its_class(variant):
  for rng in C.RANGES:
    inc, fn, fe, ref = _ref("planted", rng)
    if variant in ("by_contributors", "zero_kept"):
      for w in (0, 1):
        p, j, v = ref.cen[w]
        bp, bj, bv = C.ref_centroids(inc, w, fn, fe, variant)
        if variant == "zero_kept":
          if rng == "ones":      # no zeros: the variant is the reference
            assert np.array_equal(bp, p)
            continue
          rows = [r for l, (s, r) in inc.rows.items() if s == w and l in (
              "cen_deg1_node", "cen_zero_mean_many", "cen_deg1_edge")]
          assert rows
          for r in rows:         # the support of every targeted row changes
            assert bp[r + 1] - bp[r] > p[r + 1] - p[r], (rng, w, r)
        else:
          # same support; every entry with fewer contributors than the
          # row's degree moves by more than twice its bound
          assert np.array_equal(bp, p) and np.array_equal(bj, j)
          R, rp, col, frp, fcol, fval, ncols = C._side(inc, w, fn, fe)
          cand = C.ref_centroids(inc, w, np.ones_like(fn), np.ones_like(fe))
          assert np.array_equal(cand[0], C.candidates(inc, w, fn, fe)[0])
          key = lambda pp, jj: (np.repeat(np.arange(R, dtype=np.int64), np.diff(pp))
                                * ncols + jj)
          # contributors / degree of the kept entries
          share = cand[2][np.searchsorted(key(cand[0], cand[1]), key(p, j))]
          cls = share < 1 - 1e-12
          assert cls.sum() > 100
          moved = np.abs(bv - v) > 2 * C.centroid_bound(inc, w, p, v)
          assert np.all(moved[cls]) and not moved[~cls].any(), (rng, w)
      continue
    if variant == "wrong_side":
      bad = C.Reference(inc, fn, fe, wrong_side=True)
      a, b = _labelled(inc, C.NE, ("ne_node_in_edge", "ne_node_not_in_edge"))
      want, bound = ref.bound(C.NE, a, b)
      got, _ = bad.probs(C.NE, a, b)
      assert np.all(want > 0)
      assert np.all(np.abs(got - want) > 2 * bound), (rng, got, want)
      continue
    labels = (("swj_left_only", "swj_right_only") if variant == "intersection"
              else ("swj_tail_left", "swj_tail_right"))
    for kind in (C.NN, C.EE):
      a, b, lab = C.labelled_pairs(inc, kind)
      if not any(l in labels for l in lab):
        continue
      a, b = _labelled(inc, kind, labels)
      want, bound = ref.bound(kind, a, b)
      got = np.array([C.pair_prob64(inc, ref, kind, int(i), int(j), fn, fe, variant)
                      for i, j in zip(a, b)])
      assert np.all(want > 0)
      assert np.all(np.abs(got - want) > 2 * bound), (variant, rng, kind, got, want)


def test_oracle_and_reference_meet_on_the_golden_fixture(small_inc):
  """The oracle equals the real reference's outputs; the float64 reference
  is within the bound of them."""
  z = golden("jaccard_small.npz")
  inc = small_inc
  fn, fe = z["neigh_fn_v"], z["neigh_fe_v"]
  ref = C.Reference(inc, fn, fe)
  for w, name in ((0, "cn"), (1, "ce")):
    p, j, v = O.centroids(*C.centroid_args(inc, w, fn, fe))
    assert np.array_equal(p, z[name + "_p"]) and np.array_equal(j, z[name + "_j"])
    assert np.array_equal(v, z[name + "_v"])
    C.check_support(p, j, ref.cen[w][0], ref.cen[w][1], name)
    err = np.abs(z[name + "_v"].astype(np.float64) - ref.cen[w][2])
    assert np.all(err <= C.centroid_bound(inc, w, ref.cen[w][0], ref.cen[w][2]))
  for tag, f in (("uniform", (np.ones(inc.nnz, np.float32),) * 2), ("neigh", (fn, fe))):
    r = C.Reference(inc, *f)
    idx, tgt = z[tag + "_idx"], z[tag + "_tgt"]
    nn = (idx[:, 0] > 0) & (idx[:, 2] > 0)
    ee = (idx[:, 1] > 0) & (idx[:, 3] > 0)
    ne = (idx[:, 0] > 0) & (idx[:, 3] > 0) & (idx[:, 2] == 0)
    assert nn.sum() and ee.sum() and ne.sum()
    for kind, sel, lc, rc in ((C.NN, nn, 0, 2), (C.EE, ee, 1, 3), (C.NE, ne, 0, 3)):
      a, b = idx[sel, lc] - 1, idx[sel, rc] - 1
      assert np.array_equal(O.jaccard_probs(kind, a, b, inc, *f), tgt[sel, kind])
      want, bound = r.bound(kind, a, b)
      assert np.all(np.abs(tgt[sel, kind].astype(np.float64) - want) <= bound), (tag, kind)
