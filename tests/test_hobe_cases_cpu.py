"""CPU: the HOBE cases are what they claim (hobe_cases.py): every planted
length, position, collision chain and wave class exists and every labelled
pair takes its branch under every input set; the float64 reference agrees
with the oracle within the derived bound; the exact composition equals the
oracle and the reference's golden vectors bit for bit; every wrong variant
moves a pair of the class it is aimed at; and the oracle's weight is numpy's
norm at every k.

The variant condition is a condition on the CASES, checked with the oracle's
float32 weights alone: a variant that moves nothing is a failure of the
cases. It is checked under every input set (the tail-loop variant from
k = 32 on): some pair of every class the variant is aimed at must move by
more than twice that pair's bound (the tail-loop variant: to a different
float32 value).
"""

import numpy as np
import pytest

import hobe_cases as C
import oracle as O
from conftest import golden, golden_incidence

G = C.graph
SETS = C.input_sets()
_W = {}


def _weights(dist, k):
  """(x, y, oracle weights node-major, float64 weights, D / sqrt(k)); once."""
  if (dist, k) not in _W:
    inc = G()
    x, y = C.inputs(inc, dist, k)
    _W[dist, k] = (x, y, O.hobe_weights(inc, x, y)) + C.ref_weights(inc, x, y)
  return _W[dist, k]


def test_graph_is_as_stated():
  inc = G()
  deg, size = inc.node_degree(), inc.edge_size()
  assert deg.min() >= 1 and size.min() >= 1  # hgx_alg_set refuses isolated rows
  assert inc.N <= 8000 and inc.E <= 4096 and inc.nnz <= 60000
  for rp, col in ((inc.rp_n, inc.col_n), (inc.rp_e, inc.col_e)):
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    assert np.all(np.diff(col.astype(np.int64))[row[1:] == row[:-1]] > 0)
  e, n = inc.edge, inc.node
  want = dict(E1=1, E2=2, E63=63, E64=64, E65=65, E255=255, W256=256, E257=257,
              S=300, S2=300, P=513, Q=513, L=600)
  for name, sz in want.items():
    assert size[e[name]] == sz, name
  assert set(want.values()) <= set(size.tolist())
  for name, d in dict(H255=255, H256=256, H257=257, H300=300, N16F=16, N16L=16,
                      N16M=16, N16X=16, N16U=16, N17=17, N1=1).items():
    assert deg[n[name]] == d, name
  assert {1, 2, 16, 17, 255, 256, 257, 300} <= set(deg.tolist())

  def members(name):
    return inc.col_e[inc.rp_e[e[name]]:inc.rp_e[e[name] + 1]]

  def edges(v):
    return inc.col_n[inc.rp_n[v]:inc.rp_n[v + 1]]

  # S and L: about 40 shared, at the planted positions of S's member list
  pos = np.flatnonzero(np.isin(members("S"), members("L")))
  assert pos.size == 40 and set(C.POS_SL) <= set(pos.tolist())
  assert C.POS_SL[-1] == size[e["S"]] - 1
  pos = np.flatnonzero(np.isin(members("S2"), members("L")))
  assert pos.size == 10 and 257 in pos
  pos = np.flatnonzero(np.isin(members("E257"), members("Q")))
  assert pos.tolist() == [256]
  pos = np.flatnonzero(np.isin(members("P"), members("Q")))
  assert pos.size == 40 and set(C.POS_PQ) <= set(pos.tolist())
  # members in 40 or more edges; the sought edge first, in the middle, last
  for v, sought, where in ((n["S_63"], e["L"], "last"), (n["S_64"], e["L"], "mid"),
                           (n["P_255"], e["P"], "first"),
                           (n["P_256"], e["Q"], "last")):
    ev = edges(v)
    assert ev.size >= 40
    at = int(np.flatnonzero(ev == sought)[0])
    assert {"first": at == 0, "last": at == ev.size - 1,
            "mid": ev.size // 4 < at < 3 * ev.size // 4}[where], (v, at)
  # the lockstep search of (Q, P) seeks P, of (S, L) seeks L
  assert C.ee_walk(inc, e["Q"], e["P"]) == (e["Q"], e["P"])
  assert C.ee_walk(inc, e["P"], e["Q"]) == (e["P"], e["Q"])
  assert C.ee_walk(inc, e["L"], e["S"]) == (e["S"], e["L"])
  # hash collisions of the hub of exactly 256 edges
  ev = edges(n["H256"])
  assert ev.size == C.NE_CAP == C.NE_HASH // 2
  assert set(C.CHAIN4) <= set(ev.tolist()) and set(C.WRAP) <= set(ev.tolist())
  assert {C.ne_slot(f) for f in C.CHAIN4} == {100} and len(C.CHAIN4) >= 4
  assert [C.ne_slot(f) for f in C.WRAP] == [510, 510, 511, 511, 511]
  where = C.hash_table(ev)
  assert sorted(where[f] for f in C.WRAP) == [0, 1, 2, 510, 511]  # wraps
  assert sorted(where[f] for f in C.CHAIN4) == [100, 101, 102, 103]
  assert where[C.WRAP[4]] < C.ne_slot(C.WRAP[4])
  assert where[C.CHAIN4[3]] != C.ne_slot(C.CHAIN4[3])
  # wave classes of the edge-major CSR (hobe_weight_kernel's two reductions)
  rp = inc.rp_e.astype(np.int64)
  assert rp[e["W256"]] == 0 and rp[e["W256"] + 1] == 256  # whole waves only
  rows, live = C.wave_classes(inc)
  assert np.all(rows[:4] == 1) and (rows >= 3).sum() >= 20
  crossing = (rp[:-1] % 64 != 0) & (rp[1:] > (rp[:-1] // 64 + 1) * 64)
  assert crossing.any() and crossing[e["L"]]
  # L: whole waves inside, partial waves at both ends
  assert rp[e["L"]] % 64 != 0 and rp[e["L"] + 1] % 64 != 0
  assert inc.nnz % 64 != 0 and not live[-1] and live[:-1].all()


def _self32(wo):
  inc = G()
  return C.self_from(inc, wo[inc.t_order])


def _winner_pos(inc, we, wn, a, b):
  """Position in the walked edge of the member that gives ee(a, b)."""
  te, tn, pos = inc._composer.ee_support(a, b)
  return int(pos[np.argmax(np.minimum(we[te], wn[tn]))]) if pos.size else -1


@pytest.mark.parametrize("dist,k", SETS, ids=lambda v: str(v))
def test_every_labelled_pair_takes_its_branch(dist, k):
  inc = G()
  x, y, wo, w64, rel = _weights(dist, k)
  we = wo[inc.t_order]
  self_w = _self32(wo)
  e = inc.edge
  assert self_w[e["FAR"]] == 0 and we[inc.rp_e[e["FAR"]]:inc.rp_e[e["FAR"] + 1]].max() < 0
  if dist == "zero4":
    z = we[inc.rp_e[e["ZERO"]]:inc.rp_e[e["ZERO"] + 1]]
    assert np.all(z == 0) and not np.signbit(z).any()
  ea, eb, u = inc.plants["equal"]
  assert np.array_equal(x[u], y[ea]) and np.array_equal(y[ea], y[eb])
  # nn
  a, b, lab = C.pair_arrays(inc, C.NN)
  p = C.probs_from_weights(inc, wo, we, C.NN, a, b)
  for i, j, l, v in zip(a, b, lab, p):
    if l.startswith("nn_probe"):
      assert C.nn_path(inc, i, j) == "probe" and v > 0, l
    elif l.startswith("nn_merge"):
      assert C.nn_path(inc, i, j) == "merge" and v > 0, l
    elif l == "nn_nothing":
      assert v == 0 and not np.intersect1d(
          inc.col_n[inc.rp_n[i]:inc.rp_n[i + 1]],
          inc.col_n[inc.rp_n[j]:inc.rp_n[j + 1]]).size
    if l in ("nn_probe_first", "nn_probe_last"):
      lo, hi = (i, j) if inc.node_degree()[i] < inc.node_degree()[j] else (j, i)
      sh = np.flatnonzero(np.isin(inc.col_n[inc.rp_n[hi]:inc.rp_n[hi + 1]],
                                  inc.col_n[inc.rp_n[lo]:inc.rp_n[lo + 1]]))
      want = 0 if l == "nn_probe_first" else inc.node_degree()[hi] - 1
      assert sh.tolist() == [want]
  d = inc.node_degree()
  ratio = {l: max(d[i], d[j]) / min(d[i], d[j]) for i, j, l in zip(a, b, lab)}
  assert 15 < ratio["nn_merge_under16"] < 16 == ratio["nn_merge_exact16"]
  assert 16 < ratio["nn_probe_over16"] < 16.1
  # ee
  a, b, lab = C.pair_arrays(inc, C.EE)
  p = C.probs_from_weights(inc, wo, we, C.EE, a, b)
  for i, j, l, v in zip(a, b, lab, p):
    i, j = int(i), int(j)
    steps = C.ee_steps(inc, i, j)
    bound = min(self_w[i], self_w[j])
    win = _winner_pos(inc, we, wo, i, j) if i != j else -1
    if l in ("ee_same", "ee_self"):
      assert i == j and v == self_w[i]
    elif l == "ee_zero_bound":
      assert bound == 0 and v == 0 and win >= 0  # members are shared
    elif l == "ee_one_step":
      assert steps == 1 and 0 < v <= bound
    elif l == "ee_two_steps":
      assert steps == 2 and 0 < v <= bound
      assert win == C.POS_SL[C.sl_winner(dist, k)]
    elif l == "ee_winner_last_step":
      assert steps == 2 and win == 257 and 0 < v <= bound
    elif l == "ee_257_second_step":
      assert C.ee_walk(inc, i, j)[0] == e["E257"] and steps == 2
      assert win == 256 == inc.edge_size()[e["E257"]] - 1 and 0 < v <= bound
    elif l == "ee_equal_sizes":
      assert inc.edge_size()[i] == inc.edge_size()[j] and steps == 3
      if C.ee_walk(inc, i, j)[0] == e["P"]:
        assert win == 512
      assert 0 < v <= bound
    elif l == "ee_bound_first_step":
      assert v == bound == 1 and 0 <= win < C.EE_STEP
    elif l == "ee_nothing":
      assert win == -1 and v == 0
    elif l == "ee_zero_edge" and dist == "zero4":
      assert bound == 0 and win >= 0
  # ne
  a, b, lab = C.pair_arrays(inc, C.NE)
  p = C.probs_from_weights(inc, wo, we, C.NE, a, b)
  want = dict(ne_b0=0, ne_b0_member=0, ne_b1_chain=1, ne_b1_wrap=1,
              ne_b1_deg256=1, ne_b1_chain2=1, ne_b2_deg257_last=2,
              ne_b2_member=2, ne_b3_deg257=3, ne_b3_deg256=3,
              ne_b3_two_steps=3, ne_b3_member=3,
              ne_zero_edge=0 if dist == "zero4" else 3)
  seen = set()
  for i, j, l, v in zip(a, b, lab, p):
    i, j = int(i), int(j)
    br = C.ne_branch(inc, self_w, i, j)
    seen.add(br)
    ev = inc.col_n[inc.rp_n[i]:inc.rp_n[i + 1]]
    if l in want:
      assert br == want[l], (l, br)
      assert (v > 0) == (br != 0), l
    if l in ("ne_b0_member", "ne_b2_member", "ne_b3_member", "ne_zero_edge"):
      assert j in ev  # v is a member of e
    if l in ("ne_b2_member", "ne_b3_member"):
      assert v == self_w[j]
    if l == "ne_b3_two_steps":
      assert max(C.ee_steps(inc, j, int(f)) for f in ev) == 2
      assert int(ev[-1]) == e["FAR"]  # the last ee returns early: bound 0 < p
    if l == "ne_nothing":
      assert v == 0 and br != 0
      assert not np.isin(inc.col_n[np.isin(inc.row_n, inc.col_e[
          inc.rp_e[j]:inc.rp_e[j + 1]])], ev).any()
  assert seen == {0, 1, 2, 3}
  deg_of = {l: d[i] for i, l in zip(a, lab)}
  assert deg_of["ne_b1_deg256"] == 256 and deg_of["ne_b2_deg257_last"] == 257
  assert deg_of["ne_b3_deg256"] == 256 and deg_of["ne_b3_deg257"] == 257


def test_reference_is_within_the_bound_of_the_oracle(capsys):
  """The float64 reference against O.hobe_weights, hgref_dist_weight and
  O.hobe_probs under every input set, elementwise: the reference alone stays
  inside the bar."""
  inc = G()
  lib = O.lib()
  worst = (0.0, None)
  rng = np.random.default_rng(1)
  for dist, k in SETS:
    x, y, wo, w64, rel = _weights(dist, k)
    bw = C.weight_bound(k, w64, rel)
    r = np.abs(wo.astype(np.float64) - w64) / bw
    assert np.all(r <= 1), (dist, k, r.max())
    worst = max(worst, (float(r.max()), (dist, k, "weight")))
    for t in rng.integers(inc.nnz, size=40):
      got = lib.hgref_dist_weight(x[inc.row_n[t]].copy(), y[inc.col_n[t]].copy(), k)
      assert np.float32(got) == wo[t]
    for kind in (C.NN, C.EE, C.NE):
      a, b, _ = C.pair_arrays(inc, kind)
      want = C.ref_probs(inc, w64, kind, a, b)
      got = O.hobe_probs(kind, a, b, inc, x, y)
      r = np.abs(got.astype(np.float64) - want) / C.prob_bound(inc, bw, kind, a, b)
      assert np.all(r <= 1), (dist, k, kind, r.max())
      worst = max(worst, (float(r.max()), (dist, k, kind)))
  with capsys.disabled():
    print(f"\nworst |oracle - float64 reference| / bound: {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("dist,k", SETS, ids=lambda v: str(v))
def test_composition_equals_the_oracle(dist, k):
  inc = G()
  x, y, wo, _, _ = _weights(dist, k)
  for kind in (C.NN, C.EE, C.NE):
    a, b, _ = C.pair_arrays(inc, kind)
    got = C.probs_from_weights(inc, wo, wo[inc.t_order], kind, a, b)
    want = O.hobe_probs(kind, a, b, inc, x, y)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), kind


def test_composition_equals_the_golden_vectors():
  z = golden("probs_tiny.npz")
  c = golden("algdist_tiny.npz")
  inc = C.prep(golden_incidence("csr_tiny.npz"))
  wo = O.hobe_weights(inc, c["x_20"], c["y_20"])
  for kind, key in ((C.NN, "nn"), (C.EE, "ee"), (C.NE, "ne")):
    got = C.probs_from_weights(inc, wo, wo[inc.t_order], kind, z[f"{key}_a"],
                               z[f"{key}_b"])
    assert np.array_equal(got, z[f"{key}_p"]), key


@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_every_wrong_variant_moves_its_class(variant):
  inc = G()
  for dist, k in SETS:
    if variant == "tail_norm" and k < 32:
      continue
    x, y, wo, w64, rel = _weights(dist, k)
    we = wo[inc.t_order]
    bw = C.weight_bound(k, w64, rel)
    for kind, label in C.VARIANTS[variant]:
      a, b, lab = C.pair_arrays(inc, kind)
      sel = np.array([l == label for l in lab])
      a, b = a[sel], b[sel]
      good = C.probs_from_weights(inc, wo, we, kind, a, b)
      bad = C.probs_from_weights(inc, wo, we, kind, a, b, variant, (x, y))
      if variant == "tail_norm":  # a different float32 value
        assert np.any(good != bad), (variant, dist, k)
      else:
        big = np.abs(good.astype(np.float64) - bad) > 2 * C.prob_bound(
            inc, bw, kind, a, b)
        assert big.any(), (variant, dist, k, kind, label)


def test_tail_loop_is_numpys_norm_only_below_32():
  """What the fix is about, on the cases' own incidences: from k = 32 on the
  tail loop differs from the oracle (numpy's blocked norm) in some weight; up
  to 31 in none."""
  inc = G()
  for dist, k in SETS:
    x, y, wo, _, _ = _weights(dist, k)
    same = np.array_equal(C.tail_loop_weights(inc, x, y), wo)
    assert same == (k < 32), (dist, k)


def test_oracle_weight_is_norm32_at_every_k():
  """hgref_dist_weight = (md - hgref_norm32(...)) / md at every k; at k < 32
  that is the old tail-loop formula, restated in float32 numpy."""
  inc = G()
  lib = O.lib()
  rng = np.random.default_rng(2)
  f = np.float32
  for dist, k in SETS:
    x, y, wo, _, _ = _weights(dist, k)
    md = f(np.sqrt(float(k)))
    for t in rng.integers(inc.nnz, size=60):
      a, b = x[inc.row_n[t]].copy(), y[inc.col_n[t]].copy()
      nrm = f(lib.hgref_norm32(a, b, k, 0))
      assert f((md - nrm) / md) == f(lib.hgref_dist_weight(a, b, k)) == wo[t]
