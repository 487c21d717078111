"""GPU: the node2vec engine (_hgx.N2v, csrc/hgx_n2v.hip): walks against the
host restatement and their law, the sequential trainer against the float64
reference (n2v_reference.py), the concurrent trainer's quality, and the two
embedders end to end.

Inputs, reference and bar are n2v_cases.py's: per case and table, E = the
larger of the two NumpyBackend summation orders' max-abs distances from the
float64 reference, computed here; the sequential device trainer must be
within 8 E + 2 ulp32(max |p|) elementwise on syn0 and syn1. Before the device
is touched the reference asserts that every evaluated |x| is at least 1e-3
away from 6 (n2v_cases.MARGIN).

Which case reaches which instantiation: n2v_train<NPL> holds NPL = 1, 2, 4
or 8 columns of a padded row per lane: d8, d64 and every d = 16 case NPL 1;
d65, d128 NPL 2; d200 NPL 4; d512 NPL 8.

Measured max |device - reference| / E on an MI355X (the bar is 8 plus the
ulp term):

  case                          syn0    syn1
  test_sequential_against_float64
    d8                          1.00    1.00
    d64                         1.00    1.00
    d65                         1.07    1.00
    d128                        1.00    1.00
    d200                        1.00    1.00
    d512                        1.00    1.00
    L3w1n5 L3w3n1 L3w9n5        1.00    1.00
    L7w1n1 L7w9n1 L7w3n1 L3w1n1 1.00    1.00
    L7w3n5                      0.81    1.00
    tiny_vocab                  0.93    0.96
    hub                         0.90    0.87
  test_max_exp_skip             0.70    1.00
  test_concurrent_quality
    sequential mode             1.09    1.05

A ratio of 1.00 is an element whose error is a rounding every float32
trainer shares (the update's own additions), not the dot product's order:
there the device and both host orders sit at the same distance.

Concurrent trainer on the planted graph (2400 walks, default geometry: 152
walks per launch): J_init = 4.152, float64 sequential J_seq = 1.667, device
J_dev = 1.682, a recovery of 0.994 of the reference's decrease (the test
asks for 0.5).
"""

import numpy as np
import pytest
import scipy.stats

import n2v_cases as K
import n2v_reference as R
from conftest import golden_incidence
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import node2vec as n2v

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
  c = _hgx.Context(0)
  yield c
  c.close()


# ---- walks -------------------------------------------------------------------
@pytest.fixture(scope="module")
def bip(ctx):
  return K.walk_graph()


@pytest.mark.parametrize("p", [1.0, 0.25])
@pytest.mark.parametrize("L", [1, 2, 3, 5, 7, n2v.MAX_WALK])
def test_bipartite_walks_equal_walk_row(ctx, bip, L, p):
  inc = bip
  ctx.upload(inc)
  V = inc.N + inc.E
  rs = np.random.RandomState(L)
  src = np.concatenate([rs.permutation(V) for _ in range(3)])
  ps = np.repeat(np.arange(3), V)
  with _hgx.N2v(ctx, n2v.BIPARTITE, 8) as be:
    w = be.walks(ps, src, L, p, 12345)
    assert w.shape == (3 * V, L) and 3 * V % 64
    want = np.array([n2v.walk_row(inc, int(s), int(q), L, p, 12345)
                     for q, s in zip(ps, src)], np.int32)
    assert np.array_equal(w, want)
    # a walk does not depend on the other entries of the call
    sub = np.array([5, 84, 60, 200, 254, 129, 17])
    assert np.array_equal(be.walks(ps[sub], src[sub], L, p, 12345), want[sub])
    assert np.array_equal(be.counts(), np.bincount(want[sub].ravel(),
                                                   minlength=V))


def test_walk_errors(ctx, bip):
  ctx.upload(bip)
  with _hgx.N2v(ctx, n2v.BIPARTITE, 8) as be:
    with pytest.raises(_hgx.HgxError):
      be.walks([0], [0], n2v.MAX_WALK + 1, 1.0, 1)
    with pytest.raises(ZeroDivisionError):
      be.walks([0], [0], 5, 0.0, 1)
    with pytest.raises(AssertionError):
      be.walks([0], [0], 5, 1.5, 1)
    with pytest.raises(AssertionError):
      be.walks([0], [bip.N + bip.E], 5, 1.0, 1)
    with pytest.raises(_hgx.HgxError):  # call order
      be.counts()
    with pytest.raises(_hgx.HgxError):
      be.train()
  with pytest.raises(_hgx.HgxError):
    _hgx.N2v(ctx, n2v.BIPARTITE, 513)


# expand_w: 0 every step by rejection, 2^20 every step by expansion, 70 both
# (a node of the big edge alone has 59 paths, the others up to 107, about
# half of them more than 70)
@pytest.mark.parametrize("expand_w", [0, 70, 1 << 20])
def test_clique_walks(ctx, expand_w):
  inc = K.clique_graph()
  nb = n2v.clique_neighbours(inc)
  ctx.upload(inc)
  ctx.set_tuning("n2v_expand_w", expand_w)
  try:
    with _hgx.N2v(ctx, n2v.CLIQUE, 8) as be:
      with pytest.raises(AssertionError):
        be.walks([0], [60], 5, 1.0, 1)   # not in the clique graph
      srcs = n2v.clique_sources(inc)
      ps = np.repeat(np.arange(6), srcs.size)
      w = be.walks(ps, np.tile(srcs, 6), 7, 0.25, 99)
      st = be.stats()
      assert st["expand_steps"] + st["reject_steps"] == w.shape[0] * 6
      if expand_w == 0:
        assert st["expand_steps"] == 0
      elif expand_w == 70:
        assert st["expand_steps"] > 0 and st["reject_steps"] > 0
      else:
        assert st["reject_steps"] == 0
      assert 60 not in w
      for a, b in zip(w[:, :-1].ravel(), w[:, 1:].ravel()):
        assert a != b and b in nb[a]
      # first step: uniform over the distinct neighbours, for a node that
      # shares three edges and more with another (1 ~ 2) and for a member of
      # the big edge alone (55)
      n = 6000
      for s in (1, 55):
        f = be.walks(np.arange(n), np.full(n, s), 2, 1.0, 7)[:, 1]
        assert set(f) <= set(nb[s])
        obs = np.array([(f == v).sum() for v in nb[s]])
        assert scipy.stats.chisquare(obs).pvalue > 1e-4, (s, obs)
      # p = 0.25: back with probability (1 / p) / (D - 1 + 1 / p)
      p = 0.25
      w3 = be.walks(np.arange(n), np.full(n, 1), 3, p, 8)
      D = np.array([len(nb[v]) for v in w3[:, 1]])
      pr = (1 / p) / (D - 1 + 1 / p)
      z = ((w3[:, 2] == 1).sum() - pr.sum()) / np.sqrt((pr * (1 - pr)).sum())
      assert abs(z) < 4.5, z  # two-sided 7e-6 under the law
  finally:
    ctx.set_tuning("n2v_expand_w", 256)


# ---- sequential trainer against float64 -------------------------------------
CASES = {**K.dims(), **K.windows(), "tiny_vocab": K.tiny_vocab, "hub": K.hub}


def device_run(ctx, c, concurrent=False):
  ctx.upload(c.inc)
  with _hgx.N2v(ctx, n2v.CLIQUE, c.d) as be:
    out = c.run_backend(be, concurrent=concurrent)
    st = be.stats()
  return out, st


@pytest.mark.parametrize("name", list(CASES))
def test_sequential_against_float64(ctx, name):
  c = CASES[name]()
  c.reference()  # the |x| margin, before the device is touched
  out, st = device_run(ctx, c)
  plan = c.plan()
  assert st["words"] == sum(nk for nk, _ in plan)
  assert st["pairs"] == sum(len(p) for _, p in plan)
  K.check(c, out, name)
  again, _ = device_run(ctx, c)
  assert all(np.array_equal(a, b) for a, b in zip(out, again))


def test_max_exp_skip(ctx):
  """Targets clearly above |x| = 6 are skipped: their rows stay bitwise."""
  c = K.skip_case()
  ref, _, _ = c.reference(margin=1.0)
  for conc in (False, True):
    out, _ = device_run(ctx, c, concurrent=conc)
    assert np.array_equal(out[1][c.skipped], c.syn1[c.skipped])
    moved = np.setdiff1d(np.arange(c.V), c.skipped)
    assert not np.array_equal(out[1][moved], c.syn1[moved])
    if not conc:
      K.check(c, out, "skip")


# ---- concurrent trainer --------------------------------------------------------
def test_concurrent_quality(ctx):
  """Default geometry on the planted graph: the concurrent trainer recovers
  at least half of the float64 sequential reference's decrease of the
  epoch-0 objective J, and ends finite; sequential mode at the same
  settings meets the float64 bar."""
  c = K.quality_case()
  ref, _, _ = c.reference()
  p0 = c.plan()[:len(c.walks)]
  j_init = R.objective(c.syn0, c.syn1, p0)
  j_seq = R.objective(ref.syn0, ref.syn1, p0)
  assert j_init - j_seq > 2.0, (j_init, j_seq)
  out, st = device_run(ctx, c, concurrent=True)
  assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
  assert st["walks"] == 2 * len(c.walks)
  assert st["pairs"] == sum(len(p) for _, p in c.plan())
  j_dev = R.objective(out[0], out[1], p0)
  rec = (j_init - j_dev) / (j_init - j_seq)
  print(f"QUALITY J_init {j_init:.3f} J_seq {j_seq:.3f} J_dev {j_dev:.3f} "
        f"recovery {rec:.3f}")
  assert j_init - j_dev >= 0.5 * (j_init - j_seq), (j_init, j_seq, j_dev)
  seq, _ = device_run(ctx, c)
  K.check(c, seq, "quality_seq")


# ---- end to end -------------------------------------------------------------------
def test_embedders_end_to_end(ctx):
  inc = golden_incidence("csr_small.npz")
  srcs = set(n2v.clique_sources(inc))
  for fn, tag in ((n2v.EmbedNode2VecBipartide, "BIPARTIDE"),
                  (n2v.EmbedNode2VecClique, "CLIQUE")):
    if tag == "BIPARTIDE" and (np.diff(inc.rp_n).min() == 0 or
                               np.diff(inc.rp_e).min() == 0):
      with pytest.raises(AssertionError):
        fn(inc, 8, ctx=ctx)
      continue
    out = []
    for _ in range(2):
      np.random.seed(3)
      out.append(fn(inc, 8, num_walks_per_node=2, walk_length=3,
                    run_in_parallel=False, ctx=ctx))
    e = out[0]
    assert e.SerializeToString() == out[1].SerializeToString()
    assert e.dim == 8 and e.method_name == f"N2V3_{tag}"
    assert sorted(e.node) == sorted(int(i) for i in inc.node_ids)
    assert sorted(e.edge) == sorted(int(i) for i in inc.edge_ids)
    x = np.array([e.node[int(i)].values for i in inc.node_ids], np.float32)
    y = np.array([e.edge[int(i)].values for i in inc.edge_ids], np.float32)
    assert x.shape == (inc.N, 8) and y.shape == (inc.E, 8)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
    if tag == "CLIQUE":
      for v in range(inc.N):
        assert (v in srcs) == bool(np.any(x[v])), v
      assert np.array_equal(y, n2v.edge_centroids(inc, x))
    else:
      assert np.all(np.any(x, axis=1)) and np.all(np.any(y, axis=1))
    # concurrent: finite, and trained away from the initial vectors
    np.random.seed(3)
    info = {}
    V = inc.N + inc.E if tag == "BIPARTIDE" else inc.N
    n_src = V if tag == "BIPARTIDE" else len(srcs)
    [np.random.permutation(n_src) for _ in range(2)]
    [np.random.randint(0, 2**31 - 1) for _ in range(2)]
    init = (np.random.random((V, 8)).astype(np.float32) - np.float32(0.5)) / 8
    np.random.seed(3)
    e2 = fn(inc, 8, num_walks_per_node=2, walk_length=3, ctx=ctx, info=info)
    x2 = np.array([e2.node[int(i)].values for i in inc.node_ids], np.float32)
    assert np.all(np.isfinite(x2))
    live = np.any(x2, axis=1)
    assert live.sum() == (inc.N if tag == "BIPARTIDE" else len(srcs))
    same = np.all(x2[live] == init[:inc.N][live], axis=1)
    assert same.sum() < live.sum() / 2, (same.sum(), live.sum())
    assert info["stats"]["pairs"] > 0
