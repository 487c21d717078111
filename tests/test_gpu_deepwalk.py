"""GPU: the DeepWalk trainer (_hgx.N2v.set_tree / train_hs, n2v_train_hs of
csrc/hgx_n2v.hip): the sequential trainer against the float64 reference
(dw_reference.py), the concurrent kernel with one walk per launch at the
sequential bar, a lossless-ness bound across workgroups, the |x| >= 6 skip,
the concurrent trainer's quality, the errors and the embedder end to end.

Inputs, reference and bar are dw_cases.py's: per case and table, E = the
larger of the two NumpyBackendHS summation orders' max-abs distances from the
float64 reference, computed here; the device must be within 8 E + 2
ulp32(max |p|) elementwise on syn0 and syn1. Before the device is touched the
reference asserts that every evaluated |x| is at least 1e-3 away from 6.

Which case reaches which instantiation: n2v_train_hs<NPL> holds NPL = 1, 2, 4
or 8 columns of a padded row per lane: d8, d64 and every d = 16 case NPL 1;
d65, d128 NPL 2; d200 NPL 4; d512 NPL 8.

Measured max |device - reference| / E on an MI355X (the bar is 8 plus the
ulp term):

  case                          syn0    syn1
  test_sequential_against_float64
    d8                          1.00    1.00
    d64                         1.00    1.04
    d65                         1.00    1.00
    d128                        1.02    1.00
    d200 d512                   1.00    1.00
    L3w1 L7w3                   1.00    1.00
    L3w9                        1.00    0.90
    L7w1                        1.00    0.95
    L7w9                        0.93    1.08
    chain64_d16                 1.00    1.00
    chain64_d128                0.82    1.00
    tiny3                       1.10    1.00
    two                         1.00    0.79
    hub zero_count              1.00    1.00
  test_one_walk_per_launch_meets_the_sequential_bar (dw_hot_levels 0, 1, 3, 6)
    d16                         0.90 1.10 0.95 0.83   0.91 0.82 0.70 0.21
    d200                        0.91 0.85 0.94 0.94   1.00 0.48 0.35 0.21
  test_max_exp_skip             1.00    1.00

A ratio of 1.00 is an element whose error is a rounding every float32
trainer shares. The hot rows' sums are kept apart from the row and added to
it once, so syn1's error falls as more levels are hot.

test_nothing_lost_across_workgroups: D = 2.59e-3; staleness emulation (a)
4.07e-6 = 1.57e-3 D, loss emulation (b) 4.90e-4 = 0.189 D, device 3.33e-6 =
1.29e-3 D at dw_hot_levels 6 and 4.02e-6 = 1.55e-3 D at 0 (the bound is
sqrt((a)(b)) = 4.46e-5 = 1.7e-2 D).

test_concurrent_quality (2400 walks of 3, window 2, 152 walks per launch):
J_init = 6.447, float64 sequential J_seq = 4.473, device J_dev = 4.526, a
recovery of 0.974 of the reference's decrease (the test asks for 0.5).

test_quality_settings_sequential_against_float64: margin 0.42 (the largest
|x| is 5.58), ratio 1.24 (syn0) and 1.00 (syn1). The corpus is sized by the
margin, see dw_cases.quality_case: with walks of 5 and window 3 the float64
trajectory crosses |x| = 6 and comes within 1.5e-4 of it.
"""

import numpy as np
import pytest

import dw_cases as C
import dw_reference as R
from conftest import golden_incidence
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import deepwalk as dw
from hypergraphembedding_amd import node2vec as n2v

pytestmark = pytest.mark.gpu

HOT_DEFAULT = 6  # dw_hot_levels as a context starts (include/hgx.h)


@pytest.fixture(scope="module")
def ctx():
  c = _hgx.Context(0)
  yield c
  c.close()


def device_run(ctx, c, concurrent=False):
  ctx.upload(c.inc)
  with _hgx.N2v(ctx, n2v.CLIQUE, c.d) as be:
    out = c.run_backend(be, concurrent=concurrent)
    st = be.stats()
  return out, st


def check_counts(c, st):
  plan = c.plan()
  assert st["words"] == sum(nk for nk, _ in plan)
  assert st["pairs"] == sum(len(p) for _, p in plan)
  assert st["path_nodes"] == sum(c.path_lengths())
  assert st["walks"] == len(plan)


# ---- 1. sequential trainer against float64 ----------------------------------
CASES = {**C.dims(), **C.windows(),
         "chain64_d16": lambda: C.chain64(16),
         "chain64_d128": lambda: C.chain64(128),
         "tiny3": C.tiny3, "two": C.two, "hub": C.hub,
         "zero_count": C.zero_count}


@pytest.mark.parametrize("name", list(CASES))
def test_sequential_against_float64(ctx, name):
  c = CASES[name]()
  c.reference()  # the |x| margin, before the device is touched
  out, st = device_run(ctx, c)
  check_counts(c, st)
  C.check(c, out, name)
  again, _ = device_run(ctx, c)
  assert all(np.array_equal(a, b) for a, b in zip(out, again))
  if name == "zero_count":
    assert np.array_equal(out[0][c.absent], c.syn0[c.absent])


# ---- 2. the concurrent kernel, one walk per launch ---------------------------
@pytest.mark.parametrize("hot", [0, 1, 3, HOT_DEFAULT])
@pytest.mark.parametrize("d", [16, 200])
def test_one_walk_per_launch_meets_the_sequential_bar(ctx, d, hot):
  """n_walks = 1: every concurrent launch holds one wave, so the concurrent
  kernel (global atomics, and the LDS sums of the hot rows with their flush)
  is deterministic and is held to the sequential bar."""
  c = C.long1(d)
  c.reference()
  assert sum(len(p) for _, p in c.plan()) > 3000
  ctx.set_tuning("dw_hot_levels", hot)
  try:
    out, st = device_run(ctx, c, concurrent=True)
    again, _ = device_run(ctx, c, concurrent=True)
  finally:
    ctx.set_tuning("dw_hot_levels", HOT_DEFAULT)
  check_counts(c, st)
  C.check(c, out, f"long1_d{d}_hot{hot}")
  assert all(np.array_equal(a, b) for a, b in zip(out, again))


# ---- 3. nothing lost across workgroups ----------------------------------------
@pytest.fixture(scope="module")
def lossless():
  """The case, its float64 reference and the two host emulations' distances
  from it on syn1: (a) every walk of a launch reads the launch's start tables
  plus its own updates (staleness), (b) the same with the root-row updates of
  one workgroup's four walks dropped in every launch (loss)."""
  c = C.lossless_case()
  ref, _, _ = c.reference()
  root = int(c.tree[1][0])
  assert np.all(c.tree[1][c.tree[0][:-1]] == root)
  args = (c.syn0, c.syn1, c.plan(), c.tree, float(c.alpha), float(c.min_alpha),
          len(c.walks), 64)
  a = np.abs(R.launch_emulation(*args)[1] - ref.syn1).max()
  b = np.abs(R.launch_emulation(*args, drop=(range(4, 8), root))[1] -
             ref.syn1).max()
  D = np.abs(ref.syn1 - c.syn1.astype(np.float64)).max()
  return c, ref, a, b, D


@pytest.mark.parametrize("hot", [HOT_DEFAULT, 0])
def test_nothing_lost_across_workgroups(ctx, lossless, hot):
  """One launch of 16 workgroups per epoch. The device's distance from the
  sequential float64 reference must stay below the geometric mean of the
  staleness error (a) and of the error (b) of losing one workgroup's updates
  to the root row, with (b) >= 10 (a) asserted."""
  c, ref, a, b, D = lossless
  assert b >= 10 * a, (a, b)
  ctx.set_tuning("dw_hot_levels", hot)
  try:
    out, st = device_run(ctx, c, concurrent=True)
  finally:
    ctx.set_tuning("dw_hot_levels", HOT_DEFAULT)
  check_counts(c, st)
  err = np.abs(out[1].astype(np.float64) - ref.syn1).max()
  print(f"LOSSLESS hot {hot}: D {D:.3g} staleness (a) {a:.3g} = {a / D:.3g} D "
        f"loss (b) {b:.3g} = {b / D:.3g} D device {err:.3g} = {err / D:.3g} D")
  assert err <= np.sqrt(a * b), (err, a, b)


# ---- 4. skip ----------------------------------------------------------------------
def test_max_exp_skip(ctx):
  """Inner nodes clearly above |x| = 6 are skipped: their rows stay bitwise,
  in both modes, while the other nodes of the same paths move."""
  c = C.skip_case()
  c.reference(margin=1.0)
  for conc in (False, True):
    out, _ = device_run(ctx, c, concurrent=conc)
    assert np.array_equal(out[1][c.skipped], c.syn1[c.skipped])
    assert not np.any(np.all(out[1][c.moved] == c.syn1[c.moved], axis=1))
    if not conc:
      C.check(c, out, "skip")


# ---- 5. concurrent quality ----------------------------------------------------------
@pytest.fixture(scope="module")
def quality():
  """The case and its float64 sequential trajectory, the |x| margin asserted
  as for every case (dw_cases.quality_case sizes the corpus by it)."""
  c = C.quality_case()
  ref, _, _ = c.reference()
  return c, ref


def test_concurrent_quality(ctx, quality):
  """Default geometry on the planted graph: the concurrent trainer recovers
  at least half of the float64 sequential reference's decrease of the
  epoch-0 mean hierarchical-softmax loss J, and ends finite."""
  c, ref = quality
  p0 = c.plan()[:len(c.walks)]
  j_init = R.objective(c.syn0, c.syn1, p0, c.tree)
  j_seq = R.objective(ref.syn0, ref.syn1, p0, c.tree)
  # the reference itself must learn: of the 6.4 nats of a 9-node path at
  # x = 0 (9 log 2 = 6.2) at least one, or the recovery is a quotient of noise
  assert j_init - j_seq > 1.0, (j_init, j_seq)
  out, st = device_run(ctx, c, concurrent=True)
  assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
  check_counts(c, st)
  j_dev = R.objective(out[0], out[1], p0, c.tree)
  rec = (j_init - j_dev) / (j_init - j_seq)
  print(f"QUALITY J_init {j_init:.3f} J_seq {j_seq:.3f} J_dev {j_dev:.3f} "
        f"recovery {rec:.3f}")
  assert j_init - j_dev >= 0.5 * (j_init - j_seq), (j_init, j_seq, j_dev)


def test_quality_settings_sequential_against_float64(ctx, quality):
  """Sequential mode at the quality settings against the float64 bar, after
  the |x| margin as for every case."""
  c, _ = quality
  c.reference()  # the |x| margin, before the device is touched
  seq, st = device_run(ctx, c)
  check_counts(c, st)
  C.check(c, seq, "quality_seq")


# ---- 6. errors ------------------------------------------------------------------------
def test_errors(ctx):
  V = 70
  ctx.upload(C.K.one_edge_inc(V))
  walks = np.array([[0, 1, 2]])
  with _hgx.N2v(ctx, n2v.CLIQUE, 8) as be:
    be.set_vocab(np.full(V, 2**32 - 1, np.uint32), np.arange(1, V + 1))
    with pytest.raises(_hgx.HgxError):  # HGX_ESTATE: no tree yet
      be.train_hs(walks)
    init = np.random.RandomState(0).uniform(-0.5, 0.5, (2, V, 8))
    be.set_vectors(init[0], init[1])
    ptr = np.array([0, 65] + [65] * (V - 1))
    with pytest.raises(_hgx.HgxError):  # HGX_EUNSUP: a path of 65
      be.set_tree(ptr, np.arange(65), np.zeros(65))
    ptr = np.array([0, 2, 3] + [3] * (V - 2))
    good = (ptr, np.array([5, 4, 5]), np.array([0, 0, 1]))
    bad = [(ptr, np.array([5, V - 1, 5]), good[2]),
           (ptr, np.array([5, -1, 5]), good[2]),
           (ptr, good[1], np.array([0, 2, 1])),
           (np.array([0, 2, 1] + [3] * (V - 2)), good[1], good[2]),
           (np.array([1, 2, 3] + [3] * (V - 2)), good[1], good[2]),
           (ptr, np.array([5, 5, 5]), good[2]),    # a node twice on a path
           (ptr, np.array([5, 4, 6]), good[2])]    # two roots
    for t in bad:
      with pytest.raises(AssertionError):  # HGX_EINVAL
        be.set_tree(*t)
      with pytest.raises(_hgx.HgxError):   # and no tree was set
        be.train_hs(walks)
    be.set_tree(*good)
    be.train_hs(walks, epochs=0)
    with pytest.raises(AssertionError):
      be.train_hs(np.array([[0, V]]))
    with pytest.raises(AssertionError):
      be.train_hs(walks, window=0)
    with pytest.raises(_hgx.HgxError):
      be.train_hs(np.zeros((1, n2v.MAX_WALK + 1), np.int32))
    # nothing was launched: the tables are as they were set
    out = be.get_vectors()
    assert np.array_equal(out[0], init[0].astype(np.float32))
    assert np.array_equal(out[1], init[1].astype(np.float32))
  with pytest.raises(AssertionError):
    ctx.set_tuning("dw_hot_levels", 7)
  with pytest.raises(AssertionError):
    ctx.set_tuning("dw_hot_levels", -1)


# ---- 7. end to end -------------------------------------------------------------------
def test_embedder_end_to_end(ctx):
  inc = golden_incidence("csr_small.npz")
  srcs = set(n2v.clique_sources(inc))
  for graph in (dw.BIPARTITE, dw.CLIQUE):
    kw = dict(num_walks_per_node=2, walk_length=5, graph=graph, ctx=ctx)
    if graph == dw.BIPARTITE and (np.diff(inc.rp_n).min() == 0 or
                                  np.diff(inc.rp_e).min() == 0):
      with pytest.raises(AssertionError):
        dw.EmbedDeepWalk(inc, 8, **kw)
      continue
    out = []
    for _ in range(2):
      np.random.seed(3)
      out.append(dw.EmbedDeepWalk(inc, 8, run_in_parallel=False, **kw))
    e = out[0]
    assert e.SerializeToString() == out[1].SerializeToString()
    assert e.dim == 8 and e.method_name == "deepwalk"
    assert sorted(e.node) == sorted(int(i) for i in inc.node_ids)
    assert sorted(e.edge) == sorted(int(i) for i in inc.edge_ids)
    x = np.array([e.node[int(i)].values for i in inc.node_ids], np.float32)
    y = np.array([e.edge[int(i)].values for i in inc.edge_ids], np.float32)
    assert x.shape == (inc.N, 8) and y.shape == (inc.E, 8)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(y))
    if graph == dw.CLIQUE:
      for v in range(inc.N):
        assert (v in srcs) == bool(np.any(x[v])), v
      assert np.array_equal(y, n2v.edge_centroids(inc, x))
    else:
      assert np.all(np.any(x, axis=1)) and np.all(np.any(y, axis=1))
    # concurrent: finite, and trained away from the initial vectors
    V = inc.N + inc.E if graph == dw.BIPARTITE else inc.N
    n_src = V if graph == dw.BIPARTITE else len(srcs)
    np.random.seed(3)
    [np.random.permutation(n_src) for _ in range(2)]
    [np.random.randint(0, 2**31 - 1) for _ in range(2)]
    init = (np.random.random((V, 8)).astype(np.float32) - np.float32(0.5)) / 8
    np.random.seed(3)
    info = {}
    e2 = dw.EmbedDeepWalk(inc, 8, info=info, **kw)
    x2 = np.array([e2.node[int(i)].values for i in inc.node_ids], np.float32)
    assert np.all(np.isfinite(x2))
    live = np.any(x2, axis=1)
    assert live.sum() == (inc.N if graph == dw.BIPARTITE else len(srcs))
    same = np.all(x2[live] == init[:inc.N][live], axis=1)
    assert same.sum() < live.sum() / 2, (same.sum(), live.sum())
    assert info["stats"]["pairs"] > 0 and info["stats"]["path_nodes"] > 0
    assert info["max_code"] == np.diff(dw.huffman_tree(info["counts"])[0]).max()


def test_bipartite_zero_degree_row_raises(ctx):
  from hypergraphembedding_amd.hypergraph_util import Incidence
  inc = Incidence(3, 2, [0, 1, 1, 2], [0, 1])  # node 1 without an edge
  with pytest.raises(AssertionError):
    dw.EmbedDeepWalk(inc, 4, ctx=ctx)
