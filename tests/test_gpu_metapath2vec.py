"""GPU: the metapath2vec engine (_hgx.N2v.mp_walks / mp_counts /
set_vocab_typed / train_mp, n2v_train_mp of csrc/hgx_n2v.hip): the streamed
corpus against metapath2vec.mp_walk, the 64-bit counts, the sequential
trainer against the float64 reference (mp2v_reference.py), the clamped
sigmoid, the concurrent kernel where it is deterministic, a lossless-ness
bound across workgroups, the concurrent trainer's quality, the errors and the
embedder end to end.

Inputs, reference and bar are mp2v_cases.py's: per case and table, E = the
larger of the two NumpyBackendMp summation orders' max-abs distances from the
float64 reference, computed here; the device must be within 8 E + 2
ulp32(max |p|) elementwise on syn0 and syn1. Before the device is touched the
reference asserts that every evaluated |x| is at least 1e-3 (the clamp case:
1.0) away from 6.

Which case reaches which instantiation: n2v_train_mp<NPL> holds NPL = 1, 2, 4
or 8 columns of a padded row per lane: d8 and every d = 16 case NPL 1, d65
NPL 2, d200 NPL 4, d512 NPL 8. L2, L65, L129 and L256 fill one to four
64-lane passes of the keeps.

One wave per launch. "mp_chunk_walks" is a multiple of 4, so a launch is at
least one workgroup of four waves. Two arrangements make the concurrent
kernel deterministic: blocks_case (four components, one source in each, no
negatives: the four waves of a launch touch disjoint rows; with negatives
they would not, a negative comes from the whole type), and one_walk_case (a
corpus of one walk: one wave per launch, with negatives). Both are held to
the sequential bar.

Measured max |device - reference| / E on an MI355X (the bar is 8 plus the ulp
term), syn0 / syn1:

  test_sequential_against_float64
    d8 d200 K1 K8 min_count L2      1.00 / 1.00
    d65                             1.00 / 0.94
    d512                            0.81 / 1.00
    K0                              1.06 / 1.00
    untyped                         0.92 / 1.00
    holes                           0.86 / 1.00
    tiny                            1.00 / 0.80
    L65                             1.31 / 1.00
    L129                            1.00 / 0.96
    L256                            0.87 / 1.00
  test_clamped_targets              1.00 / 1.00
  test_one_wave_per_launch_meets_the_sequential_bar
    blocks d16 d200                 1.00 / 1.00
    one_walk d16 d200               1.00 / 1.00
  test_embedder_end_to_end
    youtube_tiny                    1.00 / 1.00

test_nothing_lost_across_workgroups: D = 9.80e-4, staleness emulation (a)
6.88e-7, loss emulation (b) 4.22e-4, device 4.59e-7 (the bound is
sqrt((a)(b)) = 1.7e-5).

test_concurrent_quality (32 walks per launch): J_init 4.141, float64
sequential 3.695, device 3.726, recovery 0.931 (the test asks for 0.5).
"""

import numpy as np
import pytest

import mp2v_cases as C
import mp2v_reference as R
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import metapath2vec as M
from hypergraphembedding_amd import node2vec as n2v
from hypergraphembedding_amd.hypergraph_util import Incidence

pytestmark = pytest.mark.gpu

CHUNK_DEFAULT = 0  # mp_chunk_walks as a context starts (include/hgx.h)


@pytest.fixture(scope="module")
def ctx():
  c = _hgx.Context(0)
  yield c
  c.close()


def device_run(ctx, c, concurrent=False, chunk=CHUNK_DEFAULT):
  ctx.upload(c.inc)
  ctx.set_tuning("mp_chunk_walks", chunk)
  try:
    with _hgx.N2v(ctx, M.BIPARTITE, c.d) as be:
      out = c.run_backend(be, concurrent=concurrent)
      st = be.stats()
  finally:
    ctx.set_tuning("mp_chunk_walks", CHUNK_DEFAULT)
  return out, st


def check_counts(c, st, ref):
  assert st["mp"] == dict(walks=c.epochs * c.n_walks, words=ref.words,
                          pairs=ref.pairs, targets=ref.targets,
                          clamped=ref.clamped)
  assert st["walks"] == c.epochs * c.n_walks
  assert st["words"] == ref.words and st["pairs"] == ref.pairs
  assert st["walk_ms"] > 0 and st["train_ms"] > 0


# ---- 1. the draws ----------------------------------------------------------------
@pytest.mark.parametrize("graph", [C.graph_g, C.holes_graph])
def test_walks_equal_the_host(ctx, graph):
  inc = graph()
  src = M.mp_sources(inc)
  assert src.size == 25
  ctx.upload(inc)
  try:
    with _hgx.N2v(ctx, M.BIPARTITE, 8) as be:
      for L in (1, 2, 64, 65, 128, 129, 201, 256):
        for chunk, g0, count in ((CHUNK_DEFAULT, 0, 30), (4, 20, 10),
                                 (4, 49, 3)):  # across the pass boundaries
          ctx.set_tuning("mp_chunk_walks", chunk)
          dev = be.mp_walks(src, 3, L, 777, g0, count)
          host = [M.mp_walk(inc, g, src, L, 777)
                  for g in range(g0, g0 + count)]
          assert dev.shape == (count, L) and dev.dtype == np.int32
          assert np.array_equal(dev, np.array(host).reshape(count, L)), (
              L, chunk, g0)
      assert be.mp_walks(src, 3, 9, 777, 75, 0).shape == (0, 9)
  finally:
    ctx.set_tuning("mp_chunk_walks", CHUNK_DEFAULT)


# ---- 2. the counts -----------------------------------------------------------------
@pytest.mark.parametrize("chunk", [4, 28, CHUNK_DEFAULT])
def test_counts_equal_the_host(ctx, chunk):
  inc = C.holes_graph()
  src = M.mp_sources(inc)
  host = M.NumpyBackendMp(inc, M.BIPARTITE, 8).mp_counts(src, 3, 201, 5)
  assert host.sum() == 75 * 201 and 75 % 28
  ctx.upload(inc)
  ctx.set_tuning("mp_chunk_walks", chunk)
  try:
    with _hgx.N2v(ctx, M.BIPARTITE, 8) as be:
      dev = be.mp_counts(src, 3, 201, 5)
      assert be.stats()["walk_ms"] > 0
  finally:
    ctx.set_tuning("mp_chunk_walks", CHUNK_DEFAULT)
  assert dev.dtype == np.int64 and np.array_equal(dev, host)


# ---- 3. sequential trainer against float64 -------------------------------------------
CASES = {**C.dims(), **C.d16()}


@pytest.mark.parametrize("name", list(CASES))
def test_sequential_against_float64(ctx, name):
  c = CASES[name]()
  ref, _, _ = c.reference()  # the |x| margin, before the device is touched
  out, st = device_run(ctx, c)
  check_counts(c, st, ref)
  C.check(c, out, name)
  again, _ = device_run(ctx, c)
  assert all(np.array_equal(a, b) for a, b in zip(out, again))
  small, st4 = device_run(ctx, c, chunk=4)  # the chunk size changes nothing
  assert all(np.array_equal(a, b) for a, b in zip(out, small))
  check_counts(c, st4, ref)
  dead = c.live == 0
  assert np.array_equal(out[1][dead], c.syn1[dead])  # never a target
  assert np.array_equal(out[0][dead], c.syn0[dead])


# ---- 4. the clamped sigmoid ------------------------------------------------------------
def test_clamped_targets(ctx):
  """Many |x| far beyond 6 (all four (label, sign) kinds, asserted on the
  host): the sequential device meets the bar, and both modes count the
  reference's clamped targets."""
  c = C.clamp_case()
  ref, _, _ = c.reference(margin=1.0)
  assert ref.clamped > 0
  out, st = device_run(ctx, c)
  check_counts(c, st, ref)
  C.check(c, out, c.name)
  conc, st = device_run(ctx, c, concurrent=True)
  check_counts(c, st, ref)
  assert all(np.all(np.isfinite(t)) for t in conc)


# ---- 5. the concurrent kernel where it is deterministic ---------------------------------
@pytest.mark.parametrize("d", [16, 200])
@pytest.mark.parametrize("kind", ["blocks", "one_walk"])
def test_one_wave_per_launch_meets_the_sequential_bar(ctx, kind, d):
  """mp_chunk_walks = 4 (one workgroup per launch): blocks_case, whose four
  waves touch disjoint rows, and one_walk_case, one wave per launch (the
  module docstring); the concurrent kernel (agent-scope loads, atomic adds)
  is deterministic there and is held to the sequential bar."""
  c = C.blocks_case(d) if kind == "blocks" else C.one_walk_case(d)
  ref, _, _ = c.reference()
  out, st = device_run(ctx, c, concurrent=True, chunk=4)
  again, _ = device_run(ctx, c, concurrent=True, chunk=4)
  check_counts(c, st, ref)
  C.check(c, out, c.name)
  assert all(np.array_equal(a, b) for a, b in zip(out, again))


# ---- 6. nothing lost across workgroups ---------------------------------------------------
def test_nothing_lost_across_workgroups(ctx):
  """Two launches of 16 waves (4 workgroups). The device's distance from the
  sequential float64 reference on syn1 must stay below the geometric mean of
  the staleness error (a) and of the error (b) of losing the updates of waves
  4..7 (one workgroup) to row N + 0, the edge that holds every node, with
  (b) >= 10 (a) asserted on the host first."""
  c = C.lossless_case()
  ref = c.float64()
  assert ref.margin >= C.MARGIN
  hub = c.inc.N + 0
  assert c.inc.edge_size()[0] == c.inc.N and c.n_walks == 32
  args = (c.syn0, c.syn1, c.plan(), c.alpha, c.min_alpha, c.n_walks, 16)
  a = np.abs(R.launch_emulation(*args)[1] - ref.syn1).max()
  b = np.abs(R.launch_emulation(*args, drop=(range(4, 8), hub))[1] -
             ref.syn1).max()
  D = np.abs(ref.syn1 - c.syn1.astype(np.float64)).max()
  assert b >= 10 * a, (a, b)
  out, st = device_run(ctx, c, concurrent=True, chunk=16)
  check_counts(c, st, ref)
  err = np.abs(out[1].astype(np.float64) - ref.syn1).max()
  print(f"LOSSLESS: D {D:.3g} staleness (a) {a:.3g} = {a / D:.3g} D loss "
        f"(b) {b:.3g} = {b / D:.3g} D device {err:.3g} = {err / D:.3g} D")
  assert err <= np.sqrt(a * b), (err, a, b)


# ---- 7. concurrent quality -------------------------------------------------------------------
def test_concurrent_quality(ctx):
  """The planted graph at 32 walks per launch (8 workgroups): the float64
  sequential reference must itself learn (J over the pairs of the first 100
  walks falls by at least 0.35; it fell by 0.446 when the case was written),
  and the concurrent device ends finite and recovers at least half of that
  decrease."""
  c = C.quality_case()
  ref = c.float64()
  p0 = c.plan()[:100]
  j_init = R.objective(c.syn0, c.syn1, p0)
  j_seq = R.objective(ref.syn0, ref.syn1, p0)
  print(f"QUALITY: J_init {j_init:.3f} J_seq {j_seq:.3f} max |x| "
        f"{ref.max_x:.2f}")
  assert j_init - j_seq >= 0.35, (j_init, j_seq)
  out, st = device_run(ctx, c, concurrent=True, chunk=32)
  assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
  assert st["mp"]["words"] == ref.words and st["mp"]["pairs"] == ref.pairs
  assert st["mp"]["targets"] == ref.targets
  j_dev = R.objective(out[0], out[1], p0)
  rec = (j_init - j_dev) / (j_init - j_seq)
  print(f"QUALITY: J_dev {j_dev:.3f} recovery {rec:.3f} clamped "
        f"{st['mp']['clamped']}")
  assert j_init - j_dev >= 0.5 * (j_init - j_seq), (j_init, j_seq, j_dev)


# ---- 8. errors ----------------------------------------------------------------------------------
def test_errors(ctx):
  c = C.Case("errors", 8, seed=99)
  inc, src, V, N = c.inc, c.sources, 85, 60
  ctx.upload(inc)
  init = np.random.RandomState(0).uniform(-0.5, 0.5,
                                          (2, V, 8)).astype(np.float32)

  def unchanged(be):
    out = be.get_vectors()
    assert np.array_equal(out[0], init[0]) and np.array_equal(out[1], init[1])

  def unsup(fn, *a, **kw):
    with pytest.raises(_hgx.HgxError) as ei:
      fn(*a, **kw)
    assert type(ei.value) is _hgx.HgxError

  with _hgx.N2v(ctx, n2v.CLIQUE, 8) as be:  # HGX_ESTATE: not bipartite
    unsup(be.mp_walks, src, 1, 5, 0, 0, 1)
    unsup(be.mp_counts, src, 1, 5, 0)
    unsup(be.set_vocab_typed, c.keep[:N], np.arange(1, N + 1), False)
    unsup(be.train_mp, src, 1, 5)
  with _hgx.N2v(ctx, M.BIPARTITE, 8) as be:
    unsup(be.train_mp, src, 1, 5)  # HGX_ESTATE: no vocabulary, no vectors
    be.set_vectors(init[0], init[1])
    unsup(be.train_mp, src, 1, 5)  # still no vocabulary
    # set_vocab_typed: violations set nothing
    down = c.cum.copy()
    down[40] = down[39] - 1
    down_e = c.cum.copy()
    down_e[70] = down_e[69] - 1
    no_node = c.cum.copy()
    no_node[:N] = 0
    for bad, typed in ((down, True), (down_e, True), (no_node, True),
                       (c.cum, False),  # the typed table falls at N
                       (np.zeros(V, np.int32), False)):
      with pytest.raises(AssertionError):  # HGX_EINVAL
        be.set_vocab_typed(c.keep, bad, typed)
      unsup(be.train_mp, src, 1, 5)
    be.set_vocab_typed(c.keep, c.cum, True)
    with _hgx.N2v(ctx, M.BIPARTITE, 8) as fresh:  # vocabulary, no vectors
      fresh.set_vocab_typed(c.keep, c.cum, True)
      unsup(fresh.train_mp, src, 1, 5)
    # HGX_EINVAL
    empty_edge = C.holes_graph()
    for kw in (dict(L=0), dict(num_walks=0), dict(sources=[]),
               dict(negative=-1), dict(window=0), dict(epochs=-1),
               dict(sources=[59]), dict(sources=[60, 85]),
               dict(sources=[-1])):
      a = dict(sources=src, num_walks=1, L=5, negative=5, window=3, epochs=1)
      a.update(kw)
      with pytest.raises(AssertionError):
        be.train_mp(a["sources"], a["num_walks"], a["L"], window=a["window"],
                    negative=a["negative"], epochs=a["epochs"])
      unchanged(be)
      if set(kw) <= {"L", "num_walks", "sources"}:
        with pytest.raises(AssertionError):
          be.mp_counts(a["sources"], a["num_walks"], a["L"], 0)
        with pytest.raises(AssertionError):
          be.mp_walks(a["sources"], a["num_walks"], a["L"], 0, 0, 1)
    for g0, count in ((-1, 1), (0, -1), (20, 6)):  # outside the corpus
      with pytest.raises(AssertionError):
        be.mp_walks(src, 1, 5, 0, g0, count)
    # HGX_EUNSUP
    big = 2**31 // 25 + 1
    assert 25 * big >= 2**31 > 25 * (big - 1)
    for kw in (dict(L=257), dict(negative=9), dict(num_walks=big),
               dict(L=256, window=40, negative=8)):  # 81 x 8 > 512 staged
      a = dict(num_walks=1, L=5, negative=5, window=3)
      a.update(kw)
      unsup(be.train_mp, src, a["num_walks"], a["L"], window=a["window"],
            negative=a["negative"], epochs=1)
      unchanged(be)
    unsup(be.mp_counts, src, 1, 257, 0)
    unsup(be.mp_walks, src, 1, 257, 0, 0, 1)
    unsup(be.mp_counts, src, big, 5, 0)
    be.train_mp(src, 1, 5, epochs=0)  # trains nothing and succeeds
    unchanged(be)
    assert be.stats()["mp"] == dict(walks=0, words=0, pairs=0, targets=0,
                                    clamped=0)
    # a window the staging holds: 31 x 8 = 248, and no negatives at any window
    be.train_mp(src, 1, 5, window=15, negative=8, epochs=1, concurrent=False)
    be.train_mp(src, 1, 5, window=10**6, negative=0, epochs=1)
  # an empty edge as a source
  ctx.upload(empty_edge)
  with _hgx.N2v(ctx, M.BIPARTITE, 8) as be:
    with pytest.raises(AssertionError):
      be.mp_counts([61 + 25], 1, 5, 0)
    be.mp_counts([61 + 24], 1, 5, 0)
  for v in (-1, 2**16 + 1):
    with pytest.raises(AssertionError):
      ctx.set_tuning("mp_chunk_walks", v)
  ctx.set_tuning("mp_chunk_walks", 2**16)
  ctx.set_tuning("mp_chunk_walks", CHUNK_DEFAULT)


# ---- 9. end to end ------------------------------------------------------------------------------
def test_embedder_end_to_end(ctx, tiny_hypergraph):
  inc = Incidence.from_hypergraph(tiny_hypergraph)
  V, d = inc.N + inc.E, 8
  kw = dict(num_walks=10, walk_length=4, epochs=2, min_count=2, ctx=ctx)
  out = []
  for _ in range(2):
    np.random.seed(3)
    out.append(M.EmbedMetapath2Vec(inc, d, run_in_parallel=False, **kw))
  e = out[0]
  assert e.SerializeToString() == out[1].SerializeToString()
  assert e.dim == d and e.method_name == "metapath2vec++"
  assert sorted(e.node) == sorted(int(i) for i in inc.node_ids)
  assert sorted(e.edge) == sorted(int(i) for i in inc.edge_ids)
  # concurrent: finite, zero exactly where dropped, trained elsewhere
  np.random.seed(3)
  np.random.randint(0, 2**31 - 1)
  np.random.randint(0, 2**31 - 1)
  init = (np.random.random((V, d)).astype(np.float32) - np.float32(0.5)) / d
  np.random.seed(3)
  info = {}
  e2 = M.EmbedMetapath2Vec(inc, d, plus_plus=False, info=info, **kw)
  assert e2.method_name == "metapath2vec"
  x = np.array([e2.node[int(i)].values for i in inc.node_ids] +
               [e2.edge[int(i)].values for i in inc.edge_ids], np.float32)
  assert x.shape == (V, d) and np.all(np.isfinite(x))
  live = info["counts"] >= 2
  assert info["dropped"] == (~live).sum() and live.sum() > 2 * inc.E
  assert np.array_equal(np.any(x, axis=1), live)
  same = np.all(x[live] == init[live], axis=1)
  assert same.sum() < live.sum() / 2, (same.sum(), live.sum())
  n_src = int((inc.edge_size() > 0).sum())
  assert info["n_walks"] == 10 * n_src
  assert info["counts"].sum() == 10 * n_src * 9
  assert info["stats"]["mp"]["walks"] == 20 * n_src
  # the device against float64 on the same graph, four walks of 9 per edge
  c = C.Case("youtube_tiny", d, inc=inc, num_walks=4, L=9, min_count=2,
             sample=1e-3, epochs=1, seed=95)
  ref, _, _ = c.reference()
  dev, st = device_run(ctx, c)
  check_counts(c, st, ref)
  C.check(c, dev, c.name)
