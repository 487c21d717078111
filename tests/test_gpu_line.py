"""GPU: the LINE trainer (_hgx.N2v.set_arcs / line_samples / train_line,
n2v_train_line of csrc/hgx_n2v.hip): the draws against line.line_plan, the
sequential trainer against the float64 reference (line_reference.py), the
clamped sigmoid, the concurrent kernel with one wave per launch at the
sequential bar, a lossless-ness bound across workgroups, the concurrent
trainer's quality, the errors and the embedder end to end.

Inputs, reference and bar are line_cases.py's: per case and table, E = the
larger of the two NumpyBackendLine summation orders' max-abs distances from
the float64 reference, computed here; the device must be within 8 E + 2
ulp32(max |p|) elementwise on syn0 and syn1. Before the device is touched the
reference asserts that every evaluated |x| is at least 1e-3 (the clamp cases:
1.0) away from 6.

Which case reaches which instantiation: n2v_train_line<NPL> holds NPL = 1, 2,
4 or 8 columns of a padded row per lane: d8, d64 and every d = 16 case NPL 1;
d65, d128 NPL 2; d200 NPL 4; d512 NPL 8.

Measured max |device - reference| / E on an MI355X (the bar is 8 plus the ulp
term; at order 1 syn1 is untouched and compared bitwise):

  case                          order 1 syn0    order 2 syn0 / syn1
  test_sequential_against_float64
    d8 d128 d512                1.00            1.00 / 1.00
    d64                         0.96            0.86 / 1.00
    d65                         0.89            1.00 / 1.00
    d200                        1.00            0.85 / 1.00
    K0 K1 K8                    1.00            1.00 / 1.00
    weighted                    1.12            1.00 / 1.00
    tiny                        1.00            1.00 / 0.95
  test_clamped_targets          1.00            1.00 / 1.00
  test_one_wave_per_launch_meets_the_sequential_bar
    d16 d200                    1.00            1.00 / 1.00

test_nothing_lost_across_workgroups: order 1 D = 1.05e-2, staleness emulation
(a) 1.04e-4, loss emulation (b) 3.55e-3, device 5.52e-6 (the bound is
sqrt((a)(b)) = 6.1e-4); order 2 D = 2.83e-3, (a) 1.15e-5, (b) 7.48e-4, device
1.00e-6 (bound 9.3e-5).

test_concurrent_quality (1024 samples per launch): order 1 J_init 4.250,
float64 sequential 3.813, device 3.814, recovery 1.000; order 2 4.159, 3.084,
3.097, recovery 0.988 (the test asks for 0.5). DESIGN §4.12 has the sweep over
`line_chunk_samples`.
"""

import numpy as np
import pytest

import line_cases as C
import line_reference as R
from conftest import golden_incidence
from hypergraphembedding_amd import _hgx
from hypergraphembedding_amd import line as L
from hypergraphembedding_amd import node2vec as n2v

pytestmark = pytest.mark.gpu

CHUNK_DEFAULT = 0  # line_chunk_samples as a context starts (include/hgx.h)


@pytest.fixture(scope="module")
def ctx():
  c = _hgx.Context(0)
  yield c
  c.close()


def device_run(ctx, c, concurrent=False, chunk=CHUNK_DEFAULT):
  ctx.upload(c.inc)
  ctx.set_tuning("line_chunk_samples", chunk)
  try:
    with _hgx.N2v(ctx, L.BIPARTITE, c.d) as be:
      out = c.run_backend(be, concurrent=concurrent)
      st = be.stats()
  finally:
    ctx.set_tuning("line_chunk_samples", CHUNK_DEFAULT)
  return out, st


def check_counts(c, st, clamped):
  assert st["samples"] == c.T
  assert st["targets"] == c.T * (1 + c.negative)
  assert st["clamped"] == clamped
  assert st["train_ms"] > 0


# ---- 1. the draws ----------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_draws_equal_the_host_plan(ctx, weighted):
  inc = C.graph_g()
  w = C.weights_g() if weighted else None
  arcs = C.tables(inc, w)
  ctx.upload(inc)
  with _hgx.N2v(ctx, L.BIPARTITE, 8) as be:
    be.set_arcs(*arcs)
    for neg in (0, 5, 8):
      for s0 in (0, 1000, 2**33 + 5):
        dev = be.line_samples(s0, 1000, neg, 12345)
        host = L.line_plan(inc, *arcs, neg, 1000, 12345, s0=s0)
        assert dev.shape == (1000, 2 + neg) and dev.dtype == np.int32
        assert np.array_equal(dev, host), (neg, s0)


# ---- 2. sequential trainer against float64 ---------------------------------------
CASES = {**C.dims(), **C.d16()}


@pytest.mark.parametrize("name", list(CASES))
def test_sequential_against_float64(ctx, name):
  c = CASES[name]()
  ref, _, _ = c.reference()  # the |x| margin, before the device is touched
  out, st = device_run(ctx, c)
  check_counts(c, st, ref.clamped)
  C.check(c, out, name)
  again, _ = device_run(ctx, c)
  assert all(np.array_equal(a, b) for a, b in zip(out, again))
  if c.order == 1:
    assert np.array_equal(out[1], c.syn1)


# ---- 3. the clamped sigmoid ---------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_clamped_targets(ctx, order):
  """Many |x| far beyond 6 (all four (label, sign) kinds, asserted on the
  host): the sequential device meets the bar, and both modes count the
  reference's clamped targets."""
  c = C.clamp_case(order)
  ref, _, _ = c.reference(margin=1.0)
  assert ref.clamped > 0
  out, st = device_run(ctx, c)
  check_counts(c, st, ref.clamped)
  C.check(c, out, c.name)
  conc, st = device_run(ctx, c, concurrent=True)
  check_counts(c, st, ref.clamped)
  assert all(np.all(np.isfinite(t)) for t in conc)


# ---- 4. the concurrent kernel, one wave per launch -----------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("d", [16, 200])
def test_one_wave_per_launch_meets_the_sequential_bar(ctx, d, order):
  """line_chunk_samples = 64: every concurrent launch holds one wave, so the
  concurrent kernel (agent-scope loads, atomic adds) is deterministic and is
  held to the sequential bar."""
  c = C.one_wave(d, order)
  ref, _, _ = c.reference()
  out, st = device_run(ctx, c, concurrent=True, chunk=64)
  again, _ = device_run(ctx, c, concurrent=True, chunk=64)
  check_counts(c, st, ref.clamped)
  C.check(c, out, c.name)
  assert all(np.array_equal(a, b) for a, b in zip(out, again))


# ---- 5. nothing lost across workgroups -------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_nothing_lost_across_workgroups(ctx, order):
  """Two launches of 16 waves (4 workgroups). The device's distance from the
  sequential float64 reference on the target table must stay below the
  geometric mean of the staleness error (a) and of the error (b) of losing
  the updates of waves 4..7 (one workgroup) to row N + 0, the edge that holds
  every node, with (b) >= 10 (a) asserted on the host first."""
  c = C.lossless_case(order)
  ref = c.float64()
  assert ref.margin >= C.MARGIN
  t = 0 if order == 1 else 1
  rt = (ref.syn0, ref.syn1)[t]
  hub = c.inc.N + 0
  assert c.inc.edge_size()[0] == c.inc.N
  args = (c.syn0, c.syn1, c.plan(), order, c.rho, 1024)
  a = np.abs(R.launch_emulation(*args)[t] - rt).max()
  b = np.abs(R.launch_emulation(*args, drop=(range(4, 8), hub))[t] - rt).max()
  D = np.abs(rt - (c.syn0, c.syn1)[t].astype(np.float64)).max()
  assert b >= 10 * a, (a, b)
  out, st = device_run(ctx, c, concurrent=True, chunk=1024)
  check_counts(c, st, ref.clamped)
  err = np.abs(out[t].astype(np.float64) - rt).max()
  print(f"LOSSLESS order {order}: D {D:.3g} staleness (a) {a:.3g} = "
        f"{a / D:.3g} D loss (b) {b:.3g} = {b / D:.3g} D device {err:.3g} = "
        f"{err / D:.3g} D")
  assert err <= np.sqrt(a * b), (err, a, b)


# ---- 6. concurrent quality ----------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
def test_concurrent_quality(ctx, order):
  """The planted graph at 1024 samples per launch: the float64 sequential
  reference must itself learn (J over the first 4000 samples falls by at
  least 0.25 at order 1, 0.8 at order 2), and the concurrent device ends
  finite and recovers at least half of that decrease."""
  c = C.quality_case(order)
  ref = c.float64()
  p0 = c.plan()[:4000]
  j_init = R.objective(c.syn0, c.syn1, p0, order)
  j_seq = R.objective(ref.syn0, ref.syn1, p0, order)
  print(f"QUALITY order {order}: J_init {j_init:.3f} J_seq {j_seq:.3f} "
        f"max |x| {ref.max_x:.2f}")
  assert j_init - j_seq >= (0.25 if order == 1 else 0.8), (j_init, j_seq)
  out, st = device_run(ctx, c, concurrent=True, chunk=1024)
  assert np.all(np.isfinite(out[0])) and np.all(np.isfinite(out[1]))
  assert st["samples"] == c.T and st["targets"] == 6 * c.T
  j_dev = R.objective(out[0], out[1], p0, order)
  rec = (j_init - j_dev) / (j_init - j_seq)
  print(f"QUALITY order {order}: J_dev {j_dev:.3f} recovery {rec:.3f} "
        f"clamped {st['clamped']}")
  assert j_init - j_dev >= 0.5 * (j_init - j_seq), (j_init, j_seq, j_dev)


# ---- 7. errors -------------------------------------------------------------------------------
def test_errors(ctx):
  inc = C.graph_g()
  V, nnz = 85, 166
  thr, alias, cum = C.tables(inc, C.weights_g())
  ctx.upload(inc)
  init = np.random.RandomState(0).uniform(-0.5, 0.5, (2, V, 8)).astype(np.float32)

  def unchanged(be):
    out = be.get_vectors()
    assert np.array_equal(out[0], init[0]) and np.array_equal(out[1], init[1])

  with _hgx.N2v(ctx, n2v.CLIQUE, 8) as be:
    with pytest.raises(_hgx.HgxError):  # HGX_ESTATE: not the bipartite graph
      be.set_arcs(None, None, np.arange(1, inc.N + 1))
    with pytest.raises(_hgx.HgxError):
      be.train_line(2, 5, 10)
  with _hgx.N2v(ctx, L.BIPARTITE, 8) as be:
    with pytest.raises(_hgx.HgxError):  # HGX_ESTATE: no arcs, no vectors
      be.train_line(2, 5, 10)
    with pytest.raises(_hgx.HgxError):
      be.line_samples(0, 10, 5, 1)
    be.set_vectors(init[0], init[1])
    with pytest.raises(_hgx.HgxError):  # HGX_ESTATE: still no arcs
      be.train_line(2, 5, 10)
    down = cum.copy()
    down[40] = down[39] - 1
    out_of = alias.copy()
    out_of[7] = nnz
    neg = alias.copy()
    neg[0] = -1
    for bad in ((thr, None, cum), (None, alias, cum), (thr, out_of, cum),
                (thr, neg, cum), (thr, alias, down),
                (None, None, np.zeros(V, np.int32))):
      with pytest.raises(AssertionError):  # HGX_EINVAL
        be.set_arcs(*bad)
      with pytest.raises(_hgx.HgxError):   # and no tables were set
        be.train_line(2, 5, 10)
      unchanged(be)
    be.set_arcs(thr, alias, cum)
    with pytest.raises(_hgx.HgxError) as ei:  # HGX_EUNSUP
      be.train_line(2, 9, 10)
    assert type(ei.value) is _hgx.HgxError
    for kw in (dict(order=0), dict(order=3), dict(negative=-1),
               dict(n_samples=-1)):
      a = dict(order=2, negative=5, n_samples=10)
      a.update(kw)
      with pytest.raises(AssertionError):  # HGX_EINVAL
        be.train_line(a["order"], a["negative"], a["n_samples"])
      unchanged(be)
    with pytest.raises(_hgx.HgxError):
      be.line_samples(0, 10, 9, 1)
    with pytest.raises(AssertionError):
      be.line_samples(-1, 10, 5, 1)
    unchanged(be)
    be.train_line(2, 5, 0)  # trains nothing and succeeds
    be.train_line(1, 5, 0, concurrent=False)
    unchanged(be)
    assert be.stats()["samples"] == 0
    # a failed set_arcs leaves the tables that were set
    ok = be.line_samples(0, 50, 5, 3)
    with pytest.raises(AssertionError):
      be.set_arcs(thr, out_of, cum)
    assert np.array_equal(be.line_samples(0, 50, 5, 3), ok)
  with pytest.raises(_hgx.HgxError):  # d <= 512 at create
    _hgx.N2v(ctx, L.BIPARTITE, 513)
  for v in (-1, 2**20 + 1):
    with pytest.raises(AssertionError):
      ctx.set_tuning("line_chunk_samples", v)
  ctx.set_tuning("line_chunk_samples", 2**20)
  ctx.set_tuning("line_chunk_samples", CHUNK_DEFAULT)


# ---- 8. end to end --------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, "both"])
def test_embedder_end_to_end(ctx, order):
  inc = golden_incidence("csr_small.npz")
  V, d = inc.N + inc.E, 8
  kw = dict(order=order, samples=20000, ctx=ctx)
  out = []
  for _ in range(2):
    np.random.seed(3)
    out.append(L.EmbedLine(inc, d, run_in_parallel=False, **kw))
  e = out[0]
  assert e.SerializeToString() == out[1].SerializeToString()
  assert e.dim == d and e.method_name == "LINE"
  assert sorted(e.node) == sorted(int(i) for i in inc.node_ids)
  assert sorted(e.edge) == sorted(int(i) for i in inc.edge_ids)
  # concurrent: finite, and trained away from the initial vectors
  dh = d // 2 if order == "both" else d
  np.random.seed(3)
  np.random.randint(0, 2**31 - 1)
  init = (np.random.random((V, dh)).astype(np.float32) - np.float32(0.5)) / dh
  if order == "both":
    init = L._unit_rows(init)
  np.random.seed(3)
  info = {}
  e2 = L.EmbedLine(inc, d, info=info, **kw)
  x = np.array([e2.node[int(i)].values for i in inc.node_ids] +
               [e2.edge[int(i)].values for i in inc.edge_ids], np.float32)
  assert x.shape == (V, d) and np.all(np.isfinite(x))
  live = info["degrees"] > 0
  assert np.array_equal(np.any(x, axis=1), live)
  same = np.all(x[live][:, :dh] == init[live], axis=1)
  assert same.sum() < live.sum() / 2, (same.sum(), live.sum())
  assert info["stats"]["samples"] == 20000
  assert info["stats"]["targets"] == 120000
  if order == "both":
    for half in (x[live][:, :dh], x[live][:, dh:]):
      assert np.allclose(np.linalg.norm(half.astype(np.float64), axis=1), 1.0,
                         atol=1e-6)
