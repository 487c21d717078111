"""GPU: every alg-dist kernel instantiation a release build can select,
against the float64 reference and the derived float32 bound of
algdist_cases.py. Every check is |device - reference| <= bound elementwise;
a NaN never passes. The bound is derived there, not measured here.

Which test reaches which instantiation (release build: quad M = 4, narrow
M = 2; G by the swept side's average degree, algdist_cases.SEVEN):

  algdist_half_quad<KS 4/8/12/16, G 4/8/16/32/64, MODE_FULL, 4, PM_GATHER>:
    test_quad_and_narrow_every_width_and_group (every G on the node side and
    on the edge side; k = 1, 3 -> KS 4; 4, 7 -> 8; 8, 10, 11 -> 12; 12, 15
    -> 16), test_row_width_tuning (k = 3 in rows of 8, 12, 16; k = 10 in 16),
    test_grid_stride (KS 4, G 4 and 64, the rr += ngroups loop).
  algdist_half_narrow<20, G 1/2/4/8/16/32/64, MODE_FULL, 2>:
    test_quad_and_narrow_every_width_and_group (k = 16, 19),
    test_row_width_tuning (k = 3 and 10 in rows of 20).
  algdist_half_quad<KS, G, MODE_FULL, 4, PM_PUSH> (node side) and
  <..., PM_STREAM> (edge side), every KS <= 16 and every G: test_push_form
    (which asserts the library's conditions for the push form, and that the
    result differs from gather's in some bit).
  algdist_half_wide<MODE_FULL>: test_wide (k = 20, 23: one float4 column per
    lane; 255: the last lane of q = 0; 256, 300: the q = 1 lane loop; 2046:
    all eight).
  algdist_seg_partial<KS 4/8/12/16/20, 4, false> and
  algdist_long_finish<KS, MODE_FULL>: test_long_rows (k = 3, 7, 10, 15, 19;
    rows of 2, 3, 8, 9, 17 and 65 pieces: the last is long_finish's lane-strided
    loop).
  algdist_seg_partial<KS 4/8/12/16, 4, true> (PRE): test_push_form on the
    long-row graphs.
  algdist_half_quad<KS 4/8/12/16, G 4/8/16/32/64, MODE_PARTIAL, 4, PM_GATHER>
  and algdist_half_narrow<20, G, MODE_PARTIAL, 2>: test_sharded_every_group
    (k = 3, 7, 10, 15, 19 on the seven graphs), test_sharded_in_process.
  algdist_half_wide<MODE_PARTIAL>: test_sharded_in_process (k = 24, 300).
  algdist_seg_partial<KS, 4, false> + algdist_long_finish<KS, MODE_PARTIAL>:
    test_sharded_in_process on the long-row graph (k = 3 ... 19).
  algdist_edge_final, algdist_edge_final_wire, algdist_wire_pack:
    test_sharded_in_process (dense / compact, 1 and 3 edge ranges, local
    edge rows of length 0 with rank 0 owning no node row).
  pack_rows, apply_affine, unpack_rows, load_affine, flush_minmax: all.

Selectable in a release build and not reached: none of launch_half's
instantiations. (M = 1 / 2 / 4 variants other than the defaults, the narrow
kernel at KS <= 16 and algdist_half_flat are selected only through
HGX_DEBUG_KNOBS environment knobs, which a release build does not read. The
widening of 12-float rows to 16 on tables above 256 MiB is the same
instantiation as alg_ks = 16.)

Measured worst |device - reference| / bound on an MI355X (the bar is 1):

  test                                          ratio  at
  test_quad_and_narrow_..._group[d3x200]        0.240  k 15, u01, 1 it, node
  test_quad_and_narrow_..._group[d6x100]        0.159  k 15, u01, 1 it, node
  test_quad_and_narrow_..._group[d12x48]        0.130  k 11, sym, 1 it, node
  test_quad_and_narrow_..._group[d24x24]        0.092  k 15, u01, 1 it, node
  test_quad_and_narrow_..._group[d48x12]        0.070  k 11, sym, 1 it, node
  test_quad_and_narrow_..._group[d100x6]        0.045  k 16, sym, 1 it, edge
  test_quad_and_narrow_..._group[d200x3]        0.024  k 16, sym, 1 it, edge
  test_small_graph_fewer_rows_than_a_workgroup  0.136  k 15, sym, 1 it, edge
  test_row_width_tuning                         0.161  d3x200, k 10 in 16, node
  test_wide                                     0.206  k 2046, u01, 1 it, node
  test_long_rows                                0.253  long512, k 19, near1, alg_long 64
  test_push_form                                0.215  long512, k 10, near1, PRE pieces
  test_grid_stride                              0.113  node
  test_sharded_every_group                      0.020  d6x100, k 3, rank 1 node
  test_sharded_in_process[d12x48]               0.045  k 300, rank 0 without rows
  test_sharded_in_process[d100x6]               0.046  k 300, compact, rank 1
  test_sharded_in_process[long64]               0.255  k 300, near1, compact, rank 0

The largest ratios are at one iteration and on short rows: the bound counts
n roundings per sum in the worst order, which a row of a few incidences
comes closest to; over iterations the worst case compounds faster than the
device's error does.

Measured wall time of the test functions on an MI355X: 0.18, 0.23 and 0.27 s
for the three parameters of test_sharded_in_process (56 sharded relaxations
each), 0.31 s for test_sharded_every_group, 0.2 s or less for every other;
the module takes 4.3 s. The products are therefore left whole.
"""

import numpy as np
import pytest
# before libhgx loads, so that both use one HIP runtime (torch brings its own)
import torch

import algdist_cases as C

pytestmark = pytest.mark.gpu

KS_OF = lambda k: (k + 4) // 4 * 4  # round_up(k + 1, 4)
NARROW_KS = (1, 3, 4, 7, 8, 10, 11, 12, 15, 16, 19)
LONGS = (C.LONG64, C.LONG512)


@pytest.fixture(scope="module")
def ctxs():
  from hypergraphembedding_amd import _hgx
  cs = [_hgx.Context(0), _hgx.Context(0)]
  yield cs
  for c in cs:
    c.close()


@pytest.fixture(scope="module")
def ctx(ctxs):
  return ctxs[0]


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
    print(f"\nworst err/bound {self.name}: {self.ratio:.3f} at {self.where}")


_REF = {}


def _reference(case, k, dist, iters, extra=0):
  """(x0, y0, x, y, bx, by), computed once per module and left unchanged."""
  key = (case.name, k, dist, iters, extra)
  if key not in _REF:
    x0, y0 = C.case_inputs(case, k, dist)
    x, y, h = C.reference(case.inc, x0, y0, iters)
    _REF[key] = (x0, y0, x, y) + C.bound(case.inc, h, extra)
  return _REF[key]


def _run(ctx, w, case, k, dist, iters, tag=""):
  x0, y0, x, y, bx, by = _reference(case, k, dist, iters)
  gx, gy = ctx.alg_dist(x0, y0, iters)
  where = (case.name, k, dist, iters, tag)
  w.check(gx, x, bx, where + ("node",))
  w.check(gy, y, by, where + ("edge",))
  return gx, gy


def _thinned(ks):
  """(k, iterations, distribution): every k runs 1, 2 and 3 iterations and
  all three distributions, rotated by the position of k."""
  for i, k in enumerate(ks):
    for it in (1, 2, 3):
      yield k, it, C.DISTS[(i + it) % 3]


@pytest.mark.parametrize("case", C.SEVEN, ids=lambda c: c.name)
def test_quad_and_narrow_every_width_and_group(ctx, case):
  """KS 4 ... 20 at this graph's G on either side. Both k of a KS run every
  iteration count and every distribution, so each (KS, G, side) keeps the
  three iteration counts and each (KS, G) the three distributions."""
  w = Worst("quad_and_narrow " + case.name)
  ctx.upload(case.inc)
  assert {KS_OF(k) for k in NARROW_KS} == {4, 8, 12, 16, 20}
  for k, it, dist in _thinned(NARROW_KS):
    _run(ctx, w, case, k, dist, it)
  w.report()


def test_small_graph_fewer_rows_than_a_workgroup(ctx):
  w = Worst("small_graph")
  ctx.upload(C.SMALL.inc)
  for k, it, dist in _thinned((3, 7, 10, 15, 19)):
    _run(ctx, w, C.SMALL, k, dist, it)
  w.report()


def test_row_width_tuning(ctx):
  w = Worst("row_width_tuning")
  try:
    for i, case in enumerate(C.SEVEN):
      ctx.upload(case.inc)
      for k, widths in ((3, (8, 12, 16, 20)), (10, (16, 20))):
        for j, ks in enumerate(widths):
          ctx.set_tuning("alg_ks", ks)
          _run(ctx, w, case, k, C.DISTS[(i + j) % 3], 1 + (i + j) % 3,
               f"alg_ks={ks}")
  finally:
    ctx.set_tuning("alg_ks", 0)
  w.report()


def test_wide(ctx):
  from hypergraphembedding_amd._hgx import HgxError
  w = Worst("wide")
  inc = C.SMALL.inc
  ctx.upload(inc)
  for i, k in enumerate((20, 23, 255, 256, 300, 2046)):
    for it in (1, 2):
      _run(ctx, w, C.SMALL, k, C.DISTS[(i + it) % 3], it)
  with pytest.raises(HgxError):
    ctx.alg_set(np.zeros((inc.N, 2047), np.float32),
                np.zeros((inc.E, 2047), np.float32))
  w.report()


def test_long_rows(ctx):
  """Pieces of seg_partial, rows of long_finish: 65, 128, 129, 4097 under
  alg_long = 64 (2, 2, 3, 65 pieces) and 512 as one row; 513, 1025 under
  the default (2, 3 pieces) and 512 as one row; each graph under the other
  threshold too (4097 as 9 pieces of 512; 512, 513, 1025 as 8, 9, 17 of 64)."""
  w = Worst("long_rows")
  try:
    for thresh in (64, 0):
      ctx.set_tuning("alg_long", thresh)
      for case in LONGS:
        ctx.upload(case.inc)  # long rows are split at upload
        for i, k in enumerate((3, 7, 10, 15, 19)):
          _run(ctx, w, case, k, C.LONG_DISTS[(i + (thresh > 0)) % 3], 1,
               f"alg_long={thresh}")
        # a real offset of 100 on the long rows (outside the mutant condition)
        _run(ctx, w, case, 10, "off100", 1, f"alg_long={thresh}")
  finally:
    ctx.set_tuning("alg_long", 0)
  w.report()


def _assert_pushes(case, k, thresh=C.DEFAULT_LONG):
  """hgx_alg_run takes the push form only at KS <= 16 and without a long
  node row; otherwise it quietly gathers."""
  assert KS_OF(k) <= 16 and case.inc.node_degree().max() <= thresh


def test_push_form(ctx):
  w = Worst("push_form")
  try:
    differs = 0
    for case in C.SEVEN:
      ctx.set_tuning("alg_push", 1)
      ctx.upload(case.inc)
      for k, it, dist in _thinned((3, 7, 10, 15)):
        _assert_pushes(case, k)
        px, py = _run(ctx, w, case, k, dist, it, "push")
      # the push and stream kernels ran: they round differently from gather
      ctx.set_tuning("alg_push", 0)
      gx, gy = _run(ctx, w, case, k, dist, it, "gather")
      differs += not (np.array_equal(px, gx) and np.array_equal(py, gy))
    assert differs > 0
    # long edge rows: the PRE piece kernel reads the contribution rows
    ctx.set_tuning("alg_push", 1)
    for thresh, case in ((64, C.LONG64), (0, C.LONG512)):
      ctx.set_tuning("alg_long", thresh)
      ctx.upload(case.inc)
      for i, k in enumerate((3, 7, 10, 15)):
        _assert_pushes(case, k, case.long_thresh)
        _run(ctx, w, case, k, C.LONG_DISTS[i % 3], 1, "push, long edge rows")
      _run(ctx, w, case, 10, "off100", 1, "push, long edge rows")
    # a long node row: the library falls back to the gather form
    ctx.set_tuning("alg_long", 0)
    case = C.LONGNODE
    ctx.upload(case.inc)
    assert case.inc.node_degree().max() > C.DEFAULT_LONG
    for i, k in enumerate((3, 10)):
      ctx.set_tuning("alg_push", 1)
      px, py = _run(ctx, w, case, k, C.DISTS[i], 1, "push, long node row")
      ctx.set_tuning("alg_push", 0)
      gx, gy = _run(ctx, w, case, k, C.DISTS[i], 1, "gather, long node row")
      assert np.array_equal(px, gx) and np.array_equal(py, gy)
  finally:
    ctx.set_tuning("alg_push", 0)
    ctx.set_tuning("alg_long", 0)
  w.report()


def test_grid_stride(ctx):
  w = Worst("grid_stride")
  ctx.upload(C.GRID.inc)
  _run(ctx, w, C.GRID, 3, "sym", 1)
  w.report()


# ---- sharded form, two contexts on one device ----

def _sharded(ctxs, case, k, dist, iters, split, compact, ranges, w):
  """Drives hgx_alg_shard_* on two contexts; the test does the exchange
  (sum of the partials or wire rows, elementwise max of the min/max words)
  with both sides synchronised before and after."""
  dev = torch.device("cuda", ctxs[0].device)
  inc = case.inc
  x0, y0, x, y, bx, by = _reference(case, k, dist, iters, extra=1)
  E = inc.E
  ks_max = KS_OF(k)
  ks_max = max(ks_max, 20) if ks_max <= 20 else ks_max
  rows = [(0, split), (split, inc.N)]
  part = [torch.zeros(E * ks_max, dtype=torch.float32, device=dev)
          for _ in ctxs]
  mm = [torch.zeros(iters * 2 * ks_max * 64, dtype=torch.int32, device=dev)
        for _ in ctxs]

  def sync():
    for c in ctxs:
      c.synchronize()
    torch.cuda.synchronize(dev)

  slots = None
  if compact:
    touched = []
    for r0, r1 in rows:
      t = np.zeros(E, np.int32)
      t[inc.col_n[inc.rp_n[r0]:inc.rp_n[r1]]] = 1
      touched.append(t)
    shared = touched[0] + touched[1] >= 2
    n_shared = int(shared.sum())
    slots = [np.where(shared, np.cumsum(shared) - 1,
                      np.where(t == 1, -1, -2)).astype(np.int32)
             for t in touched]
    wire = [torch.zeros(max(n_shared, 1) * (k + 1), dtype=torch.float32,
                        device=dev)[:n_shared * (k + 1)] for _ in ctxs]
  sync()
  for c in ctxs:
    c.alg_set(x0, y0)
  ks = [c.alg_shard_begin(r0, r1, p.data_ptr(), m.data_ptr(), iters)
        for c, (r0, r1), p, m in zip(ctxs, rows, part, mm)]
  assert ks[0] == ks[1] <= ks_max
  ks = ks[0]
  M = 2 * ks * 64
  if compact:
    for c, wr, sl in zip(ctxs, wire, slots):
      c.alg_shard_wire(wr.data_ptr() if n_shared else None, n_shared, sl)
  if ranges > 1:
    b = [c.alg_shard_ranges(ranges) for c in ctxs]
    assert np.array_equal(b[0], b[1])
  exch = wire if compact else [p[:E * ks] for p in part]
  for it in range(iters):
    for c in ctxs:
      c.alg_shard_node(it)
      if ranges > 1:
        for r in range(ranges):
          c.alg_shard_edge_partial_range(it, r)
      else:
        c.alg_shard_edge_partial(it)
    sync()
    if exch[0].numel():
      s = exch[0] + exch[1]
      exch[0].copy_(s)
      exch[1].copy_(s)
    sync()
    for c in ctxs:
      c.alg_shard_edge_final(it)
    sync()
    s = torch.maximum(mm[0][it * M:(it + 1) * M], mm[1][it * M:(it + 1) * M])
    for m in mm:
      m[it * M:(it + 1) * M].copy_(s)
    sync()
  for c in ctxs:
    c.alg_shard_end()
  out = [c.alg_get() for c in ctxs]
  where = (case.name, k, dist, iters, f"split={split}",
           "compact" if compact else "dense", f"ranges={ranges}")
  for g, ((r0, r1), (gx, gy)) in enumerate(zip(rows, out)):
    w.check(gx[r0:r1], x[r0:r1], bx[r0:r1], where + (f"rank{g}", "node"))
    own = np.ones(E, bool) if slots is None else slots[g] != -2
    w.check(gy[own], y[own], by[own], where + (f"rank{g}", "edge"))
  both = (np.ones(E, bool) if slots is None
          else (slots[0] != -2) & (slots[1] != -2))
  assert np.array_equal(out[0][1][both], out[1][1][both]), where


def test_sharded_every_group(ctxs):
  """MODE_PARTIAL of the quad and narrow kernels at every KS and every G of
  the edge side: the seven graphs, dense exchange, an uneven split."""
  w = Worst("sharded_every_group")
  for i, case in enumerate(C.SEVEN):
    for c in ctxs:
      c.upload(case.inc)
    for j, k in enumerate((3, 7, 10, 15, 19)):
      _sharded(ctxs, case, k, C.DISTS[(i + j) % 3], 2, case.inc.N // 3,
               False, 1, w)
  w.report()


@pytest.mark.parametrize("case", [C.SEVEN[2], C.SEVEN[5], C.LONG64],
                         ids=lambda c: c.name)
def test_sharded_in_process(ctxs, case):
  w = Worst("sharded_in_process " + case.name)
  iters = 2 if len(case.iters) > 1 else 1
  dists = C.LONG_DISTS + ("off100",) if case is C.LONG64 else C.DISTS
  try:
    for c in ctxs:
      if case is C.LONG64:
        c.set_tuning("alg_long", 64)
      c.upload(case.inc)
    n = 0
    for k in (3, 7, 10, 15, 19, 24, 300):
      for split in (case.inc.N // 3, 0):  # uneven; rank 0 owns no row
        for compact in (False, True):
          for ranges in (1, 3):
            _sharded(ctxs, case, k, dists[n % len(dists)], iters, split,
                     compact, ranges, w)
            n += 1
  finally:
    for c in ctxs:
      c.set_tuning("alg_long", 0)
  w.report()
