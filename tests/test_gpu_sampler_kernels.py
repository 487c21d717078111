"""GPU: the keyed samplers' whole record stream against its host definition.

tests/sampler_cases.py restates the sampler (csrc/hgx_sample.hip) from its
header comment: the proposals follow the hash arithmetic, acceptance comes
from the definition by enumerating a row's paths, pass 2 keeps the smallest
keys. The sampler is deterministic for a seed, so the device's idx array
must equal that prediction record for record: for every case graph there
(small, hub, big, full, stall, wide), every family (FOBE with negatives at
K = 1, 5, 16; HOBE with row quotas on the small graph; the weighted-Jaccard
pair blocks, which sample the same four patterns, wherever a graph has an
isolated node or an empty edge and so cannot have HOBE coordinates) and
every tuning setting a case names (expansion only, rejection of every row,
a threshold that splits the rows, forced and automatic 3-hop modes with
positive and negative shifts that differ between node and edge rows), plus
the 724,792 records of the tiny graph. The statistics the device reports
(rejection rows, stall fallbacks, uniform-column rows) and the kind-block
bounds must equal the predicted ones, and the chosen columns must ascend
within a row.

That the restatement itself draws uniform subsets, and that the cases reach
every branch of the kernels, is tested without a device in
tests/test_sampler_cases_cpu.py.

With HGX_SAMPLER_EXACT_OUT set to a file name, every test appends the number
of records it compared and of mismatches (profiles/samplers/gpu_exact.txt)."""

import os

import numpy as np
import pytest

import oracle as O
import sampler_cases as S
from conftest import golden

pytestmark = pytest.mark.gpu

CASES = S.cases()
RUNS = [(name, run[0]) for name, case in CASES.items() for run in case["runs"]]


@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.close()


def _note(line):
  out = os.environ.get("HGX_SAMPLER_EXACT_OUT")
  print(line)
  if out:
    with open(out, "a") as fh:
      fh.write(line + "\n")


def _row_of(rec):
  """(kind, row, column) of an idx record."""
  ln, le, rn, re = (int(x) for x in rec[:4])
  if ln and rn:
    return "nn", ln - 1, rn - 1
  if le and re:
    return "ee", le - 1, re - 1
  return "ne", ln - 1, re - 1


def _compare(what, got, want, bounds, traces):
  """Record-for-record equality; on a mismatch, the first differing record,
  its block, row and the restatement's trace for that row."""
  n = min(got.shape[0], want.shape[0])
  same_shape = got.shape == want.shape
  bad = np.nonzero(np.any(got[:n] != want[:n], 1))[0] if got.shape[1] == want.shape[1] else \
      np.arange(n)
  nbad = int(bad.size) + abs(got.shape[0] - want.shape[0])
  _note("%s: %d records compared, %d mismatches" % (what, want.shape[0], nbad))
  if same_shape and nbad == 0:
    return
  msg = ["%s: device %s, restatement %s, %d mismatching records" %
         (what, got.shape, want.shape, nbad), "block bounds %s" % (bounds,)]
  if bad.size:
    i = int(bad[0])
    block = int(np.searchsorted(bounds, i, side="right")) - 1
    msg.append("first difference at record %d (block %d):" % (i, block))
    msg.append("  device      %s" % got[i].tolist())
    msg.append("  restatement %s" % want[i].tolist())
    kind, r, c = _row_of(want[i])
    msg.append("  restatement's record: %s row/col (%d, %d)" % (kind, r, c))
    pat = {0: (S.PAT_NN,), 1: (S.PAT_EE,), 2: (S.PAT_A, S.PAT_NNE), 3: (S.PAT_AT, S.PAT_EEN)}
    rows = {r, c}
    for tr in traces:
      if tr["pattern"] in pat.get(block, ()) and tr["row"] in rows:
        msg.append("  trace %s" % {k: v for k, v in tr.items()})
  pytest.fail("\n".join(msg))


def _check_ascending(idx, bounds):
  """Positive blocks: rows ascending, columns strictly ascending in a row."""
  for b, (rc, cc) in enumerate(((0, 2), (1, 3), (0, 3), (3, 0))):
    blk = idx[bounds[b]:bounds[b + 1]].astype(np.int64)
    key = blk[:, rc] * (1 << 32) + blk[:, cc]
    assert np.all(np.diff(key) > 0), "block %d is not ascending" % b


def _set(ctx, tuning):
  for k, v in tuning.items():
    ctx.set_tuning(k, v)


def _sample(ctx, case, run, seed):
  label, family, _, K, quotas, negatives, tuning = run
  inc = case["inc"]
  ctx.upload(inc)
  if family == "hobe":
    # (only the small graph: coordinates need a graph without isolated rows)
    z = golden("hobe_small.npz")
    ctx.alg_set(z["alg_x"], z["alg_y"])
  elif family == "pairs4":
    one = np.ones(inc.nnz, np.float32)
    ctx.features_set(one, one)
  try:
    _set(ctx, tuning)
    if family == "fobe":
      neg = negatives or (None, None)
      n = ctx.sample_fobe(seed, K, quotas[0], quotas[1], neg[0], neg[1])
    elif family == "hobe":
      n = ctx.sample_hobe(seed, K, 0, node_q=quotas[0], edge_q=quotas[1])
    else:
      n = ctx.sample_jaccard(seed, K, quotas[0], quotas[1])
    stats = ctx.sample_stats() + (ctx.sample_uniform_rows(),)
  finally:
    _set(ctx, S.DEFAULT_TUNING)
  idx, tgt = ctx.records_get()
  assert n == idx.shape[0]
  return idx, tgt, stats


@pytest.mark.parametrize("name,label", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_stream_equals_restatement(ctx, name, label):
  case = CASES[name]
  run = next(r for r in case["runs"] if r[0] == label)
  seed = S.run_seed(case, run)
  traces = []
  want, wstats, bounds = S.run_stream(case, run, traces)
  idx, tgt, stats = _sample(ctx, case, run, seed)
  _compare("%s / %s" % (name, label), idx, want, bounds, traces)
  assert stats == tuple(int(s) for s in wstats), (stats, wstats)
  assert ctx.records_blocks().tolist() == bounds
  _check_ascending(idx, bounds)
  if name == "small" and run[1] == "hobe":
    # the probabilities of these pairs, as in test_hobe_small_counts_and_probs
    z = golden("hobe_small.npz")
    inc = case["inc"]
    for kind, col, (b, e), (rc, cc) in ((O.HOBE_NN, 0, bounds[0:2], (0, 2)),
                                        (O.HOBE_EE, 1, bounds[1:3], (1, 3)),
                                        (O.HOBE_NE, 2, (bounds[2], bounds[4]), (0, 3))):
      p = O.hobe_probs(kind, idx[b:e, rc] - 1, idx[b:e, cc] - 1, inc, z["alg_x"], z["alg_y"])
      assert np.array_equal(tgt[b:e, col], p), kind


def test_tiny_fobe_expansion_stream(ctx, tiny_inc):
  """The call of test_fobe_tiny_counts_validity with every row expanded: all
  724,792 records (1- and 2-hop expansion, neighbour lists)."""
  inc = tiny_inc
  nq = np.full(inc.N, 200, np.int32)
  eq = np.full(inc.E, 200, np.int32)
  tuning = S._t(reject_w=0)
  want, wstats, bounds = S.stream(inc, "fobe", 7, 5, (nq, eq), None, tuning)
  assert want.shape[0] == 724792
  case = dict(inc=inc)
  idx, _, stats = _sample(ctx, case, ("tiny", "fobe", 7, 5, (nq, eq), None, tuning), 7)
  _compare("tiny / fobe-expand", idx, want, bounds, [])
  assert stats == (0, 0, 0)
  _check_ascending(idx, bounds)


def test_hub_negative_on_empty_endpoint_raises(ctx):
  """The first seed at which the restatement draws a node-edge negative with
  an endpoint without neighbours (the empty edge, the isolated node): the
  device raises there, as np.random.choice does in the reference."""
  case = CASES["hub"]
  run = next(r for r in case["runs"] if r[0] == "fobe-K5")
  _, _, _, K, quotas, negatives, tuning = run
  seed = None
  for s in range(53, 53 + 64):
    try:
      S.stream(case["inc"], "fobe", s, K, quotas, negatives, S._t(reject_w=0))
    except ValueError:
      seed = s
      break
  assert seed is not None
  with pytest.raises(ValueError):
    _sample(ctx, case, run, seed)
