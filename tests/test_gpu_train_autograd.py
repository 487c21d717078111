"""GPU: ctx.train against the float64 autograd reference (hg2v_autograd.py)
directly, at three Adagrad settings -- Keras' (0.01, 1e-7), where a constant
factor on every gradient cancels; (1, 10), where the step is proportional to
the gradient; lr = 0.01 with eps of the size of sqrt(a), where both show --
over every kernel instantiation hgx_train selects for d <= 1024, K <= 16.

Each case: n = 2 batch + 1 records in order (three batches, the last of one
record; batch = 256, or 200 at K = 16, where 256 records exceed the 8,192
slots hgx_train prepares per batch), 2 epochs, min_delta = -1, tables of 64
rows (the hub cases: 2,000). K = 8 and 9 at 256 records are the batches of
more than 4,096 slots (the bitonic preparation at P = 8,192).

Inputs. Rows are s_r (u + noise), s_r = +-1: every relu pre-activation the
REFERENCE sees in any batch is either an exact constructed value (0 from rows
of disjoint support, 2^-20) or has |z| >= 16 d 2^-24 sum |a_i b_i|, asserted
before the device is touched, so no float32 summation order can put a head
on the other side of its kink.

Bar. Per case, setting and table, E = the larger of the two hgref_train
summation orders' max-abs distances from the reference: the float32 floor of
a correct implementation, computed here. The device must be within
8 E + 2 ulp32(max |p|) elementwise (8 x: the suite's convention for a
float32 floor, as 8 x amb in test_gpu_c4.py; it also covers the hardware
rcp / sqrt of the step) and its epoch losses within rtol 1e-4.

Which case reaches which instantiation (L lanes x VPL float4 per lane):
  train_fwd_bwd generic K <= 2 / 5 / 8 / 16 at every geometry:
    test_generic_widths_every_geometry (d = 2, 5, 24, 64, 256, 512, 1024 x
    K = 2, 3, 8, 16) and test_k_sweep (d = 16, 128 x K = 1 ... 16; K = 1, 3
    and 9 run below their template's width); the 5-wide generic kernel with
    K = 5 by the mixed head pairs of test_loss_act_pairs;
  train_fwd_bwd specialised K = 5 (KLD + sigmoid, MSE + relu), 256 threads
    for L < 64 and 512 for L = 64: test_d_sweep (d = 1, 2 -> L 1; 5 -> 2;
    16 -> 4; 24 -> 8; 64 -> 16; 257, 512 -> 64 x 2; 1000, 1024 -> 64 x 4)
    and its fused = 0 cases (65, 100, 128 -> 32; 129, 255, 256 -> 64);
  train_update at every geometry: the same cases;
  train_step / train_flush (d in 65 ... 256, K = 5, matched heads):
    test_d_sweep fused = 1 (float2 x 64 lanes at 256 threads for dp = 128,
    float4 x 64 lanes for dp = 256), test_step_geometries (float4 x 32 lanes
    at 128 and 256 threads, float2 x 64 lanes at 128, 256 and 512), and their
    MULTI pending-slot forms by test_hub_batches at each of those.

Measured max |device - reference| / E on an MI355X (max over both tables and
the cases of each test; the bar is 8 plus the ulp term):

  test                                  (0.01, 1e-7)   (1, 10)   mid eps
  test_k_sweep                              4.48         1.00      1.13
  test_d_sweep                              3.14         1.17      1.06
  test_generic_widths_every_geometry        1.49         1.00      1.18
  test_small_batches, batch 1               1.00         1.25      1.00
  test_small_batches, batch 37              2.83         1.03      1.05
  test_loss_act_pairs                       2.61         1.08      1.18
  test_step_geometries                      1.39         1.00      1.00
  test_hub_batches                          1.00         1.00      1.00
  test_edge_records_single_batch            1.15         1.00      1.47

The largest, 4.48 (K = 9, d = 128, KLD + sigmoid, node table), is 0.55 of its
bar. At eps = 1e-7 an element whose gradient nearly cancels over the batch
turns a float32 rounding difference dg into lr dg / eps: every float32
summation order, the oracle's two included, lands somewhere else on such an
element, which is what E measures.
"""

import numpy as np
import pytest

import hg2v_autograd as A
import oracle as O

pytestmark = pytest.mark.gpu

KLD_SIG = (O.LOSS_KLD, O.ACT_SIGMOID)
MSE_RELU = (O.LOSS_MSE, O.ACT_RELU)
MODELS = {"kld-sig": KLD_SIG, "mse-relu": MSE_RELU}
PAIRS = dict(MODELS, **{"kld-relu": (O.LOSS_KLD, O.ACT_RELU),
                        "mse-sig": (O.LOSS_MSE, O.ACT_SIGMOID)})
EPOCHS = 2

@pytest.fixture(scope="module")
def ctx():
  from hypergraphembedding_amd import _hgx
  c = _hgx.Context(0)
  yield c
  c.close()


class Case:

  def __init__(self, idx, tgt, K, nt, et, loss, act, batch, epochs=EPOCHS):
    self.idx, self.tgt, self.K, self.nt, self.et = idx, tgt, K, nt, et
    self.loss, self.act, self.batch, self.epochs = loss, act, batch, epochs
    self.d = nt.shape[1]
    self.perms = np.tile(np.arange(idx.shape[0]), (epochs, 1))


def make_case(K, d, pair, batch=256, seed=0, rows=64):
  loss, act = pair
  if K == 16:  # hgx_train prepares at most 8,192 slots per batch: 227 records
    batch = min(batch, 200)
  rs = np.random.RandomState(1000 * seed + 16 * d + K)
  nt, et = A.signed_tables(rs, rows, rows, d, A.amp_for(loss, act, d))
  idx, tgt = A.random_records(rs, 2 * batch + 1, K, rows, rows)
  return Case(idx, tgt, K, nt, et, loss, act, batch)


def make_hub_case(d, pair, batch=128, seed=0, rows=2000):
  """Two hub batches (every id from rows 1-5), a wide batch, a ragged one."""
  loss, act = pair
  K = 5
  rs = np.random.RandomState(77 + seed + d)
  nt, et = A.signed_tables(rs, rows, rows, d, A.amp_for(loss, act, d))
  parts = [A.random_records(rs, batch, K, 6, 6),
           A.random_records(rs, batch, K, 6, 6),
           A.random_records(rs, batch, K, rows, rows),
           A.random_records(rs, 37, K, rows, rows)]
  idx = np.concatenate([p[0] for p in parts])
  tgt = np.concatenate([p[1] for p in parts])
  return Case(idx, tgt, K, nt, et, loss, act, batch)


def make_edge_case(d, pair, seed=0):
  loss, act = pair
  idx, tgt, nt, et = A.edge_batch(np.random.RandomState(3 + seed), d, 5, loss,
                                  act)
  return Case(idx, tgt, 5, nt, et, loss, act, 256, epochs=1)


def settings(c):
  e3, med = A.mid_eps(c.idx, c.tgt, c.K, c.nt, c.et, c.loss, c.act, c.batch)
  assert med / 10 <= e3 <= med * 10, (e3, med)
  return (("keras", 0.01, 1e-7), ("prop", 1.0, 10.0), ("mid", 0.01, e3))


def reference(c, lr, eps):
  """The float64 reference, the input condition, and the float32 floor E of
  the two hgref_train summation orders (per table)."""
  ref = A.train(c.idx, c.tgt, c.K, c.nt, c.et, c.loss, c.act, batch=c.batch,
                lr=lr, eps=eps, epochs=c.epochs, perms=c.perms)
  if c.act == O.ACT_RELU:
    m = A.relu_margin(ref, c.d)
    assert m >= 1.0, ("relu pre-activation too close to 0 for float32", m)
  E = [0.0, 0.0]
  for f64 in (False, True):
    o = O.train(c.idx, c.tgt, c.K, c.nt, c.et, c.loss, c.act, batch=c.batch,
                lr=lr, eps=eps, max_epochs=c.epochs, perms=c.perms,
                min_delta=-1.0, dup_f64=f64)
    for t, r in enumerate((ref.nt, ref.et)):
      E[t] = max(E[t], float(np.abs(o[t] - r).max()))
  return ref, E


def device(ctx, c, lr, eps):
  ctx.records_set(c.idx, c.tgt)
  ctx.model_init(c.d, c.nt.shape[0], c.et.shape[0], node_tab=c.nt,
                 edge_tab=c.et)
  gl = ctx.train(batch=c.batch, max_epochs=c.epochs, lr=lr, eps=eps, loss=c.loss,
                 act=c.act, perms=c.perms, min_delta=-1.0)
  return ctx.model_get() + (gl,)


def check(c, run, tag, path=None):
  """run(lr, eps) -> (node table, edge table, epoch losses[, path stats])."""
  worst = 0.0
  nb = c.epochs * -(-c.idx.shape[0] // c.batch)
  for name, lr, eps in settings(c):
    ref, E = reference(c, lr, eps)
    out = run(lr, eps)
    for t, r in enumerate((ref.nt, ref.et)):
      err = np.abs(out[t].astype(np.float64) - r)
      bar = 8 * E[t] + 2 * A.ulp32(np.abs(r).max())
      ratio = err.max() / E[t] if E[t] > 0 else 0.0
      worst = max(worst, ratio)
      r_, c_ = np.unravel_index(err.argmax(), err.shape)
      print(f"RATIO {tag} {name} table {t}: device {err.max():.3g} E "
            f"{E[t]:.3g} ratio {ratio:.2f} bar {bar:.3g} at row {r_} col {c_}")
      assert err.max() <= bar, (tag, name, t, err.max(), E[t], bar, r_, c_)
      assert not np.array_equal(out[t], (c.nt, c.et)[t])
    assert out[2].shape == ref.losses.shape
    assert np.allclose(out[2], ref.losses, rtol=1e-4, atol=0), (tag, name,
                                                                 out[2],
                                                                 ref.losses)
    if path is not None:
      want = (nb, 0) if path == "fused" else (0, nb)
      assert out[3] == want, (tag, name, out[3], want)
  return worst


def step_applies(c):
  return 64 < c.d <= 256 and c.K == 5 and c.loss == c.act


def run_on(ctx, c, tag, fused=1, lanes=(0, 0)):
  ctx.set_tuning("train_fused", fused)
  ctx.set_tuning("train_lanes", lanes[0])
  ctx.set_tuning("train_tb", lanes[1])
  try:
    path = "fused" if fused and step_applies(c) else "split"
    return check(c, lambda lr, eps: device(ctx, c, lr, eps) +
                 (ctx.train_path_stats(),), tag, path)
  finally:
    ctx.set_tuning("train_fused", 1)
    ctx.set_tuning("train_lanes", 0)
    ctx.set_tuning("train_tb", 0)


K_SWEEP = [(K, d, m) for d in (16, 128) for K in (1, 2, 3, 5, 8, 9, 16)
           for m in MODELS]
D_SWEEP = [(d, m, f) for d in (1, 2, 5, 24, 64, 65, 100, 128, 129, 255, 256,
                               257, 512, 1000, 1024)
           for m in MODELS for f in ((1, 0) if 64 < d <= 256 else (1,))]
GENERIC = [(K, d, ("kld-sig", "mse-relu", "mse-sig")[(i + j) % 3])
           for i, d in enumerate((2, 5, 24, 64, 256, 512, 1024))
           for j, K in enumerate((2, 3, 8, 16))]
STEP_GEOMETRIES = [(32, 0), (32, 256), (64, 128), (64, 0), (64, 512)]
LANES_IDS = ["f4x32-tb128", "f4x32-tb256", "f2x64-tb128", "f2x64-tb256",
             "f2x64-tb512"]


@pytest.mark.parametrize("K,d,model", K_SWEEP)
def test_k_sweep(ctx, K, d, model):
  c = make_case(K, d, MODELS[model])
  run_on(ctx, c, f"k_sweep K={K} d={d} {model}")


@pytest.mark.parametrize("d,model,fused", D_SWEEP)
def test_d_sweep(ctx, d, model, fused):
  c = make_case(5, d, MODELS[model], seed=1)
  run_on(ctx, c, f"d_sweep d={d} {model} fused={fused}", fused=fused)


@pytest.mark.parametrize("K,d,pair", GENERIC)
def test_generic_widths_every_geometry(ctx, K, d, pair):
  c = make_case(K, d, PAIRS[pair], seed=2)
  run_on(ctx, c, f"generic K={K} d={d} {pair}")


@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("batch", [1, 37])
@pytest.mark.parametrize("model", list(MODELS))
def test_small_batches(ctx, model, batch, d):
  c = make_case(5, d, MODELS[model], batch=batch, seed=3,
                rows=8 if batch == 1 else 24)
  run_on(ctx, c, f"batch={batch} d={d} {model}")


@pytest.mark.parametrize("d", [16, 128])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_loss_act_pairs(ctx, pair, d):
  c = make_case(5, d, PAIRS[pair], seed=4)
  run_on(ctx, c, f"pairs {pair} d={d}")


@pytest.mark.parametrize("lanes", STEP_GEOMETRIES, ids=LANES_IDS)
@pytest.mark.parametrize("d", [100, 128])
@pytest.mark.parametrize("model", list(MODELS))
def test_step_geometries(ctx, model, d, lanes):
  c = make_case(5, d, MODELS[model], seed=5)
  run_on(ctx, c, f"step {lanes} d={d} {model}", lanes=lanes)


HUB = [(128, g) for g in STEP_GEOMETRIES] + [(256, (0, 0))]


@pytest.mark.parametrize("d,lanes", HUB,
                         ids=[f"d{d}-{l[0]}-{l[1]}" for d, l in HUB])
@pytest.mark.parametrize("model", list(MODELS))
def test_hub_batches(ctx, model, d, lanes):
  """Every id of two consecutive batches from five rows (nearly every row
  deferred, records naming several pending rows: the MULTI form), then a wide
  batch (flushes the hub rows it does not touch), then a ragged one."""
  c = make_hub_case(d, MODELS[model])
  seen = []

  def run(lr, eps):
    out = device(ctx, c, lr, eps)
    seen.append(ctx.train_multi_pending())
    return out + (ctx.train_path_stats(),)

  ctx.set_tuning("train_lanes", lanes[0])
  ctx.set_tuning("train_tb", lanes[1])
  try:
    check(c, run, f"hub d={d} {lanes} {model}", "fused")
  finally:
    ctx.set_tuning("train_lanes", 0)
    ctx.set_tuning("train_tb", 0)
  assert all(v > 0 for v in seen), seen


@pytest.mark.parametrize("d,fused", [(16, 1), (128, 1), (128, 0)])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_edge_records_single_batch(ctx, pair, d, fused):
  """hg2v_autograd.edge_batch in one batch, so that the constructed
  pre-activations hold exactly: relu z == 0 (gradient 0) and z == 2^-20
  (gradient 1), an ne head with every relu pre-activation <= 0 (P == 0,
  dQ == 0), KLD heads clipped at 1e-7 (sigmoid(-20); P Q at z ~ -8.5),
  sigmoid(40) == 1, ln == rn, le == re, a neighbour equal to ln, repeated
  neighbours, all three targets, row 0 in every inactive slot."""
  c = make_edge_case(d, PAIRS[pair])
  if c.act == O.ACT_RELU:
    z = np.concatenate(A.train(c.idx, c.tgt, 5, c.nt, c.et, c.loss, c.act,
                               batch=c.batch).relu_z)
    assert (z == 0.0).sum() >= 12 and (z == 2.0 ** -20).sum() == 2
  run_on(ctx, c, f"edge {pair} d={d} fused={fused}", fused=fused)
