"""Interleaved A/B of the trainer step's quad form (tuning `train_wave_pair`:
1 one record on two waves, 3 on four waves with 2 records per 512-thread
workgroup, 4 on four waves with 1 record per 256-thread workgroup; arms the
library does not build, such as the 4-record geometry 2
of the first measurements, are skipped) in one process: epochs alternate between
the settings on the same records and initial model, per-batch device time
(hgx_train_last_stats, HIP events) per setting. Diagnostic only.

  python tools/ab_wave_quad.py 128 [rounds=6]         d = 128, C3 HOBE records
  python tools/ab_wave_quad.py 256 [rounds=6] [frac=0.02]
                                                      d = 256, the C4 HOBE slice

The rule for a geometry's default: a quad arm faster than the
paired arm in every alternation, and its mean gain at least three standard
deviations of the paired arm's runs. Round 0 (warm-up) is not counted."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hypergraphembedding_amd import _hgx  # noqa: E402
from hypergraphembedding_amd.synthetic import powerlaw_hypergraph, random_hypergraph  # noqa: E402

d = int(sys.argv[1]) if len(sys.argv) > 1 else 128
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
frac = float(sys.argv[3]) if len(sys.argv) > 3 else 0.02
ctx = _hgx.Context(0)
ARMS = [1]
for arm in (2, 3, 4):
  try:
    ctx.set_tuning("train_wave_pair", arm)
    ARMS.append(arm)
  except Exception:
    pass
if d == 128:  # C3: random 100k/50k graph, 2M of its HOBE records
  inc = random_hypergraph(seed=0)
  ctx.upload(inc)
  r = np.random.RandomState(4)
  ctx.alg_set(r.random_sample((inc.N, 10)), r.random_sample((inc.E, 10)))
  ctx.alg_run(20)
  m = ctx.sample_hobe(17, 5, 200)
  idx, tgt = ctx.records_get()
  sel = np.random.RandomState(1).permutation(m)[:2_000_000]
  ctx.records_set(np.ascontiguousarray(idx[sel]), np.ascontiguousarray(tgt[sel]))
  n = len(sel)
else:  # C4: power-law 10M/5M, a seeded row slice, full-size tables
  inc = powerlaw_hypergraph(seed=0)
  ctx.upload(inc)
  r = np.random.RandomState(1)
  ctx.alg_set(r.random_sample((inc.N, 10)).astype(np.float32),
              r.random_sample((inc.E, 10)).astype(np.float32))
  ctx.alg_run(20)
  rq = np.random.RandomState(2)
  nq = np.where(rq.random_sample(inc.N) < frac, 200, 0).astype(np.int32)
  eq = np.where(rq.random_sample(inc.E) < frac, 200, 0).astype(np.int32)
  n = ctx.sample_hobe(4000, 5, 200, node_q=nq, edge_q=eq)
print(json.dumps({"d": d, "records": int(n)}), flush=True)
res = {arm: [] for arm in ARMS}
for rnd in range(rounds + 1):
  for arm in ARMS:
    ctx.set_tuning("train_wave_pair", arm)
    ctx.model_init(d, inc.N + 2, inc.E + 2, seed=11)
    ctx.train(batch=256, max_epochs=1, loss=_hgx.LOSS_MSE, act=_hgx.ACT_RELU,
              min_delta=-1e30, shuffle_seed=2)
    ms, rec, bat = ctx.train_stats()
    us = ms * 1e3 / bat
    if rnd > 0:
      res[arm].append(us)
    print(json.dumps({"round": rnd, "arm": arm, "per_batch_us": round(us, 4),
                      "geometry": ctx.train_step_geometry(),
                      "loss": float(ctx.train_loss_sum() / rec)}), flush=True)
p = np.array(res[1])
out = {"d": d, "paired_us": {"mean": round(float(p.mean()), 4),
                             "std": round(float(p.std(ddof=1)), 4)}}
for arm in ARMS[1:]:
  u = np.array(res[arm])
  gain = p - u
  out[f"quad{arm}"] = {
      "us": {"mean": round(float(u.mean()), 4), "std": round(float(u.std(ddof=1)), 4)},
      "gain_us": {"mean": round(float(gain.mean()), 4), "min": round(float(gain.min()), 4)},
      "faster_every_round": bool((gain > 0).all()),
      "gain_over_3_sigma": bool(gain.mean() >= 3 * p.std(ddof=1)),
  }
print(json.dumps(out), flush=True)
ctx.close()
