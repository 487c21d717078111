#!/usr/bin/env python
"""LINE baseline on the C2 graph (random 100k x 50k, bench.py's): one JSON
line with the samples/s of the edge-sampling trainer, d = 128, K = 5
negatives, both orders: the concurrent mode at each `line_chunk_samples` of
`--chunks` (0 = the default from the vertex count), and the sequential mode
(one wave) over `--seq-samples`. Times are hgx_n2v_last_stats' train_ms (HIP
events around the launches); every figure is the median of `--repeats` runs
after one warm-up run of the same shape, with the least and the largest
beside it. The derived atomic bytes/s = samples/s x (K + 2) x 4 x padded d
(every target row and the closing row of u, one float atomic per column) is
set against the chip-wide rate of global float atomic adds, about 1.3 TB/s,
which at d = 128 and K = 5 is about 360 M samples/s. A measurement for
DESIGN §4.12, not a gate: there is no earlier LINE to compare with.

  python tools/line_bench.py [--dim 128] [--negative 5] [--samples 8000000]
                             [--seq-samples 20000] [--repeats 5]
                             [--chunks 0,4096,16384,65536,262144]
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ATOMIC_RATE = 1.3e12  # bytes/s of global float atomic adds, chip-wide


def timed(be, init, order, K, T, conc, repeats):
  ms, st = [], None
  for i in range(repeats + 1):
    be.set_vectors(init, None)
    be.train_line(order, K, T, rho=0.025, seed=2, concurrent=conc)
    st = be.stats()
    assert st["samples"] == T
    if i:  # run 0 warms the shape up
      ms.append(st["train_ms"])
  syn0, syn1 = be.get_vectors()
  return ms, st, bool(np.all(np.isfinite(syn0)) and np.all(np.isfinite(syn1)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dim", type=int, default=128)
  ap.add_argument("--negative", type=int, default=5)
  ap.add_argument("--samples", type=int, default=8_000_000)
  ap.add_argument("--seq-samples", type=int, default=20000)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--chunks", default="0,4096,16384,65536,262144")
  args = ap.parse_args()
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd import line as L
  from hypergraphembedding_amd import node2vec as n2v
  from hypergraphembedding_amd.synthetic import random_hypergraph

  inc = random_hypergraph(seed=0)
  ctx = _hgx.Context(0)
  ctx.upload(inc)
  d, K = args.dim, args.negative
  V = inc.N + inc.E
  dp = 64
  while dp < d:
    dp *= 2
  row_bytes = (K + 2) * 4 * dp
  default_chunk = min(65536, max(256, V // 4 // 256 * 256))
  out = {"workload": "LINE baseline, C2 graph %d x %d (nnz %d), d = %d, "
                     "negative %d, unit weights" % (inc.N, inc.E, inc.nnz, d, K),
         "vertices": V, "padded_dim": dp, "atomic_bytes_per_sample": row_bytes,
         "atomic_rate_bytes_per_s": ATOMIC_RATE,
         "samples_per_s_at_atomic_rate": ATOMIC_RATE / row_bytes,
         "default_chunk": default_chunk, "repeats": args.repeats}
  np.random.seed(0)
  init = (np.random.random((V, d)).astype(np.float32) - 0.5) / d
  cum = n2v.cum_table(L.line_degrees(inc), 0.75)
  with _hgx.N2v(ctx, L.BIPARTITE, d) as be:
    be.set_arcs(None, None, cum)
    for order in (1, 2):
      res = {"concurrent": [], "sequential": None}
      for chunk in [int(c) for c in args.chunks.split(",")]:
        ctx.set_tuning("line_chunk_samples", chunk)
        ms, st, finite = timed(be, init, order, K, args.samples, True,
                               args.repeats)
        med = float(np.median(ms))
        rate = args.samples / med * 1e3
        res["concurrent"].append({
            "line_chunk_samples": chunk,
            "samples_per_launch": chunk or default_chunk,
            "samples": args.samples, "train_ms": med,
            "train_ms_min": min(ms), "train_ms_max": max(ms),
            "samples_per_s": rate, "atomic_bytes_per_s": rate * row_bytes,
            "share_of_atomic_rate": rate * row_bytes / ATOMIC_RATE,
            "clamped": st["clamped"], "finite": finite})
      ctx.set_tuning("line_chunk_samples", 0)
      ms, st, finite = timed(be, init, order, K, args.seq_samples, False,
                             args.repeats)
      med = float(np.median(ms))
      res["sequential"] = {"samples": args.seq_samples, "train_ms": med,
                           "train_ms_min": min(ms), "train_ms_max": max(ms),
                           "samples_per_s": args.seq_samples / med * 1e3,
                           "clamped": st["clamped"], "finite": finite}
      out["order%d" % order] = res
  ctx.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
