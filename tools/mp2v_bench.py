#!/usr/bin/env python
"""metapath2vec++ baseline on C1 (the golden youtube_tiny hypergraph, E = 50)
and on the C2 graph (random 100k x 50k, bench.py's): one JSON line with
walk_ms, train_ms and pairs/s of the streamed-corpus trainer at d = 128, K = 5
negatives, window 7, sentences of 201 vertices, one epoch, `--walks1` /
`--walks2` walks per edge (reduced from the usual 1000 so that a run fits a
minute). Concurrent mode over the whole corpus, sequential mode (one wave)
over the first `--seq-sources` edges' walks. Times are hgx_n2v_last_stats'
(HIP events: walk_ms the walk kernels, train_ms the rest of the run); every
figure is the median of `--repeats` runs after one warm-up run of the same
shape, with the least and the largest beside it. The derived atomic bytes/s =
(evaluated targets + pairs) x 4 x padded d / train_ms (every target row and
the closing row of the input word, one float atomic per column; a clamped
target whose update is zero sends none, so the figure is an upper bound) is
set against the chip-wide rate of global float atomic adds, about 1.3 TB/s.
A measurement for DESIGN §4.13, not a gate.

  python tools/mp2v_bench.py [--dim 128] [--walks1 100] [--walks2 1]
                             [--seq-sources 16] [--repeats 3]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ATOMIC_RATE = 1.3e12  # bytes/s of global float atomic adds, chip-wide


def run(ctx, inc, name, d, num_walks, seq_sources, repeats):
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd import metapath2vec as M
  from hypergraphembedding_amd import node2vec as n2v
  K, window, L = 5, 7, 201
  V = inc.N + inc.E
  dp = 64
  while dp < d:
    dp *= 2
  src = M.mp_sources(inc)
  ctx.upload(inc)
  np.random.seed(0)
  init = (np.random.random((V, d)).astype(np.float32) - 0.5) / d
  out = {"graph": name, "N": inc.N, "E": inc.E, "nnz": int(inc.nnz),
         "sources": int(src.size), "num_walks": num_walks,
         "n_walks": int(num_walks * src.size), "L": L, "padded_dim": dp}
  with _hgx.N2v(ctx, M.BIPARTITE, d) as be:
    ms = []
    for i in range(repeats + 1):
      counts = be.mp_counts(src, num_walks, L, 1)
      if i:
        ms.append(be.stats()["walk_ms"])
    out["counts_ms"] = float(np.median(ms))
    out["tokens"] = int(counts.sum())
    live = np.where(counts >= 5, counts, 0)
    be.set_vocab_typed(n2v.keep_thresholds(live, 1e-3),
                       M.typed_cum_table(live, inc.N, True), True)
    for mode, sources, conc in (("concurrent", src, True),
                                ("sequential", src[:seq_sources], False)):
      nw = num_walks if conc else 1
      wm, tm, st = [], [], None
      for i in range(repeats + 1):
        be.set_vectors(init, None)
        be.train_mp(sources, nw, L, window=window, negative=K, epochs=1,
                    alpha=0.025, min_alpha=2.5e-6, walk_seed=1, train_seed=2,
                    concurrent=conc)
        st = be.stats()
        if i:  # run 0 warms the shape up
          wm.append(st["walk_ms"])
          tm.append(st["train_ms"])
      s0, s1 = be.get_vectors()
      mp = st["mp"]
      w, t = float(np.median(wm)), float(np.median(tm))
      nbytes = (mp["targets"] + mp["pairs"]) * 4 * dp
      out[mode] = {
          "walks": mp["walks"], "words": mp["words"], "pairs": mp["pairs"],
          "targets": mp["targets"], "clamped": mp["clamped"],
          "walk_ms": w, "walk_ms_min": min(wm), "walk_ms_max": max(wm),
          "train_ms": t, "train_ms_min": min(tm), "train_ms_max": max(tm),
          "walk_share": w / (w + t), "pairs_per_s": mp["pairs"] / t * 1e3,
          "atomic_bytes_per_s": nbytes / t * 1e3,
          "share_of_atomic_rate": nbytes / t * 1e3 / ATOMIC_RATE,
          "finite": bool(np.all(np.isfinite(s0)) and np.all(np.isfinite(s1)))}
  print(name, "done", file=sys.stderr, flush=True)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dim", type=int, default=128)
  ap.add_argument("--walks1", type=int, default=100)
  ap.add_argument("--walks2", type=int, default=1)
  ap.add_argument("--seq-sources", type=int, default=16)
  ap.add_argument("--repeats", type=int, default=3)
  args = ap.parse_args()
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd.hypergraph_util import Incidence
  from hypergraphembedding_amd.proto import Hypergraph
  from hypergraphembedding_amd.synthetic import random_hypergraph

  hg = Hypergraph()
  with open(os.path.join(ROOT, "tests", "golden",
                         "snap_youtube_tiny.hypergraph.pb"), "rb") as f:
    hg.ParseFromString(f.read())
  ctx = _hgx.Context(0)
  out = {"workload": "metapath2vec++ baseline, d = %d, negative 5, window 7, "
                     "L 201, one epoch" % args.dim,
         "atomic_rate_bytes_per_s": ATOMIC_RATE, "repeats": args.repeats,
         "C1": run(ctx, Incidence.from_hypergraph(hg), "youtube_tiny",
                   args.dim, args.walks1, args.seq_sources, args.repeats),
         "C2": run(ctx, random_hypergraph(seed=0), "random 100k x 50k",
                   args.dim, args.walks2, args.seq_sources, args.repeats)}
  ctx.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
