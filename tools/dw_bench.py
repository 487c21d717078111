#!/usr/bin/env python
"""DeepWalk baseline on the C2 graph (random 100k x 50k, bench.py's), the
bipartite graph: one JSON line per dimension with the walk kernel's walks/s
and, for the hierarchical-softmax trainer, the HIP-event time, walks/s,
pairs/s and path nodes/s of the concurrent mode at each `dw_hot_levels` of
`--hot-levels`, and of the sequential mode (one wave) on `--seq-walks` walks.

`atomic_bytes_per_s` is derived, not counted: every path node outside the hot
levels is one global atomic row add of dp x 4 bytes, every pair one more (the
input word's row of syn0), and every workgroup sends at most 2^T - 1 hot rows;
the share of path nodes inside the hot levels is the corpus mean of
min(path length, T). A measurement for DESIGN §4.11, not a gate.

  python tools/dw_bench.py [--dims 64,128] [--walk-length 40] [--passes 10]
                           [--epochs 1] [--hot-levels 0,2,4,6]
                           [--seq-walks 2000]
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dims", default="64,128")
  ap.add_argument("--walk-length", type=int, default=40)
  ap.add_argument("--passes", type=int, default=10)
  ap.add_argument("--epochs", type=int, default=1)
  ap.add_argument("--window", type=int, default=5)
  ap.add_argument("--hot-levels", default="0,2,4,6")
  ap.add_argument("--seq-walks", type=int, default=2000)
  ap.add_argument("--chunk-walks", type=int, default=0)
  args = ap.parse_args()
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd import deepwalk as dw
  from hypergraphembedding_amd import node2vec as n2v
  from hypergraphembedding_amd.synthetic import random_hypergraph

  inc = random_hypergraph(seed=0)
  ctx = _hgx.Context(0)
  ctx.upload(inc)
  ctx.set_tuning("n2v_chunk_walks", args.chunk_walks)
  L = args.walk_length
  V = inc.N + inc.E
  np.random.seed(0)
  order = np.concatenate([np.random.permutation(V)
                          for _ in range(args.passes)])
  passes = np.repeat(np.arange(args.passes, dtype=np.int32), V)
  for d in [int(x) for x in args.dims.split(",")]:
    out = {"workload": "DeepWalk, C2 graph %d x %d (bipartite), d = %d, walk "
                       "length %d, %d passes, window %d, hierarchical softmax"
                       % (inc.N, inc.E, d, L, args.passes, args.window),
           "epochs": args.epochs}
    with _hgx.N2v(ctx, n2v.BIPARTITE, d) as be:
      dp = 64
      while dp < d:
        dp *= 2
      init = (np.random.random((V, d)).astype(np.float32) - 0.5) / d
      be.walks(passes, order, L, 1.0, 1, copy=False)  # warm-up
      walks = be.walks(passes, order, L, 1.0, 1)
      st = be.stats()
      out.update(vertices=V, walks=int(order.size), walk_ms=st["walk_ms"],
                 walks_per_s=order.size * 1e3 / st["walk_ms"])
      counts = be.counts()
      be.set_vocab(n2v.keep_thresholds(counts), n2v.cum_table(counts))
      ptr, point, code = dw.huffman_tree(counts)
      lens = np.diff(ptr)
      out.update(max_code=int(lens.max()),
                 mean_code=float((lens * counts).sum() / counts.sum()))
      be.set_tree(ptr, point, code)
      runs = [("hot%d" % t, t) for t in
              (int(x) for x in args.hot_levels.split(","))]
      for name, t in runs:
        ctx.set_tuning("dw_hot_levels", t)
        be.set_vectors(init)
        be.train_hs(window=args.window, epochs=args.epochs, seed=2)
        st = be.stats()
        syn0, _ = be.get_vectors()
        per_s = 1e3 / st["train_ms"]
        hot = float((np.minimum(lens, t) * counts).sum() / counts.sum())
        res = {"train_ms": st["train_ms"], "walks_per_s": st["walks"] * per_s,
               "words_per_s": st["words"] * per_s,
               "pairs_per_s": st["pairs"] * per_s,
               "path_nodes_per_s": st["path_nodes"] * per_s,
               "path_nodes_per_pair": st["path_nodes"] / max(st["pairs"], 1),
               "finite": bool(np.all(np.isfinite(syn0)))}
        groups = st["walks"] / 4.0  # four walks to a workgroup
        adds = (st["path_nodes"] - hot * st["pairs"] + st["pairs"] +
                groups * ((1 << t) - 1))
        res["atomic_bytes_per_s"] = adds * dp * 4 * per_s
        out[name] = res
      ctx.set_tuning("dw_hot_levels", 6)
      be.set_vectors(init)
      be.train_hs(walks[:args.seq_walks], window=args.window, epochs=1, seed=2,
                  concurrent=False)
      st = be.stats()
      per_s = 1e3 / st["train_ms"]
      out["sequential"] = {"train_ms": st["train_ms"],
                           "walks_trained": st["walks"],
                           "walks_per_s": st["walks"] * per_s,
                           "pairs_per_s": st["pairs"] * per_s,
                           "path_nodes_per_s": st["path_nodes"] * per_s}
    print(json.dumps(out), flush=True)
  ctx.close()


if __name__ == "__main__":
  main()
