#!/usr/bin/env python
"""node2vec baselines on the C2 graph (random 100k x 50k, bench.py's): one
JSON line with walks/s of the walk kernels and walks/s and trained (kept)
words/s of the skip-gram trainer, d = 128, walk length 5, 10 passes, for the
bipartite graph in both trainer modes and for the clique graph (concurrent).
The sequential mode is one wave, so it trains `--seq-walks` walks of the
corpus for one epoch. A measurement for DESIGN §4.10, not a gate.

  python tools/n2v_bench.py [--dim 128] [--walk-length 5] [--passes 10]
                            [--epochs 5] [--seq-walks 20000]
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rates(st, what):
  ms = st[what + "_ms"]
  return ms, (1e3 / ms if ms > 0 else 0.0)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--dim", type=int, default=128)
  ap.add_argument("--walk-length", type=int, default=5)
  ap.add_argument("--passes", type=int, default=10)
  ap.add_argument("--epochs", type=int, default=5)
  ap.add_argument("--window", type=int, default=3)
  ap.add_argument("--seq-walks", type=int, default=20000)
  ap.add_argument("--chunk-walks", type=int, default=0)
  args = ap.parse_args()
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd import node2vec as n2v
  from hypergraphembedding_amd.synthetic import random_hypergraph

  inc = random_hypergraph(seed=0)
  ctx = _hgx.Context(0)
  ctx.upload(inc)
  ctx.set_tuning("n2v_chunk_walks", args.chunk_walks)
  d, L = args.dim, args.walk_length
  out = {"workload": "node2vec baselines, C2 graph %d x %d, d = %d, walk "
                     "length %d, %d passes, window %d, negative 5" %
                     (inc.N, inc.E, d, L, args.passes, args.window),
         "epochs": args.epochs}
  np.random.seed(0)
  for graph, name in ((n2v.BIPARTITE, "bipartite"), (n2v.CLIQUE, "clique")):
    src = (np.arange(inc.N + inc.E) if graph == n2v.BIPARTITE
           else n2v.clique_sources(inc))
    order = np.concatenate([np.random.permutation(src)
                            for _ in range(args.passes)])
    passes = np.repeat(np.arange(args.passes, dtype=np.int32), src.size)
    with _hgx.N2v(ctx, graph, d) as be:
      V = be.V
      init = (np.random.random((V, d)).astype(np.float32) - 0.5) / d
      be.walks(passes, order, L, 1.0, 1, copy=False)  # warm-up
      walks = be.walks(passes, order, L, 1.0, 1)
      st = be.stats()
      ms, per_ms = rates(st, "walk")
      res = {"vertices": V, "walks": int(order.size), "walk_ms": ms,
             "walks_per_s": order.size * per_ms,
             "expand_steps": st["expand_steps"],
             "reject_steps": st["reject_steps"]}
      counts = be.counts()
      be.set_vocab(n2v.keep_thresholds(counts), n2v.cum_table(counts))
      modes = [("concurrent", True)]
      if graph == n2v.BIPARTITE:
        modes.append(("sequential", False))
      for mode, conc in modes:
        be.set_vectors(init)
        if conc:
          be.train(window=args.window, epochs=args.epochs, seed=2)
        else:
          be.train(walks[:args.seq_walks], window=args.window, epochs=1,
                   seed=2, concurrent=False)
        st = be.stats()
        ms, per_ms = rates(st, "train")
        syn0, _ = be.get_vectors()
        res[mode] = {"train_ms": ms, "walks_trained": st["walks"],
                     "walks_per_s": st["walks"] * per_ms,
                     "words_per_s": st["words"] * per_ms,
                     "pairs_per_s": st["pairs"] * per_ms,
                     "pairs_per_word": st["pairs"] / max(st["words"], 1),
                     "finite": bool(np.all(np.isfinite(syn0)))}
      out[name] = res
  ctx.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
