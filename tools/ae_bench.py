#!/usr/bin/env python
"""Auto-encoder baseline on the C2 graph (random 100k x 50k, bench.py's):
one JSON line with, per side, the ms per batch, samples/s and achieved
algorithmic flops (6 M C d per batch, hgx_ae_last_stats) of `--steps` batches
of `--idx-per-batch` rows after `--warmup`, d = 128. A measurement for
DESIGN §4.9, not a gate.

  python tools/ae_bench.py [--steps 20] [--warmup 5] [--dim 128]
"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_PEAK = 157.3e12  # MI355X, v_mfma_f32_32x32x2_f32 (spec)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--steps", type=int, default=20)
  ap.add_argument("--warmup", type=int, default=5)
  ap.add_argument("--dim", type=int, default=128)
  ap.add_argument("--idx-per-batch", type=int, default=200)
  ap.add_argument("--samples-per-idx", type=int, default=100)
  ap.add_argument("--chunk-rows", type=int, default=0)
  args = ap.parse_args()
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd import auto_encoder as ae
  from hypergraphembedding_amd.synthetic import random_hypergraph

  inc = random_hypergraph(seed=0)
  ctx = _hgx.Context(0)
  ctx.upload(inc)
  ctx.set_tuning("ae_chunk_rows", args.chunk_rows)
  out = {"workload": "auto-encoder baseline, C2 graph %d x %d, d = %d, %d rows "
                     "per batch, %d samples per row" %
                     (inc.N, inc.E, args.dim, args.idx_per_batch,
                      args.samples_per_idx),
         "steps": args.steps, "warmup": args.warmup}
  np.random.seed(0)
  for side, name in ((ae.NODE, "node"), (ae.EDGE, "edge")):
    R, C, _, _ = ae.side_csr(inc, side)
    with _hgx.Ae(ctx, side, args.dim) as be:
      be.set_weights(ae.glorot_uniform(C, args.dim), np.zeros(args.dim),
                     ae.glorot_uniform(args.dim, C), np.zeros(C))
      perm = np.random.permutation(R)
      ms = flops = 0.0
      samples = 0
      for b in range(args.warmup + args.steps):
        rows = perm[b * args.idx_per_batch:(b + 1) * args.idx_per_batch]
        row, drop = be.draw(rows, args.samples_per_idx, 1, 0)
        loss = be.step(row, drop)
        if b >= args.warmup:
          st = be.stats()
          ms += st["ms"]
          flops += st["flops"]
          samples += st["samples"]
      # bytes of the logit block: written by the logits, read four times and
      # written twice by the softmax / dZ passes, read by the two backward
      # GEMMs and the bias sum
      z_bytes = 10.0 * 4.0 * samples * C
      out[name] = {"rows": R, "columns": C,
                   "ms_per_batch": ms / args.steps,
                   "samples_per_batch": samples / args.steps,
                   "samples_per_s": samples / (ms * 1e-3),
                   "tflops": flops / (ms * 1e-3) / 1e12,
                   "of_fp32_mfma_peak": flops / (ms * 1e-3) / FP32_MFMA_PEAK,
                   "logit_block_tb_per_s": z_bytes / (ms * 1e-3) / 1e12,
                   "last_loss": loss}
  ctx.close()
  print(json.dumps(out))


if __name__ == "__main__":
  main()
