"""Measure the device truncated SVD (hypergraphembedding_amd/svd.py,
csrc/hgx_spmm.hip) on one MI355X and write one JSON file.

  python tools/perf_svd.py --out profiles/svd/perf_svd.json

* floors: on the three inputs of tests/svd_cases.py the solver is asked for a
  residual it cannot reach (1e-9): every cycle whose Ritz estimate passes
  measures the true residual, and the smallest of those figures is the floor
  (further restarts do not lower it).
* c3: svd_incidence on the 100k / 50k random graph at k = 128 (one warm-up
  solve, then timed solves on a host clock; the solve ends in a device
  synchronise), its restarts and products, the device time of the sparse
  products by HIP events and their achieved GB/s from the algorithmic bytes
  4 nnz + 4 b nnz + 4 b rows; scipy.sparse.linalg.svds on the float32 matrix
  (what the reference's asfptype() hands it) on the same host.
* per_product: each orientation of the product alone at b = 16 and b = 136,
  next to hgx_probe_gather's random 64-byte-row rate (its widest row, the row
  of a b = 16 panel).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hypergraphembedding_amd import _hgx, synthetic  # noqa: E402
from hypergraphembedding_amd.runtime import get_context  # noqa: E402
from hypergraphembedding_amd.svd import svd_incidence  # noqa: E402


def floors():
  import svd_cases as C
  out = {}
  for name in C.CASES:
    inc, k = C.case(name)[:2]
    np.random.seed(11)
    try:
      info = svd_incidence(inc, k, tol=1e-9, max_restarts=30)[3]
    except _hgx.HgxError as e:
      info = e.info
    m = info["measured"]
    out[name] = {"k": k, "measured": m, "floor": min(m) if m else None,
                 "restarts": info["restarts"]}
    print("floor", name, out[name], flush=True)
  return out


def per_product(ctx, inc, widths=(16, 136), reps=20):
  out = {}
  for b in widths:
    svd = _hgx.Svd(ctx)
    svd.panel(0, svd.EDGE, b)
    svd.panel(1, svd.NODE, b)
    svd.set(0, 0, np.random.default_rng(b).standard_normal(
        (inc.E, b)).astype(np.float32))
    for dst, src, key in ((1, 0, "A_X"), (0, 1, "At_Y")):
      svd.spmm(dst, 0, src, 0, b)  # warm-up
      s0 = svd.stats()
      for _ in range(reps):
        svd.spmm(dst, 0, src, 0, b)
      s1 = svd.stats()
      ms = (s1["spmm_ms"] - s0["spmm_ms"]) / reps
      by = (s1["spmm_bytes"] - s0["spmm_bytes"]) / reps
      out[f"b{b}_{key}"] = {"ms": ms, "algorithmic_bytes": by,
                            "GBps": by / ms / 1e6,
                            "gathered_rows_per_s": inc.nnz / ms * 1e3}
      print("product", b, key, out[f"b{b}_{key}"], flush=True)
    svd.close()
  rates = {f: ctx.probe_gather(inc.E * 64, 16, f, 3) for f in (4, 8, 16)}
  best = max(rates.values())
  out["probe_gather_64B_rows"] = {"rows_per_s": best, "GBps": best * 64 / 1e9,
                                  "table_bytes": inc.E * 64,
                                  "by_in_flight": rates}
  print("probe", out["probe_gather_64B_rows"], flush=True)
  return out


def c3(k, repeats, with_scipy):
  inc = synthetic.random_hypergraph()
  ctx = get_context()
  out = {"N": inc.N, "E": inc.E, "nnz": inc.nnz, "k": k}
  np.random.seed(0)
  svd_incidence(inc, k, ctx=ctx)  # warm-up: code objects, allocations
  runs = []
  for r in range(repeats):
    np.random.seed(r + 1)
    t = time.perf_counter()
    U, s, Vt, info = svd_incidence(inc, k, ctx=ctx)
    wall = time.perf_counter() - t
    st = info["stats"]
    runs.append({"wall_s": wall, "restarts": info["restarts"],
                 "products": info["products"],
                 "product_columns": info["product_columns"],
                 "spmm_ms": st["spmm_ms"], "spmm_calls": st["spmm_calls"],
                 "spmm_GBps": st["spmm_bytes"] / st["spmm_ms"] / 1e6,
                 "dense_calls": st["dense_calls"],
                 "residual_max": float(info["residuals"].max()),
                 "tol": info["tol"], "block": info["block"],
                 "steps": info["steps"]})
    print("c3 run", runs[-1], flush=True)
  out["runs"] = runs
  out["sigma_top"] = float(s[-1])
  out["sigma_kth"] = float(s[0])
  out["per_product"] = per_product(ctx, inc)
  if with_scipy:
    import scipy.sparse.linalg as sla
    a = inc.to_scipy()[0].astype(np.float32)
    print("scipy svds on the float32 matrix ...", flush=True)
    t = time.perf_counter()
    _, sr, _ = sla.svds(a, k)
    out["scipy_svds_float32_s"] = time.perf_counter() - t
    sr = np.sort(sr)
    out["scipy_max_rel_sigma_diff"] = float(np.abs(sr - s).max() / sr[-1])
    print("scipy", out["scipy_svds_float32_s"], flush=True)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--k", type=int, default=128)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--no-scipy", action="store_true")
  ap.add_argument("--no-c3", action="store_true")
  a = ap.parse_args()
  res = {"floors": floors()}
  if not a.no_c3:
    res["c3"] = c3(a.k, a.repeats, not a.no_scipy)
  text = json.dumps(res, indent=1)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
      f.write(text + "\n")
  print(text)


if __name__ == "__main__":
  main()
