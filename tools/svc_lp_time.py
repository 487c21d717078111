#!/usr/bin/env python3
"""Time the per-edge SVC link-prediction classifiers at the C3 size: the
100k / 50k random graph (synthetic.random_hypergraph), a d = 128 node table,
one problem per edge (all 50k).

Device: hgx_svc_fit and hgx_svc_decision timed separately with HIP events
(hgx_svc_last_stats) after a warm-up on a slice, best and median of --reps.
CPU yardstick: a 2,000-edge slice (every 25th edge) of the same problems
through the reference's loop, SVC(C=1, gamma=0.1).fit per edge, on a pool of
16 processes started before the device is touched (the slice run seven
times, the median taken); its time is scaled by n_problems / 2000 and
reported as scaled. Without sklearn the CPU part is
reported as not measured.

  python tools/svc_lp_time.py --out profiles/svc_lp_time.json
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_shared = {}


def build_problems(inc, n_edges, seed):
  from hypergraphembedding_amd.evaluation_util import _draw_rows_without
  gen = np.random.default_rng(seed)
  mark = np.zeros(inc.N, bool)
  off, rows, labs = [0], [], []
  for e in range(n_edges):
    pos = inc.col_e[inc.rp_e[e]:inc.rp_e[e + 1]].astype(np.int64)
    k = min(inc.N - len(pos), 2 * len(pos))
    neg = _draw_rows_without(gen, inc.N, pos, mark, k)
    rows += [pos, neg]
    labs += [np.ones(len(pos), np.uint8), np.zeros(k, np.uint8)]
    off.append(off[-1] + len(pos) + k)
  return (np.array(off, np.int64), np.concatenate(rows).astype(np.int32),
          np.concatenate(labs))


def _cpu_fit(p):
  from sklearn.svm import SVC
  off, row, lab, tab = (_shared[k] for k in ("off", "row", "lab", "tab"))
  sl = slice(off[p], off[p + 1])
  clf = SVC(C=1, gamma=0.1).fit(tab[row[sl]], lab[sl])
  return int(clf.n_support_.sum())


def cpu_baseline(off, row, lab, tab, n_slice, procs, reps=7):
  try:
    import sklearn  # noqa: F401
  except ImportError:
    return {"measured": False, "why": "sklearn is not importable here"}
  import multiprocessing as mp
  n = len(off) - 1
  picks = list(range(0, n, max(1, n // n_slice)))[:n_slice]
  _shared.update(off=off, row=row, lab=lab, tab=tab.astype(np.float64))
  times = []
  with mp.get_context("fork").Pool(procs) as pool:
    pool.map(_cpu_fit, picks[:procs * 4], chunksize=4)  # warm-up
    for _ in range(reps):
      t0 = time.perf_counter()
      pool.map(_cpu_fit, picks, chunksize=16)
      times.append(time.perf_counter() - t0)
  dt = float(np.median(times))
  return {"measured": True, "slice_problems": len(picks), "processes": procs,
          "slice_seconds_each_run": times,
          "slice_seconds": dt, "problems_per_s": len(picks) / dt,
          "scaled_seconds_all_problems": dt * n / len(picks)}


def pct(a):
  q = np.percentile(a, [0, 25, 50, 75, 95, 99, 100])
  return {k: float(v) for k, v in zip(
      ("min", "p25", "p50", "p75", "p95", "p99", "max"), q)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--nodes", type=int, default=100_000)
  ap.add_argument("--edges", type=int, default=50_000)
  ap.add_argument("--mean-degree", type=float, default=20)
  ap.add_argument("--dim", type=int, default=128)
  ap.add_argument("--scale", type=float, default=0.3)
  ap.add_argument("--reps", type=int, default=3)
  ap.add_argument("--queries", type=int, default=1_000_000)
  ap.add_argument("--cpu-slice", type=int, default=2000)
  ap.add_argument("--cpu-procs", type=int, default=16)
  ap.add_argument("--no-cpu", action="store_true")
  ap.add_argument("--no-device", action="store_true")
  ap.add_argument("--out", default=None)
  a = ap.parse_args()

  from hypergraphembedding_amd.synthetic import random_hypergraph
  inc = random_hypergraph(N=a.nodes, E=a.edges, mean_degree=a.mean_degree,
                          seed=0)
  rs = np.random.default_rng(1)
  tab = rs.normal(0.0, a.scale, (inc.N, a.dim)).astype(np.float32)
  t0 = time.perf_counter()
  off, row, lab = build_problems(inc, inc.E, seed=2)
  m = np.diff(off)
  res = {"graph": {"nodes": inc.N, "edges": inc.E, "nnz": int(inc.nnz)},
         "table": {"dim": a.dim, "values": f"normal(0, {a.scale})"},
         "problems": int(len(m)), "samples": int(off[-1]),
         "host_sampling_seconds": time.perf_counter() - t0,
         "m": pct(m),
         "tiers": {"m<=32": int((m <= 32).sum()),
                   "33..64": int(((m > 32) & (m <= 64)).sum()),
                   "65..128": int(((m > 64) & (m <= 128)).sum()),
                   "129..192": int(((m > 128) & (m <= 192)).sum()),
                   ">192": int((m > 192).sum())}}

  if not a.no_cpu:  # before the device is opened: the pool forks
    res["cpu"] = cpu_baseline(off, row, lab, tab, a.cpu_slice, a.cpu_procs)
  else:
    res["cpu"] = {"measured": False, "why": "--no-cpu"}

  if not a.no_device:
    from hypergraphembedding_amd import _hgx
    from hypergraphembedding_amd.runtime import get_context
    svc = _hgx.Svc(get_context(), tab)
    w = min(2000, len(m))  # warm-up: every kernel, a slice of the problems
    big = np.argsort(m)[-8:]
    warm = np.unique(np.concatenate([np.arange(w), big]))
    wo = np.concatenate([[0], np.cumsum(m[warm])])
    wr = np.concatenate([row[off[p]:off[p + 1]] for p in warm])
    wl = np.concatenate([lab[off[p]:off[p + 1]] for p in warm])
    svc.fit(wo, wr, wl)
    svc.decision(np.zeros(64, np.int32), np.arange(64, dtype=np.int32))
    # the LDS cut of the one-workgroup-per-problem solver, alternating
    by_cut = {64: [], 128: [], 192: []}
    for _ in range(a.reps):
      for cut in by_cut:
        svc.ctx.set_tuning("svc_lds_m", cut)
        svc.fit(off, row, lab)
        by_cut[cut].append(svc.stats()["fit_ms"])
    svc.ctx.set_tuning("svc_lds_m", 128)
    fit_ms, wall = [], []
    for _ in range(a.reps):
      t0 = time.perf_counter()
      iters, status = svc.fit(off, row, lab)
      wall.append(time.perf_counter() - t0)
      fit_ms.append(svc.stats()["fit_ms"])
    qp = rs.integers(0, len(m), a.queries).astype(np.int32)
    qr = rs.integers(0, inc.N, a.queries).astype(np.int32)
    dec_ms = []
    for _ in range(a.reps):
      f = svc.decision(qp, qr)
      dec_ms.append(svc.stats()["decision_ms"])
    coef, _ = svc.get()
    nsv = np.add.reduceat((coef != 0).astype(np.int64), off[:-1])
    res["device"] = {
        "measured": True,
        "fit_ms_by_svc_lds_m": {str(k): v for k, v in by_cut.items()},
        "fit_ms": fit_ms, "fit_ms_best": min(fit_ms),
        "fit_ms_median": float(np.median(fit_ms)),
        "fit_wall_seconds_with_upload": wall,
        "fit_problems_per_s": len(m) / (min(fit_ms) * 1e-3),
        "decision_queries": a.queries, "decision_ms": dec_ms,
        "decision_queries_per_s": a.queries / (min(dec_ms) * 1e-3),
        "iterations": pct(iters), "iterations_total": int(iters.sum()),
        "hit_iteration_cap": int(np.count_nonzero(status)),
        "support_vectors": pct(nsv),
        "predicted_positive_share": float(np.mean(f > 0))}
    if res["cpu"].get("measured"):
      res["cpu_scaled_over_device_fit"] = (
          res["cpu"]["scaled_seconds_all_problems"] / (min(fit_ms) * 1e-3))
    svc.close()
  else:
    res["device"] = {"measured": False, "why": "--no-device"}

  text = json.dumps(res, indent=1)
  print(text)
  if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
      fh.write(text + "\n")


if __name__ == "__main__":
  main()
