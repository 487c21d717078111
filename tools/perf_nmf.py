"""Measure the device NMF (hypergraphembedding_amd/nmf.py, the cd_sweep
kernel of csrc/hgx_spmm.hip) on one MI355X and write one JSON file.

  python tools/perf_nmf.py --out profiles/nmf/perf_nmf.json

For the 4000 x 2000 random graph at k = 16 and the 100k / 50k benchmark graph
at k = 128:

* default: ``nmf_incidence`` as ``EmbedNMF`` calls it (NNDSVDa start from the
  converged SVD), host clock around the call;
* the same solve with the start computed apart (``init_s``: svd_incidence
  and the NNDSVD arithmetic) and handed over as ``init="custom"``, so that
  ``loop_s`` is the iterations and the final error. They split into the
  fused sweeps, which gather their product rows themselves (device time by
  HIP events), the one sparse product of the final error, and the rest (the
  Grams, each a host round trip, the Q uploads, and the host itself);
* a sweep's device time per side (first, median, last), its nominal float64
  rate (4 k^2 flop per row: the gradient build and the updates, both counted
  in full although zero coordinates skip theirs) and its bytes per second
  (4 nnz + 4 k nnz gathered, 8 k + 8 bytes per row: P read and written, one
  violation).

``--sklearn`` adds sklearn's NMF(16) on the dense 4000 x 2000 matrix on this
host (it cannot densify the 100k / 50k graph: 40 GB in float64).
"""

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hypergraphembedding_amd import _hgx, synthetic  # noqa: E402
from hypergraphembedding_amd.nmf import nmf_incidence, nndsvd_init  # noqa: E402
from hypergraphembedding_amd.runtime import get_context  # noqa: E402
from hypergraphembedding_amd.svd import svd_incidence  # noqa: E402


class PerSide:
  """_hgx.Svd with every sweep's device time kept per factor slot."""

  def __init__(self, eng):
    self.e, self.rows, self.sweep = eng, eng.rows, {}

  def __getattr__(self, name):
    return getattr(self.e, name)

  def cd_sweep_fused(self, pslot, pcol0, xslot, xcol0, Q):
    m0 = self.e.cd_stats()["sweep_ms"]
    v = self.e.cd_sweep_fused(pslot, pcol0, xslot, xcol0, Q)
    self.sweep.setdefault(pslot, []).append(self.e.cd_stats()["sweep_ms"] - m0)
    return v


def run(inc, k):
  ctx = get_context()
  ctx.upload(inc)
  r = {"N": inc.N, "E": inc.E, "nnz": inc.nnz, "k": k}
  np.random.seed(0)
  t = time.perf_counter()
  W, H, info = nmf_incidence(inc, k, ctx=ctx)
  r["default_total_s"] = time.perf_counter() - t
  r["default_n_iter"] = info["n_iter"]
  r["reconstruction_err"] = info["reconstruction_err"]
  eng = _hgx.Svd(ctx)
  try:
    np.random.seed(0)
    t = time.perf_counter()
    U, s, Vt, _ = svd_incidence(inc, k, backend=eng)
    W0, H0 = nndsvd_init(U[:, ::-1], s[::-1], Vt[::-1],
                         inc.nnz / (float(inc.N) * inc.E))
    r["init_s"] = time.perf_counter() - t
    st0 = eng.stats()
    be = PerSide(eng)
    t = time.perf_counter()
    W2, H2, info = nmf_incidence(inc, k, init="custom", W0=W0, H0=H0,
                                 backend=be)
    r["loop_s"] = time.perf_counter() - t
  finally:
    eng.close()
  st = info["stats"]
  r["n_iter"], r["converged"] = info["n_iter"], info["converged"]
  r["same_as_default"] = bool(np.array_equal(W, W2) and np.array_equal(H, H2))
  r["sweep_ms"] = info["sweep_ms"]
  r["spmm_ms"] = st["spmm_ms"] - st0["spmm_ms"]
  r["spmm_bytes"] = st["spmm_bytes"] - st0["spmm_bytes"]
  r["rest_ms"] = r["loop_s"] * 1e3 - r["sweep_ms"] - r["spmm_ms"]
  for slot, label, rows in ((0, "node", inc.N), (1, "edge", inc.E)):
    ms = np.array(be.sweep[slot])
    med = float(np.median(ms))
    r["sweep_" + label] = {
        "ms_first_median_last": [float(ms[0]), med, float(ms[-1])],
        "nominal_gflops": 4.0 * k * k * rows / med / 1e6,
        "gbytes_s": (4.0 * inc.nnz * (k + 1) + rows * (8.0 * k + 8.0))
                    / med / 1e6}
  r["zeros_W"], r["zeros_H"] = float((W2 == 0).mean()), float((H2 == 0).mean())
  return r


def sklearn_dense(inc, k):
  from sklearn.decomposition import NMF
  a = inc.to_scipy()[0].astype(np.float64).toarray()
  out = []
  for _ in range(2):
    np.random.seed(0)
    m = NMF(k)
    t = time.perf_counter()
    m.fit(a)
    out.append({"s": time.perf_counter() - t, "n_iter": m.n_iter_,
                "reconstruction_err": float(m.reconstruction_err_)})
  return {"runs": out, "cpus": os.cpu_count()}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--sklearn", action="store_true")
  args = ap.parse_args()
  warnings.simplefilter("ignore")
  small = synthetic.random_hypergraph(4000, 2000, 20, seed=0)
  out = {"random_4000x2000_k16": run(small, 16),
         "random_100k_50k_k128": run(synthetic.random_hypergraph(), 128)}
  if args.sklearn:
    out["sklearn_4000x2000_k16"] = sklearn_dense(small, 16)
  text = json.dumps(out, indent=1)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
