#!/usr/bin/env python3
"""Golden fixture of the batched RBF C-SVC (csrc/hgx_svc.hip): svc_small.npz.

The oracle is the reference's own call, sklearn.svm.SVC(C=1, gamma=0.1)
(evaluation_util.py:352), run here on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_svc.py

Per dimension d in DIMS the file holds one float32 table (``tab{d}``), the
problems as rows of it (``off{d}`` int64, ``row{d}`` int32, ``lab{d}`` uint8),
the queries (``qprob{d}``, ``qrow{d}``) and per query the decision value of
three solves of its problem:
  ``f_tight{d}``    SVC(C=1, gamma=0.1, tol=1e-8) on the float64 table
  ``f_default{d}``  SVC(C=1, gamma=0.1) on the same data
  ``f_resh{d}``     a second default solve with the sample order reversed: the
                    reference's own slack, which its shuffle makes visible
``A`` is the largest |f_default - f_tight| and |f_resh - f_tight| over the
file; ``identical`` = (d, problem) of the problem that holds two identical
rows of opposite label.

A table is three blocks of rows at the value scales 0.05, 0.3 (normal) and
1.0 (uniform in [0, 1]): trained Keras tables, intermediate values and
algebraic-distance coordinates. A block is [base rows | twins]: twin k is
base row k moved by about 1% of the scale; base rows 6-17 are a tight
cluster. A problem draws its rows from the base rows of one block. Its
queries are some of its own rows, the twins of its rows and rows it never
saw. Table values are rounded to float16 precision (they stay float32) so
that the file compresses; the sizes hit every tier of the solver and each
boundary between two (32 | 33, 64 | 65, 128 | 129 samples).
"""

import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "svc_small.npz")
DIMS = (2, 16, 100, 128, 256)
SCALES = (0.05, 0.3, 1.0)
N_TWIN = 12
CLUSTER = range(6, 18)
C, GAMMA = 1.0, 0.1
# base rows per block: every block holds the 65-sample problems; the 129-
# and ~700-sample ones live where a row is cheap
N_BASE = {2: (70, 720, 140), 16: (70, 70, 720), 100: (66, 66, 66),
          128: (66, 66, 66), 256: (40, 24, 66)}
# (positives, negatives) of the fixed-size problems of every block
FIXED = ((1, 2), (2, 2), (3, 1), (21, 42), (31, 33), (40, 25), (11, 21),
         (11, 22), (15, 17))
N_RANDOM = 11


def _table(rng, d):
  blocks, layout, at = [], [], 0
  for scale, nb in zip(SCALES, N_BASE[d]):
    if scale == 1.0:
      base = rng.uniform(0.0, 1.0, (nb, d))
    else:
      base = rng.normal(0.0, scale, (nb, d))
    c = list(CLUSTER)
    base[c] = base[c[0]] + 0.03 * scale * rng.normal(0.0, 1.0, (len(c), d))
    twins = base[:N_TWIN] + 0.01 * scale * rng.normal(0.0, 1.0, (N_TWIN, d))
    blocks += [base, twins]
    layout.append((at, nb))  # first base row, base rows; twins follow
    at += nb + N_TWIN
  tab = np.concatenate(blocks).astype(np.float16).astype(np.float32)
  return tab, layout


def _draw(rng, nb, npos, nneg, cluster):
  """Base-row positions: positives then negatives. At least one positive and
  one negative have a twin; `cluster` draws the positives from the tight
  cluster."""
  pool = np.arange(nb)
  if cluster:
    pos = rng.choice(np.array(CLUSTER), min(npos, len(CLUSTER)), replace=False)
  else:
    pos = np.concatenate([rng.choice(N_TWIN, 1),
                          rng.choice(pool[N_TWIN:], npos - 1, replace=False)])
  rest = np.setdiff1d(pool, pos)
  lead = rest[rest < N_TWIN]
  first = rng.choice(lead, 1)
  neg = np.concatenate([first, rng.choice(np.setdiff1d(rest, first), nneg - 1,
                                          replace=False)])
  return pos, neg


def _problems(rng, d, layout):
  probs = []  # (block, positions, labels)
  for b, (_, nb) in enumerate(layout):
    # Where the rows of a block are too close for the kernel to tell apart
    # (scale * sqrt(d) < 1: every K within a few percent of 1), a problem
    # with as many positives as negatives has alpha = C throughout and f = 0
    # up to the solver's tolerance on every query: no sign to compare. Such
    # blocks keep the other ratios only.
    apart = SCALES[b] * np.sqrt(d) >= 1.0
    sizes = [s for s in FIXED if s[0] + s[1] <= nb]
    if not apart:
      sizes[1] = (1, 3)
    for k in range(N_RANDOM):
      npos = int(rng.integers(1, 21))
      nneg = (2 * npos, npos if apart else npos + 1, max(1, npos // 2))[k % 3]
      if npos + nneg <= nb:
        sizes.append((npos, nneg))
    if nb >= 140:
      sizes += [(42, 85), (43, 85), (43, 86)]  # 127, 128, 129 samples
    if nb >= 720:
      sizes.append((234, 468))  # 702 samples: kernel columns recomputed
    for k, (npos, nneg) in enumerate(sizes):
      cluster = k % 4 == 3 and npos <= len(CLUSTER)
      pos, neg = _draw(rng, nb, npos, nneg, cluster)
      probs.append((b, np.concatenate([pos, neg]),
                    np.concatenate([np.ones(npos, np.uint8),
                                    np.zeros(nneg, np.uint8)])))
  return probs


def _queries(rng, nb, pos_in_block):
  own = rng.choice(pos_in_block, min(6, len(pos_in_block)), replace=False)
  twinned = pos_in_block[pos_in_block < N_TWIN]
  twins = nb + rng.choice(twinned, min(6, len(twinned)), replace=False)
  unseen = np.setdiff1d(np.arange(nb), pos_in_block)
  unseen = rng.choice(unseen, min(3, len(unseen)), replace=False)
  return np.concatenate([own, twins, unseen])


def solve(x, y, q, **kw):
  from sklearn.svm import SVC
  return SVC(C=C, gamma=GAMMA, **kw).fit(x, y).decision_function(q)


def generate():
  out = {"dims": np.array(DIMS, np.int32), "C": C, "gamma": GAMMA}
  A = 0.0
  for d in DIMS:
    rng = np.random.default_rng(1000 + d)
    tab, layout = _table(rng, d)
    probs = _problems(rng, d, layout)
    if d == 16:
      # two identical rows of opposite label: a copy of a row joins the
      # table and the last problem of the first block as a negative
      b, posn, lab = probs[len(FIXED) - 1]
      src = layout[b][0] + posn[0]
      tab = np.concatenate([tab, tab[src:src + 1]])
      out["identical"] = np.array([d, len(FIXED) - 1], np.int32)
    off, rows, labs, qprob, qrow = [0], [], [], [], []
    for p, (b, posn, lab) in enumerate(probs):
      first, nb = layout[b]
      r = first + posn
      q = first + _queries(rng, nb, posn)
      if d == 16 and p == len(FIXED) - 1:
        r = np.append(r, len(tab) - 1)
        lab = np.append(lab, np.uint8(0))
        q = np.append(q, len(tab) - 1)
      rows.append(r)
      labs.append(lab)
      off.append(off[-1] + len(r))
      qprob.append(np.full(len(q), p))
      qrow.append(q)
    x64 = tab.astype(np.float64)
    f = {"tight": [], "default": [], "resh": []}
    for r, lab, q in zip(rows, labs, qrow):
      f["tight"].append(solve(x64[r], lab, x64[q], tol=1e-8))
      f["default"].append(solve(x64[r], lab, x64[q]))
      f["resh"].append(solve(x64[r[::-1]], lab[::-1], x64[q]))
    ft = np.concatenate(f["tight"])
    for k in ("default", "resh"):
      A = max(A, float(np.abs(np.concatenate(f[k]) - ft).max()))
    out[f"tab{d}"] = tab
    out[f"off{d}"] = np.array(off, np.int64)
    out[f"row{d}"] = np.concatenate(rows).astype(np.int32)
    out[f"lab{d}"] = np.concatenate(labs).astype(np.uint8)
    out[f"qprob{d}"] = np.concatenate(qprob).astype(np.int32)
    out[f"qrow{d}"] = np.concatenate(qrow).astype(np.int32)
    out[f"f_tight{d}"] = ft
    out[f"f_default{d}"] = np.concatenate(f["default"]).astype(np.float32)
    out[f"f_resh{d}"] = np.concatenate(f["resh"]).astype(np.float32)
  out["A"] = A
  return out


def main():
  out = generate()
  np.savez_compressed(OUT, **out)
  n_prob = sum(len(out[f"off{d}"]) - 1 for d in DIMS)
  ft = np.concatenate([out[f"f_tight{d}"] for d in DIMS])
  bar = 3 * out["A"]
  print(f"{n_prob} problems, {ft.size} queries, A = {out['A']:.3e}, "
        f"|f_tight| < 3A on {np.mean(np.abs(ft) < bar):.2%} of the queries, "
        f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
  main()
