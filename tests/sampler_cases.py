"""Host definition of the keyed record samplers (csrc/hgx_sample.hip) for
tests: the hash, the pattern rows, both passes and the whole record stream,
restated from the sampler's header comment with plain arithmetic.

  * Pass 2 (`expand_choice`) keeps the m = min(q, |row|) columns with the
    smallest keys (rand64(seed, 0x100 + pattern, row << 32 | col) >> 32) << 32
    | col of the pattern row.
  * Pass 1 (`reject_choice`) draws 256 candidates per round from the counter
    hash and keeps the first q distinct accepted ones in (round, thread)
    order. A path candidate is accepted iff its path is the lexicographically
    first path from the row to its column; a uniform-column candidate iff the
    column is in the pattern row. Acceptance comes from the definition: the
    row's paths are enumerated from the CSR. None of the device's probes
    (first_common, edges_min_common, Bloom filters, nne_meets,
    members_meet_ev) is restated.
  * `stream` assembles the idx array of hgx_sample_fobe / hgx_sample_hobe_rows
    / hgx_sample_pairs4: kind blocks in the device's order, negatives and
    neighbour lists (hgx::draw_record_neighbors) vectorised.

The case graphs below are the smallest that reach each branch of the kernels;
`labels_of` maps what a case's restatement went through to branch labels and
tests/test_sampler_cases_cpu.py asserts that all of REQUIRED_BRANCHES are
reached. `python tests/sampler_cases.py` writes the branch census
(profiles/samplers/branch_census.txt). No device import."""

import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from store_keys import mix64 as mix64_np  # noqa: E402  (uint64 arrays)

M64 = (1 << 64) - 1
INT_MAX = 0x7fffffff
K_SB = 256        # sampler workgroup (kSB)
K_SEL_CAP = 2048  # kSelCap
LDS_BITMAP_COLS = 393_216  # 48 KiB of bitmap words
EMIT_GRID = 65_536

PAT_A, PAT_AT, PAT_NN, PAT_EE, PAT_NNE, PAT_EEN = range(6)
PAT_NAME = ("A", "AT", "NN", "EE", "NNE", "EEN")
DEFAULT_TUNING = dict(sample_reject_w=32768, sample_mode3=0, sample_mode3_shift=1,
                      sample_mode3_shift_e=1)


# ---- hash: Python ints ------------------------------------------------------
def mix64(z):
  z = (z + 0x9e3779b97f4a7c15) & M64
  z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
  z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
  return z ^ (z >> 31)


def rand64_key(seed, stream):
  return mix64((seed & M64) ^ mix64((stream + 0x632be59bd9b4e019) & M64))


def rand64(seed, stream, ctr):
  return mix64((rand64_key(seed, stream) + ctr) & M64)


def bounded(h, n):
  """floor(h n / 2^64): uniform in [0, n) from 64 random bits."""
  return (h * n) >> 64


# ---- hash: uint64 arrays ----------------------------------------------------
def _u64(x):
  return np.asarray(x, np.uint64)


def rand64_np(seed, stream, ctr):
  with np.errstate(over="ignore"):
    return mix64_np(np.uint64(rand64_key(seed, stream)) + _u64(ctr))


def mulhi_np(h, n):
  """floor(h n / 2^64) elementwise, h uint64, n uint64 (array or scalar)."""
  h, n = _u64(h), _u64(n)
  m32 = np.uint64(0xffffffff)
  s32 = np.uint64(32)
  hl, hh = h & m32, h >> s32
  nl, nh = n & m32, n >> s32
  with np.errstate(over="ignore"):
    ll = hl * nl
    lh = hl * nh
    hl_ = hh * nl
    hh_ = hh * nh
    mid = (ll >> s32) + (lh & m32) + (hl_ & m32)
    return hh_ + (lh >> s32) + (hl_ >> s32) + (mid >> s32)


# ---- CSR views --------------------------------------------------------------
def _levels(inc, pattern):
  """(CSR of each expansion level, number of columns)."""
  A = (inc.rp_n, inc.col_n)
  AT = (inc.rp_e, inc.col_e)
  return {
      PAT_A: ((A,), inc.E), PAT_AT: ((AT,), inc.N),
      PAT_NN: ((A, AT), inc.N), PAT_EE: ((AT, A), inc.E),
      PAT_NNE: ((A, AT, A), inc.E), PAT_EEN: ((AT, A, AT), inc.N),
  }[pattern]


def nrows_of(inc, pattern):
  return inc.N if pattern in (PAT_A, PAT_NN, PAT_NNE) else inc.E


def _row(csr, r):
  return csr[1][csr[0][r]:csr[0][r + 1]]


def _expand(ids, csr):
  """Every (position in ids, column) of the rows `ids` of csr, in order."""
  rp, col = csr
  ids = np.asarray(ids, np.int64)
  cnt = (rp[ids + 1] - rp[ids]).astype(np.int64)
  tot = int(cnt.sum())
  src = np.repeat(np.arange(ids.size), cnt)
  start = np.cumsum(cnt) - cnt
  pos = np.repeat(rp[ids].astype(np.int64), cnt) + (np.arange(tot) - np.repeat(start, cnt))
  return src, col[pos].astype(np.int64)


def row_paths(inc, pattern, r):
  """All paths of row r as columns of an int64 array, lexicographic order:
  (m1, c) for 2-hop patterns, (m1, m2, c) for 3-hop ones."""
  lv, _ = _levels(inc, pattern)
  ids1 = _row(lv[0], r).astype(np.int64)
  s1, c2 = _expand(ids1, lv[1])
  if len(lv) == 2:
    return np.stack([ids1[s1], c2], 1)
  s2, c3 = _expand(c2, lv[2])
  return np.stack([ids1[s1][s2], c2[s2], c3], 1)


def pattern_row(inc, pattern, r):
  """Sorted distinct columns of row r of A, A^T, A A^T, A^T A, A A^T A or
  A^T A A^T, by definition."""
  lv, _ = _levels(inc, pattern)
  cur = np.array([r], np.int64)
  for csr in lv:
    cur = (np.unique(np.concatenate([_row(csr, int(m)) for m in cur]))
           if cur.size else np.zeros(0, np.int64))
  return cur.astype(np.int64)


def pattern_rows(inc, pattern, rows):
  """(indptr, indices) of the given rows of the pattern matrix (sorted
  columns), as a sparse product restricted to those rows."""
  a, at = inc.to_scipy()
  a, at = a.astype(np.int32), at.astype(np.int32)
  chain = {PAT_A: (a,), PAT_AT: (at,), PAT_NN: (a, at), PAT_EE: (at, a),
           PAT_NNE: (a, at, a), PAT_EEN: (at, a, at)}[pattern]
  m = chain[0][np.asarray(rows, np.int64)]
  for f in chain[1:]:
    m = m @ f
  m = sp.csr_matrix(m)
  m.sum_duplicates()
  m.sort_indices()
  return m.indptr.astype(np.int64), m.indices.astype(np.int64)


# ---- pass 2 -----------------------------------------------------------------
def expand_key(seed, pattern, r, col):
  return ((rand64(seed, 0x100 + pattern, ((r & 0xffffffff) << 32) | col) >> 32) << 32) | col


def expand_choice(seed, pattern, r, cols, q):
  """The min(q, len(cols)) columns with the smallest keys, sorted."""
  cols = [int(c) for c in cols]
  m = min(int(q), len(cols))
  keyed = sorted((expand_key(seed, pattern, r, c), c) for c in cols)
  return np.array(sorted(c for _, c in keyed[:m]), np.int64)


def expand_choice_rows(seed, pattern, rows, indptr, indices, quota):
  """expand_choice for many rows at once: rows[i] has columns
  indices[indptr[i]:indptr[i + 1]] and quota quota[i]. Returns (counts,
  chosen columns row after row, each row ascending)."""
  rows = np.asarray(rows, np.int64)
  cnt = np.diff(indptr)
  rr = np.repeat(rows, cnt)
  ctr = (rr.astype(np.uint64) << np.uint64(32)) | indices.astype(np.uint64)
  key = ((rand64_np(seed, 0x100 + pattern, ctr) >> np.uint64(32)) << np.uint64(32)) | \
      indices.astype(np.uint64)
  slot = np.repeat(np.arange(rows.size), cnt)
  order = np.lexsort((key, slot))
  rank = np.arange(indices.size) - np.repeat(indptr[:-1], cnt)
  keep = rank < np.repeat(np.asarray(quota, np.int64), cnt)
  sel_slot, sel_col = slot[order][keep], indices[order][keep]
  o2 = np.lexsort((sel_col, sel_slot))
  return np.minimum(cnt, np.asarray(quota, np.int64)), sel_col[o2]


# ---- pass 1 -----------------------------------------------------------------
_ROW_CACHE = {}


def _row_facts(inc, pattern, r):
  """Per row, from the CSR alone: its paths in lexicographic order, the
  level-1 ids with their path counts, which path is the first to its column,
  the distinct columns and the path count of each."""
  key = (id(inc), pattern, r)
  f = _ROW_CACHE.get(key)
  if f is not None and f["inc"] is inc:
    return f
  lv, ncols = _levels(inc, pattern)
  ids1 = _row(lv[0], r).astype(np.int64)
  paths = row_paths(inc, pattern, r)
  # weight of a level-1 entity = its number of paths
  wt = np.bincount(np.searchsorted(ids1, paths[:, 0]), minlength=ids1.size).astype(np.int64)
  cols, first, npaths = np.unique(paths[:, -1], return_index=True, return_counts=True)
  is_first = np.zeros(paths.shape[0], bool)
  is_first[first] = True
  f = dict(inc=inc, ids1=ids1, wt=wt, paths=paths, is_first=is_first, cols=cols,
           npaths=npaths, ncols=ncols)
  if len(_ROW_CACHE) > 64:
    _ROW_CACHE.clear()
  _ROW_CACHE[key] = f
  return f


def mode3_uniform(W, ncols, shift):
  """W >= ncols 2^shift, exactly (csrc/hgx_sample_mode.h)."""
  return W * (1 << max(-shift, 0)) >= ncols * (1 << max(shift, 0))


def _propose(mode, small, f, W, wmax, h):
  """The 256 proposals of one round: per thread the column (-1 where the
  draw itself rejects) and the index of the proposed path among the row's
  paths. The path offsets of the device (prefix of the level-1 weights, then
  the offset inside the level-1 entity, stepped through l2's incidences by
  their l3 row sizes) index the lexicographic path list directly."""
  if mode == 2:
    return mulhi_np(h, f["ncols"]).astype(np.int64), None
  wt = f["wt"]
  off = np.cumsum(wt) - wt  # exclusive scan of the level-1 weights
  h2 = mix64_np(h ^ np.uint64(0x51ed27))
  h3 = mix64_np(h2 ^ np.uint64(0xa5a5a5a5))
  if small:
    w = mulhi_np(h, W).astype(np.int64)
    j = np.searchsorted(off, w, side="right") - 1  # last entry with off <= w
    pidx = w
    ok = np.ones(h.size, bool)
  else:  # m1 uniform, kept with probability weight / max weight
    j = mulhi_np(h, wt.size).astype(np.int64)
    ok = mulhi_np(h2, wmax).astype(np.int64) < wt[j]
    pidx = off[j] + mulhi_np(h3, wt[j].astype(np.uint64)).astype(np.int64)
  assert np.all(f["paths"][pidx, 0] == f["ids1"][j])
  return np.where(ok, f["paths"][pidx, -1], -1), pidx


def reject_choice(inc, seed, pattern, r, q, reject_w, mode3=0, shift=1, canonical=True):
  """Pass 1 for one row. Returns (result, trace): result is the sorted chosen
  columns, or ("deferred", reason) with reason small / big / stall.
  canonical=False drops the first-path rule (a deliberately wrong sampler for
  the tests' power control)."""
  assert pattern >= PAT_NN and q > 0
  lv, ncols = _levels(inc, pattern)
  f = _row_facts(inc, pattern, r)
  n1 = int(f["ids1"].size)
  W = int(f["wt"].sum())
  wmax = int(f["wt"].max()) if n1 else 0
  tr = dict(pattern=pattern, row=r, q=int(q), n1=n1, W=W, mode=None, small=None, rounds=0,
            staged=False, walks=[0, 0], union=int(f["cols"].size))
  if q > K_SEL_CAP:
    return ("deferred", "big"), tr
  if W <= reject_w:
    return ("deferred", "small"), tr
  mode = 0
  if len(lv) == 3:
    mode = 2 if mode3 == 2 or (mode3 == 0 and mode3_uniform(W, ncols, shift)) else 1
  small = n1 <= K_SB
  tr["mode"], tr["small"] = mode, small
  tr["staged"] = mode == 2 and pattern == PAT_NNE and n1 <= K_SB
  if tr["staged"]:
    evsz = (inc.rp_e[f["ids1"] + 1] - inc.rp_e[f["ids1"]]).astype(np.int64)
  chosen = np.zeros(0, np.int64)
  stall = 0
  tid = np.arange(K_SB, dtype=np.uint64)
  for rnd in range(4096):
    tr["rounds"] = rnd + 1
    base = (((r & 0xffffffff) << 32) ^ (rnd << 12)) & M64
    with np.errstate(over="ignore"):
      h = rand64_np(seed, 0x300 + pattern, np.uint64(base) + tid)
    cand, pidx = _propose(mode, small, f, W, wmax, h)
    ok = (cand >= 0) & ~np.isin(cand, chosen)
    if mode == 2:
      if tr["staged"]:  # which membership walk the device takes (sizes only)
        nc = (inc.rp_e[cand[ok] + 1] - inc.rp_e[cand[ok]]).astype(np.int64)
        probes = np.minimum(evsz[None, :], nc[:, None]).sum(1)
        tr["walks"][0] += int(np.count_nonzero((probes > 0) & (2 * nc <= 5 * probes)))
        tr["walks"][1] += int(np.count_nonzero((probes > 0) & (2 * nc > 5 * probes)))
      ok &= np.isin(cand, f["cols"])
    elif canonical:
      ok &= f["is_first"][pidx]
    acc = cand[ok]  # in thread order; a repeat inside the round keeps its first
    fresh = acc[np.sort(np.unique(acc, return_index=True)[1])]
    got = fresh[:q - chosen.size]
    chosen = np.concatenate([chosen, got])
    if chosen.size >= q:
      return np.sort(chosen), tr
    stall = 0 if got.size else stall + 1
    if stall >= 32:
      break
  return ("deferred", "stall"), tr


# ---- the record stream ------------------------------------------------------
def sample_pattern(inc, pattern, seed, quota, tuning, traces=None):
  """Per-row chosen columns of one pattern: (rows with a quota ascending,
  counts, columns row after row, stats [rejection, stall, uniform])."""
  quota = np.asarray(quota, np.int64)
  rows = np.nonzero(quota > 0)[0]
  lv, ncols = _levels(inc, pattern)
  reject_w = int(tuning["sample_reject_w"])
  shift = tuning["sample_mode3_shift_e"] if pattern == PAT_EEN else tuning["sample_mode3_shift"]
  stats = [0, 0, 0]
  done = {}
  if len(lv) > 1 and reject_w > 0:
    for r in rows:
      res, tr = reject_choice(inc, seed, pattern, int(r), int(quota[r]), reject_w,
                              tuning["sample_mode3"], shift)
      if traces is not None:
        traces.append(tr)
      if isinstance(res, tuple):
        tr["deferred"] = res[1]
        stats[1] += res[1] == "stall"
      else:
        done[int(r)] = res
        stats[0] += 1
        stats[2] += tr["mode"] == 2
  rest = np.array([r for r in rows if int(r) not in done], np.int64)
  if rest.size:
    indptr, indices = pattern_rows(inc, pattern, rest)
    cnt, cols = expand_choice_rows(seed, pattern, rest, indptr, indices, quota[rest])
    ends = np.cumsum(cnt)
    for i, r in enumerate(rest):
      done[int(r)] = cols[ends[i] - cnt[i]:ends[i]]
      if traces is not None:
        traces.append(dict(pattern=pattern, row=int(r), q=int(quota[r]), expand=True,
                           union=int(indptr[i + 1] - indptr[i]), m=int(cnt[i]),
                           n1=int(lv[0][0][r + 1] - lv[0][0][r]), levels=len(lv)))
  counts = np.array([done[int(r)].size for r in rows], np.int64)
  cols = (np.concatenate([done[int(r)] for r in rows]) if rows.size
          else np.zeros(0, np.int64))
  return rows, counts, cols, stats


def _neighbors(inc, idx, K, b, e, seed, stream, row, key):
  """hgx::draw_record_neighbors for records [b, e): row and key per record."""
  if e <= b:
    return
  v = idx[b:e, 0].astype(np.int64) - 1
  ed = idx[b:e, 3].astype(np.int64) - 1
  nb, nl = inc.rp_e[ed].astype(np.int64), (inc.rp_e[ed + 1] - inc.rp_e[ed]).astype(np.uint64)
  eb, el = inc.rp_n[v].astype(np.int64), (inc.rp_n[v + 1] - inc.rp_n[v]).astype(np.uint64)
  if np.any(nl == 0) or np.any(el == 0):
    raise ValueError("a cannot be empty unless no samples are taken")
  urow, inv = np.unique(row, return_inverse=True)
  rk = np.array([rand64_key(seed, ((stream << 32) | int(x)) & M64) for x in urow],
                np.uint64)[inv]
  with np.errstate(over="ignore"):
    k0 = rk + key.astype(np.uint64) * np.uint64(64)
    for k in range(K):
      h = mix64_np(k0 + np.uint64(k))
      h2 = mix64_np(k0 + np.uint64(32 + k))
      idx[b:e, 4 + k] = inc.col_e[nb + mulhi_np(h, nl).astype(np.int64)] + 1
      idx[b:e, 4 + K + k] = inc.col_n[eb + mulhi_np(h2, el).astype(np.int64)] + 1


_KIND_COLS = {"nn": (0, 2), "ee": (1, 3), "ne_node": (0, 3), "ne_edge": (3, 0)}
FAMILIES = {
    # (pattern, kind, quota side) per positive block; neighbour streams
    "fobe": (((PAT_NN, "nn", 0), (PAT_EE, "ee", 1), (PAT_A, "ne_node", 0),
              (PAT_AT, "ne_edge", 1)), 0x200),
    "hobe": (((PAT_NN, "nn", 0), (PAT_EE, "ee", 1), (PAT_NNE, "ne_node", 0),
              (PAT_EEN, "ne_edge", 1)), 0x500),
    "pairs4": (((PAT_NN, "nn", 0), (PAT_EE, "ee", 1), (PAT_NNE, "ne_node", 0),
                (PAT_EEN, "ne_edge", 1)), 0x600),
}


def stream(inc, family, seed, K, quotas, negatives=None, tuning=None, traces=None):
  """The idx array of hgx_sample_fobe ("fobe"), hgx_sample_hobe_rows ("hobe")
  or hgx_sample_pairs4 ("pairs4") and the statistics the device reports:
  (idx, (rejection rows, stall fallbacks, uniform-column rows), block bounds).
  quotas = (node quota, edge quota); negatives likewise (fobe only)."""
  t = dict(DEFAULT_TUNING)
  t.update(tuning or {})
  blocks, nstream = FAMILIES[family]
  R = 4 + 2 * K
  parts, stats = [], [0, 0, 0]
  for pattern, kind, side in blocks:
    rows, cnt, cols, st = sample_pattern(inc, pattern, seed, quotas[side], t, traces)
    stats = [a + b for a, b in zip(stats, st)]
    parts.append((kind, np.repeat(rows, cnt), cols, None))
  if negatives is not None:
    assert family == "fobe"
    for k, (kind, side, ncols) in enumerate((("nn", 0, inc.N), ("ee", 1, inc.E), ("ee", 1, inc.E),
                                             ("ne_node", 0, inc.E), ("ne_edge", 1, inc.N))):
      q = np.asarray(negatives[side], np.int64)
      rr = np.repeat(np.arange(q.size), q)
      j = np.arange(rr.size) - np.repeat(np.cumsum(q) - q, q)
      ctr = (rr.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)
      c = mulhi_np(rand64_np(seed, 0x300 + k, ctr), ncols).astype(np.int64)
      parts.append((kind, rr, c, j))
  n = sum(p[1].size for p in parts)
  idx = np.zeros((n, R), np.int32)
  bounds = [0]
  for i, (kind, rr, cc, rank) in enumerate(parts):
    b, e = bounds[-1], bounds[-1] + rr.size
    bounds.append(e)
    rc, cc_ = _KIND_COLS[kind]
    idx[b:e, rc] = rr + 1
    idx[b:e, cc_] = cc + 1
    if kind.startswith("ne"):
      s = (nstream if rank is None else 0x400) + (kind == "ne_edge")
      _neighbors(inc, idx, K, b, e, seed, s, rr, cc if rank is None else rank)
  return idx, tuple(stats), bounds


# ---- case graphs ------------------------------------------------------------
def _incidence(N, E, pairs):
  from hypergraphembedding_amd.hypergraph_util import Incidence, _csr_from_pairs
  p = np.asarray(pairs, np.int64).reshape(-1, 2)
  rp, col = _csr_from_pairs(N, p[:, 0], p[:, 1])
  return Incidence(N, E, rp, col)


def small_graph():
  z = np.load(os.path.join(ROOT, "tests", "golden", "csr_small.npz"), allow_pickle=False)
  from hypergraphembedding_amd.hypergraph_util import Incidence
  return Incidence(int(z["N"]), int(z["E"]), z["rp_n"], z["col_n"], z["rp_e"], z["col_e"])


HUB = dict(N=700, E=400, hub_node=0, big_edge=399, empty_edge=398, isolated=699,
           tiny_node=698, tiny_edges=(396, 397), mid_edges=tuple(range(300, 308)),
           meet_node=1)


def hub_graph():
  """700 nodes, 400 edges. Node 0 sits in edges 0..299; edge 399 has nodes
  1..300; edges 300..307 have 33..64 members; node 698 has the two small
  edges 396 and 397, of which 397 meets edge 399; node 699 is isolated and
  edge 398 is empty."""
  g = HUB
  rs = np.random.RandomState(20260)
  pairs = []
  for e in range(300):  # the hub node's edges: the hub and 1..5 others
    pairs.append((0, e))
    for v in rs.choice(np.arange(1, 697), rs.randint(1, 6), replace=False):
      pairs.append((v, e))
  for k, e in enumerate(g["mid_edges"]):  # two-block Bloom filters
    for v in rs.choice(np.arange(1, 697), 33 + (31 * k) // 7, replace=False):
      pairs.append((v, e))
  for e in range(308, 396):
    for v in rs.choice(np.arange(1, 697), rs.randint(2, 9), replace=False):
      pairs.append((v, e))
  pairs += [(698, 396), (697, 396), (698, 397), (697, 397), (300, 397)]
  pairs += [(v, 399) for v in range(1, 301)]
  inc = _incidence(g["N"], g["E"], pairs)
  deg, size = inc.node_degree(), inc.edge_size()
  assert deg[0] == 300 and size[399] == 300 and deg[699] == 0 and size[398] == 0
  assert all(33 <= size[e] <= 64 for e in g["mid_edges"]) and size[307] == 64
  assert deg[698] == 2 and size[396] == 2 and size[397] == 3
  assert 399 in pattern_row(inc, PAT_NNE, 698)
  # 3-hop expansion of the hub row: more than one level-1 chunk, W2 > 256
  assert size[:256].sum() > 256
  return inc


def big_graph():
  """Edge 0 has 2,600 members (nodes 0..2599); edges 1..8 are small."""
  rs = np.random.RandomState(20261)
  pairs = [(v, 0) for v in range(2600)]
  for e in range(1, 9):
    for v in rs.choice(2650, 4, replace=False):
      pairs.append((v, e))
  inc = _incidence(2650, 9, pairs)
  assert inc.edge_size()[0] == 2600 and inc.node_degree()[0] >= 1
  assert pattern_row(inc, PAT_NN, 0).size >= 2600
  return inc


def full_graph():
  """Node 0 is in three overlapping edges whose union has 2,100 nodes."""
  pairs = [(v, 0) for v in range(0, 900)] + [(v, 1) for v in [0] + list(range(700, 1500))] + \
      [(v, 2) for v in [0] + list(range(1400, 2100))]
  inc = _incidence(2100, 3, pairs)
  assert pattern_row(inc, PAT_NN, 0).size == 2100
  return inc


def stall_graph():
  """Node 0 is in two edges whose union has 5 nodes (7 paths)."""
  pairs = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (3, 1), (4, 1), (5, 2), (6, 2)]
  inc = _incidence(7, 3, pairs)
  assert pattern_row(inc, PAT_NN, 0).size == 5
  return inc


WIDE_N = LDS_BITMAP_COLS + 1 + 64


def wide_graph():
  """393,281 nodes, nearly all isolated; 40 edges of 3..12 members spread
  over the whole id range, the last ids included."""
  rs = np.random.RandomState(20262)
  N, E = WIDE_N, 40
  pool = np.unique(np.concatenate([rs.choice(N, 150, replace=False),
                                   np.arange(N - 6, N), np.arange(0, 4)]))
  pairs = []
  for e in range(E):
    for v in rs.choice(pool, rs.randint(3, 13), replace=False):
      pairs.append((v, e))
  pairs += [(N - 1, 0), (N - 2, 0), (0, 0), (N - 1, 1)]
  inc = _incidence(N, E, pairs)
  assert inc.N > LDS_BITMAP_COLS and inc.N > EMIT_GRID and 100 < inc.nnz < 1000
  assert inc.node_degree()[N - 1] >= 2
  return inc


def _q(n, entries):
  q = np.zeros(n, np.int32)
  for r, v in entries:
    q[r] = v
  return q


def _t(reject_w=32768, mode3=0, shift=1, shift_e=1):
  return dict(sample_reject_w=reject_w, sample_mode3=mode3, sample_mode3_shift=shift,
              sample_mode3_shift_e=shift_e)


def hub_quotas(inc):
  """Quotas on the hub rows, the rows around them and a fixed random set."""
  g = HUB
  rs = np.random.RandomState(20263)
  nq = _q(inc.N, [(v, 7) for v in rs.choice(inc.N, 40, replace=False)] +
          [(g["hub_node"], 150), (g["tiny_node"], 40), (g["meet_node"], 60), (300, 25),
           (697, 30), (g["isolated"], 9)])
  eq = _q(inc.E, [(e, 6) for e in rs.choice(inc.E, 40, replace=False)] +
          [(g["big_edge"], 150), (307, 50), (300, 20), (397, 35), (396, 12), (5, 64),
           (g["empty_edge"], 9)])
  return nq, eq


def hub_negatives(inc):
  g = HUB
  rs = np.random.RandomState(20264)
  nn = _q(inc.N, [(v, 4) for v in rs.choice(np.arange(1, 697), 12, replace=False)] + [(0, 20)])
  ne = _q(inc.E, [(e, 4) for e in rs.choice(np.arange(0, 396), 12, replace=False)] +
          [(g["big_edge"], 20)])
  assert nn[g["isolated"]] == 0 and ne[g["empty_edge"]] == 0
  return nn, ne


def first_clean_seed(inc, K, quotas, negatives, base):
  """The first seed >= base at which no negative node-edge record has an
  endpoint without neighbours (the device raises there, as the reference's
  np.random.choice does): decided by the restatement alone."""
  for seed in range(base, base + 64):
    try:
      stream(inc, "fobe", seed, K, quotas, negatives, _t(reject_w=0))
      return seed
    except ValueError:
      continue
  raise AssertionError("no seed without an empty endpoint")


def _settings3(split_w):
  """The 3-hop tuning settings of a case; split_w is a path count that has
  rows of the case on both sides."""
  return (
    ("default", _t()),
    ("expand", _t(reject_w=0)),
    ("w1-auto", _t(reject_w=1)),
    ("w1-paths", _t(reject_w=1, mode3=1)),
    ("w1-uniform", _t(reject_w=1, mode3=2)),
    ("split-shift-2+2", _t(reject_w=split_w, shift=-2, shift_e=2)),
    ("split-shift+2-2", _t(reject_w=split_w, shift=2, shift_e=-2)),
    ("w1-shift0-2", _t(reject_w=1, shift=0, shift_e=-2)),
  )


def cases():
  """name -> dict(inc, runs): a run is (label, family, seed, K, quotas,
  negatives, tuning). Every row with a quota of every run is compared with
  the device by tests/test_gpu_sampler_kernels.py."""
  out = {}
  inc = small_graph()
  rs = np.random.RandomState(20265)
  nq = rs.randint(0, 9, inc.N).astype(np.int32)
  eq = rs.randint(0, 9, inc.E).astype(np.int32)
  nnq = rs.randint(0, 4, inc.N).astype(np.int32)
  neq = rs.randint(0, 4, inc.E).astype(np.int32)
  runs = [("hobe-" + n, "hobe", 41, 5, (nq, eq), None, t) for n, t in _settings3(60)]
  runs += [("fobe-K1-w1", "fobe", 44, 1, (nq, eq), (nnq, neq), _t(reject_w=1)),
           ("fobe-K5-w1", "fobe", 48, 5, (nq, eq), (nnq, neq), _t(reject_w=1)),
           ("fobe-K5-split", "fobe", 48, 5, (nq, eq), (nnq, neq), _t(reject_w=12)),
           ("fobe-K5-expand", "fobe", 48, 5, (nq, eq), (nnq, neq), _t(reject_w=0)),
           ("fobe-K16-w1", "fobe", 59, 16, (nq, eq), (nnq, neq), _t(reject_w=1))]
  runs += [("pairs4-" + n, "pairs4", 47, 3, (nq, eq), None, t)
           for n, t in (("default", _t()), ("w1-auto", _t(reject_w=1)))]
  out["small"] = dict(inc=inc, runs=runs)

  inc = hub_graph()
  hq = hub_quotas(inc)
  hn = hub_negatives(inc)
  # (the pair blocks of the weighted-Jaccard sampler: the same four patterns
  # as HOBE, whose coordinates a graph with an isolated node cannot have)
  runs = [("pairs4-" + n, "pairs4", 51, 2, hq, None, t) for n, t in _settings3(600)]
  for K in (1, 5, 16):
    runs.append(("fobe-K%d" % K, "fobe", ("clean", 53), K, hq, hn,
                 _t(reject_w=1) if K != 5 else _t(reject_w=8)))
  out["hub"] = dict(inc=inc, runs=runs)

  inc = big_graph()
  runs = []
  for q in (2048, 2049, 2100, 2600, 3000):
    quotas = (_q(inc.N, [(0, q), (2599, 5)]), _q(inc.E, [(0, q), (3, 3)]))
    runs.append(("fobe-q%d-expand" % q, "fobe", 61, 1, quotas, None, _t(reject_w=0)))
    if q in (2048, 2049, 3000):
      runs.append(("fobe-q%d-reject" % q, "fobe", 61, 1, quotas, None, _t(reject_w=1)))
  out["big"] = dict(inc=inc, runs=runs)

  inc = full_graph()
  out["full"] = dict(inc=inc, runs=[
      ("fobe-q2048", "fobe", 71, 1, (_q(inc.N, [(0, 2048)]), _q(inc.E, [])), None, _t(reject_w=1))])

  inc = stall_graph()
  out["stall"] = dict(inc=inc, runs=[
      ("fobe-q10", "fobe", 81, 2, (_q(inc.N, [(0, 10), (5, 1)]), _q(inc.E, [(1, 2)])), None,
       _t(reject_w=1))])

  inc = wide_graph()
  N = inc.N
  wq = (_q(N, [(0, 6), (N - 1, 50), (N - 2, 3), (int(inc.col_e[inc.rp_e[7]]), 4)]),
        _q(inc.E, [(0, 30), (1, 4), (7, 100), (39, 5)]))
  out["wide"] = dict(inc=inc, runs=[
      ("fobe-expand", "fobe", 91, 2, wq, None, _t(reject_w=0)),
      ("fobe-default", "fobe", 91, 2, wq, None, _t()),
      ("pairs4-expand", "pairs4", 93, 2, wq, None, _t(reject_w=0)),
      ("pairs4-w1", "pairs4", 93, 2, wq, None, _t(reject_w=1)),
  ])
  return out


def run_seed(case, run):
  """The seed of a run: fixed, or the first clean one from its base."""
  label, family, seed, K, quotas, negatives, tuning = run
  if isinstance(seed, tuple):
    return first_clean_seed(case["inc"], K, quotas, negatives, seed[1])
  return seed


def run_stream(case, run, traces=None):
  label, family, seed, K, quotas, negatives, tuning = run
  return stream(case["inc"], family, run_seed(case, run), K, quotas, negatives, tuning, traces)


# ---- branch labels ----------------------------------------------------------
def _reject_labels():
  out = []
  for p in ("NN", "EE"):
    out += ["reject/%s/paths/small" % p, "reject/%s/paths/large" % p]
  for p in ("NNE", "EEN"):
    out += ["reject/%s/paths/small" % p, "reject/%s/paths/large" % p]
  out += ["reject/NNE/uniform/staged", "reject/NNE/uniform/unstaged", "reject/EEN/uniform"]
  return out


REQUIRED_BRANCHES = tuple(_reject_labels() + [
    "reject/rounds>1", "reject/q=2048-hash-half-full",
    "nne_meets/members-walk", "nne_meets/min-common-walk",
    "mode/auto/uniform", "mode/auto/paths", "mode/auto/negative-shift",
    "mode/auto/shift-differs-by-side",
    "defer/small", "defer/big", "defer/stall",
    "expand/levels1", "expand/levels2", "expand/levels3",
    "expand/level1-chunks", "expand/w2-chunks",
    "expand/select/m<=2048", "expand/select/m>2048", "expand/all/m>2048/sorted",
    "expand/all/m>2048/levels1", "expand/all/m<=2048", "expand/empty-row",
    "expand/bitmap-lds", "expand/bitmap-global", "emit/grid-stride",
    "bloom/one-block", "bloom/two-blocks", "bloom/many-blocks",
    "negatives", "neighbors/positives", "neighbors/negatives", "K=1", "K=5", "K=16",
    "family/fobe", "family/hobe", "family/pairs4",
])


def labels_of(case, run, traces, idx=None):
  """Branch labels reached by one run, from its traces, the graph and (for
  the labels of whole blocks) its records."""
  label, family, seed, K, quotas, negatives, tuning = run
  inc = case["inc"]
  t = dict(DEFAULT_TUNING)
  t.update(tuning)
  out = set()
  if idx is not None:
    out = {"family/" + family, "K=%d" % K} & set(REQUIRED_BRANCHES)
    ne = (idx[:, 0] > 0) & (idx[:, 3] > 0)
    pos_end = idx.shape[0] if negatives is None else idx.shape[0] - sum(
        int(np.asarray(negatives[s_]).sum()) for s_ in (0, 1, 1, 0, 1))
    if np.any(ne[:pos_end]):
      out.add("neighbors/positives")
    if np.any(ne[pos_end:]):
      out |= {"negatives", "neighbors/negatives"}
    if max(inc.N, inc.E) > EMIT_GRID:
      out.add("emit/grid-stride")
  want = (16 * inc.edge_size().astype(np.int64) + 511) // 512  # Bloom blocks before rounding
  bloom = {"bloom/" + n for n, hit in (("one-block", want == 1), ("two-blocks", want == 2),
                                       ("many-blocks", want > 2)) if np.any(hit)}
  for tr in traces:
    p = PAT_NAME[tr["pattern"]]
    lv, ncols = _levels(inc, tr["pattern"])
    if tr.get("expand"):
      out.add("expand/levels%d" % tr["levels"])
      if tr["levels"] > 1:
        out.add("expand/bitmap-global" if ncols > LDS_BITMAP_COLS else "expand/bitmap-lds")
        if tr["n1"] > K_SB:
          out.add("expand/level1-chunks")
          if tr["levels"] == 3:
            ids = _row(lv[0], tr["row"])[:K_SB]
            if int((lv[1][0][ids + 1] - lv[1][0][ids]).sum()) > K_SB:
              out.add("expand/w2-chunks")
      m, cnt = tr["m"], tr["union"]
      if cnt == 0:
        out.add("expand/empty-row")
      elif m < cnt:
        out.add("expand/select/m>2048" if m > K_SEL_CAP else "expand/select/m<=2048")
      elif m > K_SEL_CAP:
        out.add("expand/all/m>2048/levels1" if tr["levels"] == 1 else "expand/all/m>2048/sorted")
      else:
        out.add("expand/all/m<=2048")
      continue
    if "deferred" in tr:
      out.add("defer/" + tr["deferred"])
    if tr["mode"] is None:
      continue
    if tr["mode"] == 2:
      out.add("reject/NNE/uniform/" + ("staged" if tr["staged"] else "unstaged")
              if p == "NNE" else "reject/EEN/uniform")
      if tr["walks"][0]:
        out.add("nne_meets/members-walk")
      if tr["walks"][1]:
        out.add("nne_meets/min-common-walk")
    else:
      out.add("reject/%s/paths/%s" % (p, "small" if tr["small"] else "large"))
    if len(lv) == 3:
      out |= bloom
      if t["sample_mode3"] == 0:
        out.add("mode/auto/" + ("uniform" if tr["mode"] == 2 else "paths"))
        sh = t["sample_mode3_shift_e"] if p == "EEN" else t["sample_mode3_shift"]
        if sh < 0:
          out.add("mode/auto/negative-shift")
        other = t["sample_mode3_shift"] if p == "EEN" else t["sample_mode3_shift_e"]
        if mode3_uniform(tr["W"], ncols, sh) != mode3_uniform(tr["W"], ncols, other):
          out.add("mode/auto/shift-differs-by-side")
    if "deferred" not in tr:
      if tr["rounds"] > 1:
        out.add("reject/rounds>1")
      if tr["q"] == K_SEL_CAP:
        out.add("reject/q=2048-hash-half-full")
  return out


def census():
  """(lines of the branch census, union of labels over all cases)."""
  lines, reached = [], set()
  bloom_labels = {"bloom/one-block", "bloom/two-blocks", "bloom/many-blocks"}
  for name, case in cases().items():
    for run in case["runs"]:
      traces = []
      idx, stats, bounds = run_stream(case, run, traces)
      reached |= labels_of(case, run, traces, idx)
      per = {}
      for tr in traces:
        for lab in labels_of(case, run, [tr]) - bloom_labels:
          per[lab] = per.get(lab, 0) + 1
      rounds = max([tr["rounds"] for tr in traces if not tr.get("expand")] or [0])
      lines.append("%s / %s: %d records, stats %s, max rounds %d" %
                   (name, run[0], idx.shape[0], list(stats), rounds))
      for lab in sorted(per):
        lines.append("    %-34s %d rows" % (lab, per[lab]))
  return lines, reached


if __name__ == "__main__":
  lines, reached = census()
  missing = sorted(set(REQUIRED_BRANCHES) - reached)
  out = os.path.join(ROOT, "profiles", "samplers", "branch_census.txt")
  os.makedirs(os.path.dirname(out), exist_ok=True)
  with open(out, "w") as fh:
    fh.write("Branch census of the sampler case graphs (tests/sampler_cases.py): per case and\n"
             "run, the rows of the host restatement per branch label and the largest number of\n"
             "rejection rounds of a row.\n\n")
    fh.write("\n".join(lines) + "\n\nlabels not reached: %s\n" % (", ".join(missing) or "none"))
  print("\n".join(lines))
  print("missing:", missing)
