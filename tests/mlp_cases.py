"""Inputs, the dispatch table and the host statement of the device shuffle
shared by the dense MLP tests (test_gpu_mlp.py, test_gpu_mlp_kernels.py,
test_mlp_oracle.py, test_mlp_cases_cpu.py). A helper module, not a conftest.

reach() restates, in plain Python, which kernel instantiation each launch of
one batch selects (launch_fwd, launch_bwd, launch_wgrad, head_wave and
run_batch of csrc/hgx_mlp.hip); REACHABLE is everything the dispatchers can
select under the engine's validation. test_gpu_mlp_kernels.py asserts that
its cases reach all of it.

Names. A kernel's name as the device reports it, then, after a slash, the
form a run-time branch inside that instantiation takes:
  mlp_fwd<k>           k = 2..8: every job of the launch has K = 64 k
  mlp_fwd<0>/1         the generic kernel at one chunk
  mlp_fwd<0>/9+        ... at more than 8 chunks
  mlp_fwd<0>/mixed     ... with jobs of different K (kind-2 training: the
                       hidden layer, K = 2 Kd, and the post layers, K = Kd)
  mlp_bwd<n>           n = 2..8 chunks over the job's one or two terms
  mlp_bwd<0>/1, /9+    the generic kernel
  mlp_bwd<n,true>      n = 1..8: the joint layers' launch with the label head
                       fused in; fused_head/KH=2 or 4 is the head's form
  mlp_head/KH=2,4,8    the head's own launch, label K <= 128 / 256 / 512 in
                       registers; mlp_head/loop: K > 512
  mlp_wgrad<c>         c = ceil(M / 64) = 1..4
"""

import numpy as np

M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------
# the counter-based generator (hgx::rand64) and the device shuffle
# ---------------------------------------------------------------------------
def mix64(z):
  z = (z + 0x9e3779b97f4a7c15) & M64
  z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
  z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
  return z ^ (z >> 31)


def rand64(seed, stream, ctr):
  return mix64((mix64(seed ^ mix64((stream + 0x632be59bd9b4e019) & M64)) + ctr)
               & M64)


def shuffle_perms(seed, epochs, n):
  """The order fit(perms=None, seed=seed) trains in: epoch ep is the stable
  argsort of the keys rand64(seed, 0x4d4c5053 + ep, i), i in [0, n)
  (mlp_shuffle_keys, a 64-bit radix sort of (key, i) pairs, mlp_permute)."""
  perms = []
  for ep in range(epochs):
    keys = np.array([rand64(seed, 0x4d4c5053 + ep, i) for i in range(n)],
                    np.uint64)
    assert np.unique(keys).size == n, "equal keys: the order would be the sort's"
    perms.append(np.argsort(keys, kind="stable"))
  return np.stack(perms).astype(np.int64)


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def glorot(shapes, rng, bias_scale=0.0):
  parts = []
  for k, n in shapes:
    lim = np.sqrt(6.0 / (k + n))
    parts += [rng.uniform(-lim, lim, k * n), rng.normal(0, bias_scale, n)]
  return np.concatenate(parts).astype(np.float32)


def make_case(kind, I, D, n, seed, rows=(300, 150)):
  rng = np.random.default_rng(seed)
  nt = rng.random((rows[0], I)).astype(np.float32)
  et = rng.random((rows[1], I)).astype(np.float32)
  nr = rng.integers(0, rows[0], n).astype(np.int32)
  er = rng.integers(0, rows[1], n).astype(np.int32)
  lab = (rng.random(n) < 1 / 6).astype(np.float32)
  return rng, nt, et, nr, er, lab


def run_both(ctx, kind, I, D, n, epochs, seed=3, bias_scale=0.1, batch=256,
             lr=0.01, eps=1e-7):
  """The device and the restatement trained on one case (Keras' Adagrad
  setting by default): (engine, inputs, device weights, restatement weights,
  device losses, restatement losses)."""
  import oracle as O
  from hypergraphembedding_amd import _hgx
  rng, nt, et, nr, er, lab = make_case(kind, I, D, n, seed)
  m = _hgx.Mlp(ctx, kind, I, D)
  w0 = glorot(m.shapes, rng, bias_scale)
  assert w0.size == O.mlp_num_weights(kind, I, D)
  m.set_weights(w0)
  np.testing.assert_array_equal(m.get_weights(), w0)
  m.set_tables(nt, et)
  m.set_samples(nr, er, lab)
  perms = np.stack([rng.permutation(n) for _ in range(epochs)])
  dseed = 77
  gl = m.fit(batch=batch, max_epochs=epochs, lr=lr, eps=eps, min_delta=-1e30,
             seed=dseed, perms=perms)
  wg = m.get_weights()
  wc, cl = O.mlp_fit(kind, I, D, w0, nt, et, nr, er, lab, perms, batch=batch,
                     lr=lr, eps=eps, min_delta=-1e30, seed=dseed)
  return m, (nt, et, nr, er), wg, wc, gl, cl


# ---------------------------------------------------------------------------
# the dispatch, restated
# ---------------------------------------------------------------------------
def ru(x, a):
  return (x + a - 1) // a * a


def widths(kind, I, D):
  """Padded reduction widths: (Kin, Kh, Kd, label K)."""
  ldt = ru(I, 4)
  if kind == 0:
    return ru(2 * ldt, 64), 0, 0, ru(I, 64)
  Kd = ru(D, 64)
  return ru(ldt, 64), ru((I + D) // 2, 64), Kd, Kd


def _fwd(Ks):
  """One forward launch whose non-prefetch jobs have the reduction widths
  Ks."""
  if len(set(Ks)) > 1:
    return "mlp_fwd<0>/mixed"
  k = Ks[0] // 64
  return f"mlp_fwd<{k}>" if 2 <= k <= 8 else ("mlp_fwd<0>/1" if k == 1 else "mlp_fwd<0>/9+")


def _bwd(n):
  return f"mlp_bwd<{n}>" if 2 <= n <= 8 else ("mlp_bwd<0>/1" if n == 1 else "mlp_bwd<0>/9+")


def _kh(K):
  return "KH=2" if K <= 128 else "KH=4" if K <= 256 else "KH=8" if K <= 512 else "loop"


def reach(kind, I, D, M, train, fuse_head=1):
  """The instantiations (names above) that one batch of M rows launches:
  a training batch, or a predict chunk of output 0 (outputs 1 and 2 launch a
  subset: the pre and the joint layer of one side)."""
  assert 1 <= M <= (256 if train else 4096)
  Kin, Kh, Kd, Kl = widths(kind, I, D)
  out = set()
  if train:
    out.add(f"mlp_wgrad<{(M + 63) // 64}>")
  if kind == 0:
    out.add(_fwd([Kin]))
    out.add("mlp_head/" + _kh(Kl))
    return out
  ae = kind == 2 and train
  out.add(_fwd([Kin]))                                   # pre
  out.add(_fwd([Kh]))                                    # joint
  out.add(_fwd([2 * Kd, Kd, Kd] if ae else [2 * Kd]))    # hidden (+ post)
  nj = Kd // 64 + (Kh // 64 if ae else 0)
  fuse = train and fuse_head and Kd <= 256 and nj <= 8
  if not fuse:
    out.add("mlp_head/" + _kh(Kl))
  if not train:
    return out
  if ae:
    out.add(_fwd([Kh]))                                  # rec, loss epilogue
    out.add(_bwd(ru(I, 64) // 64))                       # post
  if fuse:
    out.add(f"mlp_bwd<{nj},true>")
    out.add("fused_head/" + _kh(Kl))
  else:
    out.add(_bwd(nj))                                    # joint
  out.add(_bwd(Kd // 64))                                # pre
  return out


# Everything the dispatchers can select. Left out, unreachable under the
# engine's validation:
#   mlp_wgrad<0>     needs a batch of more than 256 rows; fit refuses those
#   head_wave_t<>    (activations read at run time) the label head is always
#                    a sigmoid over a relu layer, in all three models
#   mlp_fwd<1>, mlp_bwd<1> (unfused)   not instantiated: one chunk takes <0>
#   fused_head/KH=8, /loop             the head is fused only at Kd <= 256
REACHABLE = frozenset(
    [f"mlp_fwd<{k}>" for k in range(2, 9)] +
    ["mlp_fwd<0>/1", "mlp_fwd<0>/9+", "mlp_fwd<0>/mixed"] +
    [f"mlp_bwd<{n}>" for n in range(2, 9)] +
    ["mlp_bwd<0>/1", "mlp_bwd<0>/9+"] +
    [f"mlp_bwd<{n},true>" for n in range(1, 9)] +
    ["fused_head/KH=2", "fused_head/KH=4"] +
    ["mlp_head/KH=2", "mlp_head/KH=4", "mlp_head/KH=8", "mlp_head/loop"] +
    [f"mlp_wgrad<{c}>" for c in range(1, 5)])

# kernels of the epoch plumbing (no instantiations): every fit launches the
# last two, fit(perms=None) also the first
EPOCH_KERNELS = frozenset(["mlp_shuffle_keys", "mlp_permute", "mlp_loss_reduce"])


def kernel_names(tags):
  """The device-visible kernel names of a set of reach() names."""
  return {t.split("/")[0] for t in tags if t.startswith("mlp_")}
