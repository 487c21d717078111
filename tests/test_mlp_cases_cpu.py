"""The MLP restatement (oracle/mlpref.c) against float64 autograd over whole
runs (mlp_autograd.py; no GPU): 3 batches of 24 + 24 + 5 samples, 2 epochs,
so Adagrad's accumulator on later batches, the division by a ragged last
batch's M, the batch-size-weighted epoch loss and the second epoch's dropout
stream are all in the result. At I = 70 / 150 and D = 70 every layer reduces
over more than 64 positions (head_dot's chains beyond j = 0, waves 2 and 3
of the four-way split) and the dropout mask has a second (and third) 64-bit
word. The device is bit for bit the restatement (test_gpu_mlp.py,
test_gpu_mlp_kernels.py), so this is its float64 check too.

Bar (the suite's convention, ae_cases.py). E = the max-abs distance of the
float32 torch run from the float64 run over the flat weight vector; the
restatement must be within 8 E + 2 ulp32(max |p|), its epoch losses within
rtol 1e-5. The RATIO lines (profiles/mlp/cpu_ratios.txt) give err / E per
case and setting, and per layer for information.

Condition, asserted first: every relu unit of every batch is on the same
side of zero in the float64 and the float32 run (a unit that float32 puts on
the other side is a different function, not a rounding), and every relu
layer has units on both sides."""

import numpy as np
import pytest
import torch

import mlp_autograd as A
import oracle as O
from mlp_cases import glorot, make_case

N, BATCH, EPOCHS, DSEED = 53, 24, 2, 77
CASES = [(0, 70, 0), (1, 150, 70), (2, 150, 70)]
SETTINGS = ("keras", "prop", "mid")

_cache = {}


def case(kind, I, D):
  """Inputs (shared, never modified): small tables, glorot weights with
  biases of scale 0.1, explicit permutations. The seed is 40 + kind; no seed
  had to be moved for the relu condition."""
  key = (kind, I, D)
  if key not in _cache:
    rng, nt, et, nr, er, lab = make_case(kind, I, D, N, 40 + kind, rows=(30, 20))
    w0 = glorot(A.shapes_of(kind, I, D), rng, 0.1)
    assert w0.size == O.mlp_num_weights(kind, I, D)
    perms = np.stack([rng.permutation(N) for _ in range(EPOCHS)])
    c = dict(kind=kind, I=I, D=D, nt=nt, et=et, nr=nr, er=er, lab=lab, w0=w0,
             perms=perms)
    e3, med = A.mid_eps(kind, I, D, w0, nt, et, nr, er, lab, perms, BATCH, DSEED)
    assert med / 10 <= e3 <= med * 10, (e3, med)
    c["settings"] = {"keras": (0.01, 1e-7), "prop": (1.0, 10.0), "mid": (0.01, e3)}
    c["runs"] = {}
    _cache[key] = c
  return _cache[key]


def runs(c, setting):
  """(float64 run, float32 run) of a setting, computed once."""
  if setting not in c["runs"]:
    lr, eps = c["settings"][setting]
    args = (c["kind"], c["I"], c["D"], c["w0"], c["nt"], c["et"], c["nr"], c["er"],
            c["lab"], c["perms"])
    kw = dict(batch=BATCH, lr=lr, eps=eps, seed=DSEED)
    c["runs"][setting] = (A.fit(*args, **kw),
                          A.fit(*args, dtype=torch.float32, **kw))
  return c["runs"][setting]


def check_relu_condition(r64, r32, tag):
  s64, s32 = A.relu_sides(r64), A.relu_sides(r32)
  assert len(s64) == len(s32) == EPOCHS * 3
  for b, (l64, l32) in enumerate(zip(s64, s32)):
    assert len(l64) == len(l32) > 0
    for (name, a), (_, f) in zip(l64, l32):
      flips = int((a != f).sum())
      assert flips == 0, (tag, "batch", b, name, "units on the other side in "
                          "float32", flips)
      assert a.any() and not a.all(), (tag, "batch", b, name, "one-sided")


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("kind,I,D", CASES)
def test_fit_matches_float64(kind, I, D, setting):
  c = case(kind, I, D)
  lr, eps = c["settings"][setting]
  r64, r32 = runs(c, setting)
  tag = f"kind{kind} I{I} D{D} {setting}"
  check_relu_condition(r64, r32, tag)
  w, losses = O.mlp_fit(kind, I, D, c["w0"], c["nt"], c["et"], c["nr"], c["er"],
                        c["lab"], c["perms"], batch=BATCH, lr=lr, eps=eps,
                        min_delta=-1e30, seed=DSEED)
  w = w.astype(np.float64)
  E = float(np.abs(r32.w - r64.w).max())
  err = np.abs(w - r64.w)
  bar = 8 * E + 2 * A.ulp32(np.abs(r64.w).max())
  for name, sl in A.layer_slices(kind, I, D):
    El = float(np.abs(r32.w[sl] - r64.w[sl]).max())
    print(f"RATIO {tag} layer {name}: err {err[sl].max():.3g} E {El:.3g} "
          f"ratio {err[sl].max() / El if El > 0 else 0.0:.2f}")
  print(f"RATIO {tag} all: err {err.max():.3g} E {E:.3g} "
        f"ratio {err.max() / E:.2f} bar {bar:.3g} (lr {lr:g} eps {eps:g}) "
        f"loss {losses[-1]:.6f} ref {r64.losses[-1]:.6f}")
  assert len(losses) == EPOCHS
  assert E > 0 and not np.array_equal(w, c["w0"].astype(np.float64))
  assert err.max() <= bar, (tag, err.max(), E, bar, int(err.argmax()))
  np.testing.assert_allclose(losses, r64.losses, rtol=1e-5)


@pytest.mark.parametrize("kind,I,D", CASES)
def test_predict_matches_float64(kind, I, D):
  """All outputs of the restatement's inference on the weights it trained
  (Keras' setting), against the float64 forward pass of the same weights."""
  c = case(kind, I, D)
  lr, eps = c["settings"]["keras"]
  w, _ = O.mlp_fit(kind, I, D, c["w0"], c["nt"], c["et"], c["nr"], c["er"],
                   c["lab"], c["perms"], batch=BATCH, lr=lr, eps=eps,
                   min_delta=-1e30, seed=DSEED)
  nt, et, nr, er = c["nt"], c["et"], c["nr"], c["er"]
  for out in ((0,) if kind == 0 else (0, 1, 2)):
    a = nr if out != 2 else None
    b = er if out != 1 else None
    y = O.mlp_predict(kind, I, D, w, nt, et, out, a, b).astype(np.float64)
    y64 = A.predict(kind, I, D, w, nt, et, out, a, b)
    y32 = A.predict(kind, I, D, w, nt, et, out, a, b, dtype=torch.float32)
    assert y.shape == y64.shape
    Ey = float(np.abs(y32 - y64).max())
    err = float(np.abs(y - y64).max())
    bar = 8 * Ey + 2 * A.ulp32(1.0)
    print(f"RATIO kind{kind} I{I} D{D} predict output {out}: err {err:.3g} "
          f"E_y {Ey:.3g} ratio {err / Ey if Ey > 0 else 0.0:.2f} bar {bar:.3g}")
    assert err <= bar, (kind, out, err, Ey, bar)
    assert y64.min() > 0 and y64.max() < 1 and y64.std() > 0
