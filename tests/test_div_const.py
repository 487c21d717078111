"""CPU: the trainer step's division by the neighbour count, exhaustively.

csrc/hgx_divk.h (the text the device kernels compile) is built into a
stand-alone host program, tests/native/div_const_check.cpp, with -O2,
contraction off and OpenMP. For every K that has a step kernel it compares
div_const<K>(x) with x / (float)K under round-to-nearest for all 2^32 float
bit patterns (denormals, both zeros, infinities and NaNs; equal bits, or NaN
on both sides) on at most 16 threads and exits non-zero on the first
difference. The step uses div_const only for these K (div_k in
csrc/hgx_train_step.h)."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "div_const_check.cpp")
INC = os.path.join(ROOT, "hypergraphembedding_amd", "csrc")
STEP = os.path.join(INC, "hgx_train_step.h")

STEP_K = (5,)  # pick_step (csrc/hgx_train.hip): the step is built for K = 5


def test_div_k_uses_div_const_only_for_the_checked_k():
  text = open(STEP).read()
  m = re.search(r"if constexpr \(HGX_TRAIN_DIVK && \(?([^)]*)\)\)? return div_const<K>", text)
  assert m, "div_k's condition not found"
  ks = tuple(sorted(int(k) for k in re.findall(r"K == (\d+)", m.group(1))))
  assert ks == STEP_K, ks


def test_div_const_equals_division_for_every_float(tmp_path):
  cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
  if cxx is None:
    pytest.fail("no host C++ compiler (g++ or clang++) on PATH")
  exe = str(tmp_path / "div_const_check")
  cmd = [cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fopenmp", "-I" + INC, SRC,
         "-o", exe]
  b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  assert b.returncode == 0, b.stdout
  env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
  r = subprocess.run([exe] + [str(k) for k in STEP_K], stdout=subprocess.PIPE,
                     stderr=subprocess.STDOUT, text=True, env=env)
  print(r.stdout)
  assert r.returncode == 0, r.stdout
  for k in STEP_K:
    assert f"K = {k}: {1 << 32} patterns" in r.stdout and "identical" in r.stdout, r.stdout
