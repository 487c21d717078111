"""CPU: the trainer step's float -> 2^44 fixed-point conversion, exhaustively.

csrc/hgx_fix.h (the text the device kernels compile) is built into a
stand-alone host program, tests/native/to_fix_check.cpp, with -O2 -fopenmp
and the undefined-behaviour sanitizer. It compares to_fix_magic (the
add-constant form, used at float4 rows) with llrint((double)v * 0x1p44)
under round-to-nearest for every float bit pattern with |v| < 32
(2 x 0x42000000 patterns, denormals and -0 included) on at most 16 threads
and exits non-zero on the first difference. On the device the two forms were
compared by epoch losses of interleaved builds (tools/ab_onekernel.py, all
digits equal at d = 128 and 256)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "to_fix_check.cpp")
INC = os.path.join(ROOT, "hypergraphembedding_amd", "csrc")


def test_to_fix_equals_llrint_for_every_float_in_range(tmp_path):
  cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
  if cxx is None:
    pytest.fail("no host C++ compiler (g++ or clang++) on PATH")
  exe = str(tmp_path / "to_fix_check")
  cmd = [cxx, "-std=c++17", "-O2", "-fopenmp", "-fsanitize=undefined",
         "-fno-sanitize-recover=undefined", "-I" + INC, SRC, "-o", exe]
  b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  assert b.returncode == 0, b.stdout
  env = dict(os.environ, OMP_NUM_THREADS=str(min(16, os.cpu_count() or 1)))
  r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                     env=env)
  print(r.stdout)
  assert r.returncode == 0, r.stdout
  assert f"{2 * 0x42000000} patterns" in r.stdout, r.stdout
