"""CPU: the rejection sampler's automatic 3-hop mode choice, against 128-bit
integers.

csrc/hgx_sample_mode.h (the text reject_rows compiles) is built into a
stand-alone host program, tests/native/sample_mode_check.cpp. For a few
thousand column counts up to 2^31 - 1 and every shift in [-10, 10] it
compares sample_mode3_uniform(W, ncols, shift) with W >= ncols * 2^shift in
__int128 at the threshold and +-1, around every power of two up to 2^62 and
at pseudo-random W, and with the comparison the kernel used before wherever
that one did not overflow (so the keyed stream is unchanged). Built a second
time with -fsanitize=undefined: no shift or addition in the header may
overflow for any of these arguments."""

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sample_mode_check.cpp")
INC = os.path.join(ROOT, "hypergraphembedding_amd", "csrc")
KERNEL = os.path.join(INC, "hgx_sample.hip")


def test_reject_rows_uses_the_checked_function():
  text = open(KERNEL).read()
  assert '#include "hgx_sample_mode.h"' in text
  assert re.search(r"A\.mode3 == 0 && sample_mode3_uniform\(W, A\.ncols, A\.mode3_shift\)", text)
  # no other comparison of W against a shifted column count is left
  assert "<< -A.mode3_shift" not in text and "<< A.mode3_shift" not in text


@pytest.mark.parametrize("flags", [(), ("-fsanitize=undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "ubsan"])
def test_sample_mode_equals_int128(tmp_path, flags):
  cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
  if cxx is None:
    pytest.fail("no host C++ compiler (g++ or clang++) on PATH")
  exe = str(tmp_path / "sample_mode_check")
  cmd = [cxx, "-std=c++17", "-O2", *flags, "-I" + INC, SRC, "-o", exe]
  b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  assert b.returncode == 0, b.stdout
  r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  print(r.stdout)
  assert r.returncode == 0, r.stdout
  m = re.search(r"(\d+) ncols, 21 shifts, (\d+) comparisons identical", r.stdout)
  assert m and int(m.group(1)) > 4000 and int(m.group(2)) > 10_000_000, r.stdout
  assert "runtime error" not in r.stdout
