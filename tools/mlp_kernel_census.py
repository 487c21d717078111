"""The set of mlp_* kernels in a rocprofv3 kernel trace, next to what the
dispatch table of tests/mlp_cases.py says can be selected.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o tr -- \\
      python -m pytest tests/test_gpu_mlp_kernels.py -m gpu -q
  python tools/mlp_kernel_census.py <dir>/.../tr_kernel_trace.csv

Prints the sorted kernel names with their launch counts, then whether the
set equals the kernel names of REACHABLE plus the epoch plumbing's (the
forms after a slash in REACHABLE are run-time branches inside one kernel and
do not show in a trace). Exit status 1 when the sets differ.
"""
import collections
import csv
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", "tests"))
import mlp_cases  # noqa: E402


def short_name(full):
  n = full.replace("(anonymous namespace)::", "").replace("void ", "")
  n = n.split("(")[0].replace(" ", "")
  n = re.sub(r",(false|0)>$", ">", n)
  return re.sub(r",(true|1)>$", ",true>", n)


def main():
  seen = collections.Counter()
  for r in csv.DictReader(open(sys.argv[1])):
    n = short_name(r["Kernel_Name"])
    if n.startswith("mlp_"):
      seen[n] += 1
  want = mlp_cases.kernel_names(mlp_cases.REACHABLE) | set(mlp_cases.EPOCH_KERNELS)
  print("mlp_* kernels in the trace (launches):")
  for n in sorted(seen):
    print("  %-20s %7d" % (n, seen[n]))
  missing, extra = sorted(want - set(seen)), sorted(set(seen) - want)
  print("kernels seen: %d; kernel names of REACHABLE and the epoch plumbing: %d"
        % (len(seen), len(want)))
  print("selectable but not seen: %s" % (", ".join(missing) or "none"))
  print("seen but not in the table: %s" % (", ".join(extra) or "none"))
  print("AGREE" if not missing and not extra else "DISAGREE")
  return 0 if not missing and not extra else 1


if __name__ == "__main__":
  sys.exit(main())
