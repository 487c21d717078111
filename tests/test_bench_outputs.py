"""bench.py's plain run and its --dump-outputs.

A plain `bench.py --gpus 1 --steps N --warmup W` runs the timed steps only
(every other leg is null in the line and needs --full); --dump-outputs DIR
writes what the last timed step returned as float32 .npy files, at most 64 MB
in all, a larger table as the same seeded row sample in every run.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

# dump_outputs on a stand-in context whose table rows hold their own row id
# (bench.py is imported in a child: importing it sets OpenMP defaults)
_STUB = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench

class Ctx:
  d, node_rows, edge_rows = 128, 100001, 50001
  def model_get_rows(self, table, rows):
    r = np.asarray(rows, np.int64)
    return np.repeat((r + table * 1000000).astype(np.float32)[:, None], self.d, 1)

for out in sys.argv[2:]:
  bench.dump_outputs(out, Ctx(), np.array([0.25], np.float32))
"""


def test_dump_outputs_is_a_fixed_sample_within_64mb(tmp_path):
  a, b = str(tmp_path / "a"), str(tmp_path / "b")
  subprocess.run([sys.executable, "-c", _STUB, ROOT, a, b], check=True,
                 timeout=120)
  assert sorted(os.listdir(a)) == ["edge_table.npy", "losses.npy",
                                   "node_table.npy"]
  total = 0
  for name in os.listdir(a):
    x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
    assert x.dtype == np.float32 and np.array_equal(x, y), name
    total += x.nbytes
  assert total <= 64 * 10**6
  assert np.array_equal(np.load(os.path.join(a, "losses.npy")), [0.25])
  node = np.load(os.path.join(a, "node_table.npy"))
  edge = np.load(os.path.join(a, "edge_table.npy"))
  # the node table (51 MB) is sampled: distinct rows in ascending order, from
  # the whole range; the edge table (26 MB) is sampled too, 24 MiB of it
  for tab, rows, base in ((node, 100001, 0), (edge, 50001, 1000000)):
    assert tab.shape == (24 * 2**20 // (4 * 128), 128)
    ids = tab[:, 0] - base
    assert np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < rows
    assert ids[-1] - ids[0] > 0.9 * rows


@pytest.mark.gpu
def test_plain_run_times_the_steps_only_and_dumps_them(tmp_path):
  out = str(tmp_path / "dump")
  p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2",
                      "--warmup", "1", "--num-samples", "20",
                      "--dump-outputs", out], capture_output=True, timeout=170)
  assert p.returncode == 0, p.stderr.decode()[-2000:]
  lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
  assert len(lines) == 1
  r = json.loads(lines[0])
  assert r["steps"] == 2 and r["warmup"] == 1 and r["full"] is False
  assert r["unit"] == "records/s" and r["higher_is_better"] is True
  assert r["dtype"] == "f32" and r["ms_per_step"] > 0
  n = r["config"]["records_per_epoch"]
  assert n > 5_000_000
  assert r["value"] == pytest.approx(n / (r["ms_per_step"] * 1e-3), rel=1e-3)
  assert sum(r["roofline"]["batch_steps"].values()) == 2 * -(-n // 256)
  for leg in ("cpu_baseline", "algdist", "c2_fobe_d128", "c3_hobe_mt19937",
              "end_to_end", "algdist_c4", "c4_full"):
    assert r[leg] is None, leg
  losses = np.load(os.path.join(out, "losses.npy"))
  assert losses.dtype == np.float32 and losses.shape == (1,)
  assert np.isfinite(losses[0]) and losses[0] > 0
  total = losses.nbytes
  for name in ("node_table", "edge_table"):
    t = np.load(os.path.join(out, name + ".npy"))
    assert t.dtype == np.float32 and t.shape[1] == 128
    assert np.isfinite(t).all() and np.abs(t).max() > 0
    total += t.nbytes
  assert total <= 64 * 10**6
